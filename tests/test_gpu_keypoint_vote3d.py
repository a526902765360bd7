"""Keypoint voting in 3D on the device (slhip_keypoint_vote3d, sl.keypoint_vote3d, SceneBatch.keypoint_votes3d) against the
library's host twin of the same rules (slhip_keypoint_vote3d_host), bit for bit on every output -- floats as their int32 views --
and end to end on a placed batch: rendered points and their exact offsets through the vote and the rigid fit back to the batch's
keypoints and poses.  Every output lies between 256 poisoned guard bytes that must stay poison, and an output that `outputs` does
not name stays poison throughout.

The end-to-end bounds are computed in the tests, never from the code under test: four times the worst difference that the float64
references (tests/keypoint_vote3d_ref.py, then tests/pose_fit_ref.py's SVD) show on the same float32 inputs -- against the batch's
keypoints for the votes, against the batch's object_to_camera for the poses (pose_difference: the Frobenius norm of the [3, 4]
difference).  That difference is the data's: float32 offsets and float32 keypoints.  Every figure is printed on every run.
    measured on one MI355X: votes 1.9e-9 m from the keypoints (the reference 1.6e-9 m), poses 6.6e-7 (the reference 5.2e-7)"""
import ctypes as C

import numpy as np
import pytest
import torch

import keypoint_vote3d_ref as R
import pose_fit_ref as RF
from stillleben_amd import _abi
from stillleben_amd import keypoint_vote3d as kv
from test_gpu_object_keypoints import Guarded, bits, stream, to_dev
from test_host_keypoint_vote3d import H, KW, NAMES, make_clusters

pytestmark = pytest.mark.gpu

F = np.float32
DTYPES = dict(xyz=F, n_support=np.int32, best=np.int32, iters=np.int32, flags=np.int32, mean=F, cov=F, support=np.uint32)
WIDTH = dict(xyz=3, n_support=1, best=1, iters=1, flags=1, mean=3, cov=6)


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def make_batch(M, K, Kp, seed):
    """M sets of clusters, outliers and voters that do not count (test_host_keypoint_vote3d.make_clusters); the last set -- with
    one set, the last keypoint when there are several -- has no valid voter"""
    cam, off, _, _ = make_clusters(M, K, Kp, seed, empty_set=M - 1 if M > 1 else None)
    if M == 1 and Kp > 1:
        off[0, :, Kp - 1, 0] = np.nan
    return cam, off


def run_device(dev, cam, off, mask=255, null=None, misalign=None, **kw):
    M, K = cam.shape[:2]
    Kp = off.shape[2]
    d = {"camera": to_dev(cam, dev), "offsets": to_dev(off, dev)}
    ptr = {k: (None if null == k else t.data_ptr() + (4 if misalign == k and k == "camera" else 2 if misalign == k else 0)) for k, t in d.items()}
    sizes = {k: M * Kp * w * 4 for k, w in WIDTH.items()}
    sizes["support"] = M * Kp * kv.n_words(K) * 4
    outs = {k: Guarded(sizes[k], dev) for k in NAMES}
    o = _abi.KeypointVote3dOut(*(None if null == k else outs[k].ptr().value + (2 if misalign == k else 0) for k in NAMES))
    kw.setdefault("n_sets", M)
    p = kv.make_params(kw.pop("n_sets"), kw.pop("n_points", K), kw.pop("n_keypoints", Kp), outputs=mask, **kw).reshape(1)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_keypoint_vote3d(None if null == "params" else p.ctypes.data, C.c_void_p(ptr["camera"]), C.c_void_p(ptr["offsets"]),
                                              None if null == "record" else C.byref(o), stream(dev))
    return st, outs, d


def read(outs, M, K, Kp, mask):
    got = {}
    for i, k in enumerate(NAMES):
        if mask & (1 << i):
            shape = (M, Kp, kv.n_words(K)) if k == "support" else (M, Kp) + ((WIDTH[k],) if WIDTH[k] > 1 else ())
            got[k] = outs[k].host(DTYPES[k], shape).copy()
        else:
            assert outs[k].untouched(), k
    return got


def assert_same(got, want, what):
    for k, v in got.items():
        w = getattr(want, k)
        diff = bits(v).reshape(-1, 4).view(np.int32) != bits(w).reshape(-1, 4).view(np.int32)
        first = int(np.argwhere(diff.reshape(-1))[0][0]) if diff.any() else 0
        assert not diff.any(), "%s %s: %d of %d words differ, the first at %d: %r against %r" % (
            what, k, int(diff.sum()), diff.size, first, v.reshape(-1)[first], w.reshape(-1)[first])


# M, K, Kp, S: the smallest case, more seeds than voters, just under a wave, one wave, one past a wave (a second wave for one
# seed), seeds beyond the block (a lane takes two), the customary shape, the LDS ceiling (4 steps at most: the walk is long)
SHAPES = [(1, 1, 1, 1), (3, 2, 2, 4), (2, 63, 1, 64), (2, 64, 3, 64), (2, 65, 9, 65), (1, 257, 2, 300), (1, 1024, 9, 128), (1, 4096, 1, 64)]


@pytest.mark.parametrize("M,K,Kp,S", SHAPES)
def test_device_against_host_twin_bit_for_bit(dev, M, K, Kp, S):
    cam, off = make_batch(M, K, Kp, 7 + K + S)
    kw = dict(KW, n_seeds=S, max_iters=4 if K == 4096 else 32)
    want = kv.vote_host(cam, off, **kw)
    st, outs, keep = run_device(dev, cam, off, **kw)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, M, K, Kp, 255), want, "M %d K %d Kp %d S %d" % (M, K, Kp, S))
    if M > 1:
        assert (want.flags[M - 1] == _abi.VOTE3D_INSUFFICIENT).all() and want.found[:M - 1].all()
    elif Kp > 1:
        assert want.flags[0, Kp - 1] == _abi.VOTE3D_INSUFFICIENT and want.found[0, :Kp - 1].all()
    else:
        assert want.found.all()


def test_flags_bit_for_bit(dev):
    """the paths that write no position or a flagged one: NO_MODEL (min_support above every cluster) and NOT_CONVERGED (one
    step)"""
    cam, off = make_batch(3, 65, 2, 21)
    for kw, flag in ((dict(KW, min_support=60), _abi.VOTE3D_NO_MODEL), (dict(KW, max_iters=1, tol=0.0), _abi.VOTE3D_NOT_CONVERGED)):
        want = kv.vote_host(cam, off, n_seeds=16, **kw)
        assert (want.flags[:2] == flag).all() and (want.flags[2] == _abi.VOTE3D_INSUFFICIENT).all()
        st, outs, keep = run_device(dev, cam, off, n_seeds=16, **kw)
        assert st == 0
        assert_same(read(outs, 3, 65, 2, 255), want, "flag %d" % flag)


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 64, 128, 1 | 128, 2 | 32 | 64, 4 | 16])
def test_outputs_not_named_stay_poison(dev, mask):
    cam, off = make_batch(3, 65, 2, 3)      # the last set takes the path that writes no position
    kw = dict(KW, n_seeds=32)
    st, outs, keep = run_device(dev, cam, off, mask=mask, **kw)
    assert st == 0
    assert_same(read(outs, 3, 65, 2, mask), kv.vote_host(cam, off, **kw), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev):
    cam, off = make_batch(2, 16, 3, 4)
    for kw in (dict(null="params"), dict(null="camera"), dict(null="offsets"), dict(null="record"), dict(null="xyz"), dict(null="cov"),
               dict(null="support"), dict(null="iters"), dict(misalign="camera"), dict(misalign="offsets"), dict(misalign="mean"),
               dict(n_points=0), dict(n_points=4097), dict(n_keypoints=0), dict(n_keypoints=33), dict(n_seeds=0), dict(n_seeds=1025),
               dict(bandwidth=0.0), dict(bandwidth=float("nan")), dict(max_iters=0), dict(max_iters=65), dict(tol=-1.0),
               dict(min_support=0), dict(mask=0), dict(mask=256)):
        st, outs, keep = run_device(dev, cam, off, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, keep = run_device(dev, cam, off, n_sets=0)      # no sets: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())


def test_step_timer(dev):
    cam, off = make_batch(2, 64, 3, 5)
    L = _abi.lib()
    ms = (C.c_float * 1)()
    try:
        assert L.slhip_keypoint_vote3d_timing_enable(1) == 0
        assert run_device(dev, cam, off, mask=0)[0] < 0                        # a refused call records no event
        assert L.slhip_keypoint_vote3d_timings(C.byref(ms)) == 0 and list(ms) == [-1.0]
        assert run_device(dev, cam, off)[0] == 0
        assert L.slhip_keypoint_vote3d_timings(C.byref(ms)) == 0 and np.isfinite(ms[0]) and ms[0] >= 0.0
        assert L.slhip_keypoint_vote3d_timings(None) < 0
    finally:
        L.slhip_keypoint_vote3d_timing_enable(0)


# ---- end to end on a placed batch ------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 4, 4, (160, 120), (266.7, 266.85, 78.25, 60.3)
VOTE_KW = dict(n_seeds=32, bandwidth=H, max_iters=32, tol=1e-4, min_support=1)


@pytest.fixture(scope="module")
def placed3d(sl):
    """the fixture shape of test_gpu_keypoint_vote.py::placed, with the points' camera and coord outputs and the exact offsets"""
    from test_gpu_synth import small_table

    table = small_table(sl)
    batch = sl.SceneBatch(table, N_SCENES, N_OBJ, resolution=RES, seed=(77 << 32) | 5, render_chunk=N_SCENES, manual_exposure=1.0,
                          scene_id_base=1000)
    batch.set_camera_intrinsics(*INTRINSICS)
    batch.stage()
    batch.settle(frames=5)
    batch.place(object_to_camera=True)
    bufs = batch.render(0, object_masks=True)
    points = batch.points(bufs, n_points=256, min_px=120, outputs=("camera", "coord"))
    kbank = sl.object_keypoints.bank(table, n_fps=8)      # the centre and 8 FPS points
    kps = batch.keypoints(bufs, bank=kbank)
    off = kps.offsets(points).contiguous()
    mbank = sl.pose_error.bank(table, n_points=64)
    torch.cuda.synchronize()
    return sl, batch, points, kbank, kps, off, mbank


def truth_of(points, kps):
    """(keypoints float64 [n, Kp, 3] in the camera frame, in front bool [n, Kp]) of every set's object"""
    scene, slot = points.scene.long(), (points.slot - 1).long()
    return kps.camera[scene, slot][..., :3].cpu().numpy().astype(np.float64), kps.in_front[scene, slot].cpu().numpy()


def reference_votes(points, off):
    return R.solve_sets(points.camera.cpu().numpy(), off.cpu().numpy(), **VOTE_KW)


def pose_difference(poses, gt):
    """[n]: the Frobenius norm of poses - gt over the twelve entries of [3, 4], float64: one number for "the poses match",
    rotation entries as they are and the translation in metres.  A point p moves by |(P - G) (p, 1)| <= |P - G|_F sqrt(|p|^2 + 1)
    between the two poses (Cauchy-Schwarz, row by row): what test_gpu_pose_fit.py bounds the ADD with."""
    d = np.asarray(poses, np.float64) - np.asarray(gt, np.float64)
    return np.sqrt((d * d).sum((1, 2)))


def reference_poses(src, ref_xyz):
    """the float64 SVD fit of the bank's keypoints src [n, Kp, 4] onto the reference's votes [n, Kp, 3]"""
    dst = np.concatenate([ref_xyz, np.ones(ref_xyz.shape[:2] + (1,))], -1)
    return np.stack([RF.fit_svd(s, d)[0] for s, d in zip(src, dst)])


def check_votes_and_poses(placed3d, off, what, supporters=None):
    sl, batch, points, kbank, kps, _, mbank = placed3d
    n, Kp = len(points), len(kbank)
    assert n >= 4 and Kp == 9, "the fixture shows too few objects: %d" % n
    votes = batch.keypoint_votes3d(points, off, **VOTE_KW)
    fit = batch.pose_fit(votes, bank=kbank)
    torch.cuda.synchronize()
    truth, front = truth_of(points, kps)
    assert front.all() and bool(votes.found.all()) and bool((votes.flags == 0).all())
    ref = reference_votes(points, off)
    ref_xyz = np.array([[r.xyz for r in row] for row in ref])
    assert all(r.flags == 0 for row in ref for r in row)
    d_ref = np.linalg.norm(ref_xyz - truth, axis=-1)
    d_dev = np.linalg.norm(votes.xyz.cpu().numpy().astype(np.float64) - truth, axis=-1)
    bound = 4.0 * d_ref.max()
    print("keypoint_vote3d %s: %d sets x %d keypoints, worst distance from the batch's keypoints %.3g m, the float64 reference's "
          "%.3g m, bound %.3g m" % (what, n, Kp, d_dev.max(), d_ref.max(), bound))
    assert d_dev.max() <= bound
    # every keypoint is supported by the valid points of its set (by those whose offsets were left alone)
    valid = points.valid.cpu().numpy()
    want = valid[:, None, :] if supporters is None else supporters
    assert np.array_equal(votes.support_mask().cpu().numpy(), np.broadcast_to(want, (n, Kp, valid.shape[1])))
    assert np.array_equal(votes.n_support.cpu().numpy(), np.broadcast_to(want, (n, Kp, valid.shape[1])).sum(-1))
    # the PVN3D pose: the bank's keypoints onto the voted ones
    src, dst = votes.correspondences(kbank)
    gt = points.object_to_camera.cpu().numpy()
    p_ref = pose_difference(reference_poses(src.cpu().numpy(), ref_xyz), gt)
    p_dev = pose_difference(fit.pose.cpu().numpy(), gt)
    print("pose_fit of the votes %s: worst difference from object_to_camera %.3g, the float64 reference pipeline's %.3g, bound %.3g"
          % (what, p_dev.max(), p_ref.max(), 4.0 * p_ref.max()))
    assert bool(fit.found.all()) and bool((fit.n_used == Kp).all())
    assert p_dev.max() <= 4.0 * p_ref.max()
    return votes, fit


def test_votes_on_the_exact_offsets_land_on_the_keypoints(placed3d):
    sl, batch, points, kbank, kps, off, mbank = placed3d
    votes, fit = check_votes_and_poses(placed3d, off, "on the exact offsets")
    assert np.array_equal(votes.classes.cpu().numpy(),
                          batch.host_objects()["asset"].reshape(N_SCENES, N_OBJ)[points.scene_global.cpu().numpy(), points.slot.cpu().numpy() - 1])
    # the same through the module's own entry on the raw tensor
    again = kv.vote(points.camera, off, **VOTE_KW)
    assert torch.equal(again.xyz, votes.xyz) and torch.equal(again.support, votes.support)
    with pytest.raises(TypeError):
        batch.keypoint_votes3d(points, off, classes=None)
    with pytest.raises(TypeError):
        batch.pose_fit(votes)
    with pytest.raises(TypeError):
        batch.pose_fit(votes, points.camera, bank=kbank)


def test_damaged_offsets(placed3d):
    """30 % of every set's voters get, for every keypoint, an offset that is off by 0.3 to 1 m in a random direction: at least 6 h
    from the keypoint and, being spread over a shell of that size, nowhere near as dense as the 70 % that agree to a rounding --
    the majority is unambiguous by construction.  The positions and the poses stay; the supporters are the untouched voters"""
    sl, batch, points, kbank, kps, off, mbank = placed3d
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    n, K, Kp = off.shape[:3]
    hit = torch.zeros((n, K), dtype=torch.bool)
    for i in range(n):
        hit[i, torch.randperm(K, generator=g)[:int(0.3 * K)]] = True
    way = torch.randn((n, K, Kp, 3), generator=g)
    way = way / way.norm(dim=-1, keepdim=True) * (0.3 + 0.7 * torch.rand((n, K, Kp, 1), generator=g))
    bad = torch.where(hit[..., None, None].to(off.device), off + way.to(off.device), off).contiguous()
    valid = points.valid.cpu().numpy()
    check_votes_and_poses(placed3d, bad, "with 30 % damaged", supporters=(valid & ~hit.numpy())[:, None, :])


def test_cpu_tensors_are_refused(placed3d):
    sl, batch, points, kbank, kps, off, mbank = placed3d
    with pytest.raises(_abi.SlhipError) as e:
        kv.vote(points.camera.cpu(), off.cpu())
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        kv.vote(points, off.cpu())
    with pytest.raises(_abi.SlhipError):
        batch.keypoint_votes3d(points.map(lambda t: t.cpu()), off)
