"""The robust alignment on the device (slhip_pose_align, sl.pose_align, SceneBatch.pose_align) against the library's host twin of
the same rules (slhip_pose_align_host), bit for bit on every output -- floats as their int32 views --, and end to end on a placed
batch: rendered object coordinates of which 30 % are moved by 0.05 to 0.3 m, aligned to the camera points, recover the batch's
object_to_camera and exactly the untouched rows; so do voted keypoints of which two of nine are moved by 0.1 m, where the plain
fit is far off.  Every output lies between 256 poisoned guard bytes that must stay poison, and an output that `outputs` does not
name stays poison throughout.

The end-to-end bound is computed in the test, never from the code under test: four times the worst pose_difference (the
Frobenius norm of the [3, 4] difference, tests/test_gpu_keypoint_vote3d.py) from object_to_camera that the float64 reference
(tests/pose_align_ref.py) shows on the same float32 inputs; the ADD's bound is that times sqrt(r^2 + 1), r the largest |p| of
the model bank (tests/test_gpu_pose_fit.py derives it).  Every figure is printed on every run."""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_align_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_align as pa
from test_gpu_keypoint_vote3d import N_OBJ, N_SCENES, VOTE_KW, placed3d, pose_difference  # noqa: F401  (placed3d: a fixture)
from test_gpu_object_keypoints import Guarded, bits, stream, to_dev
from test_host_pose_align import NAMES, THR, damaged_case, moved

pytestmark = pytest.mark.gpu

F = np.float32
DTYPES = dict(pose=F, n_inliers=np.int32, rms=F, inliers=np.uint32, best=np.int32, flags=np.int32)
EDGES = (31, 32, 63, 64, 255, 256)      # the rows at the ends of a ballot word, of a wave and of the workgroup's stride


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def make_batch(M, K, seed, with_init):
    """M sets of K correspondences: rigid motions with 0.3 mm of noise (a few rows land near the threshold of 1 mm), 30 % of the
    rows damaged from K = 16 on, and rows that do not count at the word, wave and stride boundaries.  With M > 1, set 3 of every
    eight has two valid rows (insufficient) and set 5 of every eight is a line (no model; with its initial pose, a refit that
    stops).  Initial poses near the truth; set 2: NaN, set 4: the truth itself"""
    rng = np.random.default_rng(seed)
    src, dst, init = np.zeros((M, K, 4), F), np.zeros((M, K, 4), F), np.zeros((M, 3, 4), F)
    for i in range(M):
        s, d, pose, _ = damaged_case(K, int(0.3 * K) if K >= 16 else 0, seed * 1000 + i)
        if K >= 16:
            d[:, :3] += rng.normal(size=(K, 3)).astype(F) * F(3e-4)
        kinds = [(s, 3, 0.0), (d, 3, 0.0), (s, 1, np.nan), (d, 2, np.inf), (s, 3, -1.0), (d, 0, np.nan)]
        for n, j in enumerate(e for e in EDGES if e < K - 3):
            a, col, v = kinds[(n + i) % len(kinds)]
            a[j, col] = v
        if M > 1 and i % 8 == 3:
            s[2:, 3] = 0.0
        if M > 1 and i % 8 == 5:
            s[:, :3] = np.outer(np.linspace(-0.1, 0.1, K), [0.6, 0.0, 0.8]).astype(F)
            d = moved(s, pose[:, :3], pose[:, 3])
        src[i], dst[i] = s, d
        near = pose.copy()
        near[:, 3] += rng.normal(size=3) * (2e-4 if i != 4 else 0.0)
        init[i] = np.nan if i == 2 else near
    return src, dst, (init if with_init else None)


def run_device(dev, src, dst, init, mask=63, null=None, misalign=None, **kw):
    M, K = src.shape[:2]
    d = {"src": to_dev(src, dev), "dst": to_dev(dst, dev), "init": None if init is None else to_dev(init, dev)}
    ptr = {k: (None if t is None or null == k else t.data_ptr() + ((2 if k == "init" else 4) if misalign == k else 0)) for k, t in d.items()}
    sizes = dict(pose=M * 48, n_inliers=M * 4, rms=M * 4, inliers=M * pa.n_words(K) * 4, best=M * 4, flags=M * 4)
    outs = {k: Guarded(sizes[k], dev) for k in NAMES}
    o = _abi.PoseAlignOut(*(None if null == k else outs[k].ptr().value + (2 if misalign == k else 0) for k in NAMES))
    kw.setdefault("n_sets", M)
    kw.setdefault("threshold", THR)
    p = pa.make_params(kw.pop("n_sets"), kw.pop("n_points", K), outputs=mask, **kw).reshape(1)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_align(None if null == "params" else p.ctypes.data, C.c_void_p(ptr["src"]), C.c_void_p(ptr["dst"]),
                                         C.c_void_p(ptr["init"]), None if null == "record" else C.byref(o), stream(dev))
    return st, outs, d


def read(outs, M, K, mask):
    got = {}
    for i, k in enumerate(NAMES):
        if mask & (1 << i):
            shape = {"pose": (M, 3, 4), "inliers": (M, pa.n_words(K))}.get(k, (M,))
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


# M, K, Hy, refine_iters, initial poses.  K: the fewest that fit, the 16-byte tail of the score (3, 63, 65, 255, 257), one wave,
# one past it, the 256 stride and either side of it, the customary size, the raised-LDS path (4096: 96 KiB).  Hy: none (a pure
# refit), one, either side of a round of 256, the limit.  One set and 37; refits: none, one, the limit
SHAPES = [(1, 3, 64, 1, False), (1, 4, 1, 0, False), (37, 63, 255, 1, False), (1, 64, 256, 16, True), (37, 65, 257, 1, True),
          (1, 255, 64, 1, False), (37, 256, 0, 16, True), (1, 257, 256, 16, False), (1, 1024, 256, 1, False), (1, 4096, 64, 16, False),
          (1, 257, 4096, 0, False), (2, 4096, 4096, 1, True)]


@pytest.mark.parametrize("M,K,Hy,iters,with_init", SHAPES)
def test_device_against_host_twin_bit_for_bit(dev, M, K, Hy, iters, with_init):
    src, dst, init = make_batch(M, K, 7 + K + Hy, with_init)
    kw = dict(n_hypotheses=Hy, refine_iters=iters, seed=(9 << 32) | K, set_id_base=100)
    want = pa.solve_host(src, dst, init, threshold=THR, **kw)
    st, outs, keep = run_device(dev, src, dst, init, **kw)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, M, K, 63), want, "M %d K %d Hy %d" % (M, K, Hy))
    if M == 37:      # the sets built to fail did, the others did not
        assert want.flags[3] == _abi.ALIGN_INSUFFICIENT and not want.found[[3, 11]].any()
        if with_init:      # the line's initial pose holds every row, and the refit of a line stops
            assert want.flags[5] == _abi.ALIGN_REFINE_STOPPED and want.best[5] == -1 and want.found[5]
        else:
            assert want.flags[5] == _abi.ALIGN_NO_MODEL and not want.found[[5, 13]].any()
        good = [0, 1, 6, 8] + ([4] if with_init else [])
        assert (want.n_inliers[good] >= 0.5 * K).all() and want.found[good].all()
        if with_init and Hy == 0:
            assert want.flags[2] == _abi.ALIGN_NO_MODEL      # a NaN initial pose and nothing else to score
    elif Hy >= 64:
        assert want.found[0] and want.n_inliers[0] >= 0.5 * K


def test_edge_cases_bit_for_bit(dev):
    """a refit that is rejected, a refit that stops, min_inliers above what exists, identical correspondences"""
    rng = np.random.default_rng(13)
    K = 10
    src, dst, init = np.ones((4, K, 4), F), np.ones((4, K, 4), F), np.tile(np.eye(4, dtype=F)[:3], (4, 1, 1))
    src[0, :, :3] = (rng.random((K, 3)) - 0.5) * 0.25
    dst[0] = src[0]
    dst[0, 7:9, 0] += F(0.99 * 0.125)
    dst[0, 9, 0] -= F(0.99 * 0.125)                                       # test_host_pose_align: REFINE_REJECTED
    src[1, :3, :3] = np.outer([-0.1, 0.0, 0.1], [1.0, 0.0, 0.0])
    src[1, 3:, :3] = (rng.random((K - 3, 3)) - 0.5) * 0.25
    dst[1] = src[1]
    dst[1, 3:, :3] += 0.5                                                 # three collinear inliers: REFINE_STOPPED
    src[2, :, :3] = (rng.random((K, 3)) - 0.5) * 0.25
    dst[2] = src[2]
    dst[2, 4:, :3] += rng.random((K - 4, 3)).astype(F) * 0.3 + 0.2        # four agree
    src[3, :, :3], dst[3, :, :3] = [0.01, 0.02, 0.03], [0.01, 0.02, 0.03]
    for kw in (dict(n_hypotheses=0, threshold=0.125), dict(n_hypotheses=0, threshold=1e-3), dict(n_hypotheses=64, threshold=1e-3, min_inliers=5)):
        want = pa.solve_host(src, dst, init, seed=3, **kw)
        st, outs, keep = run_device(dev, src, dst, init, seed=3, **kw)
        assert st == 0, _abi.lib().slhip_last_error()
        assert_same(read(outs, 4, K, 63), want, str(kw))
        if kw["threshold"] == 0.125:
            assert want.flags[0] == _abi.ALIGN_REFINE_REJECTED and want.n_inliers[0] == 10
        elif kw["n_hypotheses"] == 0:
            assert want.flags[1] == _abi.ALIGN_REFINE_STOPPED and want.n_inliers[1] == 3
        else:
            assert want.flags[2] == _abi.ALIGN_NO_MODEL and want.flags[3] == _abi.ALIGN_REFINE_STOPPED      # (the identity holds the ten)


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 1 | 32, 2 | 4 | 8])
def test_outputs_not_named_stay_poison(dev, mask):
    src, dst, init = make_batch(9, 65, 3, False)      # set 3 and set 5 take the paths that write no pose
    kw = dict(n_hypotheses=32, refine_iters=2)
    st, outs, keep = run_device(dev, src, dst, init, mask=mask, **kw)
    assert st == 0
    assert_same(read(outs, 9, 65, mask), pa.solve_host(src, dst, threshold=THR, **kw), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev):
    src, dst, init = make_batch(2, 16, 4, True)
    for kw in (dict(null="params"), dict(null="src"), dict(null="dst"), dict(null="record"), dict(null="pose"), dict(null="rms"),
               dict(null="inliers"), dict(misalign="src"), dict(misalign="dst"), dict(misalign="init"), dict(misalign="best"),
               dict(null="init", n_hypotheses=0), dict(n_points=2), dict(n_points=4097), dict(n_hypotheses=4097), dict(threshold=0.0),
               dict(threshold=float("nan")), dict(min_gap=1.0), dict(refine_iters=17), dict(min_inliers=2), dict(mask=0), dict(mask=64)):
        st, outs, keep = run_device(dev, src, dst, init, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, keep = run_device(dev, src, dst, init, n_sets=0)      # no sets: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())


def test_step_timer(dev):
    src, dst, init = make_batch(2, 64, 5, False)
    L = _abi.lib()
    ms = (C.c_float * 1)()
    try:
        assert L.slhip_pose_align_timing_enable(1) == 0
        assert run_device(dev, src, dst, init, mask=0)[0] < 0                  # a refused call records no event
        assert L.slhip_pose_align_timings(C.byref(ms)) == 0 and list(ms) == [-1.0]
        assert run_device(dev, src, dst, init)[0] == 0
        assert L.slhip_pose_align_timings(C.byref(ms)) == 0 and np.isfinite(ms[0]) and ms[0] >= 0.0
        assert L.slhip_pose_align_timings(None) < 0
    finally:
        L.slhip_pose_align_timing_enable(0)


# ---- end to end on a placed batch ------------------------------------------------------------------------------------------------
def shifted(points, share=0.3, seed=5):
    """(coord with `share` of every set's rows moved by 0.05 to 0.3 m in a random direction, touched bool [n, K])"""
    n, K = points.coord.shape[:2]
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    coord = points.coord.cpu().clone()
    touched = torch.zeros((n, K), dtype=torch.bool)
    for i in range(n):
        touched[i, torch.randperm(K, generator=g)[:int(share * K)]] = True
    way = torch.randn((n, K, 3), generator=g)
    way = way / way.norm(dim=-1, keepdim=True) * (0.05 + 0.25 * torch.rand((n, K, 1), generator=g))
    coord[..., :3] = torch.where(touched[..., None], coord[..., :3] + way, coord[..., :3])
    return coord.to(points.coord.device).contiguous(), touched.numpy()


def test_shifted_coordinates_onto_camera_points_recover_the_pose(placed3d):  # noqa: F811
    sl, batch, points, kbank, kps, off, mbank = placed3d
    n, K = len(points), 256
    assert n >= 4, "the fixture shows too few objects: %d" % n
    coord, touched = shifted(points)
    res = batch.pose_align(points, coord=coord, threshold=THR)
    torch.cuda.synchronize()
    valid = points.valid.cpu().numpy()
    mask = res.inlier_mask().cpu().numpy()
    assert bool(res.found.all()) and bool((res.flags == 0).all()) and bool((res.best >= 0).all())
    assert np.array_equal(mask, valid & ~touched), "%d rows classified otherwise" % int((mask != (valid & ~touched)).sum())
    assert np.array_equal(res.n_inliers.cpu().numpy(), (valid & ~touched).sum(1))
    gt = points.object_to_camera.cpu().numpy()
    src, dst = coord.cpu().numpy(), points.camera.cpu().numpy()
    key = _abi.view_key(int(batch.params["seed_lo"]), int(batch.params["seed_hi"]), batch.view)
    base = int(batch.params["scene_id_base"])
    refs = [R.solve(src[i], dst[i], THR, seed=key[0] | (key[1] << 32), set_id=base + i) for i in range(n)]
    assert all(r.flags == 0 and np.array_equal(r.inliers, mask[i]) for i, r in enumerate(refs))
    assert [r.best for r in refs] == res.best.cpu().tolist()
    p_ref, p_dev = pose_difference(np.stack([r.pose for r in refs]), gt), pose_difference(res.pose.cpu().numpy(), gt)
    bound = 4.0 * p_ref.max()
    print("pose_align of shifted coord onto camera: %d sets, worst difference from object_to_camera %.3g, the float64 reference's %.3g, "
          "bound %.3g; worst rms %.3g m" % (n, p_dev.max(), p_ref.max(), bound, float(res.rms.max())))
    assert p_dev.max() <= bound

    # the poses through pose_errors: ADD <= the pose bound times sqrt(r^2 + 1), r the largest |p| of the model bank
    err = batch.pose_errors(res.dense(N_SCENES, N_OBJ, points.scene_global, points.slot), mbank, outputs=("add",))
    torch.cuda.synchronize()
    scene, slot = points.scene_global.long().cpu(), points.slot.long().cpu()
    add = err.add.cpu()[scene, slot - 1].numpy()
    assert int(torch.isfinite(err.add).sum()) == n
    r = float(mbank.points[..., :3].norm(dim=-1).max())
    print("pose_align -> pose_errors: worst ADD %.3g m, bound %.3g m (r = %.3g m)" % (add.max(), bound * np.sqrt(r * r + 1.0), r))
    assert add.max() <= bound * np.sqrt(r * r + 1.0)

    # the plain fit of the same rows is far off
    fit = batch.pose_fit(coord, points.camera)
    assert pose_difference(fit.pose.cpu().numpy(), gt).min() > 100 * bound

    # twice the same call: the same bytes; the module's own entry with the batch's key and base: the same again
    again = batch.pose_align(points, coord=coord, threshold=THR)
    direct = pa.solve(coord, points.camera, threshold=THR, seed=key, set_id_base=base)
    for k in NAMES:
        assert torch.equal(getattr(again, k), getattr(res, k)) and torch.equal(getattr(direct, k), getattr(res, k)), k

    # ICP takes the result as its initial pose
    icp = batch.pose_icp(points, res, mbank, max_iters=2)
    same = batch.pose_icp(points, res.pose, mbank, max_iters=2)
    torch.cuda.synchronize()
    assert not bool((icp.flags & (_abi.ICP_NO_INIT | _abi.ICP_BAD_CLASS)).any()) and torch.equal(icp.pose.view(torch.int32), same.pose.view(torch.int32))

    for kw in (dict(seed=3), dict(set_id_base=1)):
        with pytest.raises(TypeError, match="itself"):
            batch.pose_align(points, threshold=THR, **kw)
    with pytest.raises(TypeError):
        batch.pose_align(points, threshold=THR, bank=kbank)
    with pytest.raises(TypeError, match="threshold"):
        batch.pose_align(points)

    # a second view: other draws (another winner somewhere), the same inliers
    try:
        batch.place(view=1)
        other = batch.pose_align(points, coord=coord, threshold=THR)
        torch.cuda.synchronize()
        assert np.array_equal(other.inlier_mask().cpu().numpy(), mask) and not torch.equal(other.best, res.best)
    finally:
        batch.place(object_to_camera=True)


def test_two_of_nine_voted_keypoints_moved(placed3d):  # noqa: F811
    """the PVN3D route: exact offsets voted to keypoints, then two of the nine moved by 0.1 m.  The alignment finds the seven and
    the pose; the plain fit of the nine is far off.  The threshold of 1 mm lies far above the votes' distance from the batch's
    keypoints (1.9e-9 m, tests/test_gpu_keypoint_vote3d.py) and 100 times below the damage"""
    sl, batch, points, kbank, kps, off, mbank = placed3d
    n = len(points)
    votes = batch.keypoint_votes3d(points, off, **VOTE_KW)
    clean_fit = batch.pose_fit(votes, bank=kbank)
    g = torch.Generator(device="cpu")
    g.manual_seed(9)
    way = torch.randn((n, 2, 3), generator=g)
    way = (way / way.norm(dim=-1, keepdim=True) * 0.1).to(votes.xyz.device)
    votes.xyz[:, 2] += way[:, 0]
    votes.xyz[:, 6] += way[:, 1]
    res = batch.pose_align(votes, bank=kbank, threshold=THR)
    fit = batch.pose_fit(votes, bank=kbank)
    torch.cuda.synchronize()
    want = np.ones((n, 9), bool)
    want[:, [2, 6]] = False
    assert bool(res.found.all()) and np.array_equal(res.inlier_mask().cpu().numpy(), want) and bool((res.n_inliers == 7).all())
    gt = points.object_to_camera.cpu().numpy()
    src, dst = (t.cpu().numpy() for t in votes.correspondences(kbank))
    ref = np.stack([R.kabsch(src[i, want[i], :3], dst[i, want[i], :3]) for i in range(n)])
    p_ref, p_dev, p_fit = pose_difference(ref, gt), pose_difference(res.pose.cpu().numpy(), gt), pose_difference(fit.pose.cpu().numpy(), gt)
    print("pose_align of the votes with 2 of 9 moved: worst difference from object_to_camera %.3g, the float64 fit of the seven %.3g, "
          "bound %.3g; the plain fit of the nine: %.3g at best (of the clean nine: %.3g at worst)"
          % (p_dev.max(), p_ref.max(), 4.0 * p_ref.max(), p_fit.min(), pose_difference(clean_fit.pose.cpu().numpy(), gt).max()))
    assert p_dev.max() <= 4.0 * p_ref.max() and p_fit.min() > 100 * 4.0 * p_ref.max()
    with pytest.raises(TypeError):
        batch.pose_align(votes, threshold=THR)
    with pytest.raises(TypeError):
        batch.pose_align(votes, points.camera, bank=kbank, threshold=THR)


def test_cpu_tensors_are_refused(placed3d):  # noqa: F811
    sl, batch, points, kbank, kps, off, mbank = placed3d
    with pytest.raises(_abi.SlhipError) as e:
        pa.solve(points.coord.cpu(), points.camera.cpu(), threshold=THR)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        batch.pose_align(points.coord, points.camera.cpu(), threshold=THR)
    with pytest.raises(_abi.SlhipError):
        batch.pose_align(points, init=points.object_to_camera.cpu().contiguous(), threshold=THR)
