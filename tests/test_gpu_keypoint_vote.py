"""Keypoint voting on the device (slhip_keypoint_vote, sl.keypoint_vote, SceneBatch.keypoint_votes) against the library's host
twin of the same rules (slhip_keypoint_vote_host), bit for bit on every output -- floats as their int32 views -- in both input
modes, and end to end on a placed batch against the float64 implementation tests/keypoint_vote_ref.py.  Every output lies between
256 poisoned guard bytes that must stay poison, and an output that `outputs` does not name stays poison throughout.

The end-to-end bounds, both by the 4 x rule of tests/test_host_pose_pnp.py and both printed on every run.  UV_BOUND is four times the
worst distance, from the projected keypoints of the batch (kps.uv), of the float64 reference's positions on the target field of the
point sets of the `placed` fixture: that error is the data's (float32 unit vectors and float32 projections), not a solver's.
ADD_BOUND is four times the worst ADD, against the batch's ground truth, of the reference pipeline on the same sets: the float64
reference's positions through the float64 PnP of tests/pose_pnp_ref.py.
    measured worst: the reference against the projected keypoints 3.1e-7 px (the device 1.6e-7 px; on the damaged field 1.9e-7 px,
    the reference 3.7e-7 px); the reference pipeline against the ground truth 2.9e-7 m (the device's 6.1e-7 m)"""
import ctypes as C

import numpy as np
import pytest
import torch

import keypoint_vote_ref as R
import pose_pnp_ref as RP
from stillleben_amd import _abi
from stillleben_amd import keypoint_vote as kv
from test_gpu_object_keypoints import Guarded, bits, stream, to_dev
from test_host_keypoint_vote import NAMES, SIZE, assert_none, exact_vectors, make_sets

pytestmark = pytest.mark.gpu

F = np.float32
UV_BOUND = 4 * 3.1e-7        # px; 4 x the measured worst 3.1e-7 of the reference against the projected keypoints (the module docstring)
ADD_BOUND = 4 * 2.9e-7       # m; 4 x the measured worst 2.9e-7 of the reference pipeline against the ground truth
DTYPES = dict(uv=F, n_inliers=np.int32, best=np.int32, flags=np.int32, mean=F, cov=F, inliers=np.uint32)
WIDTH = dict(uv=2, n_inliers=1, best=1, flags=1, mean=2, cov=3)


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def plant(pixel, vec, m, what):
    """set m rebuilt so that every keypoint of it ends as `what`; voters not used get a zero vector and do not count"""
    K = pixel.shape[1]
    vec[m] = 0.0
    if what == "insufficient":                      # one valid voter
        vec[m, 0] = F([0.6, 0.8])
    elif what == "void":                            # every pair parallel: no hypothesis, NO_MODEL
        vec[m] = F([0.6, -0.8])
    elif what == "stopped":
        # 40 voters of one row looking along it, and 20 voters below the row looking away from it: the only meeting points lie
        # on the row, behind the voter below, so the inliers are the row's voters, their normals are all (0, 1) and the 2 x 2
        # is singular
        assert K >= 60
        pixel[m, :40, 0], pixel[m, :40, 1] = np.arange(40), 7
        vec[m, :40] = F([1.0, 0.0])
        pixel[m, 40:60, 0], pixel[m, 40:60, 1] = 100 + np.arange(20), 20
        vec[m, 40:60] = F([0.0, 1.0])
    elif what == "rejected":
        # a row and a column of voters that meet exactly at the centre of pixel (10, 7), the voter AT that centre looking
        # elsewhere (an inlier of the meeting point by n2 == 0 alone, and of no point beside it on the row or the column), and
        # two voters that look past the centre by a little: they pull the fit off the centre, where the voter at the centre is
        # lost, so the refined position holds one inlier fewer
        own = np.array([[2, 7], [5, 7], [14, 7], [30, 7], [10, 0], [10, 3], [10, 20], [10, 7], [30, 20], [25, 1]], np.int16)
        pixel[m, :10] = own
        v = exact_vectors(own, (10.5, 7.5))
        v[7] = (0.6, 0.8)
        v[8] = exact_vectors(own[8:9], (10.5, 7.0))[0]
        v[9] = exact_vectors(own[9:10], (10.0, 7.5))[0]
        vec[m, :10] = v[:, None]
    return what


def make_batch(M, K, Kp, seed):
    """M sets: half a degree of noise, 30 % of the vectors replaced, a sprinkle of voters that do not count; with M = 37 sets 3,
    5, 7 and 9 are planted (insufficient, all hypotheses void, refinement stopped, refinement rejected)"""
    rng = np.random.default_rng(seed)
    pixel, vec, _, _ = make_sets(M, K, Kp, 0.3 if K >= 16 else 0.0, seed)
    if K >= 16:
        for m in range(M):
            j = rng.permutation(K)[:max(1, K // 20)]
            vec[m, j[0::4]] = 0.0
            vec[m, j[1::4], :, 0] = np.nan
            vec[m, j[2::4], rng.integers(0, Kp)] = np.inf
            pixel[m, j[3::4], 0] = -1 - pixel[m, j[3::4], 0]
    planted = {}
    if M == 37:
        for m, what in ((3, "insufficient"), (5, "void"), (7, "stopped"), (9, "rejected")):
            planted[m] = plant(pixel, vec, m, what)
    return pixel, vec, planted


def dense_of(pixel, vec, n_scenes, seed):
    """a dense field [n_scenes, H, W, Kp, 2] of noise that holds vec at the sets' pixels (sets that share a scene may overwrite
    one another: the field is what both sides read), and the scene of every set; with more than 11 sets set 11 names a scene
    outside the field"""
    rng = np.random.default_rng(seed)
    M, K, Kp = vec.shape[:3]
    field = rng.normal(size=(n_scenes, SIZE[1], SIZE[0], Kp, 2)).astype(F)
    scene = (np.arange(M) % n_scenes).astype(np.int32)
    for m in range(M):
        ok = (pixel[m, :, 0] >= 0) & (pixel[m, :, 0] < SIZE[0]) & (pixel[m, :, 1] >= 0) & (pixel[m, :, 1] < SIZE[1])
        field[scene[m], pixel[m, ok, 1], pixel[m, ok, 0]] = vec[m, ok]
    if M > 11:
        scene[11] = n_scenes
    return field, scene


def run_device(dev, pixel, vec, scene=None, mask=127, null=None, misalign=None, n_field=None, **kw):
    """vec: gathered [M, K, Kp, 2], or with `scene` a dense field [B, H, W, Kp, 2]"""
    M, K = pixel.shape[:2]
    Kp = vec.shape[3] if scene is not None else vec.shape[2]
    d = {"pixel": to_dev(pixel, dev), "vectors": to_dev(vec, dev), "scene": None if scene is None else to_dev(scene, dev)}
    ptr = {k: (None if t is None or null == k else t.data_ptr() + ((4 if k == "vectors" else 2) if misalign == k else 0)) for k, t in d.items()}
    sizes = {k: M * Kp * w * 4 for k, w in WIDTH.items()}
    sizes["inliers"] = M * Kp * kv.n_words(K) * 4
    outs = {k: Guarded(sizes[k], dev) for k in NAMES}
    o = _abi.KeypointVoteOut(*(None if null == k else outs[k].ptr().value + (2 if misalign == k else 0) for k in NAMES))
    kw.setdefault("n_sets", M)
    p = kv.make_params(kw.pop("size", SIZE), kw.pop("n_sets"), kw.pop("n_points", K), kw.pop("n_keypoints", Kp), outputs=mask, **kw).reshape(1)
    if n_field is None:
        n_field = vec.shape[0] if scene is not None else 0
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_keypoint_vote(None if null == "params" else p.ctypes.data, C.c_void_p(ptr["pixel"]), C.c_void_p(ptr["vectors"]),
                                            C.c_void_p(ptr["scene"]), n_field, None if null == "record" else C.byref(o), stream(dev))
    return st, outs, d


def read(outs, M, K, Kp, mask):
    got = {}
    for i, k in enumerate(NAMES):
        if mask & (1 << i):
            shape = (M, Kp, kv.n_words(K)) if k == "inliers" else (M, Kp) + ((WIDTH[k],) if WIDTH[k] > 1 else ())
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


# M, K, Kp, Hy: every K at which the kernel takes another path (two voters, the 16-byte tail of the score, one wave, one past it,
# one past the 256 stride, several strides, the LDS limit), a single hypothesis, a partial round of hypotheses, both limits
SHAPES = [(1, 2, 1, 1), (37, 63, 9, 64), (1, 64, 1, 256), (37, 65, 32, 300), (1, 257, 9, 1024), (2, 1024, 9, 128), (1, 4096, 2, 1024)]
_batches = {}


def batch_case(M, K, Kp, Hy):
    """(inputs, the keyword arguments, the twin's result on the gathered vectors), computed once for both modes"""
    if (M, K, Kp, Hy) not in _batches:
        pixel, vec, planted = make_batch(M, K, Kp, 7 + K + Hy)
        kw = dict(n_hypotheses=Hy, inlier_cos=0.99, min_inliers=2, min_sin=1e-3, seed=(9 << 32) | K, set_id_base=100)
        _batches[(M, K, Kp, Hy)] = (pixel, vec, planted, kw, kv.vote_host(pixel, vectors=vec, size=SIZE, **kw))
    return _batches[(M, K, Kp, Hy)]


@pytest.mark.parametrize("M,K,Kp,Hy", SHAPES)
def test_device_against_host_twin_bit_for_bit_gathered(dev, M, K, Kp, Hy):
    pixel, vec, planted, kw, want = batch_case(M, K, Kp, Hy)
    st, outs, keep = run_device(dev, pixel, vec, **kw)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, M, K, Kp, 127), want, "gathered M %d K %d Kp %d Hy %d" % (M, K, Kp, Hy))
    if planted:      # the sets built to fail did, the others did not
        assert (want.flags[3] == _abi.VOTE_INSUFFICIENT).all() and (want.flags[5] == _abi.VOTE_NO_MODEL).all()
        assert (want.flags[7] == _abi.VOTE_REFINE_STOPPED).all() and (want.n_inliers[7] == 40).all()
        assert (want.flags[9] == _abi.VOTE_REFINE_REJECTED).all() and (want.n_inliers[9] == 10).all()
        assert (want.flags[[0, 1, 2, 4, 6, 8]] & 3 == 0).all() and (want.n_inliers[[0, 1, 2, 4, 6, 8]] >= 0.5 * K).all()


@pytest.mark.parametrize("M,K,Kp,Hy", SHAPES)
def test_device_against_host_twin_bit_for_bit_dense(dev, M, K, Kp, Hy):
    pixel, vec, planted, kw, _ = batch_case(M, K, Kp, Hy)
    field, scene = dense_of(pixel, vec, min(M, 4), 3 + K)
    want = kv.vote_host(pixel, field=field, scene=scene, **kw)
    st, outs, keep = run_device(dev, pixel, field, scene=scene, **kw)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, M, K, Kp, 127), want, "dense M %d K %d Kp %d Hy %d" % (M, K, Kp, Hy))
    assert want.found.any()
    if M > 11:      # the scene outside the field was not read
        assert (want.flags[11] == _abi.VOTE_INSUFFICIENT).all()


def test_edge_cases_bit_for_bit(dev):
    """the known answers of tests/test_host_keypoint_vote.py: the lattice, the voter at the keypoint, two voters, parallel vectors"""
    cases = []
    px = np.array([[39, 16], [40, 16], [39, 17], [40, 17]], np.int16)
    cases.append((px, exact_vectors(px, (40, 17)), 0))
    px = np.array([[2, 7], [5, 7], [14, 7], [30, 7], [10, 0], [10, 3], [10, 20], [10, 7]], np.int16)
    v = exact_vectors(px, (10.5, 7.5))
    v[7] = (-3.0, 0.0)
    cases.append((px, v, 0))
    px = np.array([[20, 30], [60, 35]], np.int16)
    cases.append((px, exact_vectors(px, (43.25, 71.5)), 0))
    cases.append((px, np.tile(F([0.6, 0.8]), (2, 1)), _abi.VOTE_NO_MODEL))
    for i, (pixel, vec, flag) in enumerate(cases):
        want = kv.vote_host(pixel[None], vectors=vec[None, :, None], size=SIZE, n_hypotheses=64, seed=3)
        assert want.flags[0, 0] == flag, i
        if flag:
            assert_none(want, flag)
        st, outs, keep = run_device(dev, pixel[None], vec[None, :, None], n_hypotheses=64, seed=3)
        assert st == 0
        assert_same(read(outs, 1, pixel.shape[0], 1, 127), want, "edge case %d" % i)


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 64, 1 | 64, 2 | 16 | 32, 4 | 8])
def test_outputs_not_named_stay_poison(dev, mask):
    pixel, vec, planted = make_batch(37, 65, 2, 3)      # the planted sets take the paths that write no position
    kw = dict(n_hypotheses=32, seed=5)
    st, outs, keep = run_device(dev, pixel, vec, mask=mask, **kw)
    assert st == 0
    assert_same(read(outs, 37, 65, 2, mask), kv.vote_host(pixel, vectors=vec, size=SIZE, **kw), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev):
    pixel, vec, _ = make_batch(2, 16, 3, 4)
    field, scene = dense_of(pixel, vec, 2, 4)
    for kw in (dict(null="params"), dict(null="pixel"), dict(null="vectors"), dict(null="record"), dict(null="uv"), dict(null="cov"),
               dict(null="inliers"), dict(misalign="pixel"), dict(misalign="vectors"), dict(misalign="scene"), dict(misalign="mean"),
               dict(n_field=0), dict(size=(0, 120)), dict(size=(160, 40000)), dict(n_points=1), dict(n_points=4097), dict(n_keypoints=0),
               dict(n_keypoints=33), dict(n_hypotheses=0), dict(n_hypotheses=1025), dict(inlier_cos=1.0), dict(inlier_cos=0.0),
               dict(min_inliers=1), dict(min_sin=-1.0), dict(mask=0), dict(mask=128)):
        st, outs, keep = run_device(dev, pixel, field, scene=scene, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, keep = run_device(dev, pixel, field, scene=scene, n_sets=0)      # no sets: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())
    assert run_device(dev, pixel, vec, n_field=0)[0] == 0                      # gathered vectors need no field


def test_step_timer(dev):
    pixel, vec, _ = make_batch(2, 64, 3, 5)
    field, scene = dense_of(pixel, vec, 2, 5)
    L = _abi.lib()
    ms = (C.c_float * 2)()
    try:
        assert L.slhip_keypoint_vote_timing_enable(1) == 0
        assert run_device(dev, pixel, vec, mask=0)[0] < 0                      # a refused call records no event
        assert L.slhip_keypoint_vote_timings(C.byref(ms)) == 0 and list(ms) == [-1.0, -1.0]
        assert run_device(dev, pixel, vec)[0] == 0                             # gathered vectors time step 0 alone
        assert L.slhip_keypoint_vote_timings(C.byref(ms)) == 0 and ms[0] > 0.0 and ms[1] == -1.0
        assert run_device(dev, pixel, field, scene=scene)[0] == 0
        assert L.slhip_keypoint_vote_timings(C.byref(ms)) == 0
        assert np.isfinite(ms[0]) and ms[0] > 0.0 and np.isfinite(ms[1]) and ms[1] > 0.0
        assert L.slhip_keypoint_vote_timings(None) < 0
    finally:
        L.slhip_keypoint_vote_timing_enable(0)


# ---- end to end on a placed batch ------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 4, 4, (160, 120), (266.7, 266.85, 78.25, 60.3)
VOTE_KW = dict(n_hypotheses=64, inlier_cos=0.99, min_inliers=2, min_sin=1e-3)
PNP_KW = dict(n_hypotheses=64, threshold_px=1.0, refine_iters=4)


@pytest.fixture(scope="module")
def placed(sl):
    from test_gpu_synth import small_table

    table = small_table(sl)
    batch = sl.SceneBatch(table, N_SCENES, N_OBJ, resolution=RES, seed=(77 << 32) | 5, render_chunk=N_SCENES, manual_exposure=1.0,
                          scene_id_base=1000)
    batch.set_camera_intrinsics(*INTRINSICS)
    batch.stage()
    batch.settle(frames=5)
    batch.place(object_to_camera=True)
    bufs = batch.render(0, object_masks=True)
    points = batch.points(bufs, n_points=256, min_px=120, outputs=("pixel", "coord"))
    kbank = sl.object_keypoints.bank(table, n_fps=8)      # the centre and 8 FPS points
    kps = batch.keypoints(bufs, bank=kbank)
    field = kps.field(bufs.instance, "unit")
    mbank = sl.pose_error.bank(table, n_points=64)
    torch.cuda.synchronize()
    return sl, batch, points, kbank, kps, field, mbank


def key_of(batch):
    key = _abi.view_key(int(batch.params["seed_lo"]), int(batch.params["seed_hi"]), batch.view)
    return key[0] | (key[1] << 32)


def reference_votes(batch, points, field):
    """the float64 reference on every (set, keypoint): a list of lists of Results"""
    pixel = points.pixel.cpu().numpy()
    vec = R.gather(field.cpu().numpy(), points.scene.cpu().numpy(), pixel)
    return R.solve_sets(pixel, vec, RES, seed=key_of(batch), set_id_base=int(batch.params["scene_id_base"]), **VOTE_KW)


def add_of(pose, gt, pts):
    """ADD in float64 of one pose against the ground truth over bank points [n, 3]"""
    d = pts @ (np.asarray(pose, np.float64)[:, :3] - gt[:, :3]).T + (np.asarray(pose, np.float64)[:, 3] - gt[:, 3])
    return float(np.linalg.norm(d, axis=1).mean())


def truth_of(points, kps):
    """(uv float64 [n, Kp, 2], in front bool [n, Kp]) of every set's object"""
    scene, slot = points.scene.long(), (points.slot - 1).long()
    return kps.uv[scene, slot].cpu().numpy().astype(np.float64), kps.in_front[scene, slot].cpu().numpy()


def test_votes_on_the_target_field_land_on_the_keypoints(placed):
    sl, batch, points, kbank, kps, field, mbank = placed
    n, Kp = len(points), len(kbank)
    assert n >= 4 and Kp == 9, "the fixture shows too few objects: %d" % n
    votes = batch.keypoint_votes(points, field, **VOTE_KW)
    torch.cuda.synchronize()
    truth, front = truth_of(points, kps)
    assert front.all() and bool(votes.found.all()) and bool((votes.flags == 0).all())
    ref = reference_votes(batch, points, field)
    ref_uv = np.array([[r.uv for r in row] for row in ref])
    assert all(r.flags == 0 for row in ref for r in row)
    d_ref = np.linalg.norm(ref_uv - truth, axis=-1)[front]
    d_dev = np.linalg.norm(votes.uv.cpu().numpy().astype(np.float64) - truth, axis=-1)[front]
    print("keypoint_vote end to end: %d sets x %d keypoints, worst distance from the projected keypoints %.3g px, the float64 "
          "reference's %.3g px" % (n, Kp, d_dev.max(), d_ref.max()))
    assert d_ref.max() * 4 <= UV_BOUND * 1.01      # the constant is 4 x what is measured
    assert d_dev.max() <= UV_BOUND
    # the same through the module's own entry on gathered vectors
    vec = torch.from_numpy(R.gather(field.cpu().numpy(), points.scene.cpu().numpy(), points.pixel.cpu().numpy())).to(field.device)
    again = kv.vote(points, vectors=vec, size=RES, seed=tuple(int(v) for v in _abi.view_key(int(batch.params["seed_lo"]), int(batch.params["seed_hi"]), batch.view)),
                    set_id_base=int(batch.params["scene_id_base"]), **VOTE_KW)
    assert torch.equal(again.uv, votes.uv) and torch.equal(again.inliers, votes.inliers)
    with pytest.raises(TypeError):
        batch.keypoint_votes(points, field, seed=3)

    # votes -> correspondences -> pose -> ADD
    uv, xyz = votes.correspondences(kbank)
    assert tuple(uv.shape) == (n, Kp, 2) and tuple(xyz.shape) == (n, Kp, 4) and bool((xyz[..., 3] == 1).all())
    key = _abi.view_key(int(batch.params["seed_lo"]), int(batch.params["seed_hi"]), batch.view)
    base = int(batch.params["scene_id_base"])
    res = sl.pose_pnp.solve(uv.contiguous(), xyz, intrinsics=batch.intrinsics(), seed=tuple(int(v) for v in key), set_id_base=base, **PNP_KW)
    err = batch.pose_errors(res.dense(N_SCENES, N_OBJ, points.scene_global, points.slot), mbank, outputs=("add",))
    torch.cuda.synchronize()
    scene, slot = points.scene_global.long().cpu(), points.slot.long().cpu()
    add = err.add.cpu()[scene, slot - 1].numpy()
    assert int(torch.isfinite(err.add).sum()) == n and bool((res.flags == 0).all()) and bool((res.n_inliers == Kp).all())
    gt = points.object_to_camera.cpu().numpy().astype(np.float64)
    cls = err.classes.cpu()[scene, slot - 1].numpy()
    assert np.array_equal(cls, votes.classes.cpu().numpy())
    ref_add = []
    for i in range(n):
        r = RP.solve(ref_uv[i], xyz[i].cpu().numpy(), batch.intrinsics(), seed=key_of(batch), set_id=base + i, **PNP_KW)
        assert r.n_inliers == Kp and r.flags == 0
        c = int(cls[i])
        pts = mbank.points[c, :int(mbank.count[c]), :3].cpu().numpy().astype(np.float64)
        ref_add.append(add_of(r.pose, gt[i], pts))
    print("keypoint_vote -> pose_pnp: worst ADD %.3g m, the reference pipeline's %.3g m" % (add.max(), max(ref_add)))
    assert max(ref_add) * 4 <= ADD_BOUND * 1.01      # the constant is 4 x what is measured
    assert add.max() <= ADD_BOUND


def damage(points, field, share=0.3, seed=5, clear_deg=15.0):
    """(a copy of the field with the vectors at `share` of every set's pixels, for every keypoint, replaced by uniform
    directions; touched bool [n, K]: the voter reads a replaced vector).  A replacement within `clear_deg` of the vector it
    replaces is drawn again (up to 8 times): it would be no outlier, only a second opinion inside the 8.1 degree cone."""
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    pixel, scene = points.pixel.cpu().long(), points.scene.cpu().long()
    n, K = pixel.shape[:2]
    out = field.cpu().clone()
    Kp = out.shape[3]
    hit = torch.zeros(out.shape[:3], dtype=torch.bool)
    for i in range(n):
        j = torch.randperm(K, generator=g)[:int(share * K)]
        hit[scene[i], pixel[i, j, 1], pixel[i, j, 0]] = True
    old = out[hit]                                                      # [h, Kp, 2]
    new = old.clone()
    todo = torch.ones(old.shape[:2], dtype=torch.bool)
    for _ in range(8):
        ang = torch.rand(old.shape[:2], generator=g) * (2.0 * np.pi)
        cand = torch.stack([torch.cos(ang), torch.sin(ang)], -1)
        new = torch.where(todo[..., None], cand, new)
        todo = todo & ((new * old).sum(-1) > float(np.cos(np.deg2rad(clear_deg))))
    assert not bool(todo.any())
    out[hit] = new
    touched = hit[scene[:, None], pixel[..., 1], pixel[..., 0]]
    return out.to(field.device), touched.numpy()


def test_damaged_field(placed):
    """30 % of every object's vectors replaced by other directions: the positions stay, the inliers are the untouched voters"""
    sl, batch, points, kbank, kps, field, mbank = placed
    bad, touched = damage(points, field)
    votes = batch.keypoint_votes(points, bad, **VOTE_KW)
    torch.cuda.synchronize()
    truth, front = truth_of(points, kps)
    ref = reference_votes(batch, points, bad)
    mask = votes.inlier_mask().cpu().numpy()
    for i, row in enumerate(ref):
        for k, r in enumerate(row):
            other = mask[i, k] & touched[i]      # an overwritten voter that is an inlier all the same
            assert not (other & ~r.inliers).any(), "set %d keypoint %d: %d overwritten voters are inliers against the reference" % (
                i, k, int((other & ~r.inliers).sum()))
    d = np.linalg.norm(votes.uv.cpu().numpy().astype(np.float64) - truth, axis=-1)[front]
    d_ref = np.linalg.norm(np.array([[r.uv for r in row] for row in ref]) - truth, axis=-1)[front]
    print("keypoint_vote with 30 %% overwritten: worst distance %.3g px, the float64 reference's %.3g px, %d of %d overwritten voters inliers" % (
        d.max(), d_ref.max(), int((mask & touched[:, None]).sum()), int(touched.sum()) * mask.shape[1]))
    assert bool(votes.found.all()) and d.max() <= UV_BOUND


def test_cpu_tensors_are_refused(placed):
    sl, batch, points, kbank, kps, field, mbank = placed
    with pytest.raises(_abi.SlhipError) as e:
        kv.vote(points.pixel.cpu(), field=field.cpu(), scene=points.scene.cpu())
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        kv.vote(points, field=field.cpu())
    with pytest.raises(_abi.SlhipError):
        batch.keypoint_votes(points.map(lambda t: t.cpu()), field)
