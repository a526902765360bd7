"""Pose PnP on the device (slhip_pose_pnp, sl.pose_pnp, SceneBatch.pose_pnp) against the library's host twin of the same rules
(slhip_pose_pnp_host), bit for bit on every output -- floats as their int32 views -- and end to end on a placed batch against
the float64 implementation tests/pose_pnp_ref.py.  Every output lies between 256 poisoned guard bytes that must stay poison, and
an output that `outputs` does not name stays poison throughout.

The end-to-end bounds, both by the 4 x rule of tests/test_host_pose_pnp.py and both printed on every run.  ADD_BOUND is four times
the worst ADD, against the batch's ground truth, of the float64 reference's poses on the 16 point sets of the `placed` fixture:
that error is the data's (the rendered coordinates of a pixel against its centre), not a solver's.  TWIN_BOUND is four times the
worst ADD between the device's pose and the reference's on the same sets.
    measured worst: the reference against the ground truth 8.2e-5 m (the device 8.2e-5 m); the device against the reference 1.0e-6 m"""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_pnp_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_pnp as pnp
from test_gpu_object_keypoints import Guarded, bits, stream, to_dev
from test_host_pose_pnp import K4, NAMES, assert_none, make_set

pytestmark = pytest.mark.gpu

F = np.float32
ADD_BOUND = 4 * 8.2e-5       # m; 4 x the measured worst 8.2e-5 of the reference against the ground truth (the module docstring)
TWIN_BOUND = 4 * 1.0e-6      # m; 4 x the measured worst 1.0e-6 of the device against the reference
DTYPES = dict(pose=F, n_inliers=np.int32, rms=F, inliers=np.uint32, best=np.int32, flags=np.int32)


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def make_batch(M, K, seed, per_set, with_init):
    """M sets of K correspondences: half a pixel of noise, 30 % outliers, a sprinkle of entries that do not count; set 3 with
    three valid correspondences, set 5 all identical, set 7 far too noisy for the threshold; initial poses near the truth
    (set 2: NaN, set 4: the truth itself)"""
    rng = np.random.default_rng(seed)
    uv, xyz = np.zeros((M, K, 2), F), np.ones((M, K, 4), F)
    k4 = np.tile(F(K4), (M, 1))
    init = np.zeros((M, 3, 4), F)
    for i in range(M):
        u, x, pose, _ = make_set(K, int(0.3 * K) if K >= 16 else 0, seed * 1000 + i)
        if per_set:
            s = F(0.5 + rng.random())
            k4[i] = (K4[0] * s, K4[1] * s, K4[2] * s + F(rng.integers(-50, 50)), K4[3] * s - F(rng.integers(-50, 50)))
            u = (R.project(pose, k4[i], make_set(K, 0, seed * 1000 + i)[1])[0]).astype(F)
        u = u + (rng.normal(size=u.shape) * (0.5 if i % 8 != 7 else 30.0)).astype(F) * (K >= 16)
        if K >= 16:
            j = rng.permutation(K)[:max(1, K // 20)]
            x[j[0::4], 3] = 0.0
            x[j[1::4], 3] = np.nan
            x[j[2::4], rng.integers(0, 3)] = np.inf
            u[j[3::4], 0] = np.nan
            if i % 8 == 3:
                x[3:, 3] = -1.0
            if i % 8 == 5:
                u[:], x[:] = u[0], x[0]
                x[:, 3] = 1.0
        uv[i], xyz[i] = u, x
        near = pose.copy()
        near[:, 3] += rng.normal(size=3) * (0.002 if i != 4 else 0.0)
        init[i] = np.nan if i == 2 else near
    return uv, xyz, (k4 if per_set else None), (init if with_init else None)


def run_device(dev, uv, xyz, k4, init, mask=63, null=None, misalign=None, **kw):
    M, K = uv.shape[:2]
    d = {"uv": to_dev(uv, dev), "xyz": to_dev(xyz, dev), "intrinsics": None if k4 is None else to_dev(k4, dev),
         "init": None if init is None else to_dev(init, dev)}
    ptr = {k: (None if t is None or null == k else t.data_ptr() + (4 if misalign == k else 0)) for k, t in d.items()}
    sizes = dict(pose=M * 48, n_inliers=M * 4, rms=M * 4, inliers=M * pnp.n_words(K) * 4, best=M * 4, flags=M * 4)
    outs = {k: Guarded(sizes[k], dev) for k in NAMES}
    o = _abi.PosePnpOut(*(None if null == k else outs[k].ptr() for k in NAMES))
    kw.setdefault("n_sets", M)
    p = pnp.make_params(K4, kw.pop("n_sets"), kw.pop("n_points", K), outputs=mask, **kw).reshape(1)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_pnp(None if null == "params" else p.ctypes.data, C.c_void_p(ptr["uv"]), C.c_void_p(ptr["xyz"]),
                                       C.c_void_p(ptr["intrinsics"]), C.c_void_p(ptr["init"]), None if null == "record" else C.byref(o),
                                       stream(dev))
    return st, outs, d


def read(outs, M, K, mask):
    got = {}
    for i, k in enumerate(NAMES):
        if mask & (1 << i):
            shape = {"pose": (M, 3, 4), "inliers": (M, pnp.n_words(K))}.get(k, (M,))
            got[k] = outs[k].host(DTYPES[k], shape).copy()
        else:
            assert outs[k].untouched(), k
    return got


def assert_same(got, want, what):
    for k, v in got.items():
        w = getattr(want, k)
        diff = bits(v).reshape(-1, 4).view(np.int32) != bits(w).reshape(-1, 4).view(np.int32)
        assert not diff.any(), "%s %s: %d of %d words differ, the first at %d: %r against %r" % (
            what, k, int(diff.sum()), diff.size, int(np.argwhere(diff.reshape(-1))[0][0]), v.reshape(-1)[np.argwhere(diff.reshape(-1))[0][0]],
            w.reshape(-1)[np.argwhere(diff.reshape(-1))[0][0]])


# M, K, Hy, refine_iters, per-set intrinsics, initial poses: every K at which the kernel takes another path (the 16-byte tail of
# the score, one wave, one past it, one past the 256 stride, the LDS limit), a partial round of hypotheses, both limits
SHAPES = [(1, 4, 64, 1, False, False), (1, 5, 1, 0, False, False), (37, 63, 64, 1, True, False), (1, 64, 256, 8, False, True),
          (37, 65, 300, 1, False, True), (1, 257, 300, 8, True, False), (37, 257, 0, 8, False, True), (1, 1024, 256, 1, False, False),
          (1, 4096, 64, 8, False, False), (1, 257, 4096, 0, False, False), (2, 4096, 4096, 1, True, True)]


@pytest.mark.parametrize("M,K,Hy,iters,per_set,with_init", SHAPES)
def test_device_against_host_twin_bit_for_bit(dev, M, K, Hy, iters, per_set, with_init):
    uv, xyz, k4, init = make_batch(M, K, 7 + K + Hy, per_set, with_init)
    kw = dict(n_hypotheses=Hy, refine_iters=iters, threshold_px=2.0, min_inliers=4, seed=(9 << 32) | K, set_id_base=100)
    want = pnp.solve_host(uv, xyz, K4, per_set_intrinsics=k4, init=init, **kw)
    st, outs, keep = run_device(dev, uv, xyz, k4, init, **kw)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, M, K, 63), want, "M %d K %d Hy %d" % (M, K, Hy))
    if M == 37 and Hy > 0:      # the sets built to fail did, the others did not
        assert want.flags[3] == _abi.PNP_INSUFFICIENT and want.flags[5] == _abi.PNP_NO_MODEL
        assert (want.n_inliers[[0, 1, 6, 8]] >= 0.5 * K).all()


def test_edge_cases_bit_for_bit(dev):
    """three valid of eight, identical correspondences, every point behind the camera, a coplanar object, a singular refinement"""
    u, x, pose, _ = make_set(8, 0, 21)
    cases = []
    x3 = x.copy()
    x3[3:, 3] = 0
    cases.append((u, x3, None, dict(n_hypotheses=16), _abi.PNP_INSUFFICIENT))
    cases.append((np.repeat(u[:1], 8, 0), np.repeat(x[:1], 8, 0), None, dict(n_hypotheses=64), _abi.PNP_NO_MODEL))
    cases.append((u, x, -pose, dict(n_hypotheses=0), _abi.PNP_NO_MODEL))
    uf, xf, pf, _ = make_set(8, 0, 25, flat=True)
    cases.append((uf, xf, None, dict(n_hypotheses=32), 0))
    us, xs, ps, _ = make_set(64, 0, 28)      # four copies of one correspondence: the normal equations are singular
    cases.append((np.repeat(us[:1], 4, 0), np.repeat(xs[:1], 4, 0), ps, dict(n_hypotheses=0, refine_iters=2), _abi.PNP_REFINE_STOPPED))
    for i, (uv, xyz, init, kw, flag) in enumerate(cases):
        init = None if init is None else init[None].astype(F)
        want = pnp.solve_host(uv[None], xyz[None], K4, init=init, **kw)
        assert want.flags[0] == flag, i
        if flag & 3:
            assert_none(want, flag)
        st, outs, keep = run_device(dev, uv[None], xyz[None], None, init, **kw)
        assert st == 0
        assert_same(read(outs, 1, uv.shape[0], 63), want, "edge case %d" % i)


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 1 | 8, 2 | 4 | 32])
def test_outputs_not_named_stay_poison(dev, mask):
    uv, xyz, k4, init = make_batch(9, 65, 3, False, False)      # set 3 and set 5 take the paths that write no pose
    kw = dict(n_hypotheses=32, refine_iters=2)
    st, outs, keep = run_device(dev, uv, xyz, k4, init, mask=mask, **kw)
    assert st == 0
    assert_same(read(outs, 9, 65, mask), pnp.solve_host(uv, xyz, K4, **kw), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev):
    uv, xyz, k4, init = make_batch(2, 16, 4, True, True)
    for kw in (dict(null="params"), dict(null="uv"), dict(null="xyz"), dict(null="record"), dict(null="pose"), dict(null="rms"),
               dict(null="inliers"), dict(misalign="uv"), dict(misalign="xyz"), dict(misalign="intrinsics"), dict(n_points=3),
               dict(n_points=4097), dict(n_hypotheses=4097), dict(threshold_px=0.0), dict(refine_iters=17), dict(min_inliers=3),
               dict(mask=0), dict(mask=64), dict(n_hypotheses=0, null="init")):
        st, outs, keep = run_device(dev, uv, xyz, k4, init, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, keep = run_device(dev, uv, xyz, k4, init, n_sets=0)      # no sets: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())


def test_step_timer(dev):
    uv, xyz, k4, init = make_batch(2, 64, 5, False, True)
    L = _abi.lib()
    ms = (C.c_float * 2)()
    try:
        assert L.slhip_pose_pnp_timing_enable(1) == 0
        assert run_device(dev, uv, xyz, k4, init, mask=0)[0] < 0                  # a refused call records no event
        assert L.slhip_pose_pnp_timings(C.byref(ms)) == 0 and list(ms) == [-1.0, -1.0]
        assert run_device(dev, uv, xyz, k4, init, n_hypotheses=0)[0] == 0        # a pure refinement times step 0 alone
        assert L.slhip_pose_pnp_timings(C.byref(ms)) == 0 and ms[0] > 0.0 and ms[1] == -1.0
        assert run_device(dev, uv, xyz, k4, init, n_hypotheses=64)[0] == 0
        assert L.slhip_pose_pnp_timings(C.byref(ms)) == 0
        assert np.isfinite(ms[0]) and ms[0] > 0.0 and np.isfinite(ms[1]) and ms[1] > 0.0
        assert L.slhip_pose_pnp_timings(None) < 0
    finally:
        L.slhip_pose_pnp_timing_enable(0)


# ---- end to end on a placed batch ------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 4, 4, (160, 120), (266.7, 266.85, 78.25, 60.3)
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
    bank = sl.pose_error.bank(table, n_points=64)
    torch.cuda.synchronize()
    return batch, points, bank


def reference(batch, points, coord, i):
    uv = points.pixel[i].cpu().numpy().astype(F) + F(0.5)
    key = _abi.view_key(int(batch.params["seed_lo"]), int(batch.params["seed_hi"]), batch.view)
    return R.solve(uv, coord[i].cpu().numpy(), batch.intrinsics(), seed=key[0] | (key[1] << 32),
                   set_id=int(batch.params["scene_id_base"]) + i, **PNP_KW)


def add_of(pose, gt, pts):
    """ADD in float64 of one pose against the ground truth over bank points [n, 3]"""
    d = pts @ (np.asarray(pose, np.float64)[:, :3] - gt[:, :3]).T + (np.asarray(pose, np.float64)[:, 3] - gt[:, 3])
    return float(np.linalg.norm(d, axis=1).mean())


def test_render_points_pose_errors(placed):
    batch, points, bank = placed
    n = len(points)
    assert n >= 4, "the fixture shows too few objects: %d" % n
    res = batch.pose_pnp(points, **PNP_KW)
    est = res.dense(N_SCENES, N_OBJ, points.scene_global, points.slot)
    err = batch.pose_errors(est, bank, outputs=("add",))
    torch.cuda.synchronize()
    scene, slot = points.scene_global.long().cpu(), points.slot.long().cpu()
    add = err.add.cpu()[scene, slot - 1].numpy()
    assert int(torch.isfinite(err.add).sum()) == n and (res.flags == 0).all() and (res.n_inliers == 256).all()
    gt = points.object_to_camera.cpu().numpy().astype(np.float64)
    cls = err.classes.cpu()[scene, slot - 1].numpy()
    ref_add, twin = [], []
    for i in range(n):
        ref = reference(batch, points, points.coord, i)
        assert ref.n_inliers == 256 and ref.flags == 0
        c = int(cls[i])
        pts = bank.points[c, :int(bank.count[c]), :3].cpu().numpy().astype(np.float64)
        ref_add.append(add_of(ref.pose, gt[i], pts))
        twin.append(add_of(res.pose[i].cpu().numpy(), ref.pose, pts))
    print("pose_pnp end to end: %d sets, worst ADD %.3g m, the float64 reference's %.3g m, between the two %.3g m" % (
        n, add.max(), max(ref_add), max(twin)))
    assert max(ref_add) * 4 <= ADD_BOUND * 1.01      # the constant is 4 x what is measured
    assert add.max() <= ADD_BOUND and max(twin) <= TWIN_BOUND
    # the same through the module's own entry, and a pure refinement from the ground truth keeps it
    again = pnp.solve(points, intrinsics=batch.intrinsics(), init=points.object_to_camera.contiguous(), n_hypotheses=0, refine_iters=2)
    assert (again.best == -1).all() and (again.n_inliers == 256).all()
    with pytest.raises(TypeError):
        batch.pose_pnp(points, seed=3)


def overwrite(points, share=0.3, seed=5, clear_px=3.0, intrinsics=INTRINSICS):
    """(coord with `share` of every set's points replaced by uniform points of the set's box, touched bool [n, K]).  A
    replacement that the ground truth still projects within `clear_px` of its pixel is drawn again (up to 8 times): it would be
    no outlier, only a second inlier that is wrong in depth."""
    n, K = points.coord.shape[:2]
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    coord = points.coord.cpu().clone()
    o2c = points.object_to_camera.cpu()
    uv = points.pixel.cpu().float() + 0.5
    touched = torch.zeros((n, K), dtype=torch.bool)
    lo, hi = coord[..., :3].amin(dim=1, keepdim=True), coord[..., :3].amax(dim=1, keepdim=True)
    for i in range(n):
        touched[i, torch.randperm(K, generator=g)[:int(share * K)]] = True
    todo = touched.clone()
    for _ in range(8):
        noise = lo + (hi - lo) * torch.rand((n, K, 3), generator=g)
        X = noise @ o2c[:, :, :3].transpose(1, 2) + o2c[:, None, :, 3]
        px = torch.stack([intrinsics[0] * X[..., 0] / X[..., 2] + intrinsics[2], intrinsics[1] * X[..., 1] / X[..., 2] + intrinsics[3]], -1)
        coord[..., :3] = torch.where(todo[..., None], noise, coord[..., :3])
        todo = todo & ((px - uv).norm(dim=-1) < clear_px)
    assert not bool(todo.any())
    return coord.to(points.coord.device), touched


def test_overwritten_coordinates(placed):
    """30 % of the coordinates replaced by other points of the object's box: the pose stays, the inliers are the untouched"""
    batch, points, bank = placed
    n, K = len(points), 256
    coord, touched = overwrite(points)
    res = batch.pose_pnp(points, coord=coord, **PNP_KW)
    err = batch.pose_errors(res.dense(N_SCENES, N_OBJ, points.scene_global, points.slot), bank, outputs=("add",))
    torch.cuda.synchronize()
    scene, slot = points.scene_global.long().cpu(), points.slot.long().cpu()
    add = err.add.cpu()[scene, slot - 1].numpy()
    mask = res.inlier_mask().cpu().numpy()
    for i in range(n):
        ref = reference(batch, points, coord, i)
        other = mask[i] == touched[i].numpy()      # an inlier that was overwritten, or an untouched correspondence left out
        assert not (other & (ref.inliers != touched[i].numpy())).any(), "set %d: %d correspondences classified against the reference" % (
            i, int((other & (ref.inliers != touched[i].numpy())).sum()))
    print("pose_pnp with 30 %% overwritten: worst ADD %.3g m" % add.max())
    assert add.max() <= ADD_BOUND


def test_cpu_tensors_are_refused(placed):
    batch, points, bank = placed
    with pytest.raises(_abi.SlhipError) as e:
        pnp.solve(points.pixel.cpu().float(), points.coord.cpu(), intrinsics=K4)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        pnp.solve(points.pixel.float().contiguous(), points.coord, intrinsics=K4, init=points.object_to_camera.cpu())
