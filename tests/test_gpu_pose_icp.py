"""ICP on the device (slhip_pose_icp, sl.pose_icp, SceneBatch.pose_icp) against the library's host twin of the same rules
(slhip_pose_icp_host), bit for bit on every output -- floats as their int32 views, `nearest` included --, and end to end on a
placed batch.  Every output lies between 256 poisoned guard bytes that must stay poison, an output that `outputs` does not name
stays poison throughout, and every run is on a stream that is not the default one.

End to end (a): the bank of every set is its own rendered object coordinates (classes = arange(n)), the initial pose is the
batch's object_to_camera turned by the ladder step that tests/test_host_pose_icp.py chose (LADDER_STEP, 1 degree: the largest
from which the float64 loop ends, for every set, at the float64 SVD fit of the set's true correspondences -- asserted here, with
the whole ladder printed; rendered coordinates repeat, so the poses are compared and not the indices) and shifted with it.  The bound is computed in the test, never from the code under test: the larger of four times the worst pose_difference
from object_to_camera that the float64 loop of tests/pose_icp_ref.py shows on the same downloaded float32 data, and the float32
floor of that data (test_host_pose_icp.float32_floor: sqrt(12) eps m / r).  (b): the class bank is surface_points(..., 2048); the
device must equal solve_host on the downloaded inputs bit for bit, and the median ADD before and after is printed, not asserted
-- no earlier measurement exists to set a bar.  Every figure is printed on every run."""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_fit_ref as RF
import pose_icp_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_icp as pi
from test_gpu_keypoint_vote3d import N_OBJ, N_SCENES, placed3d, pose_difference  # noqa: F401  (placed3d: a fixture)
from test_gpu_object_keypoints import Guarded, bits, to_dev
from test_host_pose_icp import CLOUD_STEP, LADDER, LADDER_STEP, NAMES, float32_floor, make_case

pytestmark = pytest.mark.gpu

F = np.float32
DTYPES = dict(pose=F, n_pairs=np.int32, rms=F, iters=np.int32, flags=np.int32, nearest=np.int32)


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


@pytest.fixture(scope="module")
def side(dev):
    """a stream that is not the default one"""
    return torch.cuda.Stream(device=dev)


def width(k, K):
    return dict(pose=12, n_pairs=1, rms=1, iters=1, flags=1, nearest=K)[k]


def make_batch(M, K, count, seed):
    """M sets on a bank of 3 classes (class 1 holds `count` points, padded rows poisoned, test_host_pose_icp.make_case): initial
    poses turned by 0.5 to 8 degrees so that the sets stop after different numbers of fits, every seventh set starved of pairs by
    w = 0, every eleventh of class 0 (its own short row), sets 5 and 9 -- where there are that many -- of a class outside the bank
    and with a NaN initial pose; a sprinkle of camera points that do not count"""
    camera, init, classes, points, cnt, truth, picks = make_case(K, count, seed, A=3)
    rng = np.random.default_rng(seed)
    cam, ini, cls = np.repeat(camera, M, 0), np.repeat(init, M, 0), np.repeat(classes, M)
    for m in range(M):
        ini[m] = R.perturbed(truth[:, :3], truth[:, 3], 0.5 * (1 + m % 16), seed + m).astype(F)
        if K >= 9:
            j = rng.permutation(K)[:max(3, K // 16)]
            cam[m, j[0::3], 3], cam[m, j[1::3], 1], cam[m, j[2::3], 2] = 0.0, np.nan, np.inf
        if m % 7 == 6:
            cam[m, 2:, 3] = 0.0
        if m % 11 == 10:
            cls[m] = 0
    if M > 5:
        cls[5] = 3
    if M > 9:
        ini[9, 0, 1] = np.nan
    return cam, ini, cls, points, cnt


def run_device(dev, side, cam, ini, cls, points, cnt, mask=63, null=None, misalign=None, bank=None, **kw):
    M, K = cam.shape[:2]
    d = {"camera": to_dev(cam, dev), "init": to_dev(ini, dev), "classes": to_dev(cls, dev), "points": to_dev(points, dev),
         "count": to_dev(cnt, dev)}
    odd = {"camera": 4, "init": 4, "points": 4, "classes": 2, "count": 2}
    ptr = {k: (None if null == k else t.data_ptr() + (odd[k] if misalign == k else 0)) for k, t in d.items()}
    outs = {k: Guarded(M * width(k, K) * 4, dev) for k in NAMES}
    o = _abi.PoseIcpOut(*(None if null == k else outs[k].ptr().value + (2 if misalign == k else 0) for k in NAMES))
    b = dict(n_assets=points.shape[0], n_points=points.shape[1])
    b.update(bank or {})
    brec = _abi.PoseBank(ptr["points"], ptr["count"], None, None, b["n_assets"], b["n_points"], 1, 0)
    kw.setdefault("min_pairs", 3)
    kw.setdefault("max_iters", 12)
    fields = {k: kw.pop(k) for k in ("n_sets", "n_points") if k in kw}
    p = pi.make_params(M, K, outputs=mask, **kw).reshape(1)
    for k, v in fields.items():
        p[k] = v
    torch.cuda.synchronize()
    with torch.cuda.device(dev), torch.cuda.stream(side):
        st = _abi.lib().slhip_pose_icp(None if null == "params" else p.ctypes.data, C.c_void_p(ptr["camera"]), C.c_void_p(ptr["init"]),
                                       C.c_void_p(ptr["classes"]), None if null == "bank" else C.byref(brec),
                                       None if null == "record" else C.byref(o), C.c_void_p(side.cuda_stream))
    side.synchronize()
    return st, outs, d


def read(outs, M, K, mask):
    got = {}
    for i, k in enumerate(NAMES):
        if mask & (1 << i):
            got[k] = outs[k].host(DTYPES[k], {"pose": (M, 3, 4), "nearest": (M, K)}.get(k, (M,))).copy()
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


def host_twin(cam, ini, cls, points, cnt, **kw):
    kw.setdefault("min_pairs", 3)
    kw.setdefault("max_iters", 12)
    return pi.solve_host(cam, ini, cls, (points, cnt), **kw)


# K: one to five camera points, either side of the 256 stride and of the tile of 1024 (one to five queries a lane); count: a
# single bank point, the fewest that fit, either side of the 16-byte read and of the 256 stride -- always less than the row
CASES = [(K, 61) for K in (1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025)] + [(70, c) for c in (1, 3, 4, 5, 255, 256, 257)]


@pytest.mark.parametrize("K,count", CASES)
def test_device_against_host_twin_bit_for_bit(dev, side, K, count):
    args = make_batch(12, K, count, 100 + K + count)
    want = host_twin(*args)
    st, outs, keep = run_device(dev, side, *args)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, 12, K, 63), want, "K %d, count %d" % (K, count))
    assert want.flags[5] == _abi.ICP_BAD_CLASS and want.flags[9] == _abi.ICP_NO_INIT and (want.nearest < max(count, 7)).all()
    if K >= 255:
        assert want.flags[6] == _abi.ICP_INSUFFICIENT and want.found[[0, 1, 2, 3, 4, 7, 8]].all()


def test_one_set(dev, side):
    args = make_batch(1, 300, 200, 7)
    want = host_twin(*args)
    st, outs, keep = run_device(dev, side, *args)
    assert st == 0 and want.found[0]
    assert_same(read(outs, 1, 300, 63), want, "M 1")


def test_three_hundred_sets_that_stop_after_different_iterations(dev, side):
    args = make_batch(300, 130, 120, 8)
    kw = dict(max_iters=30, max_dist=0.05, dist_scale=0.8, min_dist=0.004)
    want = host_twin(*args, **kw)
    st, outs, keep = run_device(dev, side, *args, **kw)
    assert st == 0
    assert_same(read(outs, 300, 130, 63), want, "M 300")
    found = want.found
    stops = np.unique(want.iters[found])
    print("300 sets: %d found, %d converged, iters of the found from %d to %d (%d different), flags %r" % (
        found.sum(), want.converged.sum(), stops.min(), stops.max(), len(stops), np.unique(want.flags).tolist()))
    assert len(stops) >= 3 and set(np.unique(want.flags)) >= {0 | _abi.ICP_CONVERGED, _abi.ICP_BAD_CLASS, _abi.ICP_NO_INIT, _abi.ICP_INSUFFICIENT}


def test_the_largest_bank_and_point_set(dev, side):
    """4096 x 4096: the whole LDS budget (48 KiB + 16 KiB), past what a kernel may ask for without the attribute"""
    args = make_batch(2, 4096, 4000, 9)
    assert args[3].shape[1] < 4096
    points = np.concatenate([args[3], np.zeros((3, 4096 - args[3].shape[1], 4), F)], 1)
    points[..., 3] = 1.0
    args = args[:3] + (points, args[4])
    want = host_twin(*args, max_iters=3)
    st, outs, keep = run_device(dev, side, *args, max_iters=3)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, 2, 4096, 63), want, "4096 x 4096")
    assert want.found.all() and (want.nearest < 4000).all()


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 1 | 16, 2 | 4 | 8, 32 | 1, 63 - 4])
def test_outputs_not_named_stay_poison(dev, side, mask):
    args = make_batch(12, 70, 61, 3)      # sets 5, 6 and 9 take the paths that write no pose
    st, outs, keep = run_device(dev, side, *args, mask=mask)
    assert st == 0
    assert_same(read(outs, 12, 70, mask), host_twin(*args), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev, side):
    args = make_batch(3, 16, 12, 4)
    refusals = [dict(null=k) for k in ("params", "camera", "init", "classes", "bank", "points", "count", "record") + NAMES]
    refusals += [dict(misalign=k) for k in ("camera", "init", "classes", "points", "count") + NAMES]
    refusals += [dict(n_points=0), dict(n_points=4097), dict(max_iters=0), dict(max_iters=65), dict(min_pairs=2), dict(dist_scale=0.0),
                 dict(dist_scale=1.5), dict(max_dist=-1.0), dict(max_dist=np.nan), dict(min_dist=-1.0), dict(min_dist=np.nan),
                 dict(tol_rot=-1.0), dict(tol_rot=np.nan), dict(tol_trans=-1.0), dict(tol_trans=np.nan), dict(min_gap=-1.0),
                 dict(min_gap=1.0), dict(mask=0), dict(mask=64), dict(bank=dict(n_assets=0)), dict(bank=dict(n_points=0)),
                 dict(bank=dict(n_points=4097))]
    for kw in refusals:
        st, outs, keep = run_device(dev, side, *args, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, keep = run_device(dev, side, *args, n_sets=0)      # no sets: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())


def test_step_timer(dev, side):
    args = make_batch(3, 64, 61, 5)
    L = _abi.lib()
    ms = (C.c_float * 1)()
    try:
        assert L.slhip_pose_icp_timing_enable(1) == 0
        assert run_device(dev, side, *args, mask=0)[0] < 0                        # a refused call records no event
        assert L.slhip_pose_icp_timings(C.byref(ms)) == 0 and list(ms) == [-1.0]
        assert run_device(dev, side, *args)[0] == 0
        assert L.slhip_pose_icp_timings(C.byref(ms)) == 0 and np.isfinite(ms[0]) and ms[0] >= 0.0
        assert L.slhip_pose_icp_timings(None) < 0
    finally:
        L.slhip_pose_icp_timing_enable(0)


# ---- end to end on a placed batch ------------------------------------------------------------------------------------------------
def perturbed_truth(gt, degrees):
    return np.stack([R.perturbed(g[:, :3], g[:, 3], degrees, 50 + i) for i, g in enumerate(np.asarray(gt, np.float64))]).astype(F)


def test_own_coordinates_as_the_bank_recover_the_pose(placed3d, side):  # noqa: F811
    sl, batch, points, kbank, kps, off, mbank = placed3d
    n, K = len(points), int(points.camera.shape[1])
    gt = points.object_to_camera.cpu().numpy()
    coord, camera, valid = points.coord.cpu().numpy(), points.camera.cpu().numpy(), points.valid.cpu().numpy()
    init = perturbed_truth(gt, LADDER_STEP)
    count = np.full(n, K, np.int32)
    bank = sl.pose_error.bank(None, points=points.coord, count=torch.from_numpy(count).to(points.coord.device))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        icp = pi.solve(points.camera, torch.from_numpy(init).to(points.camera.device), torch.arange(n, dtype=torch.int32, device=points.camera.device),
                       bank, max_iters=40)
    side.synchronize()
    exact = np.stack([RF.fit_svd(coord[i], camera[i])[0] for i in range(n)])      # the fit of the true correspondences
    recovered = {}
    for step in LADDER:      # the ladder on this data: from which steps the float64 loop ends at that fit
        rs = R.solve_svd(camera, perturbed_truth(gt, step), np.arange(n), coord, count, max_iters=40)
        recovered[step] = int(sum(r.flags in (0, R.CONVERGED) and pose_difference(r.pose[None], exact[i:i + 1])[0] <= 1e-12 for i, r in enumerate(rs)))
        print("ladder step %2d degrees: the float64 loop recovers %d of %d sets and ends %.3g from object_to_camera at the worst" % (
            step, recovered[step], n, np.nanmax(pose_difference(np.stack([r.pose for r in rs]), gt))))
        if step == LADDER_STEP:
            refs = rs
    assert recovered[LADDER_STEP] == n and all(recovered[s] < n for s in LADDER if s > LADDER_STEP)      # the step is the largest
    p_ref = pose_difference(np.stack([r.pose for r in refs]), gt)
    p_dev = pose_difference(icp.pose.cpu().numpy(), gt)
    floor = max(float32_floor(camera[i], coord[i][valid[i], :3]) for i in range(n))
    bound = max(4.0 * p_ref.max(), floor)
    print("pose_icp on the sets' own coordinates from %d degrees: %d sets, worst difference from object_to_camera %.3g, the float64 "
          "loop's %.3g, float32 floor %.3g, bound %.3g; iters %d to %d, worst rms %.3g m" % (
              LADDER_STEP, n, p_dev.max(), p_ref.max(), floor, bound, int(icp.iters.min()), int(icp.iters.max()), float(icp.rms.max())))
    assert bool(icp.found.all()) and np.array_equal(icp.n_pairs.cpu().numpy(), valid.sum(1))
    assert p_dev.max() <= bound


def test_surface_bank_through_the_batch(placed3d, side):  # noqa: F811
    sl, batch, points, kbank, kps, off, mbank = placed3d
    n = len(points)
    table = batch.table
    pts, cnt = pi.surface_points(sl.pose_vsd.surface(table), 2048)
    bank = sl.pose_error.bank(table, points=pts, count=cnt)
    gt = points.object_to_camera.cpu().numpy()
    init = torch.from_numpy(perturbed_truth(gt, CLOUD_STEP)).to(points.camera.device)      # (the issue leaves this turn open: 10 degrees)
    kw = dict(max_iters=30, max_dist=0.05, dist_scale=0.7, min_dist=0.005)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        icp = batch.pose_icp(points, init, bank, **kw)
        dense_init = pi.PoseICP(pose=init).dense(N_SCENES, N_OBJ, points.scene_global, points.slot)
        again = batch.pose_icp(points, dense_init, bank, **kw)      # [B, O, 3, 4], gathered by scene_global and slot
    side.synchronize()
    objects = batch.host_objects()["asset"].reshape(N_SCENES, N_OBJ)
    classes = objects[points.scene_global.cpu().numpy(), points.slot.cpu().numpy() - 1].astype(np.int32)
    want = pi.solve_host(points.camera.cpu().numpy(), init.cpu().numpy(), classes, (pts.cpu().numpy(), cnt.cpu().numpy()), **kw)
    got = {k: getattr(icp, k).cpu().numpy() for k in NAMES}
    assert_same(got, want, "surface bank")
    assert_same({k: getattr(again, k).cpu().numpy() for k in NAMES}, want, "dense init")

    found = icp.found.cpu().numpy()
    scene, slot = points.scene_global.long().cpu(), points.slot.long().cpu()
    adds = []
    for poses in (dense_init, icp.dense(N_SCENES, N_OBJ, points.scene_global, points.slot)):
        err = batch.pose_errors(poses, mbank, outputs=("add",))
        torch.cuda.synchronize()
        adds.append(err.add.cpu()[scene, slot - 1].numpy())
    assert int(torch.isfinite(err.add).sum()) == int(found.sum()) and np.array_equal(np.isfinite(adds[1]), found)      # (err: the refined poses')
    print("pose_icp on surface_points(2048) from %d degrees: %d of %d sets found, %d converged, iters %d to %d; median ADD before %.3g m, "
          "after %.3g m" % (CLOUD_STEP, found.sum(), n, int(icp.converged.sum()), int(icp.iters.min()), int(icp.iters.max()),
                            float(np.median(adds[0])), float(np.median(adds[1][found])) if found.any() else float("nan")))
    with pytest.raises(TypeError):
        batch.pose_icp(points, init, bank, classes=torch.zeros(n, dtype=torch.int32))
    with pytest.raises(TypeError):
        batch.pose_icp(points, None, bank)


def test_cpu_tensors_are_refused(placed3d):  # noqa: F811
    sl, batch, points, kbank, kps, off, mbank = placed3d
    n = len(points)
    init = points.object_to_camera.contiguous()
    cls = torch.zeros(n, dtype=torch.int32, device=init.device)
    with pytest.raises(_abi.SlhipError) as e:
        pi.solve(points.camera.cpu(), init, cls, mbank)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        pi.solve(points.camera, init.cpu(), cls, mbank)
    with pytest.raises(_abi.SlhipError):
        batch.pose_icp(points, init.cpu(), mbank)
