"""The rigid fit on the device (slhip_pose_fit, sl.pose_fit, SceneBatch.pose_fit) against the library's host twin of the same
rules (slhip_pose_fit_host), bit for bit on every output -- floats as their int32 views --, and end to end on a placed batch:
the rendered object coordinates of every visible object fitted to its camera points recover the batch's object_to_camera, and
the poses go through SceneBatch.pose_errors.  Every output lies between 256 poisoned guard bytes that must stay poison, and an
output that `outputs` does not name stays poison throughout.

The end-to-end bound is computed in the test, never from the code under test: four times the worst pose_difference (the
Frobenius norm of the [3, 4] difference, tests/test_gpu_keypoint_vote3d.py) from object_to_camera that the float64 SVD of
tests/pose_fit_ref.py shows on the same float32 points.  The ADD's bound follows from it: a model point p moves by
|(P - G) (p, 1)| <= |P - G|_F sqrt(|p|^2 + 1) between the fitted pose P and the ground truth G, so the mean over the model
points is at most the pose bound times sqrt(r^2 + 1), r the largest |p| of the model bank -- the bank's diameter scale.  Every
figure is printed on every run."""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_fit_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_fit as pf
from test_gpu_keypoint_vote3d import N_OBJ, N_SCENES, placed3d, pose_difference  # noqa: F401  (placed3d: a fixture)
from test_gpu_object_keypoints import Guarded, bits, stream, to_dev
from test_host_pose_fit import NAMES, motion_case

pytestmark = pytest.mark.gpu

F = np.float32
DTYPES = dict(pose=F, n_used=np.int32, rms=F, flags=np.int32)
WIDTH = dict(pose=12, n_used=1, rms=1, flags=1)


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def make_batch(N, seed):
    """5 sets of N correspondences: rigid motions with a millimetre of noise and a sprinkle of correspondences that do not count;
    set 1 is insufficient (two count) and, from N = 3 on, set 3 is degenerate (a line)"""
    rng = np.random.default_rng(seed)
    src, dst = np.zeros((5, N, 4), F), np.zeros((5, N, 4), F)
    for m in range(5):
        src[m], dst[m], Rm, t = motion_case(N, seed * 10 + m)
        dst[m, :, :3] += rng.normal(size=(N, 3)).astype(F) * 0.001
        if N >= 9:
            j = rng.permutation(N)[:max(4, N // 16)]
            src[m, j[0::4], 3], dst[m, j[1::4], 3] = 0.0, 0.0
            src[m, j[2::4], 1], dst[m, j[3::4], 2] = np.nan, np.inf
        if m == 3 and N >= 3:
            src[m, :, :3] = np.outer(np.linspace(-0.1, 0.1, N), [0.6, 0.0, 0.8]).astype(F)
            dst[m, :, :3] = (src[m, :, :3].astype(np.float64) @ Rm.T + t).astype(F)
    src[1, 2:, 3] = 0.0
    return src, dst


def run_device(dev, src, dst, mask=15, null=None, misalign=None, **kw):
    M, N = src.shape[:2]
    d = {"src": to_dev(src, dev), "dst": to_dev(dst, dev)}
    ptr = {k: (None if null == k else t.data_ptr() + (4 if misalign == k else 0)) for k, t in d.items()}
    outs = {k: Guarded(M * WIDTH[k] * 4, dev) for k in NAMES}
    o = _abi.PoseFitOut(*(None if null == k else outs[k].ptr().value + (2 if misalign == k else 0) for k in NAMES))
    kw.setdefault("n_sets", M)
    p = pf.make_params(kw.pop("n_sets"), kw.pop("n_points", N), outputs=mask, **kw).reshape(1)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_fit(None if null == "params" else p.ctypes.data, C.c_void_p(ptr["src"]), C.c_void_p(ptr["dst"]),
                                       None if null == "record" else C.byref(o), stream(dev))
    return st, outs, d


def read(outs, M, mask):
    got = {}
    for i, k in enumerate(NAMES):
        if mask & (1 << i):
            got[k] = outs[k].host(DTYPES[k], (M, 3, 4) if k == "pose" else (M,)).copy()
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


# N: a single correspondence, the fewest that fit, the keypoints' count, just under a wave, a wave, one past it, one past the
# 256 stride, the limit
@pytest.mark.parametrize("N", [1, 3, 9, 63, 64, 65, 257, 4096])
def test_device_against_host_twin_bit_for_bit(dev, N):
    src, dst = make_batch(N, 40 + N)
    want = pf.solve_host(src, dst)
    st, outs, keep = run_device(dev, src, dst)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, 5, 15), want, "N %d" % N)
    assert want.flags[1] == _abi.FIT_INSUFFICIENT and want.n_used[1] <= 2
    if N >= 3:
        assert want.flags[3] == _abi.FIT_DEGENERATE and (want.flags[[0, 2, 4]] == 0).all() and (want.rms[[0, 2, 4]] < 0.005).all()
    else:
        assert (want.flags == _abi.FIT_INSUFFICIENT).all()


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 1 | 8, 2 | 4])
def test_outputs_not_named_stay_poison(dev, mask):
    src, dst = make_batch(65, 3)      # sets 1 and 3 take the paths that write no pose
    st, outs, keep = run_device(dev, src, dst, mask=mask)
    assert st == 0
    assert_same(read(outs, 5, mask), pf.solve_host(src, dst), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev):
    src, dst = make_batch(16, 4)
    for kw in (dict(null="params"), dict(null="src"), dict(null="dst"), dict(null="record"), dict(null="pose"), dict(null="flags"),
               dict(misalign="src"), dict(misalign="dst"), dict(misalign="rms"), dict(n_points=0), dict(n_points=4097),
               dict(min_gap=-1.0), dict(min_gap=1.0), dict(mask=0), dict(mask=16)):
        st, outs, keep = run_device(dev, src, dst, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, keep = run_device(dev, src, dst, n_sets=0)      # no sets: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())


def test_step_timer(dev):
    src, dst = make_batch(64, 5)
    L = _abi.lib()
    ms = (C.c_float * 1)()
    try:
        assert L.slhip_pose_fit_timing_enable(1) == 0
        assert run_device(dev, src, dst, mask=0)[0] < 0                        # a refused call records no event
        assert L.slhip_pose_fit_timings(C.byref(ms)) == 0 and list(ms) == [-1.0]
        assert run_device(dev, src, dst)[0] == 0
        assert L.slhip_pose_fit_timings(C.byref(ms)) == 0 and np.isfinite(ms[0]) and ms[0] >= 0.0
        assert L.slhip_pose_fit_timings(None) < 0
    finally:
        L.slhip_pose_fit_timing_enable(0)


# ---- end to end on a placed batch ------------------------------------------------------------------------------------------------
def test_object_coordinates_onto_camera_points_recover_the_pose(placed3d):  # noqa: F811
    sl, batch, points, kbank, kps, off, mbank = placed3d
    n = len(points)
    fit = batch.pose_fit(points.coord, points.camera)
    torch.cuda.synchronize()
    valid = points.valid.cpu().numpy()
    assert bool(fit.found.all()) and np.array_equal(fit.n_used.cpu().numpy(), valid.sum(1))
    gt = points.object_to_camera.cpu().numpy()
    coord, camera = points.coord.cpu().numpy(), points.camera.cpu().numpy()
    ref = np.stack([R.fit_svd(coord[i], camera[i])[0] for i in range(n)])
    p_ref, p_dev = pose_difference(ref, gt), pose_difference(fit.pose.cpu().numpy(), gt)
    bound = 4.0 * p_ref.max()
    print("pose_fit of coord onto camera: %d sets, worst difference from object_to_camera %.3g, the float64 SVD's %.3g, bound %.3g; "
          "worst rms %.3g m" % (n, p_dev.max(), p_ref.max(), bound, float(fit.rms.max())))
    assert p_dev.max() <= bound

    # the poses through pose_errors: ADD <= the pose bound times sqrt(r^2 + 1), r the largest |p| of the model bank (docstring)
    err = batch.pose_errors(fit.dense(N_SCENES, N_OBJ, points.scene_global, points.slot), mbank, outputs=("add",))
    torch.cuda.synchronize()
    scene, slot = points.scene_global.long().cpu(), points.slot.long().cpu()
    add = err.add.cpu()[scene, slot - 1].numpy()
    assert int(torch.isfinite(err.add).sum()) == n
    r = float(mbank.points[..., :3].norm(dim=-1).max())
    print("pose_fit -> pose_errors: worst ADD %.3g m, bound %.3g m (r = %.3g m)" % (add.max(), bound * np.sqrt(r * r + 1.0), r))
    assert add.max() <= bound * np.sqrt(r * r + 1.0)
    with pytest.raises(TypeError):
        batch.pose_fit(points.coord)
    with pytest.raises(TypeError):
        batch.pose_fit(points.coord, points.camera, bank=kbank)


def test_cpu_tensors_are_refused(placed3d):  # noqa: F811
    sl, batch, points, kbank, kps, off, mbank = placed3d
    with pytest.raises(_abi.SlhipError) as e:
        pf.solve(points.coord.cpu(), points.camera.cpu())
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        batch.pose_fit(points.coord, points.camera.cpu())
