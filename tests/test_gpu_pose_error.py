"""Pose errors on the device (slhip_pose_error, slhip_pose_error_diameter, sl.pose_error, SceneBatch.pose_errors) against the
NumPy restatement tests/pose_error_ref.py.  Every comparison with the restatement is bit for bit -- floats as their int32
views, indices equal; every output lies between 256 poisoned guard bytes that must stay poison, and an output that `outputs`
does not name stays poison throughout.  The cases, their restatement and their float64 bound are those of
tests/test_host_pose_error.py (computed once, shared)."""
import ctypes as C

import numpy as np
import pytest
import torch

import pose_error_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_error as pe
from test_gpu_object_keypoints import Guarded, bits, stream, to_dev
from test_host_pose_error import CASES, EYE, K4, check_against_float64, compose, five_class_bank, hypotheses_case, large_class_case, rot

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("add", "adds", "mssd", "mssd_sym", "mspd", "mspd_sym")
BIT = {"add": R.ADD, "adds": R.ADDS, "mssd": R.MSSD, "mssd_sym": R.MSSD, "mspd": R.MSPD, "mspd_sym": R.MSPD}


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


class DeviceBank:
    def __init__(self, bank, dev):
        points, count, syms, n_sym = bank
        self.t = [to_dev(np.ascontiguousarray(a), dev) for a in (points, count, syms, n_sym)]
        self.shape = (points.shape[0], points.shape[1], syms.shape[1])

    def record(self, null=None, misalign=None, **kw):
        ptrs = [t.data_ptr() for t in self.t]
        for i, name in enumerate(("points", "count", "symmetries", "n_sym")):
            if null == name:
                ptrs[i] = None
            if misalign == name:
                ptrs[i] += 4
        A, N, S = self.shape
        return _abi.PoseBank(ptrs[0], ptrs[1], ptrs[2], ptrs[3], kw.get("n_assets", A), kw.get("n_points", N), kw.get("n_symmetries", S), 0)


def run_errors(dev, case, mask=R.ALL, records=False, null=None, stride=None, Hy=None, n_scenes=None, **bank_kw):
    B, O, H = case.est.shape[:3]
    bank = DeviceBank(case.bank(), dev)
    if records:
        objs = np.zeros((B, O), _abi.SYNTH_OBJECT_DTYPE)
        objs["asset"], objs["instance_index"], objs["metallic"] = case.classes.astype(np.uint32), 0x7fffffff, np.nan      # only .asset is read
        d_cls, cls_stride = to_dev(objs, dev), 4
    else:
        d_cls, cls_stride = to_dev(case.classes, dev), 1
    d_gt, d_est = to_dev(case.gt, dev), to_dev(case.est, dev)
    outs = {k: Guarded(B * O * H * 4, dev) for k in NAMES}
    o = _abi.PoseErrorOut(*(None if null == k else outs[k].ptr() for k in NAMES))
    p = pe.make_params(K4, O, H if Hy is None else Hy, mask).reshape(1)
    rec = bank.record(null=null, **bank_kw)
    args = dict(classes=C.c_void_p(d_cls.data_ptr()), gt=C.c_void_p(d_gt.data_ptr()), est=C.c_void_p(d_est.data_ptr()))
    if null in args:
        args[null] = None
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_error(None if null == "params" else p.ctypes.data, None if null == "bank" else C.byref(rec), args["classes"],
                                         cls_stride if stride is None else stride, args["gt"], args["est"], B if n_scenes is None else n_scenes,
                                         None if null == "record" else C.byref(o), stream(dev))
    return st, outs, (B, O, H), (bank, d_cls, d_gt, d_est)


def read(outs, shape, mask):
    """the outputs named in `mask` from between their guards; the others must be untouched"""
    got = {}
    for k in NAMES:
        if mask & BIT[k]:
            got[k] = outs[k].host(np.int32 if k.endswith("_sym") else F, shape).copy()
        else:
            assert outs[k].untouched(), k
    return got


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        diff = bits(got[k]).reshape(-1, 4).view(np.int32) != bits(want[k]).reshape(-1, 4).view(np.int32)
        assert not diff.any(), "%s %s: %d of %d differ, the first at %s: %r against %r" % (
            what, k, int(diff.sum()), diff.size, tuple(np.argwhere(diff.reshape(want[k].shape))[0]),
            got[k][tuple(np.argwhere(diff.reshape(want[k].shape))[0])], want[k][tuple(np.argwhere(diff.reshape(want[k].shape))[0])])


# ---- 1. the errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cases_bit_for_bit(dev, name):
    """point counts 0, 1, 63, 65, 257 and symmetry counts 1, 65, 630, 3 with Hy = 1, 3, 33 over 2 x 3 objects (a class outside
    the bank, a NaN estimate, one behind the camera); one class at 4096 points; the sl.diff shape 1 x 64 x 32"""
    case = CASES[name]()
    st, outs, shape, keep = run_errors(dev, case)
    assert st == 0, _abi.lib().slhip_last_error()
    got = read(outs, shape, R.ALL)
    assert_same(got, case.ref32(), name)
    check_against_float64(got, case, name + " device")


def test_classes_as_object_records_read_in_place(dev):
    case = hypotheses_case(3)
    st, outs, shape, keep = run_errors(dev, case, records=True)
    assert st == 0
    got = read(outs, shape, R.ALL)
    assert_same(got, case.ref32(), "records")
    for k in ("add", "adds", "mssd", "mspd"):
        assert np.isposinf(got[k][0, 2]).all() and np.isposinf(got[k][1, 2]).all(), k      # outside the bank; count 0: never 0
        assert np.isnan(got[k][0, 0, 1]) and np.isfinite(got[k][0, 0, [0, 2]]).all(), k      # the NaN estimate, its neighbours
    assert np.isposinf(got["mspd"][1, 0, 0]) and got["mspd_sym"][1, 0, 0] == -1 and np.isfinite(got["mssd"][1, 0, 0])


@pytest.mark.parametrize("mask", [R.ADD, R.ADDS, R.MSSD, R.MSPD, R.ADD | R.MSPD, R.ADDS | R.MSSD])
def test_outputs_not_named_stay_poison(dev, mask):
    case = hypotheses_case(3)
    st, outs, shape, keep = run_errors(dev, case, mask=mask)
    assert st == 0
    assert_same(read(outs, shape, mask), case.ref32(mask), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev):
    case = hypotheses_case(1)
    for kw in (dict(null="params"), dict(null="bank"), dict(null="points"), dict(null="count"), dict(null="symmetries"), dict(null="n_sym"),
               dict(null="classes"), dict(null="gt"), dict(null="est"), dict(null="record"), dict(null="adds"), dict(null="mspd_sym"),
               dict(misalign="points"), dict(misalign="symmetries"), dict(n_points=0), dict(n_points=4097), dict(n_symmetries=0),
               dict(n_symmetries=1025), dict(n_assets=0), dict(stride=0), dict(Hy=0), dict(mask=0), dict(mask=16)):
        st, outs, shape, keep = run_errors(dev, case, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, shape, keep = run_errors(dev, case, n_scenes=0)                 # no scenes: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())


def test_step_timer(dev):
    case = hypotheses_case(1)
    L = _abi.lib()
    ms = (C.c_float * 2)()
    try:
        assert L.slhip_pose_error_timing_enable(1) == 0
        assert run_errors(dev, case, Hy=0)[0] < 0                             # a refused call records no event
        assert L.slhip_pose_error_timings(C.byref(ms)) == 0 and list(ms) == [-1.0, -1.0]
        assert run_errors(dev, case)[0] == 0
        assert L.slhip_pose_error_timings(C.byref(ms)) == 0
        assert ms[0] == -1.0 and np.isfinite(ms[1]) and ms[1] >= 0.0
        assert L.slhip_pose_error_timings(None) < 0
    finally:
        L.slhip_pose_error_timing_enable(0)


# ---- 2. the diameter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["five", "N4096"])
def test_diameter(dev, which):
    bank = five_class_bank() if which == "five" else large_class_case().bank()
    points, count = bank[0], bank[1]
    d_bank = DeviceBank(bank, dev)
    out = Guarded(len(count) * 4, dev)
    rec = d_bank.record()
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_error_diameter(C.byref(rec), out.ptr(), stream(dev))
    assert st == 0
    got = out.host(F, (len(count),))
    want = R.diameter32(points, count)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert np.array_equal(bits(got), bits(pe.diameter_host(points, count)))
    assert np.abs(got - R.diameter64(points, count)).max() <= R.tol(float(np.abs(points[..., :3]).max()))
    for kw in (dict(null="points"), dict(null="count"), dict(misalign="points"), dict(n_points=4097), dict(n_assets=0)):
        out = Guarded(len(count) * 4, dev)
        rec = d_bank.record(**kw)
        with torch.cuda.device(dev):
            assert _abi.lib().slhip_pose_error_diameter(C.byref(rec), out.ptr(), stream(dev)) < 0, kw
        assert out.untouched(), kw


# ---- 3. through the public path --------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 2, 3, (320, 240), (533.4, 533.7, 156.5, 120.6)
QUARTER = rot([0, 0, 1], np.pi / 2)      # a symmetry of a centred cube


@pytest.fixture(scope="module")
def placed(sl):
    import scenes as S

    meshes = []
    for i in range(3):
        m = sl.Mesh(S.CUBE)
        m.center_bbox()
        m.scale_to_bbox_diagonal(0.12 + 0.05 * i)
        m.class_index = i + 1
        meshes.append(m)
    table = sl.AssetTable(meshes)
    batch = sl.SceneBatch(table, N_SCENES, N_OBJ, resolution=RES, seed=(77 << 32) | 5, render_chunk=N_SCENES, manual_exposure=1.0,
                          scene_id_base=1000)
    batch.set_camera_intrinsics(*INTRINSICS)
    batch.stage()
    batch.settle(frames=5)
    batch.place(object_to_camera=True)
    bank = sl.pose_error.bank(table, n_points=16, symmetries={c: [QUARTER, QUARTER @ QUARTER] for c in range(3)})
    torch.cuda.synchronize()
    return batch, table, bank


def test_bank_of_the_table(placed):
    batch, table, bank = placed
    assert isinstance(bank, pe.ModelBank) and tuple(bank.points.shape) == (3, 16, 4) and bank.count.tolist() == [16, 16, 16]
    assert tuple(bank.symmetries.shape) == (3, 3, 3, 4) and bank.n_sym.tolist() == [3, 3, 3]
    assert np.array_equal(bits(bank.symmetries[:, 0].cpu().numpy()), bits(np.tile(EYE, (3, 1, 1))))
    pos = batch.eng.pool.arrays()[0]
    want, count = pe.sample_points(torch.from_numpy(np.ascontiguousarray(pos, F).reshape(-1, 4)), table.records, table.templates, 16)
    assert np.array_equal(bits(bank.points.cpu().numpy()), bits(want.numpy()))
    points = bank.points.cpu().numpy()
    assert np.array_equal(bits(bank.diameter.cpu().numpy()), bits(R.diameter32(points, [16] * 3)))
    diag = np.array([0.12, 0.17, 0.22])
    assert np.abs(bank.diameter.cpu().numpy() - diag).max() < 1e-6            # 16 of a cube's 24 vertices span its diagonal
    over = pe.bank(table, n_points=16, diameter={1: 0.5})
    assert over.diameter[1] == 0.5 and over.diameter[0] == bank.diameter[0]


def test_the_ground_truth_scores_zero(placed):
    batch, table, bank = placed
    gt = batch.object_to_camera
    err = batch.pose_errors(gt.clone(), bank)
    torch.cuda.synchronize()
    assert tuple(err.add.shape) == (N_SCENES, N_OBJ)                          # no hypothesis axis in, none out
    for k in ("add", "adds", "mssd"):
        assert (getattr(err, k) == 0).all(), k
    assert (err.mssd_sym == 0).all()
    front = torch.isfinite(err.mspd)
    assert (err.mspd[front] == 0).all() and (err.mspd_sym[front] == 0).all() and bool(front.any())
    classes = batch.host_objects()["asset"].reshape(N_SCENES, N_OBJ)
    assert np.array_equal(err.classes.cpu().numpy(), classes.astype(np.int32))
    want = R.errors32(*(t.cpu().numpy() for t in bank.tensors()), classes, gt.cpu().numpy(), gt.cpu().numpy()[:, :, None], batch.intrinsics())
    for k, v in want.items():
        assert np.array_equal(bits(getattr(err, k).cpu().numpy()), bits(v[:, :, 0])), k
    only = batch.pose_errors(gt.clone(), bank, outputs=("adds",), chunk=0)
    assert only.add is None and only.mssd is None and only.mssd_sym is None and only.mspd is None and torch.equal(only.adds, err.adds)
    assert float(err.recall("add", [0.0])[0]) == 1.0 and float(err.recall("mssd", [0.1], bank)[0]) == 1.0


def test_a_class_symmetry_of_the_ground_truth(placed):
    batch, table, bank = placed
    gt = batch.object_to_camera.cpu().numpy().astype(np.float64)
    est = np.stack([compose(gt, EYE.astype(np.float64)), compose(gt, QUARTER[:3]), compose(gt, (QUARTER @ QUARTER)[:3])], axis=2).astype(F)
    err = batch.pose_errors(torch.from_numpy(est).to(batch.object_to_camera.device), bank)
    torch.cuda.synchronize()
    points, count, syms, n_sym = (t.cpu().numpy() for t in bank.tensors())
    classes = err.classes.cpu().numpy()
    M = R.largest_coordinate(points, count, syms, n_sym, classes, gt.astype(F), est)
    tol = R.tol(M)
    add, mssd, idx = err.add.cpu().numpy(), err.mssd.cpu().numpy(), err.mssd_sym.cpu().numpy()
    assert (add[:, :, 0] <= tol).all() and (add[:, :, 1:] > 0.01).all()       # a quarter and a half turn move a cube's corners
    assert (mssd <= tol).all()
    assert (idx == np.array([0, 1, 2])).all()
    adds = err.adds.cpu().numpy()
    assert np.isfinite(adds).all() and (adds <= add + tol).all()
    auto = err.add_auto(bank)
    assert torch.equal(auto, err.adds)                                        # every class has symmetries
    near = err.closest_gt(batch.object_to_camera, bank).cpu().numpy()
    assert near.shape == est.shape and np.abs(near - est).max() <= tol


def test_pose_errors_need_object_to_camera_of_the_last_view(placed):
    batch, table, bank = placed
    gt = batch.object_to_camera.clone()
    with pytest.raises(TypeError):
        batch.pose_errors(gt, bank, intrinsics=K4)
    batch.place(view=1)
    with pytest.raises(RuntimeError) as e:
        batch.pose_errors(gt, bank)
    assert "place(object_to_camera=True)" in str(e.value)
    batch.place(object_to_camera=True)
    assert (batch.pose_errors(batch.object_to_camera.clone(), bank).add == 0).all()


def test_cpu_tensors_are_refused(placed):
    batch, table, bank = placed
    gt = batch.object_to_camera
    with pytest.raises(_abi.SlhipError) as e:
        pe.evaluate(gt, gt.cpu(), batch.d_objects, bank, K4)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        pe.evaluate(gt, gt, torch.zeros((N_SCENES, N_OBJ), dtype=torch.int32), bank, K4)
