"""Pose VSD on the device (slhip_pose_vsd, slhip_pose_depth, sl.pose_vsd, SceneBatch.pose_vsd) against the NumPy restatement
tests/pose_vsd_ref.py.  Every comparison with the restatement is bit for bit -- floats as their int32 views, counts equal; every
output lies between 256 poisoned guard bytes that must stay poison, and an output that `outputs` does not name stays poison
throughout.  The cases and their restatement are those of tests/test_host_pose_vsd.py (computed once, shared)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pose_vsd_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_vsd as pv
from test_gpu_object_keypoints import Guarded, bits, stream, to_dev
from test_host_pose_vsd import BIT, CASES, CUBE, DTYPE, FIXED, NAMES, PLATE, assert_same, case, hypotheses_case, pose

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


class DeviceSurface:
    FIELDS = ("vertices", "triangles", "tri_begin", "tri_count", "diameter")

    def __init__(self, bank, dev):
        self.t = [to_dev(np.ascontiguousarray(a), dev) for a in bank]
        self.n = (len(bank[2]), len(bank[0]), len(bank[1]))

    def record(self, null=None, misalign=None, **kw):
        ptrs = [t.data_ptr() for t in self.t]
        for i, name in enumerate(self.FIELDS):
            if null == name:
                ptrs[i] = None
            if misalign == name:
                ptrs[i] += 4
        return _abi.PoseSurface(*ptrs, kw.get("n_assets", self.n[0]), kw.get("n_vertices", self.n[1]), kw.get("n_triangles", self.n[2]), 0)


def params_of(c, mask, **pkw):
    B, O, Hy = c.est.shape[:3]
    kw = dict(c.kw)
    kw.update(pkw)
    size = kw.pop("size", c.size)
    return pv.make_params(c.K, size, O, kw.pop("n_hypotheses", Hy), outputs=mask, **kw).reshape(1)


def run_vsd(dev, c, mask=R.ALL, records=False, null=None, misalign=None, stride=None, depth_stride=1, n_scenes=None, surface_kw=None, **pkw):
    B, O, Hy = c.est.shape[:3]
    surf = DeviceSurface(c.bank, dev)
    if records:
        objs = np.zeros((B, O), _abi.SYNTH_OBJECT_DTYPE)
        objs["asset"], objs["instance_index"], objs["metallic"] = c.classes.astype(np.uint32), 0x7fffffff, np.nan      # only .asset is read
        d_cls, cls_stride = to_dev(objs, dev), 4
    else:
        d_cls, cls_stride = to_dev(c.classes, dev), 1
    depth = c.depth if depth_stride != 4 else np.ascontiguousarray(np.stack([np.full_like(c.depth, np.nan)] * 3 + [c.depth], axis=-1))
    d_gt, d_est, d_depth = to_dev(c.gt, dev), to_dev(c.est, dev), to_dev(depth, dev)
    p = params_of(c, mask, **pkw)
    T = max(1, min(int(p["n_taus"][0]), 16))
    shapes = {"vsd": (B, O, Hy, T), "counts": (B, O, Hy, 4), "n_cost": (B, O, Hy, T), "flags": (B, O, Hy)}
    outs = {k: Guarded(int(np.prod(shapes[k])) * 4, dev) for k in NAMES}
    o = _abi.PoseVsdOut(*(None if null == k else outs[k].ptr() for k in NAMES))
    rec = surf.record(null=null, misalign=misalign, **(surface_kw or {}))
    args = dict(classes=C.c_void_p(d_cls.data_ptr()), gt=C.c_void_p(d_gt.data_ptr()), est=C.c_void_p(d_est.data_ptr()),
                depth=C.c_void_p(d_depth.data_ptr() + (12 if depth_stride == 4 else 0)))
    if null in args:
        args[null] = None
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_vsd(None if null == "params" else p.ctypes.data, None if null == "surface" else C.byref(rec), args["classes"],
                                       cls_stride if stride is None else stride, args["gt"], args["est"], args["depth"], depth_stride,
                                       B if n_scenes is None else n_scenes, None if null == "record" else C.byref(o), stream(dev))
    return st, outs, shapes, (surf, d_cls, d_gt, d_est, d_depth)


def read(outs, shapes, mask):
    """the outputs named in `mask` from between their guards; the others must be untouched"""
    got = {}
    for k in NAMES:
        if mask & BIT[k]:
            got[k] = outs[k].host(DTYPE[k], shapes[k]).copy()
        else:
            assert outs[k].untouched(), k
    return got


def device_result(dev, c, mask=R.ALL, **kw):
    st, outs, shapes, keep = run_vsd(dev, c, mask, **kw)
    assert st == 0, _abi.lib().slhip_last_error()
    return read(outs, shapes, mask)


def run_depth(dev, c, poses, null=None, with_flags=True, **pkw):
    B, O, Hy = poses.shape[:3]
    W, H = pkw.get("size", c.size)
    surf = DeviceSurface(c.bank, dev)
    d_cls, d_poses = to_dev(c.classes, dev), to_dev(np.ascontiguousarray(poses, F), dev)
    p = pv.make_params(c.K, (W, H), O, Hy, normalized=False, **{k: v for k, v in c.kw.items() if k == "z_near"}).reshape(1)
    depth, flags = Guarded(B * O * Hy * H * W * 4, dev), Guarded(B * O * Hy * 4, dev)
    rec = surf.record()
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_pose_depth(None if null == "params" else p.ctypes.data, C.byref(rec), C.c_void_p(d_cls.data_ptr()), 1,
                                         None if null == "poses" else C.c_void_p(d_poses.data_ptr()), B, None if null == "depth" else depth.ptr(),
                                         flags.ptr() if with_flags else None, stream(dev))
    return st, depth, flags, (B, O, Hy, H, W), (surf, d_cls, d_poses)


# ---- 1. the errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_cases_bit_for_bit(dev, name):
    """the plate (two large triangles: a wave per triangle), cube, tetrahedron and the icosphere of 1280 sub-pixel triangles on
    about 20 px (a lane per triangle, five passes of 256 lanes) with Hy = 1, 3, 33 over 2 x 3 objects: classes without a
    surface, a NaN estimate, a cube through z_near"""
    c = CASES[name]()
    assert_same(device_result(dev, c), c.ref32(), name)


@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_cases_bit_for_bit(dev, name):
    c = FIXED[name]
    got = device_result(dev, c)
    assert_same(got, c.ref32(), name)
    r64 = c.ref64()
    assert np.array_equal(got["counts"], r64["counts"]) and np.array_equal(got["n_cost"], r64["n_cost"])


def test_depth_read_at_stride_four_and_one(dev):
    c = hypotheses_case(3)
    assert_same(device_result(dev, c, depth_stride=4), c.ref32(), "stride 4")
    assert_same(device_result(dev, c, depth_stride=1), c.ref32(), "stride 1")


def test_classes_as_object_records_read_in_place(dev):
    c = hypotheses_case(3)
    got = device_result(dev, c, records=True)
    assert_same(got, c.ref32(), "records")
    assert np.isposinf(got["vsd"][0, 2]).all() and np.isposinf(got["vsd"][1, 2]).all() and (got["counts"][:, 2] == -1).all()
    assert np.isnan(got["vsd"][0, 0, 1]).all() and np.isfinite(got["vsd"][0, 0, [0, 2]]).all()
    assert got["flags"][0, 1, 2] == R.CLIPPED and (got["vsd"][0, 0, 0] == 0).all()


@pytest.mark.parametrize("mask", [R.VSD, R.COUNTS, R.COST, R.FLAGS, R.VSD | R.FLAGS, R.COUNTS | R.COST])
def test_outputs_not_named_stay_poison(dev, mask):
    c = hypotheses_case(3)
    assert_same(device_result(dev, c, mask=mask), c.ref32(mask), "mask %d" % mask)


# ---- 2. the raster alone ---------------------------------------------------------------------------------------------------------
def test_depth_planes_bit_for_bit(dev):
    """slhip_pose_depth of every class, the 0 of uncovered pixels, of classes without a surface and of a NaN pose included"""
    c = hypotheses_case(3)
    poses = np.ascontiguousarray(c.est)
    st, depth, flags, shape, keep = run_depth(dev, c, poses)
    assert st == 0, _abi.lib().slhip_last_error()
    want, wflags = R.depth32(c.bank, c.classes, poses, c.K, c.size)
    got = depth.host(F, shape)
    assert np.array_equal(bits(got), bits(want)), "%d pixels differ" % int((got.view(np.int32) != want.view(np.int32)).sum())
    assert np.array_equal(flags.host(np.uint32, shape[:3]), wflags)
    assert (got[0, 2] == 0).all() and (got[0, 0, 1] == 0).all() and (got[1, 0] > 0).sum() > 200 and wflags[0, 1, 2] == R.CLIPPED
    st, depth, flags, shape, keep = run_depth(dev, c, poses[:, :, :1], with_flags=False)      # the flags are optional
    assert st == 0 and np.array_equal(bits(depth.host(F, shape)), bits(want[:, :, :1]))
    for null in ("params", "poses", "depth"):
        st, depth, flags, shape, keep = run_depth(dev, c, poses, null=null)
        assert st < 0 and depth.untouched() and flags.untouched(), null


# ---- 3. bands --------------------------------------------------------------------------------------------------------------------
def band_case(extra_rows):
    """the plate stretched by its pose to 128 columns x (band_pixels / 128 + extra_rows) rows of a 160-wide picture: a window of
    exactly one band, or one band and `extra_rows` more rows; the estimate a little deeper and shifted"""
    rows = pv.band_pixels() // 128
    W, H = 160, rows + 24
    n = rows + extra_rows
    K = (128.0, 128.0, 80.0, 12.0 + n / 2.0)                                  # u in [16, 144], v in [12, 12 + n]: no centre on an edge
    g = pose((0, 0, 1), scale=(4.0, n / 32.0, 1.0))
    e = pose((0.01, 0.0, 1.03125), scale=(4.0, n / 32.0, 1.0))
    py, px = np.mgrid[0:H, 0:W]
    depth = (1.01 + 0.0005 * (px - 80)).astype(F)[None]                        # in front of the ground truth on the left
    return case([[PLATE]], g[None, None], np.stack([g, e])[None, None], depth, K=K), n


@pytest.mark.parametrize("extra_rows", [0, 1])
def test_a_window_of_one_band_and_of_one_band_plus_a_row(dev, extra_rows):
    c, n = band_case(extra_rows)
    got = device_result(dev, c)
    assert_same(got, c.ref32(), "band + %d" % extra_rows)
    assert got["counts"][0, 0, 0, 3] <= 128 * n and got["counts"][0, 0, 0, 3] > 0 and (got["vsd"][0, 0, 0] == 0).all()
    st, depth, flags, shape, keep = run_depth(dev, c, c.est)
    assert st == 0
    plane = depth.host(F, shape)
    assert int((plane[0, 0, 0] > 0).sum()) == 128 * n                         # the window is exactly 128 x n pixels
    assert np.array_equal(bits(plane), bits(R.depth32(c.bank, c.classes, c.est, c.K, c.size)[0]))


@functools.lru_cache(maxsize=None)
def close_cube_case():
    """the cube close to the camera at 160 x 120: its window is the whole picture, 19200 pixels, more than any band"""
    W, H = 160, 120
    K = (128.0, 128.0, 79.5, 60.25)
    g = pose((0.01, -0.005, 0.22), (1, 2, 0.5), 0.3)
    e = pose((0.015, -0.005, 0.23), (1, 2, 0.4), 0.35)
    py, px = np.mgrid[0:H, 0:W]
    depth = (0.14 + 0.0004 * px + 0.0002 * py).astype(F)[None]
    depth[0, 100:, :30] = 0.0
    depth[0, :40, 100:] = 0.08                                                # an occluder in front of a corner
    return case([[CUBE]], g[None, None], np.stack([g, e, g])[None, None], depth, K=K)


def test_a_window_of_several_bands(dev):
    c = close_cube_case()
    assert c.size[0] * c.size[1] > pv.band_pixels()
    got = device_result(dev, c)
    assert_same(got, c.ref32(), "close cube")
    assert pv.band_pixels() < got["counts"][0, 0, 1, 3] < 19200 and (got["vsd"][0, 0, [0, 2]] == 0).all()
    st, depth, flags, shape, keep = run_depth(dev, c, c.est)
    assert st == 0 and np.array_equal(bits(depth.host(F, shape)), bits(R.depth32(c.bank, c.classes, c.est, c.K, c.size)[0]))


# ---- 4. refusals, timing ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_device_untouched(dev):
    c = FIXED["equal"]
    for kw in (dict(null="params"), dict(null="surface"), dict(null="vertices"), dict(null="triangles"), dict(null="tri_begin"),
               dict(null="tri_count"), dict(null="diameter"), dict(null="classes"), dict(null="gt"), dict(null="est"), dict(null="depth"),
               dict(null="record"), dict(null="vsd"), dict(null="counts"), dict(null="n_cost"), dict(null="flags"), dict(misalign="vertices"),
               dict(surface_kw=dict(n_assets=0)), dict(surface_kw=dict(n_vertices=0)), dict(surface_kw=dict(n_triangles=0)), dict(stride=0),
               dict(depth_stride=0), dict(n_hypotheses=0), dict(mask=0), dict(mask=16), dict(taus=(0.1,) * 17), dict(delta=-1.0),
               dict(z_near=0.0), dict(size=(4097, 64))):
        st, outs, shapes, keep = run_vsd(dev, c, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, shapes, keep = run_vsd(dev, c, n_scenes=0)                      # no scenes: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())


def test_step_timer(dev):
    c = FIXED["equal"]
    L = _abi.lib()
    ms = (C.c_float * 2)()
    try:
        assert L.slhip_pose_vsd_timing_enable(1) == 0
        assert run_vsd(dev, c, n_hypotheses=0)[0] < 0                          # a refused call records no event
        assert L.slhip_pose_vsd_timings(C.byref(ms)) == 0 and list(ms) == [-1.0, -1.0]
        assert run_vsd(dev, c)[0] == 0
        assert L.slhip_pose_vsd_timings(C.byref(ms)) == 0
        assert np.isfinite(ms[0]) and ms[0] >= 0.0 and ms[1] == -1.0
        assert run_depth(dev, c, c.est)[0] == 0
        assert L.slhip_pose_vsd_timings(C.byref(ms)) == 0 and ms[1] >= 0.0
        assert L.slhip_pose_vsd_timings(None) < 0
    finally:
        L.slhip_pose_vsd_timing_enable(0)


# ---- 5. through the public path --------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 2, 4, (160, 120), (266.7, 266.85, 78.25, 60.3)


@pytest.fixture(scope="module")
def placed(sl):
    import scenes as S

    meshes = []
    for i in range(4):
        m = sl.Mesh(S.CUBE)
        m.center_bbox()
        m.scale_to_bbox_diagonal(0.12 + 0.04 * i)
        m.class_index = i + 1
        meshes.append(m)
    table = sl.AssetTable(meshes)
    batch = sl.SceneBatch(table, N_SCENES, N_OBJ, resolution=RES, seed=(78 << 32) | 6, render_chunk=N_SCENES, manual_exposure=1.0,
                          scene_id_base=2000)
    batch.set_camera_intrinsics(*INTRINSICS)
    batch.stage()
    batch.settle(frames=5)
    batch.place(object_to_camera=True)
    buffers = batch.render(0)
    surf = sl.pose_vsd.surface(table)
    torch.cuda.synchronize()
    return batch, table, surf, buffers


def host_bank(surf):
    return tuple(t.cpu().numpy() for t in (surf.vertices, surf.triangles, surf.tri_begin, surf.tri_count, surf.diameter))


def test_surface_of_the_table(placed):
    batch, table, surf, buffers = placed
    assert isinstance(surf, pv.SurfaceBank) and len(surf) == 4
    n_verts = [int(a["n_verts"]) for a in table.records]
    assert surf.vertices.shape[0] == sum(n_verts) and (surf.vertices[:, 3] == 1).all()
    assert surf.tri_count.tolist() == [12] * 4 and surf.tri_begin.tolist() == [0, 12, 24, 36]
    tris = surf.triangles.cpu().numpy()
    for c in range(4):
        t = tris[12 * c:12 * c + 12]
        assert t.min() >= sum(n_verts[:c]) and t.max() < sum(n_verts[:c + 1])
    diag = np.array([0.12, 0.16, 0.20, 0.24])
    assert np.abs(surf.diameter.cpu().numpy() - diag).max() < 1e-6


def test_the_ground_truth_scores_zero_and_a_shift_by_a_diameter_one(placed):
    batch, table, surf, buffers = placed
    gt = batch.object_to_camera
    same = batch.pose_vsd(gt.clone(), surf, buffers, chunk=0)
    torch.cuda.synchronize()
    assert tuple(same.vsd.shape) == (N_SCENES, N_OBJ, 10) and tuple(same.counts.shape) == (N_SCENES, N_OBJ, 4)      # no hypothesis axis in, none out
    seen = same.counts[..., 3] > 0
    assert bool(seen.any()) and (same.vsd[seen] == 0).all() and (same.vsd[~seen] == 1).all()
    assert (same.counts[..., 0] == same.counts[..., 3]).all() and (same.counts[..., 2] == same.counts[..., 3]).all()
    assert float(same.recall()) == float(seen.float().mean())
    classes = batch.host_objects()["asset"].reshape(N_SCENES, N_OBJ).astype(np.int32)
    assert np.array_equal(same.classes.cpu().numpy(), classes)
    shifted = gt.clone()
    shifted[:, :, 0, 3] += surf.diameter[torch.from_numpy(classes).long().to(gt.device)]
    moved = batch.pose_vsd(shifted, surf, buffers)                            # chunk None: the buffers hold the whole batch
    torch.cuda.synchronize()
    disjoint = (moved.counts[..., 2] == 0) & (moved.counts[..., 3] > 0)
    assert bool(disjoint.any()) and (moved.vsd[disjoint] == 1).all()
    bank, depth, K = host_bank(surf), buffers.coord[:N_SCENES, :, :, 3].cpu().numpy(), batch.intrinsics()
    for res, est in ((same, gt), (moved, shifted)):
        want = R.evaluate(bank, classes, gt.cpu().numpy(), est.cpu().numpy()[:, :, None], depth, K)
        for k in NAMES:
            assert np.array_equal(bits(getattr(res, k).cpu().numpy()), bits(want[k][:, :, 0])), k
    only = batch.pose_vsd(gt.clone(), surf, buffers, chunk=0, outputs=("counts",), normalized=False, taus=(0.02,))
    assert only.vsd is None and only.flags is None and torch.equal(only.counts, same.counts)
    planes, flags = pv.render_depth(gt, batch.d_objects, surf, batch.intrinsics(), RES)
    torch.cuda.synchronize()
    want, wflags = R.depth32(bank, classes, gt.cpu().numpy()[:, :, None], K, RES)
    assert np.array_equal(bits(planes.cpu().numpy()), bits(want[:, :, 0]))
    # the raster is the render's picture of the object: where the render shows object o, the plane of o is covered and agrees
    inst, z = buffers.instance[:N_SCENES].cpu().numpy().reshape(N_SCENES, RES[1], RES[0]), planes.cpu().numpy()
    shown = covered = 0
    for b in range(N_SCENES):
        for o in range(N_OBJ):
            own = inst[b] == o + 1
            shown, covered = shown + int(own.sum()), covered + int((z[b, o][own] > 0).sum())
            both = own & (z[b, o] > 0)
            if both.any():
                assert np.median(np.abs(z[b, o][both] - depth[b][both])) < 1e-4, (b, o)
    print("render pixels of the objects: %d, covered by their depth planes: %d" % (shown, covered))
    assert shown > 500 and covered >= 0.98 * shown
    assert int(same.counts[..., 0].sum()) >= 0.98 * shown                     # and the ground truth is visible where the render shows it


def test_pose_vsd_needs_object_to_camera_of_the_last_view(placed):
    batch, table, surf, buffers = placed
    gt = batch.object_to_camera.clone()
    with pytest.raises(TypeError):
        batch.pose_vsd(gt, surf, buffers, intrinsics=INTRINSICS)
    batch.place(view=1)
    with pytest.raises(RuntimeError) as e:
        batch.pose_vsd(gt, surf, buffers)
    assert "place(object_to_camera=True)" in str(e.value)
    batch.place(object_to_camera=True)
    with pytest.raises(_abi.SlhipError) as e:
        pv.evaluate(gt, gt.cpu(), batch.d_objects, surf, buffers.coord, INTRINSICS)
    assert "no CPU path" in str(e.value)
