"""Render flow on the device (slhip_render_flow, slhip_render_flow_motion, sl.render_flow, SceneBatch.view_state / .flow) against
the host twins and the NumPy restatement tests/render_flow_ref.py.  Every comparison of the kernels is bit for bit -- floats as
their bytes; every device output lies between poisoned guard bytes that must stay poison.

The end-to-end tests hold the flow of a rendered batch to T_FLOW of test_host_render_flow.py (4 x 3.7e-4 px, the float32
restatement's worst against float64) where the motion is nothing, and to an independent float64 route where it is something:
the object coordinates coord_a.xyz moved by object_to_camera of view b (plane pixels: the camera point of a through the two
world_to_cam) and projected.  The two routes differ by what the render's float32 channels carry (coord.xyz and coord.w are
rounded separately), which nobody had measured; the first run on an MI355X gave a worst difference of
    objects  2.2e-3 px      plane  2.5e-4 px
(MEASURED_OBJECT and MEASURED_PLANE below; the flows themselves reach hundreds of pixels) and the tests bound at four times
that, which must stay under 0.25 px: a convention error (pixel centre, transposed motion, wrong slot) shows as half a pixel or
more."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_flow_ref as R
from stillleben_amd import _abi
from stillleben_amd import render_flow as rf
from test_host_render_flow import ALL, T_FLOW, T_SCENE, bits, as_coord, edge_case, occlusion_case, rigid, same, seeded_case

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0x5B
GUARD = 256
MEASURED_OBJECT, MEASURED_PLANE = 2.2e-3, 2.5e-4      # px, the first device run (see the header)
NAMES = ("flow", "scene_flow", "flags", "counts")


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def to_dev(a, dev):
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(dev)


class Guarded:
    """`nbytes` of poisoned device memory between two poisoned guards"""

    def __init__(self, nbytes, dev):
        self.raw = torch.full((GUARD + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev)
        self.n = nbytes

    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + GUARD)

    def host(self, dtype, shape):
        torch.cuda.synchronize()
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == POISON).all() and (h[GUARD + self.n:] == POISON).all(), "a guard byte was written"
        return h[GUARD:GUARD + self.n].view(dtype).reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == POISON).all())


def run(dev, intr, depth_a, inst_a, table, depth_b=None, inst_b=None, null=(), B=None, stride_a=None, stride_b=None, **kw):
    """slhip_render_flow with every output guarded: (status, {name: Guarded}, the shapes, the record)"""
    Bn, H, W = depth_a.shape[:3]
    S = table.shape[1]
    p = rf.make_params(intr, (W, H), S, **{k: v for k, v in kw.items() if k in ("max_depth", "depth_tol", "depth_rel", "match_instance", "outputs")}).reshape(1)
    for k, v in kw.items():
        if k in p.dtype.names:
            p[k] = v
    shapes = dict(flow=((Bn, H, W, 2), F), scene_flow=((Bn, H, W, 3), F), flags=((Bn, H, W), np.uint8), counts=((Bn, S, 4), np.int32))
    out = {n: Guarded(max(1, int(np.prod(s)) * np.dtype(t).itemsize), dev) for n, (s, t) in shapes.items()}
    d = dict(depth_a=to_dev(depth_a, dev), inst_a=to_dev(inst_a, dev), table=to_dev(table, dev),
             depth_b=None if depth_b is None else to_dev(depth_b, dev), inst_b=None if inst_b is None else to_dev(inst_b, dev))

    def plane(name, a):
        if a is None or name in null:
            return None, 0
        return (d[name].data_ptr() + 12, 4) if a.ndim == 4 else (d[name].data_ptr(), 1)

    pa, sa = plane("depth_a", depth_a)
    pb, sb = plane("depth_b", depth_b)
    ptr = {n: (None if n in null or d[n] is None else d[n].data_ptr()) for n in ("inst_a", "table", "inst_b")}
    outs = [None if n in null else out[n].ptr() for n in NAMES]
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_render_flow(None if "params" in null else p.ctypes.data, pa, sa if stride_a is None else stride_a, ptr["inst_a"],
                                          ptr["table"], pb, sb if stride_b is None else stride_b, ptr["inst_b"], Bn if B is None else B,
                                          *outs, stream(dev))
    torch.cuda.synchronize()
    return st, out, shapes, p[0]


def assert_outputs(out, shapes, want, mask, what):
    """the outputs of `mask` equal `want` (a RenderFlow of numpy arrays) bit for bit, the others are still poison"""
    for k, n in enumerate(NAMES):
        if mask >> k & 1:
            got = out[n].host(shapes[n][1], shapes[n][0])
            w = getattr(want, n)
            diff = bits(got) != bits(w)
            assert not diff.any(), "%s, %s: %d bytes differ, the first at %s" % (what, n, int(diff.sum()), tuple(np.argwhere(diff)[0]))
        else:
            assert out[n].untouched(), (what, n)


# ---- 1. the kernel is the host twin, bit for bit ---------------------------------------------------------------------------------
VARIANTS = [(coord, with_b, with_ib, match) for coord in (False, True) for with_b, with_ib in ((True, True), (True, False), (False, False))
            for match in (True, False)]


@pytest.mark.parametrize("W,H", [(1, 1), (70, 37), (256, 1)])
@pytest.mark.parametrize("S", [1, 3, 256])
def test_kernel_equals_the_host_twin(dev, W, H, S):
    """B = 3, scene 1 with a NaN row.  Every variant (depth as a plane or as the coord target, with and without picture b, its
    instances and the instance condition) with all outputs, then every other subset of the outputs on the variants in turn"""
    depth_a, inst_a, table, depth_b, inst_b = seeded_case(W, H, S)
    intr = (64.0, 61.5, W / 2 + 0.25, H / 2 - 0.125)
    tol = dict(depth_tol=0.01, depth_rel=0.02)
    twins = {}

    def inputs(variant):
        coord, with_b, with_ib, match = variant
        da = as_coord(depth_a) if coord else depth_a
        db = (as_coord(depth_b, 2) if coord else depth_b) if with_b else None
        return da, inst_a, table, db, (inst_b if with_ib else None)

    def twin(variant):
        if variant not in twins:
            da, ia, tb, db, ib = inputs(variant)
            twins[variant] = rf.compute_host(da, ia, tb, intr, db, ib, match_instance=variant[3], outputs=ALL, **tol)
        return twins[variant]

    runs = [(v, 15) for v in VARIANTS] + [(VARIANTS[m % len(VARIANTS)], m) for m in range(1, 15)]
    for variant, mask in runs:
        da, ia, tb, db, ib = inputs(variant)
        st, out, shapes, _ = run(dev, intr, da, ia, tb, db, ib, match_instance=variant[3], outputs=mask, **tol)
        assert st == 0, (variant, mask)
        assert_outputs(out, shapes, twin(variant), mask, "variant %s outputs %d" % (variant, mask))
    full = twin(VARIANTS[0])
    i = inst_a.view(np.uint16).astype(np.int64)
    for b in range(3):                                                          # counts = np.bincount of the flags by slot
        for col, bit in enumerate((0, 1, 2, 4)):
            pick = (i[b] < S) & ((full.flags[b] & bit) != 0 if bit else True)
            assert np.array_equal(full.counts[b, :, col], np.bincount(i[b][pick], minlength=S))
    if S > 1:
        assert not full.counts[1, S // 2, 1:].any()                             # the NaN row


def test_one_slot_owns_the_workgroups(dev):
    """256 x 5 pixels of one instance: every wave adds its counts by ballot, and they say 1280 exactly; mixed waves beside them"""
    depth = np.full((2, 5, 256), 1.25, F)
    inst = np.full((2, 5, 256), 2, np.int16)
    inst[1, :, ::3] = 1
    inst[1, 2, 100:200] = 7                                                    # outside the table
    table = np.zeros((2, 3, 3, 4), F)
    table[..., :3] = np.eye(3)
    table[..., :2, 3] = 1 / 1024                                               # a twentieth of a pixel: nothing leaves, nothing hides
    intr = (64.0, 64.0, 128.0, 2.5)
    st, out, shapes, _ = run(dev, intr, depth, inst, table, depth, inst, outputs=15)
    assert st == 0
    want = rf.compute_host(depth, inst, table, intr, depth, inst, outputs=ALL)
    assert_outputs(out, shapes, want, 15, "uniform waves")
    assert want.counts[0].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1280, 1280, 1280, 1280]] and want.counts[1, :, 0].sum() == 1280 - 100


def test_landings_on_the_border_and_the_exact_occlusion(dev):
    intr, depth, inst, table = edge_case()
    st, out, shapes, _ = run(dev, intr, depth, inst, table, depth, inst, depth_tol=0.0, depth_rel=0.0, outputs=15)
    assert st == 0
    assert_outputs(out, shapes, rf.compute_host(depth, inst, table, intr, depth, inst, depth_tol=0.0, depth_rel=0.0, outputs=ALL), 15, "edge")
    flags = out["flags"].host(np.uint8, (1, 8, 8))
    assert (flags[0, :, 7] == 1).all() and (flags[0, 7, 2:6] == 1).all() and flags[0, 3, 0] == 7 and flags[0, 0, 3] == 7
    intr, depth_a, inst_a, table, depth_b, inst_b = occlusion_case()
    st, out, shapes, _ = run(dev, intr, depth_a, inst_a, table, depth_b, inst_b, depth_tol=0.125, depth_rel=0.0, outputs=15)
    assert st == 0
    assert out["counts"].host(np.int32, (1, 3, 4)).tolist() == [[[1728, 1728, 1728, 1503], [256, 256, 256, 256], [64, 64, 0, 0]]]
    assert_outputs(out, shapes, rf.compute_host(depth_a, inst_a, table, intr, depth_b, inst_b, depth_tol=0.125, depth_rel=0.0, outputs=ALL), 15, "occlusion")


def test_refusals_leave_the_device_untouched(dev):
    depth_a, inst_a, table, depth_b, inst_b = seeded_case(70, 37, 3)
    intr = (64.0, 64.0, 35.0, 18.5)
    for kw in (dict(null=("params",)), dict(null=("depth_a",)), dict(null=("inst_a",)), dict(null=("table",)), dict(null=("flow",)),
               dict(null=("scene_flow",)), dict(null=("flags",)), dict(null=("counts",)), dict(stride_a=0), dict(stride_b=0), dict(B=65536),
               dict(n_slots=0), dict(n_slots=257), dict(outputs=0), dict(outputs=16), dict(W=0), dict(H=32769), dict(fx=0.0),
               dict(max_depth=0.0), dict(depth_tol=-1.0), dict(depth_rel=np.inf), dict(flags=2)):
        kw.setdefault("outputs", 15)
        st, out, shapes, _ = run(dev, intr, depth_a, inst_a, table, depth_b, inst_b, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in out.values()), kw
    assert b"" != _abi.lib().slhip_last_error()
    st, out, shapes, _ = run(dev, intr, depth_a, inst_a, table, depth_b, inst_b, B=0, outputs=15)      # no scenes: fine, nothing is written
    assert st == 0 and all(o.untouched() for o in out.values())


def test_motion_kernel_equals_its_twin(dev):
    rng = np.random.default_rng(5)
    n = 700                                                                    # three workgroups, the last one partly filled
    a, b = rigid(rng, 3.0, 2.0, n).astype(F), rigid(rng, 3.0, 2.0, n).astype(F)
    a[3, 1, 2], b[9, 2, 3], a[300, 0, 0], b[699, 1, 1] = np.nan, np.inf, -np.inf, np.nan
    out = Guarded(n * 48, dev)
    d_a, d_b = to_dev(a, dev), to_dev(b, dev)
    with torch.cuda.device(dev):
        assert _abi.lib().slhip_render_flow_motion(d_a.data_ptr(), d_b.data_ptr(), n, out.ptr(), stream(dev)) == 0
    want = rf.motion_host(a, b)
    assert same(out.host(F, (n, 3, 4)), want) and np.isnan(want[[3, 9, 300, 699]]).all()
    untouched = Guarded(n * 48, dev)
    with torch.cuda.device(dev):
        assert _abi.lib().slhip_render_flow_motion(d_a.data_ptr(), d_b.data_ptr(), 0, untouched.ptr(), stream(dev)) == 0
        assert _abi.lib().slhip_render_flow_motion(None, d_b.data_ptr(), n, untouched.ptr(), stream(dev)) < 0
        assert _abi.lib().slhip_render_flow_motion(d_a.data_ptr(), d_b.data_ptr(), n, None, stream(dev)) < 0
    assert untouched.untouched()
    t_a, t_b = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    got = rf.motion(t_a.view(7, 100, 3, 4), t_b.view(7, 100, 3, 4))             # the Python surface, [..., 3, 4] and [..., 4, 4]
    assert tuple(got.shape) == (7, 100, 3, 4) and same(got.cpu().numpy().reshape(n, 3, 4), want)
    four = torch.cat([t_a, torch.tensor([[[0.0, 0, 0, 1]]], device=dev).expand(n, 1, 4)], dim=1)
    assert same(rf.motion(four, t_b).cpu().numpy(), want)
    with pytest.raises(ValueError):
        rf.motion(t_a, t_b[:5])


# ---- 2. end to end ---------------------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 2, 3, (320, 240), (533.4, 533.7, 156.5, 120.6)


def np_state(state):
    return state.object_to_camera.cpu().numpy(), state.world_to_cam.cpu().numpy()


def host_buffers(bufs):
    return bufs.coord.cpu().numpy(), bufs.instance.cpu().numpy()[..., 0]


@pytest.fixture(scope="module")
def pictures(sl):
    """the batch of the regions' and keypoints' device tests (three cubes, two scenes, 320 x 240, settle(frames=5)): view 0 rendered
    twice, view 1, and -- same camera -- the pile settled until it rests and then five frames more"""
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
    p = {"batch": batch}
    batch.place(object_to_camera=True)
    p["a"], p["state_a"] = batch.render(0, object_stats=True), batch.view_state()
    p["a2"] = batch.render(0)
    p["same"] = batch.flow(p["a"], p["state_a"], p["a2"], outputs=ALL)
    cameras = torch.from_numpy(batch.host_cameras()).to(batch.eng.device)
    batch.place(view=1, object_to_camera=True)
    p["b"] = batch.render(0)
    p["a_to_b"] = batch.flow(p["a"], p["state_a"], p["b"], outputs=ALL)        # state_b = None: the view now placed
    p["state_b"] = batch.view_state()
    batch.settle(frames=200)
    batch.place(camera_poses=cameras, object_to_camera=True)
    p["c"], p["state_c"] = batch.render(0), batch.view_state()
    batch.settle(frames=5)
    batch.place(camera_poses=cameras, object_to_camera=True)
    p["d"], p["state_d"] = batch.render(0), batch.view_state()
    p["c_to_d"] = batch.flow(p["c"], p["state_c"], p["d"], outputs=ALL)
    p["c_to_c"] = batch.flow(p["c"], p["state_c"], p["c"], p["state_c"], outputs=ALL)
    torch.cuda.synchronize()
    return p


def test_the_same_view_twice(pictures):
    f, a = pictures["same"], pictures["a"]
    flow, flags, counts = f.flow.cpu().numpy(), f.flags.cpu().numpy(), f.counts.cpu().numpy()
    assert tuple(flow.shape) == (N_SCENES, RES[1], RES[0], 2) and tuple(counts.shape) == (N_SCENES, N_OBJ + 1, 4)
    worst = float(np.abs(flow).max())
    print("the same view twice: |flow| <= %.3g px (bound %.3g)" % (worst, T_FLOW))
    assert worst <= T_FLOW
    assert np.abs(f.scene_flow.cpu().numpy()).max() <= T_SCENE
    valid = (flags & 1) != 0
    assert (flags[valid] == 7).all() and bool(f.visible.equal(f.valid)) and not bool(f.occluded.any())
    coord, inst = host_buffers(a)
    assert np.array_equal(valid, (coord[..., 3] < 3000.0) & (inst <= N_OBJ))      # everything but the background
    stats = a.object_stats.records().cpu().numpy().view(_abi.OBJECT_STATS_DTYPE).reshape(N_SCENES, N_OBJ + 1)
    assert np.array_equal(counts[:, 1:, 0], stats["px_visib"][:, 1:].astype(np.int32)) and counts[:, 1:, 0].sum() > 20000
    assert np.array_equal(counts[:, 1:, 0], counts[:, 1:, 3]) and np.array_equal(counts[:, 0, 1], counts[:, 0, 3])      # (slot 0 counts the background too)
    cov = f.covisibility().cpu().numpy()
    assert (cov[counts[:, :, 1] > 0] == 1.0).all()


def independent_route(coord_a, inst_a, o2c_b, w2c_a, w2c_b, intr):
    """float64, none of the library's steps: object pixels -- coord_a.xyz (the object frame) by object_to_camera of view b; plane
    pixels -- the camera point of a back to the world by inv(world_to_cam a), on by world_to_cam b.  (u, v) per pixel, NaN
    elsewhere."""
    fx, fy, cx, cy = (float(F(v)) for v in intr)
    B, H, W = inst_a.shape
    uv = np.full((B, H, W, 2), np.nan)
    px, py = (np.arange(W) + 0.5)[None, :], (np.arange(H) + 0.5)[:, None]
    bottom = np.array([[0.0, 0, 0, 1]])
    for b in range(B):
        for o in range(o2c_b.shape[1]):
            m = inst_a[b] == o + 1
            P = coord_a[b][m][:, :3].astype(np.float64) @ o2c_b[b, o, :, :3].astype(np.float64).T + o2c_b[b, o, :, 3].astype(np.float64)
            uv[b][m] = np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], axis=-1)
        m = (inst_a[b] == 0) & (coord_a[b][..., 3] < 3000.0)
        z = coord_a[b][..., 3].astype(np.float64)
        cam = np.stack([(px - cx) * z / fx, (py - cy) * z / fy, z, np.ones_like(z)], axis=-1)[m]
        A = np.concatenate([w2c_a[b].astype(np.float64), bottom])
        Bm = np.concatenate([w2c_b[b].astype(np.float64), bottom])
        P = cam @ (Bm @ np.linalg.inv(A)).T
        uv[b][m] = np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], axis=-1)
    return uv


def test_view_0_against_view_1(pictures):
    f, batch = pictures["a_to_b"], pictures["batch"]
    coord_a, inst_a = host_buffers(pictures["a"])
    coord_b, inst_b = host_buffers(pictures["b"])
    o2c_a, w2c_a = np_state(pictures["state_a"])
    o2c_b, w2c_b = np_state(pictures["state_b"])
    assert not np.array_equal(w2c_a, w2c_b)                                      # another camera
    # (1) the library is the restatement run on the downloaded buffers, bit for bit
    table = np.concatenate([R.motion(w2c_a, w2c_b)[:, None], R.motion(o2c_a, o2c_b)], axis=1)
    want = R.flow(f.params, coord_a, inst_a, table, coord_b, inst_b)
    for name, w in zip(ALL, want):
        assert same(getattr(f, name).cpu().numpy(), w), name
    flags, counts = want[2], want[3]
    assert (counts[:, 0, 1] > 0).all() and counts[:, 1:, 1].sum() > 20000 and (counts[:, 1:, 3] > 0).any() and (counts[:, :, 3] <= counts[:, :, 2]).all()
    assert 0 < int(f.occluded.sum()) < int(f.inside.sum())                      # another view hides something, not everything
    # (2) the independent float64 route
    uv = independent_route(coord_a, inst_a, o2c_b, w2c_a, w2c_b, INTRINSICS)
    px, py = (np.arange(RES[0]) + 0.5)[None, None, :], (np.arange(RES[1]) + 0.5)[None, :, None]
    landed = want[0].astype(np.float64) + np.stack(np.broadcast_arrays(px, py, inst_a)[:2], axis=-1)
    valid = (flags & 1) != 0
    objects, plane = valid & (inst_a >= 1), valid & (inst_a == 0)
    assert objects.sum() > 20000 and plane.sum() > 20000 and np.isfinite(uv[valid]).all()
    worst_o, worst_p = float(np.abs(landed - uv)[objects].max()), float(np.abs(landed - uv)[plane].max())
    print("view 0 -> view 1 against the float64 route: objects %.3g px, plane %.3g px; the largest flow %.3g px"
          % (worst_o, worst_p, float(np.abs(want[0]).max())))
    assert 4 * MEASURED_OBJECT < 0.25 and 4 * MEASURED_PLANE < 0.25
    assert worst_o <= 4 * MEASURED_OBJECT and worst_p <= 4 * MEASURED_PLANE
    assert np.abs(want[0][valid]).max() > 5.0                                   # the views differ by many pixels: the test has teeth


def test_the_pile_settled_further(pictures):
    f, still = pictures["c_to_d"], pictures["c_to_c"]
    o2c_c, w2c_c = np_state(pictures["state_c"])
    o2c_d, w2c_d = np_state(pictures["state_d"])
    assert same_bits(w2c_c, w2c_d)                                              # the same camera
    coord_c, inst_c = host_buffers(pictures["c"])
    flow, flags = f.flow.cpu().numpy(), f.flags.cpu().numpy()
    # slot 0 is exactly the identity's result: the plane's pixels get what the same picture against itself gives them
    plane = inst_c == 0
    assert same(flow[plane], still.flow.cpu().numpy()[plane]) and same(f.scene_flow.cpu().numpy()[plane], still.scene_flow.cpu().numpy()[plane])
    assert np.array_equal(flags[plane] & 3, still.flags.cpu().numpy()[plane] & 3)
    assert np.abs(flow[plane]).max() <= T_FLOW
    asleep = [(b, o) for b in range(N_SCENES) for o in range(N_OBJ) if same_bits(o2c_c[b, o], o2c_d[b, o])]
    print("asleep after 205 frames: %d of %d objects" % (len(asleep), N_SCENES * N_OBJ))
    assert asleep, "no object of the pile rests after 205 frames: the case shows nothing"
    for b, o in asleep:
        mine = inst_c[b] == o + 1
        if mine.any():
            assert np.abs(flow[b][mine]).max() <= T_FLOW and (flags[b][mine] & 1).all(), (b, o)
    # and the whole of it is the restatement
    table = np.concatenate([R.motion(w2c_c, w2c_d)[:, None], R.motion(o2c_c, o2c_d)], axis=1)
    coord_d, inst_d = host_buffers(pictures["d"])
    for name, w in zip(ALL, R.flow(f.params, coord_c, inst_c, table, coord_d, inst_d)):
        assert same(getattr(f, name).cpu().numpy(), w), name


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def test_flow_argument_errors(pictures, sl):
    batch, a, state_a, b = pictures["batch"], pictures["a"], pictures["state_a"], pictures["b"]
    for name in ("intrinsics", "motion"):
        with pytest.raises(TypeError) as e:
            batch.flow(a, state_a, b, **{name: None})
        assert "sets `%s` itself" % name in str(e.value)
    small = type("Buffers", (), {"coord": a.coord[:1], "instance": a.instance[:1]})()
    with pytest.raises(IndexError) as e:
        batch.flow(small, state_a, b)
    assert "fewer scenes" in str(e.value)
    with pytest.raises(IndexError):
        batch.flow(a, state_a, b, chunk=1)
    none = type("Buffers", (), {"coord": None, "instance": a.instance})()
    with pytest.raises(RuntimeError):
        batch.flow(none, state_a, b)
    batch.place()                                                              # a place() that does not keep object_to_camera
    with pytest.raises(RuntimeError) as e:
        batch.view_state()
    assert "place(object_to_camera=True)" in str(e.value)
    with pytest.raises(RuntimeError):
        batch.flow(a, state_a, b)                                              # state_b = None reads the view now placed
    out = batch.flow(a, state_a, b, pictures["state_b"], outputs=("flags",))   # with both states it needs nothing of the batch's view
    assert out.flow is None and out.counts is None and bool(out.flags.equal(pictures["a_to_b"].flags))
    # the plain surface: shapes, dtypes and devices
    dev = a.coord.device
    table = torch.zeros((N_SCENES, 2, 3, 4), device=dev)
    for bad in (dict(depth_a=a.coord.double()), dict(depth_a=a.coord[..., :3]), dict(instance_a=a.instance.int()), dict(instance_a=a.instance[:1]),
                dict(motion=table[:1]), dict(motion=table[..., :3]), dict(depth_b=a.coord[:, ::2]), dict(instance_b=a.instance[:, :, ::2])):
        kw = dict(depth_a=a.coord, instance_a=a.instance, motion=table, intrinsics=INTRINSICS)
        kw.update(bad)
        with pytest.raises(ValueError):
            rf.compute(**kw)
    with pytest.raises(_abi.SlhipError) as e:
        rf.compute(a.coord, a.instance, torch.zeros((N_SCENES, 257, 3, 4), device=dev), INTRINSICS)
    assert "n_slots" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        rf.compute(a.coord, a.instance, table.cpu(), INTRINSICS)
    r = rf.compute(a.coord[..., 3].contiguous(), a.instance[..., 0].contiguous(), table, INTRINSICS)      # planes; the defaults: flow and flags
    assert r.scene_flow is None and r.counts is None and tuple(r.flow.shape) == (N_SCENES, RES[1], RES[0], 2) and not bool(r.valid.any())
