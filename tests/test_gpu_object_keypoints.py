"""Object keypoints on the device (slhip_object_keypoints_fps, _project, _field, sl.object_keypoints, SceneBatch.keypoints)
against the NumPy restatement tests/object_keypoints_ref.py.  Every comparison with the restatement is bit for bit -- floats as
their int32 views; every output lies between poisoned guard bytes that must stay poison."""
import ctypes as C

import numpy as np
import pytest
import torch

import object_keypoints_ref as R
from stillleben_amd import _abi
from stillleben_amd import object_keypoints as ok
from test_host_object_keypoints import cloud

pytestmark = pytest.mark.gpu

F = np.float32
K4 = (61.5, 60.25, 27.125, 17.75)
POISON = 0x5B
GUARD = 256      # bytes of poison before and after every output (a multiple of the 16-byte alignment the wide stores want)


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class Guarded:
    """`nbytes` of device memory between two guards, everything poisoned"""

    def __init__(self, nbytes, dev, offset=0):
        self.raw = torch.full((GUARD + offset + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev)
        self.lo, self.n = GUARD + offset, nbytes

    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + self.lo)

    def host(self, dtype, shape):
        torch.cuda.synchronize()
        h = self.raw.cpu().numpy()
        assert (h[:self.lo] == POISON).all() and (h[self.lo + self.n:] == POISON).all(), "a guard byte was written"
        return h[self.lo:self.lo + self.n].view(dtype).reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == POISON).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def to_dev(a, dev):
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(dev)


# ---- 1. FPS ----------------------------------------------------------------------------------------------------------------------
def fps_pool():
    """Four classes with 0, 1, 70 and 2 500 vertices in one pool, each at its own non-zero vtx_base with vertices of nobody
    between them, each under its own non-identity mesh_to_object.  70 is ragged against a wave and holds duplicates on either
    side of the wave's end; 2 500 takes three strides of the workgroup and ties across waves and strides (cloud())."""
    rng = np.random.default_rng(4)
    small = (rng.integers(-64, 65, (70, 3)) / 32.0).astype(F)
    small[66], small[3] = [2.5, -2.5, 2.5], [2.5, -2.5, 2.5]               # the farthest position in lane 3 of wave 0 and lane 2 of wave 1
    small[69] = [-2.5, 2.5, -2.5]                                          # its mirror in the last lane in use
    parts = [(13, np.zeros((0, 3), F)), (5, np.array([[0.5, -1.0, 2.0]], F)), (3, small), (11, cloud())]
    pos, assets, templates = [], np.zeros(4, _abi.ASSET_DTYPE), np.zeros(5, _abi.DRAW_DTYPE)
    at = 0
    for c, (pad, p) in enumerate(parts):
        pos.append(np.full((pad, 3), 1e9, F))
        at += pad
        m = np.eye(4, dtype=F)
        m[:3, :3] = [[[0, 0.5, 0], [0, 0, 2], [1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0.5, 0, 0], [0, 2, 0], [0, 0, 1]],
                     [[0, 0.5, 0], [0, 0, 2], [1, 0, 0]]][c]
        m[:3, 3] = [0.25, -0.5, 0.125]
        assets[c]["mesh_to_object"] = m.reshape(-1)
        # a box whose centre is the image of the mesh's origin: the mirror images tie to the bit
        assets[c]["bbox_min"][:3], assets[c]["bbox_max"][:3] = m[:3, 3] - F(1.5), m[:3, 3] + F(1.5)
        assets[c]["draw_begin"], assets[c]["draw_count"], assets[c]["n_verts"] = c + 1, 1, len(p)      # template 0 is nobody's
        templates[c + 1]["vtx_base"], templates[c + 1]["n_verts"] = at, len(p)
        pos.append(p)
        at += len(p)
    pos.append(np.full((9, 3), 1e9, F))
    pos = np.concatenate(pos)
    return np.concatenate([pos, np.ones((len(pos), 1), F)], axis=1).astype(F), assets, templates


def run_fps(dev, pool, assets, templates, n_fps, max_verts):
    A = len(assets)
    d_pos, d_assets, d_templates = to_dev(pool, dev), to_dev(assets, dev), to_dev(templates, dev)
    nbytes = C.c_uint64(0)
    L = _abi.lib()
    assert L.slhip_object_keypoints_fps_bytes(A, max_verts, C.byref(nbytes)) == 0 and nbytes.value == A * max_verts * 4
    scratch, kps, idx = Guarded(int(nbytes.value), dev), Guarded(A * n_fps * 16, dev), Guarded(A * n_fps * 4, dev)
    with torch.cuda.device(dev):
        st = L.slhip_object_keypoints_fps(C.c_void_p(d_pos.data_ptr()), len(pool), C.c_void_p(d_assets.data_ptr()), A,
                                          C.c_void_p(d_templates.data_ptr()), len(templates), n_fps, max_verts, scratch.ptr(),
                                          kps.ptr(), idx.ptr(), stream(dev))
    return st, scratch, kps, idx


def test_fps_four_classes(dev):
    pool, assets, templates = fps_pool()
    st, scratch, kps, idx = run_fps(dev, pool, assets, templates, 8, 2500)
    assert st == 0
    got_k, got_i = kps.host(F, (4, 8, 4)), idx.host(np.int32, (4, 8))
    scratch.host(F, (4, 2500))                                              # (its guards)
    want_k, want_i = R.fps(pool, assets, templates, 8)
    assert np.array_equal(got_i, want_i), (got_i, want_i)
    assert np.array_equal(bits(got_k), bits(want_k))
    host_k, host_i = ok.fps_host(pool, assets, templates, 8)                # and the host entry says the same
    assert np.array_equal(got_i, host_i) and np.array_equal(bits(got_k), bits(host_k))
    assert (got_i[0] == -1).all() and (got_i[1] == 0).all()                 # no vertices; one vertex, repeated
    assert got_i[2, 0] == 3 and got_i[3, 0] == 5                            # ties across waves and strides: the lowest index
    assert len(set(got_i[2].tolist())) == 8 and len(set(got_i[3].tolist())) == 8


def test_fps_row_limit_and_refusals(dev):
    pool, assets, templates = fps_pool()
    st, scratch, kps, idx = run_fps(dev, pool, assets, templates, 4, 70)     # the 2 500 do not fit a row of 70: no vertices
    assert st == 0
    got_i = idx.host(np.int32, (4, 4))
    want_k, want_i = R.fps(pool, assets[:3], templates, 4)
    assert np.array_equal(got_i[:3], want_i) and (got_i[3] == -1).all()
    assert np.array_equal(bits(kps.host(F, (4, 4, 4))[:3]), bits(want_k))
    scratch.host(F, (4, 70))
    L = _abi.lib()
    out = Guarded(64, dev)
    for n_fps, n_assets in ((0, 4), (33, 4), (8, 0)):
        with torch.cuda.device(dev):
            assert L.slhip_object_keypoints_fps(out.ptr(), 4, out.ptr(), n_assets, out.ptr(), 1, n_fps, 4, out.ptr(), out.ptr(), out.ptr(),
                                                stream(dev)) < 0
    with torch.cuda.device(dev):
        assert L.slhip_object_keypoints_fps(out.ptr(), 4, None, 1, out.ptr(), 1, 8, 4, out.ptr(), out.ptr(), out.ptr(), stream(dev)) < 0
        assert L.slhip_object_keypoints_fps(out.ptr(), 4, out.ptr(), 1, out.ptr(), 1, 8, 4, out.ptr(), None, out.ptr(), stream(dev)) < 0
    assert out.untouched()


# ---- 2. projection ---------------------------------------------------------------------------------------------------------------
W, H = 53, 37
TOL = 0.25


def project_case():
    """B = 2, O = 3, Kp = 5.  Object (0, 0) stands at Z = fx = 61.5 under the identity, so u = X + cx to the bit: keypoint 0
    lands on u = 0 exactly (inside), keypoint 1 on u = W exactly (outside), 2 has Z = 0, 3 has Z < 0, 4 is an ordinary one.
    (0, 1) and (1, 2) are general poses, (0, 2) a pose with a NaN, (1, 0) names an asset the bank does not have, (1, 1) is
    asset 0 again, shifted."""
    bank = np.ones((2, 5, 4), F)
    bank[0, :, :3] = [[-27.125, 0, 0], [25.875, 0, 0], [0, 0, -61.5], [0, 0, -100], [1.5, -2.25, 0]]
    bank[1, :, :3] = np.random.default_rng(8).uniform(-0.2, 0.2, (5, 3))
    ids = np.array([[0, 1, 0], [7, 0, 1]], np.uint32)
    o2c = np.zeros((2, 3, 3, 4), F)
    o2c[0, 0] = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 61.5]]
    c, s = np.cos(0.7), np.sin(0.7)
    o2c[0, 1] = [[c, -s, 0, 0.31], [s * 0.8, c * 0.8, -0.6, -0.17], [s * 0.6, c * 0.6, 0.8, 2.9]]
    o2c[0, 2] = o2c[0, 1]
    o2c[0, 2, 1, 2] = np.nan
    o2c[1, 0] = o2c[0, 0]
    o2c[1, 1] = [[1, 0, 0, 3.0], [0, 1, 0, -5.5], [0, 0, 1, 70.25]]
    o2c[1, 2] = [[0, 0, 1, -0.4], [0, 1, 0, 0.21], [-1, 0, 0, 1.7]]
    return bank, ids, o2c


def depth_plane(bank, ids, o2c):
    """a far plane (everything unoccluded) with, under chosen keypoints: an occluder, a hole, and a surface exactly depth_tol
    in front of the keypoint"""
    cam, uv, flags = R.project(bank, ids, o2c, K4, (W, H))
    plane = np.full((2, H, W), 1000.0, F)

    def under(b, o, k):
        assert flags[b, o, k] & R.INSIDE
        return b, int(np.floor(uv[b, o, k, 1])), int(np.floor(uv[b, o, k, 0]))

    plane[under(0, 0, 0)] = 10.0                                            # an occluder in front of the keypoint on u = 0
    plane[under(0, 0, 4)] = cam[0, 0, 4, 2] - F(TOL)                        # Z == z + depth_tol exactly (61.25 + 0.25): unoccluded
    plane[under(1, 1, 4)] = 0.0                                             # a hole of a sensor's plane
    k = int(np.flatnonzero(flags[0, 1] & R.INSIDE)[0])
    plane[under(0, 1, k)] = np.nextafter(F(cam[0, 1, k, 2] - F(TOL)), F(0))      # one step too near: occluded
    return plane


def run_project(dev, bank, ids, o2c, depth=None, stride=1, n_assets=None, tol=TOL, Kp=None, null=None):
    B, O = ids.shape
    Kp = bank.shape[1] if Kp is None else Kp
    objs = np.zeros((B, O), _abi.SYNTH_OBJECT_DTYPE)
    objs["asset"], objs["instance_index"], objs["metallic"] = ids, 0x7fffffff, np.nan      # only .asset is read
    d_bank, d_objs, d_o2c = to_dev(bank, dev), to_dev(objs, dev), to_dev(o2c, dev)
    d_depth = None if depth is None else to_dev(depth, dev)
    n = B * O * Kp
    cam, uv, flags = Guarded(n * 16, dev), Guarded(n * 8, dev), Guarded(n, dev)
    p = ok.make_params(K4, (W, H), Kp, O, depth_tol=tol).reshape(1)
    args = dict(bank=C.c_void_p(d_bank.data_ptr()), objs=C.c_void_p(d_objs.data_ptr()), o2c=C.c_void_p(d_o2c.data_ptr()),
                cam=cam.ptr(), uv=uv.ptr(), flags=flags.ptr())
    if null:
        args[null] = None
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_object_keypoints_project(p.ctypes.data, args["bank"], bank.shape[0] if n_assets is None else n_assets,
                                                       args["objs"], args["o2c"], B,
                                                       None if d_depth is None else C.c_void_p(d_depth.data_ptr() + (12 if stride == 4 else 0)),
                                                       stride, args["cam"], args["uv"], args["flags"], stream(dev))
    return st, cam, uv, flags, (B, O, Kp)


@pytest.mark.parametrize("plane", ["none", "stride1", "stride4"])
def test_project(dev, plane):
    bank, ids, o2c = project_case()
    depth, flat, stride = None, None, 1
    if plane != "none":
        flat = depth_plane(bank, ids, o2c)
        depth = flat
        if plane == "stride4":                                              # the w of a coord-like target, read in place
            stride = 4
            depth = np.full((2, H, W, 4), np.nan, F)
            depth[..., 3] = flat
    st, cam, uv, flags, shape = run_project(dev, bank, ids, o2c, depth, stride)
    assert st == 0
    got = cam.host(F, shape + (4,)), uv.host(F, shape + (2,)), flags.host(np.uint8, shape)
    want = R.project(bank, ids, o2c, K4, (W, H), None if flat is None else flat.reshape(-1), 1, TOL)
    for g, w, name in zip(got, want, ("camera", "uv", "flags")):
        assert np.array_equal(bits(g), bits(w)), name
    f = got[2]
    un = R.UNOCCLUDED if plane != "none" else 0
    assert f[0, 0].tolist() == [3, 1, 0, 0, 3 | un]                         # occluded on u = 0; u = W is outside; Z = 0; Z < 0; at the tolerance
    assert got[1][0, 0, 0, 0] == 0.0 and got[1][0, 0, 1, 0] == float(W)
    assert (f[0, 2] == 0).all() and (f[1, 0] == 0).all()                    # the NaN pose; the asset outside the bank
    assert not got[0][0, 2].any() and not got[1][0, 2].any() and not got[0][1, 0].any()
    assert not got[0][0, 0, 2].any() and not got[1][0, 0, 3].any()          # not in front: zeros
    if plane != "none":
        assert f[1, 1, 4] == 3                                              # the hole
        k = int(np.flatnonzero(f[0, 1] & R.INSIDE)[0])
        assert f[0, 1, k] == 3                                              # one step nearer than the tolerance
        assert ((f & 3) == 3).sum() > (f == 7).sum() > 4


def test_project_refusals_leave_the_device_untouched(dev):
    bank, ids, o2c = project_case()
    for kw in (dict(null="bank"), dict(null="objs"), dict(null="o2c"), dict(null="cam"), dict(null="uv"), dict(null="flags"),
               dict(Kp=33), dict(tol=-1.0), dict(n_assets=0), dict(depth=np.zeros((2, H, W), F), stride=0)):
        st, cam, uv, flags, _ = run_project(dev, bank, ids, o2c, **kw)
        assert st < 0, kw
        assert cam.untouched() and uv.untouched() and flags.untouched(), kw
    assert b"" != _abi.lib().slhip_last_error()


def test_step_timer_reads_an_untimed_step_as_minus_one(dev):
    """slhip_object_keypoints_timings (the step timer under the keypoints' convention): -1.0 for a step that was not timed
    since the last timing_enable(1); a call refused by its checks leaves the flags as they were."""
    bank, ids, o2c = project_case()
    L = _abi.lib()
    ms = (C.c_float * 3)()

    def read():
        assert L.slhip_object_keypoints_timings(C.byref(ms)) == 0
        return list(ms)

    try:
        assert L.slhip_object_keypoints_timing_enable(1) == 0
        assert run_project(dev, bank, ids, o2c, Kp=33)[0] < 0
        assert read() == [-1.0, -1.0, -1.0]
        assert run_project(dev, bank, ids, o2c)[0] == 0                     # project alone
        t = read()
        assert t[0] == -1.0 and t[2] == -1.0 and np.isfinite(t[1]) and t[1] >= 0.0
        assert run_project(dev, bank, ids, o2c, tol=-1.0)[0] < 0
        t = read()
        assert t[0] == -1.0 and t[2] == -1.0 and np.isfinite(t[1]) and t[1] >= 0.0
        assert L.slhip_object_keypoints_timing_enable(1) == 0               # clears the flags
        assert read() == [-1.0, -1.0, -1.0]
    finally:
        L.slhip_object_keypoints_timing_enable(0)


# ---- 3. field --------------------------------------------------------------------------------------------------------------------
FH, FW, FO = 19, 37, 3


def field_case(Kp):
    """A 2 x 19 x 37 picture of 3 objects: instances 0, -1 and n_objects + 1 among the objects' own; keypoint 0 of object 1 lies
    exactly on the centre of a pixel that shows object 1 (l == 0); the last keypoint of object 0 is behind the camera (no flag,
    a uv that would show if it were read)."""
    rng = np.random.default_rng(21 + Kp)
    inst = rng.choice(np.array([-1, 0, 0, 1, 2, 3, 4], np.int16), (2, FH, FW))
    uv = rng.uniform(-20, 60, (2, FO, Kp, 2)).astype(F)
    flags = rng.choice(np.array([1, 3, 7], np.uint8), (2, FO, Kp))
    uv[:, 1, 0] = [10.5, 7.5]
    inst[:, 7, 10] = 2
    flags[:, 1, 0] = 3
    flags[:, 0, Kp - 1] = 0
    uv[:, 0, Kp - 1] = [123.0, -45.0]
    if Kp > 1:
        flags[1, 2, 1] = 2                                                  # bits without bit 1 do not count
    return inst, uv, flags


def run_field(dev, inst, uv, flags, mode, first, count, slots=None, offset=0, Kp=None, null=None, n_scenes=None):
    B, O, K = flags.shape
    Kp = K if Kp is None else Kp
    slots = count if slots is None else slots
    d_inst, d_uv, d_flags = to_dev(inst, dev), to_dev(uv, dev), to_dev(flags, dev)
    out = Guarded(slots * FH * FW * K * 8, dev, offset)
    p = ok.make_params(K4, (FW, FH), Kp, O, mode=mode).reshape(1)
    args = dict(inst=C.c_void_p(d_inst.data_ptr()), uv=C.c_void_p(d_uv.data_ptr()), flags=C.c_void_p(d_flags.data_ptr()), out=out.ptr())
    if null:
        args[null] = None
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_object_keypoints_field(p.ctypes.data, args["inst"], args["uv"], args["flags"], B if n_scenes is None else n_scenes,
                                                     first, count, args["out"], stream(dev))
    return st, out


@pytest.mark.parametrize("mode", ["offset", "unit"])
@pytest.mark.parametrize("Kp", [1, 4, 5])      # 4: a scene's pairs are even, the 16-byte stores; 1 and 5: odd, the 8-byte ones
def test_field(dev, Kp, mode):
    inst, uv, flags = field_case(Kp)
    want = R.field(inst, uv, flags, ok.MODES[mode])
    assert want[:, 7, 10, 0].tolist() == [[0.0, 0.0]] * 2 and not want[:, :, :, Kp - 1][inst == 1].any()
    assert not want[(inst < 1) | (inst > FO)].any() and want[(inst >= 1) & (inst <= FO)].any()
    # the whole picture
    st, out = run_field(dev, inst, uv, flags, mode, 0, 2)
    assert st == 0
    got = out.host(F, (2, FH, FW, Kp, 2))
    diff = (got.view(np.int32) != want.view(np.int32))
    assert not diff.any(), "%d of %d floats differ, the first at %s" % (int(diff.sum()), diff.size, tuple(np.argwhere(diff)[0]))
    # range (1, 1) into a buffer of three slices, starting 8 bytes off a 16-byte boundary as well: the bytes around stay poison
    for offset in (0, 8):
        st, out = run_field(dev, inst, uv, flags, mode, 1, 1, slots=3, offset=offset)
        assert st == 0
        got = out.host(F, (3, FH, FW, Kp, 2))
        assert np.array_equal(got[0].view(np.int32), want[1].view(np.int32))
        assert (bits(got[1:]) == POISON).all()


def test_field_stores_are_wide_on_an_even_picture(dev):
    """38 columns: every Kp gives an even number of pairs, so Kp = 5 takes the 16-byte stores with lanes that span two pixels
    and two rows"""
    rng = np.random.default_rng(3)
    inst = rng.integers(-1, 5, (2, 7, 38)).astype(np.int16)
    uv = rng.uniform(-20, 60, (2, FO, 5, 2)).astype(F)
    flags = rng.choice(np.array([0, 1, 3], np.uint8), (2, FO, 5))
    want = R.field(inst, uv, flags, R.UNIT)
    d_inst, d_uv, d_flags = to_dev(inst, dev), to_dev(uv, dev), to_dev(flags, dev)
    out = Guarded(2 * 7 * 38 * 5 * 8, dev)
    p = ok.make_params(K4, (38, 7), 5, FO, mode="unit").reshape(1)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_object_keypoints_field(p.ctypes.data, C.c_void_p(d_inst.data_ptr()), C.c_void_p(d_uv.data_ptr()),
                                                     C.c_void_p(d_flags.data_ptr()), 2, 0, 2, out.ptr(), stream(dev))
    assert st == 0
    assert np.array_equal(out.host(F, want.shape).view(np.int32), want.view(np.int32))


def test_field_refusals_leave_the_device_untouched(dev):
    inst, uv, flags = field_case(5)
    for kw in (dict(null="inst"), dict(null="uv"), dict(null="flags"), dict(null="out"), dict(Kp=33), dict(first=2, count=1),
               dict(first=1, count=2), dict(first=0, count=3), dict(first=0xFFFFFFFF, count=2), dict(offset=4)):
        first, count = kw.pop("first", 0), kw.pop("count", 1)
        st, out = run_field(dev, inst, uv, flags, "unit", first, count, slots=1, **kw)
        assert st < 0, kw
        assert out.untouched(), kw
    st, out = run_field(dev, inst, uv, flags, "unit", 2, 0, slots=1)      # an empty range at the end is fine, and writes nothing
    assert st == 0 and out.untouched()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 2, 3, (320, 240), (533.4, 533.7, 156.5, 120.6)


@pytest.fixture(scope="module")
def rendered(sl):
    meshes = []
    for i in range(3):
        import scenes as S

        m = sl.Mesh(S.CUBE)
        m.center_bbox()
        m.scale_to_bbox_diagonal(0.12 + 0.05 * i)
        m.class_index = i + 1
        meshes.append(m)
    table = sl.AssetTable(meshes)
    # seed: checked with the host cameras and poses (the CPU oracle's stage, settle and place of these records): scene 0 shows
    # all eight corners of three cubes inside the picture, scene 1 of two
    batch = sl.SceneBatch(table, N_SCENES, N_OBJ, resolution=RES, seed=(77 << 32) | 5, render_chunk=N_SCENES, manual_exposure=1.0,
                          scene_id_base=1000)
    batch.set_camera_intrinsics(*INTRINSICS)
    batch.stage()
    batch.settle(frames=5)
    batch.place(object_to_camera=True)
    bufs = batch.render(0, object_masks=True)
    bank = sl.object_keypoints.bank(table, 8, corners=True)
    kps = batch.keypoints(bufs, bank=bank, depth=True)
    pts = batch.points(bufs, n_points=64)
    torch.cuda.synchronize()
    return batch, table, bufs, bank, kps, pts


def test_bank_of_the_table(rendered):
    batch, table, bufs, bank, kps, pts = rendered
    assert bank.names == ("center",) + tuple("fps%d" % i for i in range(8)) + tuple("corner%d" % i for i in range(8))
    assert tuple(bank.points.shape) == (3, 17, 4) and tuple(bank.vertex.shape) == (3, 8)
    pos = batch.eng.pool.arrays()[0]
    want_k, want_i = R.fps(pos, table.records, table.templates, 8)
    assert np.array_equal(bank.vertex.cpu().numpy(), want_i)
    assert np.array_equal(bits(bank.points[:, 1:9].cpu().numpy()), bits(want_k))
    fps_xyz, corners = bank.points[:, 1:9, :3].cpu().numpy(), bank.points[:, 9:, :3].cpu().numpy()
    for a in range(3):                                                      # a cube's 8 FPS points are its 8 corners
        d = np.abs(fps_xyz[a][:, None] - corners[a][None]).max(axis=2)
        assert (d.min(axis=1) < 1e-6).all() and len(set(d.argmin(axis=1).tolist())) == 8


def test_coord_lands_on_its_own_pixel(rendered):
    """(a) object_to_camera applied to the rendered object coordinates of a pixel, projected by the batch's intrinsics, is the
    pixel's own centre: this ties object_to_camera's frame to the intrinsics of the keypoints.  Measured on the CPU with the
    oracle's render of the same records (46 733 object pixels): 0.00233 px at the worst, the interpolation error of `coord`.
    Allowed: 0.0032 px = that + 16 float32 roundings of a metre-sized camera coordinate seen at Z >= 0.6 m under fx = 533
    (16 x 2^-24 x 533 / 0.6 = 0.00085 px: the nine of the three row sums, the three of the projection, four for an entry of
    object_to_camera formed in another order than the CPU measurement formed it).  A wrong pixel-centre convention shows as
    0.5 px, a wrong frame as tens of pixels."""
    batch, table, bufs, bank, kps, pts = rendered
    inst = bufs.instance.cpu().numpy()[..., 0]
    coord = bufs.coord.cpu().numpy()
    o2c = batch.object_to_camera.cpu().numpy()
    worst, n = 0.0, 0
    for s in range(N_SCENES):
        for o in range(N_OBJ):
            ys, xs = np.nonzero(inst[s] == o + 1)
            if not len(ys):
                continue
            xyz1 = np.concatenate([coord[s, ys, xs, :3], np.ones((len(ys), 1), F)], axis=1)
            _, uv, flags = R.project(xyz1[None], np.zeros((1, 1), np.uint32), o2c[s, o][None, None], batch.intrinsics(), RES)
            assert (flags == 3).all()
            worst = max(worst, float(np.hypot(uv[0, 0, :, 0].astype(np.float64) - (xs + 0.5), uv[0, 0, :, 1].astype(np.float64) - (ys + 0.5)).max()))
            n += len(ys)
    print("coord through object_to_camera and the intrinsics: %.6f px from the pixel centre at the worst, %d pixels" % (worst, n))
    assert n > 20000 and worst <= 0.0032


def test_corners_meet_the_amodal_box(rendered):
    """(b) a corner keypoint inside the picture lies within one pixel of the object's amodal box whenever the picture does not
    clip that box; every scene has an object with all eight corners inside"""
    batch, table, bufs, bank, kps, pts = rendered
    stats = bufs.object_stats.records().cpu().numpy().view(_abi.OBJECT_STATS_DTYPE).reshape(N_SCENES, N_OBJ + 1)
    uv, inside = kps.uv.cpu().numpy()[:, :, 9:], kps.inside.cpu().numpy()[:, :, 9:]
    checked = 0
    for s in range(N_SCENES):
        assert inside[s].all(axis=1).any(), "scene %d: no object shows all eight corners" % s
        for o in range(N_OBJ):
            x, y, w, h = (int(v) for v in stats[s, o + 1]["bbox_obj"])
            if w <= 0 or x <= 0 or y <= 0 or x + w >= RES[0] or y + h >= RES[1]:
                continue                                                    # empty, or clipped by the picture
            px, py = np.floor(uv[s, o, inside[s, o], 0]), np.floor(uv[s, o, inside[s, o], 1])
            assert (px >= x - 1).all() and (px <= x + w).all() and (py >= y - 1).all() and (py <= y + h).all(), (s, o)
            if inside[s, o].all():                                          # the silhouette of a cube ends at corners
                assert px.min() <= x + 1 and px.max() >= x + w - 2 and py.min() <= y + 1 and py.max() >= y + h - 2, (s, o)
            checked += int(inside[s, o].sum())
    assert checked >= 16


def test_offsets_reproduce_the_keypoints(rendered):
    """(c) offsets(points) + the points' camera coordinates = the keypoints' camera coordinates"""
    batch, table, bufs, bank, kps, pts = rendered
    off = kps.offsets(pts)
    assert tuple(off.shape) == (len(pts), 64, 17, 3) and len(pts) >= 4 and bool(pts.valid.all())
    back = off + pts.camera[:, :, None, :3]
    want = kps.camera[pts.scene_global.long(), (pts.slot - 1).long()][:, None, :, :3].expand_as(back)
    assert float((back - want).abs().max()) <= 2e-7 * float(want.abs().max())      # (a - b) + b: one rounding of metre-sized values
    assert torch.equal(off, want - pts.camera[:, :, None, :3])


def test_field_of_the_render(rendered):
    batch, table, bufs, bank, kps, pts = rendered
    for mode in ("offset", "unit"):
        got = kps.field(bufs.instance, mode=mode, scenes=(1, 1))
        assert tuple(got.shape) == (1, RES[1], RES[0], 17, 2)
        want = R.field(bufs.instance.cpu().numpy()[..., 0], kps.uv.cpu().numpy(), kps.flags.cpu().numpy(), ok.MODES[mode], 1, 1)
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), mode
    # the visible surface keypoints of the render are unoccluded against its own depth within the default tolerance somewhere,
    # and the centre of a cube never is
    assert bool(kps.unoccluded[:, :, 1:].any()) and not bool(kps.unoccluded[:, :, 0].any())
    with pytest.raises(ValueError):
        kps.field(bufs.instance, scenes=(1, 2))
    with pytest.raises(ValueError):
        kps.field(bufs.instance, mode="heatmap")


def test_keypoints_need_object_to_camera_of_the_last_view(rendered):
    """(d) after a place() that did not keep object_to_camera the tensor is another view's: keypoints() refuses"""
    batch, table, bufs, bank, kps, pts = rendered
    with pytest.raises(TypeError):
        batch.keypoints(bufs, bank=bank, intrinsics=K4)
    batch.place(view=1)
    with pytest.raises(RuntimeError) as e:
        batch.keypoints(bufs, bank=bank)
    assert "place(object_to_camera=True)" in str(e.value)
    batch.place(object_to_camera=True)
    again = batch.keypoints(bufs, bank=bank, depth=True)
    assert torch.equal(again.flags, kps.flags) and torch.equal(again.uv, kps.uv)
