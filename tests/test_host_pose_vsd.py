"""Pose VSD without a device: the parameter and argument rules, and the host twins (slhip_pose_vsd_host, slhip_pose_depth_host)
against tests/pose_vsd_ref.py -- bit for bit against its float32 restatement (floats as their int32 views, counts equal) --, with
known answers derived here by hand (pixel counts in integers from the snapped corners of a fronto-parallel plate), and the
float32 counts against the float64 restatement over the same snapped integers on the fixed cases, none of which may hold a
pixel within 64 * 2^-24 * (the largest distance) of a threshold.

The fixed cases: a square plate of side 0.25 (diameter 0.25 sqrt 2) in front of a 96 x 64 camera with fx = fy = 128,
cx = 47.5, cy = 32: at Z = 1 it covers u in [31.5, 63.5], v in [16, 48], every corner exact in float32; the centres of columns
31 and 63 lie on its edge and count (no ownership bias): 33 x 32 = 1056 pixels."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import pose_vsd_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_vsd as pv

F = np.float32
K4 = (128.0, 128.0, 47.5, 32.0)
SIZE = (96, 64)
POISON = 0x5B
NAMES = ("vsd", "counts", "n_cost", "flags")
BIT = {"vsd": R.VSD, "counts": R.COUNTS, "n_cost": R.COST, "flags": R.FLAGS}
DTYPE = {"vsd": F, "counts": np.int32, "n_cost": np.int32, "flags": np.uint32}
PLATE, CUBE, TETRA, SPHERE, EMPTY, OUTSIDE = 0, 1, 2, 3, 4, 7
HALF = 0.125


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the bank --------------------------------------------------------------------------------------------------------------------
def icosphere(levels, radius):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, g = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v) * radius, np.array(f)


@functools.lru_cache(maxsize=None)
def five_class_bank():
    """plate (2 triangles), cube (12), tetrahedron (4, and a fifth with an index outside the table), icosphere (1280), a class
    without triangles"""
    h = HALF
    plate = (np.array([[-h, -h, 0], [h, -h, 0], [h, h, 0], [-h, h, 0]]), np.array([[0, 1, 2], [0, 2, 3]]))
    c = 0.1
    cv = np.array([[x, y, z] for z in (-c, c) for y in (-c, c) for x in (-c, c)])
    cf = np.array([[0, 1, 3], [0, 3, 2], [4, 7, 5], [4, 6, 7], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    tv = np.array([[0.1, 0.1, 0.1], [0.1, -0.1, -0.1], [-0.1, 0.1, -0.1], [-0.1, -0.1, 0.1]])
    tf = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    sv, sf = icosphere(3, 0.075)
    assert len(sf) == 1280
    verts, tris, begin, count, diam, first = [], [], [], [], [], []
    n_v = 0
    for v, f in (plate, (cv, cf), (tv, tf), (sv, sf)):
        begin.append(sum(len(t) for t in tris))
        first.append(n_v)
        tris.append(f + n_v)
        count.append(len(f))
        verts.append(v)
        diam.append(max(np.linalg.norm(v[:, None] - v[None], axis=-1).max(), 0.0))
        n_v += len(v)
    total = n_v
    tris[2] = np.concatenate([tris[2], [[first[2], first[2] + 1, total + 5]]])      # an index outside the table: dropped
    count[2] += 1
    begin[3] += 1
    begin.append(sum(len(t) for t in tris))
    count.append(0)
    diam.append(0.0)
    vertices = np.ones((total, 4), F)
    vertices[:, :3] = np.concatenate(verts)
    return (vertices, np.concatenate(tris).astype(np.uint32), np.array(begin, np.uint32), np.array(count, np.uint32), np.array(diam, F))


def pose(t=(0, 0, 1), axis=None, angle=0.0, scale=(1, 1, 1)):
    m = np.zeros((3, 4))
    m[:, :3] = np.eye(3) if axis is None else pv._pe._rotation(axis, angle)
    m[:, :3] = m[:, :3] * np.asarray(scale, np.float64)[None]
    m[:, 3] = t
    return m.astype(F)


def case(classes, gt, est, depth, **kw):
    """classes [B, O], gt [B, O, 3, 4], est [B, O, Hy, 3, 4], depth [B, H, W]; kw: taus, delta, normalized, z_near, K, bank"""
    c = SimpleNamespace(classes=np.asarray(classes, np.int32), gt=np.ascontiguousarray(gt, F), est=np.ascontiguousarray(est, F),
                        depth=np.ascontiguousarray(depth, F), K=kw.pop("K", K4), bank=kw.pop("bank", None) or five_class_bank(), kw=kw)
    c.size = (c.depth.shape[2], c.depth.shape[1])
    c.ref32 = functools.lru_cache(maxsize=None)(lambda mask=R.ALL: R.evaluate(c.bank, c.classes, c.gt, c.est, c.depth, c.K, mask=mask, **c.kw))
    c.ref64 = functools.lru_cache(maxsize=None)(lambda: R.evaluate(c.bank, c.classes, c.gt, c.est, c.depth, c.K, dtype=np.float64, **c.kw))
    return c


def one(gt, est, depth=None, cls=PLATE, **kw):
    """one scene, one object, the estimates `est` (a list of poses)"""
    W, H = SIZE
    depth = np.zeros((1, H, W), F) if depth is None else np.asarray(depth, F).reshape(1, H, W)
    return case([[cls]], np.asarray(gt, F)[None, None], np.stack(est)[None, None], depth, **kw)


def wall(z, columns=slice(None), back=0.0):
    """a scene depth of z in `columns`, no measurement elsewhere (a background at 3000 would set the float64 margin of every
    threshold of the case: the margin scales with the largest distance)"""
    W, H = SIZE
    d = np.full((H, W), back, F)
    d[:, columns] = z
    return d


def host_call(c, mask=R.ALL, null=None, stride=None, depth_stride=1, n_scenes=None, surface=None, misalign=None, **pkw):
    """slhip_pose_vsd_host between poisoned bytes: (status, the raw output arrays, keep)"""
    B, O, Hy = c.est.shape[:3]
    kw = dict(c.kw)
    kw.update(pkw)
    W, H = kw.pop("size", c.size)
    p = pv.make_params(kw.pop("K", c.K), (W, H), kw.pop("n_objects", O), kw.pop("n_hypotheses", Hy), outputs=mask, **kw).reshape(1)
    T = max(1, min(int(p["n_taus"][0]), 16))
    rec, keep = pv._surface_record(*c.bank)
    for k, v in (surface or {}).items():
        setattr(rec, k, v)
    if misalign is not None:
        setattr(rec, misalign, getattr(rec, misalign) + 4)
    shapes = {"vsd": (B, O, Hy, T), "counts": (B, O, Hy, 4), "n_cost": (B, O, Hy, T), "flags": (B, O, Hy)}
    outs = {k: np.full(shapes[k], POISON, np.uint8).repeat(4).view(DTYPE[k]).reshape(shapes[k]).copy() for k in NAMES}
    o = _abi.PoseVsdOut(*(None if null == k else outs[k].ctypes.data for k in NAMES))
    depth = c.depth if depth_stride == 1 else np.ascontiguousarray(np.stack([np.full_like(c.depth, np.nan)] * 3 + [c.depth], axis=-1))
    ptr = dict(classes=c.classes.ctypes.data, gt=c.gt.ctypes.data, est=c.est.ctypes.data, depth=depth.ctypes.data + (12 if depth_stride == 4 else 0))
    if null in ptr:
        ptr[null] = None
    st = _abi.lib().slhip_pose_vsd_host(None if null == "params" else p.ctypes.data, None if null == "surface" else C.byref(rec), ptr["classes"],
                                        1 if stride is None else stride, ptr["gt"], ptr["est"], ptr["depth"], depth_stride,
                                        B if n_scenes is None else n_scenes, None if null == "record" else C.byref(o))
    return st, outs, (keep, depth, p)


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == POISON).all())


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        diff = g.view(np.int32) != w.view(np.int32)
        if diff.any():
            at = tuple(np.argwhere(diff)[0])
            raise AssertionError("%s %s: %d of %d differ, the first at %s: %r against %r" % (what, k, int(diff.sum()), diff.size, at, g[at], w[at]))


def run_host(c, mask=R.ALL, **kw):
    st, outs, keep = host_call(c, mask, **kw)
    assert st == 0, _abi.lib().slhip_last_error()
    got = {}
    for k in NAMES:
        if mask & BIT[k]:
            got[k] = outs[k]
        else:
            assert untouched(outs[k]), k
    return got


# ---- pixel counts in integers ------------------------------------------------------------------------------------------------------
def columns(centre, f, lo, hi, Z, n):
    """the pixels whose centre 256 px + 128 lies inside the snapped span of the object coordinates lo .. hi at depth Z: a range.
    The snap is done in float64 here and must not sit near a rounding boundary, where float32 could differ."""
    xs = []
    for x in (lo, hi):
        s = (centre + f * x / Z) * 256.0 + 0.5
        assert abs(s - round(s)) > 1e-2 or float(s).is_integer(), s
        xs.append(math.floor(s))
    first = max(0, -((128 - xs[0]) // 256))      # ceil((X - 128) / 256)
    last = min(n - 1, (xs[1] - 128) // 256)
    return range(first, last + 1)


def plate_box(Z=1.0, dx=0.0):
    W, H = SIZE
    return columns(K4[2], K4[0], dx - HALF, dx + HALF, Z, W), columns(K4[3], K4[1], -HALF, HALF, Z, H)


N_PLATE = 33 * 32
DIAMETER = 0.25 * math.sqrt(2.0)
DZ = 0.0625


def test_the_plate_covers_1056_pixels():
    cols, rows = plate_box()
    assert (cols[0], cols[-1], rows[0], rows[-1]) == (31, 63, 16, 47) and len(cols) * len(rows) == N_PLATE
    depth, flags = pv.render_depth_host(pose()[None, None, None], [[PLATE]], *five_class_bank()[:4], K4, SIZE)
    want = np.zeros((SIZE[1], SIZE[0]), F)
    want[16:48, 31:64] = 1.0
    assert np.array_equal(depth[0, 0, 0] != 0, want != 0) and flags[0, 0, 0] == 0
    assert np.abs(depth[0, 0, 0][want != 0] - 1.0).max() <= 2.0 ** -22
    ref, rflags = R.depth32(five_class_bank(), np.array([[PLATE]]), pose()[None, None, None], K4, SIZE)
    assert same_bits(depth, ref) and same_bits(flags, rflags)


# ---- the fixed cases: known answers, the restatement bit for bit, float64 ------------------------------------------------------------
def fixed_cases():
    g = pose()
    far = pose((0, 0, 1 + DZ))
    behind_shifted = pose((0.03125, 0, 1 + DZ))
    return {
        "equal": one(g, [g]),
        "equal_occluded": one(g, [g], wall(0.5, slice(0, 48))),
        "disjoint": one(g, [pose((0.3, 0, 1))]),
        "deeper": one(g, [far]),
        "slightly_behind": one(g, [g], wall(1.0 - 0.01)),
        "no_measurement_0": one(g, [g], wall(0.0)),
        "no_measurement_nan": one(g, [g], wall(np.nan)),
        "no_measurement_inf": one(g, [g], wall(np.inf)),
        "background_3000": one(g, [g], wall(3000.0)),
        "est_rule": one(g, [behind_shifted], wall(1.03)),
        "hidden": one(g, [g], wall(0.5)),
        "absolute_taus": one(g, [far], normalized=False, taus=(0.05, 0.07), delta=0.02),
    }


FIXED = fixed_cases()


@pytest.mark.parametrize("name", list(FIXED))
def test_fixed_case_against_the_restatement_and_float64(name):
    c = FIXED[name]
    got = run_host(c)
    assert_same(got, c.ref32(), name)
    r64 = c.ref64()
    print(name, "counts", got["counts"].reshape(-1), "n_cost", got["n_cost"].reshape(-1), "near a threshold:", r64["edge"])
    assert r64["edge"] == 0, "a pixel of a fixed case sits within 64 * 2^-24 of a threshold: change the case's constants"
    assert np.array_equal(got["counts"], r64["counts"]) and np.array_equal(got["n_cost"], r64["n_cost"])
    assert same_bits(got["vsd"], r64["vsd"])


def test_equal_poses_score_zero():
    """1. an estimate bit-equal to the ground truth: vsd 0, union = inter = visib_gt = the 1056 pixel centres inside the square"""
    got = run_host(FIXED["equal"])
    assert (got["vsd"] == 0).all() and got["counts"].reshape(-1).tolist() == [N_PLATE] * 4 and (got["n_cost"] == 0).all()
    assert (got["flags"] == 0).all()


def test_disjoint_silhouettes_score_one():
    """2. a sideways shift by more than the plate: vsd exactly 1, no intersection"""
    got = run_host(FIXED["disjoint"])
    cols, rows = plate_box(dx=0.3)
    n_est = len(cols) * len(rows)
    assert n_est > 0 and cols[0] > 63
    assert (got["vsd"] == 1).all() and got["counts"].reshape(-1).tolist() == [N_PLATE, n_est, 0, N_PLATE + n_est] and (got["n_cost"] == 0).all()


def test_the_plate_at_z_and_z_plus_dz():
    """3. taus below dz / d cost every intersection pixel, taus above dz max ray / d none: vsd = (union - inter) / union"""
    got = run_host(FIXED["deeper"])
    cols, rows = plate_box(Z=1 + DZ)
    n_inter = len(cols) * len(rows)
    assert (len(cols), len(rows)) == (31, 30)
    assert got["counts"].reshape(-1).tolist() == [N_PLATE, n_inter, n_inter, N_PLATE]
    max_ray = math.sqrt(1 + (16.5 / 128) ** 2 + (16.0 / 128) ** 2)
    low = [t for t, tau in enumerate(R.TAUS) if tau < DZ / DIAMETER * (1 - 1e-3)]
    high = [t for t, tau in enumerate(R.TAUS) if tau > DZ * max_ray / DIAMETER * (1 + 1e-3)]
    assert low == [0, 1, 2] and high == list(range(3, 10))
    assert got["n_cost"][0, 0, 0, low].tolist() == [n_inter] * 3 and (got["vsd"][0, 0, 0, low] == 1).all()
    assert (got["n_cost"][0, 0, 0, high] == 0).all()
    assert same_bits(got["vsd"][0, 0, 0, high], np.full(7, F(N_PLATE - n_inter) / F(N_PLATE), F))
    got = run_host(FIXED["absolute_taus"])                                   # thresholds in the table's unit: 0.05 < dz, 0.07 > dz max ray
    assert got["n_cost"].reshape(-1).tolist() == [n_inter, 0]


def test_an_occluder_hides_the_left_half():
    """4. a wall 0.5 in front of columns 0 .. 47: the counts are those of columns 48 .. 63; equal poses still score 0"""
    got = run_host(FIXED["equal_occluded"])
    assert got["counts"].reshape(-1).tolist() == [16 * 32] * 4 and (got["vsd"] == 0).all()


def test_slightly_behind_and_no_measurement_remove_nothing():
    """5. a wall nearer than the object by less than delta; 6. a scene depth of 0, NaN, an infinity or the background's 3000"""
    for name in ("slightly_behind", "no_measurement_0", "no_measurement_nan", "no_measurement_inf", "background_3000", "equal"):
        got = run_host(FIXED[name])
        assert got["counts"].reshape(-1).tolist() == [N_PLATE] * 4, name


def test_the_estimate_counts_where_the_ground_truth_is_visible():
    """7. an estimate behind the scene's surface by more than delta is visible exactly where the visible ground truth covers it"""
    got = run_host(FIXED["est_rule"])
    cols, rows = plate_box(Z=1 + DZ, dx=0.03125)
    shared = [x for x in cols if 31 <= x <= 63]
    assert len(shared) < len(cols) and len(rows) == 30
    assert got["counts"].reshape(-1).tolist() == [N_PLATE, len(shared) * 30, len(shared) * 30, N_PLATE]


def test_an_empty_union_scores_one():
    got = run_host(FIXED["hidden"])
    assert got["counts"].reshape(-1).tolist() == [0] * 4 and (got["vsd"] == 1).all() and (got["n_cost"] == 0).all()


# ---- the cases the host and the device tests share -----------------------------------------------------------------------------------
def random_poses(rng, shape, z=(0.8, 1.2)):
    q = rng.normal(size=shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, zz, w = (q[..., i] for i in range(4))
    Rm = np.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - zz * w), 2 * (x * zz + y * w), 2 * (x * y + zz * w), 1 - 2 * (x * x + zz * zz),
                   2 * (y * zz - x * w), 2 * (x * zz - y * w), 2 * (y * zz + x * w), 1 - 2 * (x * x + y * y)], axis=-1).reshape(shape + (3, 3))
    T = np.zeros(shape + (3, 4))
    T[..., :3] = Rm
    T[..., 0, 3], T[..., 1, 3] = rng.uniform(-0.1, 0.1, shape), rng.uniform(-0.05, 0.05, shape)
    T[..., 2, 3] = rng.uniform(z[0], z[1], shape)
    return T


def scene_depth(rng, B, size):
    """a tilted plane through the objects' depths, with patches of 0, NaN and the background's 3000"""
    W, H = size
    py, px = np.mgrid[0:H, 0:W]
    d = np.stack([(1.0 + 0.004 * (px - W / 2) - 0.003 * (py - H / 2) + 0.05 * b) for b in range(B)]).astype(F)
    d[:, : H // 4, : W // 3] = 0.0
    d[:, H // 2:, W // 2: W // 2 + 7] = np.nan
    d[:, H // 3: H // 2, 2 * W // 3:] = 3000.0
    return d


@functools.lru_cache(maxsize=None)
def hypotheses_case(Hy):
    """2 x 3 objects: plate, cube, a class outside the bank; icosphere (1280 triangles on about 20 px), tetrahedron (with a
    triangle whose index leaves the table), a class without triangles.  With Hy >= 3: a NaN estimate and a cube pushed through
    z_near."""
    rng = np.random.default_rng(100 + Hy)
    classes = np.array([[PLATE, CUBE, OUTSIDE], [SPHERE, TETRA, EMPTY]], np.int32)
    gt = random_poses(rng, (2, 3))
    est = np.repeat(gt[:, :, None], Hy, axis=2)
    for idx in np.ndindex(2, 3, Hy):
        d = pose(rng.uniform(-0.03, 0.03, 3), rng.normal(size=3), rng.uniform(-0.2, 0.2)).astype(np.float64)
        g = gt[idx[:2]]
        est[idx][:, :3] = g[:, :3] @ d[:, :3]
        est[idx][:, 3] = g[:, :3] @ d[:, 3] + g[:, 3]
    est = est.astype(F)
    est[0, 0, 0] = gt[0, 0].astype(F)                                         # bit-equal
    if Hy >= 3:
        est[0, 0, 1, 1, 2] = np.nan
        est[0, 1, 2, 2, 3] = 0.05                                             # the cube's half side is 0.1: vertices behind z_near
    return case(classes, gt, est, scene_depth(rng, 2, SIZE))


CASES = {"Hy1": lambda: hypotheses_case(1), "Hy3": lambda: hypotheses_case(3), "Hy33": lambda: hypotheses_case(33)}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_bit_for_bit(name):
    c = CASES[name]()
    got = run_host(c)
    assert_same(got, c.ref32(), name)
    assert np.isposinf(got["vsd"][0, 2]).all() and np.isposinf(got["vsd"][1, 2]).all()            # no surface: +inf and -1, never 1
    assert (got["counts"][0, 2] == -1).all() and (got["n_cost"][1, 2] == -1).all() and (got["flags"][:, 2] == 0).all()
    assert (got["vsd"][0, 0, 0] == 0).all() and got["counts"][0, 0, 0, 3] > 0                        # bit-equal, whatever the occlusion
    assert (got["counts"][1, 0, :, 0] > 100).all() and (got["counts"][1, 1, :, 0] > 0).all()         # the sphere and the tetrahedron are seen
    if name != "Hy1":
        assert np.isnan(got["vsd"][0, 0, 1]).all() and (got["counts"][0, 0, 1] == -1).all()          # the NaN estimate only
        assert np.isfinite(got["vsd"][0, 0, [0, 2]]).all()
        assert got["flags"][0, 1, 2] == R.CLIPPED and got["flags"][0, 1, 0] == 0
        assert np.isfinite(got["vsd"][0, 1, 2]).all()


def test_depth_read_at_stride_four():
    c = hypotheses_case(3)
    assert_same(run_host(c, depth_stride=4), c.ref32(), "stride 4")


def test_evaluate_host_and_render_depth_host():
    c = hypotheses_case(3)
    coord = np.stack([np.full_like(c.depth, np.nan)] * 3 + [c.depth], axis=-1)
    got = pv.evaluate_host(c.gt, c.est, c.classes, *c.bank[:4], coord, c.K, diameter=c.bank[4])
    want = c.ref32()
    for k in NAMES:
        assert same_bits(got[k], want[k]), k
    only = pv.evaluate_host(c.gt, c.est, c.classes, *c.bank[:4], c.depth, c.K, diameter=c.bank[4], outputs=("counts",))
    assert list(only) == ["counts"] and same_bits(only["counts"], want["counts"])
    poses = np.ascontiguousarray(c.est[:, :, :2])
    depth, flags = pv.render_depth_host(poses, c.classes, *c.bank[:4], c.K, c.size)
    rdepth, rflags = R.depth32(c.bank, c.classes, poses, c.K, c.size)
    assert same_bits(depth, rdepth) and same_bits(flags, rflags)
    assert (depth[0, 2] == 0).all() and (depth[1, 2] == 0).all() and (depth[0, 0, 1] == 0).all()   # no surface; the NaN pose
    assert (depth[1, 0] > 0).sum() > 200


def test_a_vertex_behind_z_near_drops_its_triangles():
    """the cube (half side 0.1) at Z = 0.35 with z_near 0.3: the four front vertices are clipped, the two triangles of the back
    face stay; the plate turned through the camera plane loses both triangles"""
    g = pose((0, 0, 0.35))
    c = one(g, [g], cls=CUBE, z_near=0.3)
    got = run_host(c)
    assert_same(got, c.ref32(), "cube")
    cols, rows = columns(K4[2], K4[0], -0.1, 0.1, 0.45, SIZE[0]), columns(K4[3], K4[1], -0.1, 0.1, 0.45, SIZE[1])
    assert got["flags"].reshape(-1).tolist() == [R.CLIPPED] and got["counts"].reshape(-1).tolist() == [len(cols) * len(rows)] * 4
    assert (got["vsd"] == 0).all()
    through = pose((0, 0, 0.1), (0, 1, 0), math.pi / 3)
    c = one(through, [through])
    got = run_host(c)
    assert_same(got, c.ref32(), "plate")
    assert got["flags"].reshape(-1).tolist() == [R.CLIPPED] and got["counts"].reshape(-1).tolist() == [0] * 4 and (got["vsd"] == 1).all()


@pytest.mark.parametrize("mask", [R.VSD, R.COUNTS, R.COST, R.FLAGS, R.VSD | R.FLAGS, R.COUNTS | R.COST])
def test_outputs_not_named_stay_poison(mask):
    c = hypotheses_case(3)
    assert_same(run_host(c, mask=mask), c.ref32(mask), "mask %d" % mask)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def refused(text, **kw):
    c = kw.pop("case", None) or FIXED["equal"]
    st, outs, keep = host_call(c, **kw)
    msg = (_abi.lib().slhip_last_error() or b"").decode()
    assert st < 0 and text in msg, (kw, st, msg)
    assert all(untouched(o) for o in outs.values()), kw


def test_check_params_refuses_one_broken_rule_at_a_time():
    good = pv.make_params(K4, SIZE, 3, 2)
    assert pv.check_params(good)["n_taus"][0] == 10
    for field, value, text in (("fx", 0.0, "fx and fy must be positive"), ("fy", -1.0, "fx and fy must be positive"), ("cx", np.nan, "all four finite"),
                               ("cy", np.inf, "all four finite"), ("W", 0, "bad picture size"), ("W", 4097, "bad picture size"),
                               ("H", 0, "bad picture size"), ("H", 32769, "bad picture size"), ("n_objects", 0, "n_objects 0 must be in [1, 64]"),
                               ("n_objects", 65, "n_objects 65"), ("n_hypotheses", 0, "n_hypotheses 0"), ("n_taus", 0, "n_taus 0 must be in [1, 16]"),
                               ("n_taus", 17, "n_taus 17"), ("delta", -0.001, "delta"), ("delta", np.nan, "delta"), ("z_near", 0.0, "z_near"),
                               ("z_near", np.inf, "z_near"), ("flags", 2, "flags 0x2"), ("outputs", 0, "outputs 0x0"), ("outputs", 16, "outputs 0x10")):
        bad = good.copy()
        bad[field] = value
        with pytest.raises(_abi.SlhipError) as e:
            pv.check_params(bad)
        assert text in str(e.value), (field, value, str(e.value))
    for value in (-0.1, np.nan, np.inf):
        bad = good.copy()
        bad["taus"][9] = value
        with pytest.raises(_abi.SlhipError) as e:
            pv.check_params(bad)
        assert "taus[9]" in str(e.value)
    bad = good.copy()
    bad["taus"][10] = np.nan                                                   # past n_taus: not read
    pv.check_params(bad)
    assert _abi.lib().slhip_pose_vsd_check_params(None) < 0
    with pytest.raises(ValueError):
        pv.make_params(K4, SIZE, 3, 2, outputs=("vsd", "add"))
    assert pv.band_pixels() in (4096, 8192, 16384)


def test_the_entries_refuse_one_broken_argument_at_a_time():
    for null, text in (("params", "null parameter record"), ("surface", "null argument (the surface"), ("classes", "classes and poses are required"),
                       ("gt", "classes and poses are required"), ("est", "estimates, the scene's depth and the output record"),
                       ("depth", "estimates, the scene's depth and the output record"), ("record", "estimates, the scene's depth and the output record"),
                       ("vsd", "has a null pointer"), ("counts", "has a null pointer"), ("n_cost", "has a null pointer"), ("flags", "has a null pointer")):
        refused(text, null=null)
    for field in ("vertices", "triangles", "tri_begin", "tri_count"):
        refused("null argument (the surface", surface={field: None})
    refused("normalised thresholds need the surface's diameter", surface={"diameter": None})
    refused("vertices must be 16-byte aligned", misalign="vertices")
    refused("n_assets 0", surface={"n_assets": 0})
    refused("n_assets 1025", surface={"n_assets": 1025})
    refused("n_vertices 0", surface={"n_vertices": 0})
    refused("n_triangles 0", surface={"n_triangles": 0})
    refused("class_stride must be at least 1", stride=0)
    refused("depth_stride must be at least 1", depth_stride=0)
    refused("n_hypotheses 0", n_hypotheses=0)
    refused("outputs 0x10", mask=16)
    refused("bad picture size", size=(4097, 64))
    st, outs, keep = host_call(FIXED["equal"], n_scenes=0)                     # no scenes: fine, and writes nothing
    assert st == 0 and all(untouched(o) for o in outs.values())
    st, outs, keep = host_call(FIXED["deeper"], surface={"diameter": None}, normalized=False)      # no diameter needed
    assert st == 0
    bank = five_class_bank()
    args = (pv.make_params(K4, SIZE, 1, 1).reshape(1), pv._surface_record(*bank)[0], np.zeros((1, 1), np.int32), pose()[None, None, None])
    depth = np.full((1, 1, 1, SIZE[1], SIZE[0]), 7.0, F)

    def depth_call(params=True, surface=True, classes=True, stride=1, poses=True, out=True):
        return _abi.lib().slhip_pose_depth_host(args[0].ctypes.data if params else None, C.byref(args[1]) if surface else None,
                                                args[2].ctypes.data if classes else None, stride, args[3].ctypes.data if poses else None, 1,
                                                depth.ctypes.data if out else None, None)

    for kw in (dict(params=False), dict(surface=False), dict(classes=False), dict(stride=0), dict(poses=False), dict(out=False)):
        assert depth_call(**kw) < 0 and (depth == 7.0).all(), kw
    assert depth_call() == 0 and (depth != 7.0).all()                          # the flags are optional
