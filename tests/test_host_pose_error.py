"""Pose errors without a device: the symmetry lists, the sampling, the parameter and argument rules, and the host twins
(slhip_pose_error_host, slhip_pose_error_diameter_host) against tests/pose_error_ref.py -- bit for bit against its float32
restatement (floats as their int32 views, indices equal), and both within the float64 bound of the issue
(64 * 2^-24 * M metres, times fx M / Z_min + max(|cx|, |cy|) for mspd) against its float64 definition.

The float32 restatement alone against the float64 definition on the cases of this module, the largest deviation as a share of
the bound (measured on the CPU, printed by test_cases_against_float64): 0.039 at the worst (Hy3; 0.022 Hy1, 0.016 Hy33, 0.003
N4096, 0.007 diff) -- e.g. Hy33: 8.7e-8 m of 5.4e-6 m for adds, 6.4e-5 px of 4.8e-3 px for mspd.  Left out of the arg-min
comparison as near-ties: 3 of 131 hypotheses of Hy33 for mssd_sym (2.3 %, the 65-fold class), none elsewhere (the cap is 5 %)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pose_error_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_error as pe

F = np.float32
K4 = (533.4, 533.7, 156.5, 120.6)
EYE = np.eye(4, dtype=F)[:3]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def rot(axis, angle):
    m = np.eye(4)
    m[:3, :3] = pe._rotation(axis, angle)
    return m


# ---- symmetry lists --------------------------------------------------------------------------------------------------------------
def test_one_axis_gives_315_rotations_identity_first():
    s = pe.symmetry_transforms(continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}], max_step=0.01)
    assert s.shape == (315, 3, 4) and s.dtype == F
    assert same_bits(s[0], EYE)
    want = rot([0, 0, 1], 2 * np.pi * 7 / 315)[:3].astype(F)
    assert same_bits(s[7], want)
    assert len({m.tobytes() for m in s}) == 315


def test_an_offset_axis_leaves_its_points_fixed():
    off, axis = np.array([0.02, -0.01, 0.03]), np.array([1.0, 2.0, -2.0]) / 3.0
    s = pe.symmetry_transforms(continuous=[{"axis": list(axis * 5), "offset": list(off)}], max_step=0.5).astype(np.float64)
    assert len(s) == 7
    for t in (-0.2, 0.0, 0.35):
        p = off + t * axis                                                    # a point on the axis
        assert np.abs(s[:, :, :3] @ p + s[:, :, 3] - p).max() < 1e-7
    p = off + np.array([0.1, 0.0, 0.05])                                      # and one off it moves, at the same distance from it
    moved = s[:, :, :3] @ p + s[:, :, 3]
    assert np.abs(moved[1] - p).max() > 1e-3
    assert np.abs(np.linalg.norm(np.cross(moved - off, axis), axis=1) - np.linalg.norm(np.cross(p - off, axis))).max() < 1e-7
    mm = pe.symmetry_transforms(continuous=[{"axis": list(axis), "offset": list(off * 1000)}], max_step=0.5, scale=0.001)
    assert np.abs(mm - s).max() < 1e-6                                        # millimetres in, metres out


def test_one_discrete_times_one_axis_gives_630():
    flip = rot([1, 0, 0], np.pi)
    s = pe.symmetry_transforms(discrete=[flip.reshape(-1)], continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}])
    assert s.shape == (630, 3, 4) and same_bits(s[0], EYE)
    assert np.abs(s[315] - flip[:3]).max() < 1e-7                             # cont = identity, disc = the flip
    assert np.abs(s[315 + 5].astype(np.float64) - (rot([0, 0, 1], 2 * np.pi * 5 / 315) @ flip)[:3]).max() < 1e-7


def test_too_many_symmetries_raise_and_name_the_class():
    flips = [rot([1, 0, 0], np.pi).reshape(-1)] * 3
    with pytest.raises(ValueError) as e:
        pe.symmetry_transforms(discrete=flips, continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}], name="bowl")
    assert "bowl" in str(e.value) and "max_step" in str(e.value) and "1024" in str(e.value)
    assert len(pe.symmetry_transforms(discrete=flips, continuous=[{"axis": [0, 0, 1], "offset": [0, 0, 0]}], max_step=0.02)) == 4 * 158


# ---- sampling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,n", [(5, 8), (8, 8), (2500, 1024)])
def test_sample(V, n):
    from test_host_object_keypoints import one_class

    import object_keypoints_ref as K

    rng = np.random.default_rng(V)
    pos = rng.uniform(-1, 1, (V, 3)).astype(F)
    m2o = np.eye(4, dtype=F)
    m2o[:3, :3] = [[0, 0.5, 0], [0, 0, 2], [1, 0, 0]]
    m2o[:3, 3] = [0.25, -0.5, 0.125]
    pool, a, t = one_class(pos, m2o=m2o, pad_before=11)
    idx = pe.sample_indices(V, n)
    if V <= n:
        assert idx.tolist() == list(range(V))
    else:
        assert len(idx) == n and idx.tolist() == [k * V // n for k in range(n)] and idx[0] == 0 and idx[-1] == (n - 1) * V // n
        assert (np.diff(idx) >= 1).all()
    points, count = pe.sample_points(torch.from_numpy(pool), a, t, n)
    assert count.tolist() == [min(V, n)] and tuple(points.shape) == (1, min(V, n), 4)
    want = K.object_points(m2o.reshape(-1), pos[idx])
    assert same_bits(points[0, :, :3].numpy(), want) and (points[0, :, 3] == 1).all()


# ---- the cases the host and the device tests share ---------------------------------------------------------------------------------
def random_poses(rng, shape, z=(0.6, 1.5)):
    q = rng.normal(size=shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    x, y, zz, w = (q[..., i] for i in range(4))
    Rm = np.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - zz * w), 2 * (x * zz + y * w), 2 * (x * y + zz * w), 1 - 2 * (x * x + zz * zz),
                   2 * (y * zz - x * w), 2 * (x * zz - y * w), 2 * (y * zz + x * w), 1 - 2 * (x * x + y * y)], axis=-1).reshape(shape + (3, 3))
    T = np.zeros(shape + (3, 4))
    T[..., :3] = Rm
    T[..., 0, 3], T[..., 1, 3] = rng.uniform(-0.25, 0.25, shape), rng.uniform(-0.2, 0.2, shape)
    T[..., 2, 3] = rng.uniform(z[0], z[1], shape)
    return T


def compose(a, b):
    """a b of 3 x 4 transforms (float64)"""
    out = np.zeros(np.broadcast_shapes(a.shape, b.shape))
    out[..., :3] = a[..., :3] @ b[..., :3]
    out[..., 3] = (a[..., :3] @ b[..., 3:])[..., 0] + a[..., 3]
    return out


def estimates_near(rng, gt, Hy, syms, n_sym, classes, angle=0.15, shift=0.02):
    """gt [B, O, 3, 4] -> [B, O, Hy, 3, 4]: the ground truth times a symmetry of the object's class times a small motion"""
    B, O = gt.shape[:2]
    est = np.zeros((B, O, Hy, 3, 4))
    for b in range(B):
        for o in range(O):
            c = int(classes[b, o])
            for h in range(Hy):
                S = syms[c, rng.integers(0, n_sym[c])].astype(np.float64) if 0 <= c < len(n_sym) and n_sym[c] >= 1 else EYE.astype(np.float64)
                axis = rng.normal(size=3)
                d = rot(axis, rng.uniform(-angle, angle))[:3]
                d[:, 3] = rng.uniform(-shift, shift, 3)
                est[b, o, h] = compose(compose(gt[b, o], S), d)
    return est.astype(F)


@functools.lru_cache(maxsize=None)
def five_class_bank():
    """Point counts 0, 1, 63, 65, 257 (ragged against a wave, a lane's four queries and the workgroup's stride) with 1, 1, 65
    (more than a wave), 630 and 3 symmetries."""
    rng = np.random.default_rng(20261019)
    count = np.array([0, 1, 63, 65, 257], np.int32)
    points = np.zeros((5, 257, 4), F)
    for c, n in enumerate(count):
        points[c, :n, :3] = rng.uniform(-0.1, 0.1, (n, 3))
        points[c, :n, 3] = 1
    lists = [EYE[None], EYE[None], np.stack([rot([0, 0, 1], 2 * np.pi * k / 65)[:3] for k in range(65)]).astype(F),
             pe.symmetry_transforms(discrete=[rot([1, 0, 0], np.pi).reshape(-1)], continuous=[{"axis": [0, 0, 1], "offset": [0.01, 0, 0]}]),
             np.stack([rot([0, 1, 0], 2 * np.pi * k / 3)[:3] for k in range(3)]).astype(F)]
    n_sym = np.array([len(l) for l in lists], np.int32)
    syms = np.tile(EYE, (5, 630, 1, 1))
    for c, l in enumerate(lists):
        syms[c, :len(l)] = l
    return points, count, syms, n_sym


class Case:
    def __init__(self, bank, classes, gt, est):
        self.points, self.count, self.syms, self.n_sym = bank
        self.classes, self.gt, self.est = np.asarray(classes, np.int32), gt, est
        self._r32, self._r64 = {}, None

    def bank(self):
        return self.points, self.count, self.syms, self.n_sym

    def ref32(self, mask=R.ALL):
        if mask not in self._r32:
            self._r32[mask] = R.errors32(*self.bank(), self.classes, self.gt, self.est, K4, mask)
        return self._r32[mask]

    def ref64(self):
        if self._r64 is None:
            self._r64 = R.errors64(*self.bank(), self.classes, self.gt, self.est, K4)
        return self._r64

    def bounds(self):
        M = R.largest_coordinate(*self.bank(), self.classes, self.gt, self.est)
        z = [R.move(T, self.points[c, :self.count[c], :3].astype(np.float64))[:, 2].min()
             for T, c in self._poses() if np.isfinite(T).all()]
        z_min = min(v for v in z if v > 0)
        return R.tol(M), R.tol_px(M, K4, z_min)

    def _poses(self):
        B, O, Hy = self.est.shape[:3]
        for b in range(B):
            for o in range(O):
                c = int(self.classes[b, o])
                if 0 <= c < len(self.count) and self.count[c] >= 1:
                    yield self.gt[b, o], c
                    for h in range(Hy):
                        yield self.est[b, o, h], c


@functools.lru_cache(maxsize=None)
def hypotheses_case(Hy):
    """B x O = 2 x 3 over the five-class bank: class 7 lies outside the bank, class 0 has no points; one estimate holds a NaN,
    one lies behind the camera."""
    bank = five_class_bank()
    rng = np.random.default_rng(100 + Hy)
    classes = np.array([[4, 2, 7], [3, 1, 0]], np.int32)
    gt = random_poses(rng, (2, 3)).astype(F)
    est = estimates_near(rng, gt.astype(np.float64), Hy, bank[2], bank[3], classes)
    est[0, 0, Hy // 2, 1, 2] = np.nan
    est[1, 0, 0, 2, 3] = -1.0
    return Case(bank, classes, gt, est)


@functools.lru_cache(maxsize=None)
def large_class_case():
    """one class at 4096 points, 1 x 1 x 1: the LDS capacity and the last tile"""
    rng = np.random.default_rng(4096)
    points = np.ones((1, 4096, 4), F)
    points[0, :, :3] = rng.uniform(-0.15, 0.15, (4096, 3))
    syms = np.stack([rot([0, 0, 1], np.pi * k)[:3] for k in range(2)]).astype(F)[None]
    bank = (points, np.array([4096], np.int32), syms, np.array([2], np.int32))
    classes = np.zeros((1, 1), np.int32)
    gt = random_poses(rng, (1, 1)).astype(F)
    return Case(bank, classes, gt, estimates_near(rng, gt.astype(np.float64), 1, syms, bank[3], classes))


@functools.lru_cache(maxsize=None)
def diff_shape_case():
    """the sl.diff shape 1 x 64 x 32 at N = 64: the hypotheses of an object split over workgroups"""
    rng = np.random.default_rng(6432)
    points = np.ones((3, 64, 4), F)
    points[:, :, :3] = rng.uniform(-0.1, 0.1, (3, 64, 3))
    syms = np.tile(EYE, (3, 4, 1, 1))
    syms[1, :4] = np.stack([rot([0, 0, 1], np.pi * k / 2)[:3] for k in range(4)])
    bank = (points, np.array([64, 64, 40], np.int32), syms, np.array([1, 4, 1], np.int32))
    classes = rng.integers(0, 3, (1, 64)).astype(np.int32)
    gt = random_poses(rng, (1, 64)).astype(F)
    return Case(bank, classes, gt, estimates_near(rng, gt.astype(np.float64), 32, syms, bank[3], classes))


def host_errors(case, outputs=("add", "adds", "mssd", "mspd")):
    return pe.evaluate_host(case.gt, case.est, case.classes, *case.bank(), K4, outputs)


def check_against_float64(got, case, what):
    """every output of `got` within the bound of the float64 definition; the arg-min equal wherever float64's best and
    runner-up are at least 2 tol apart, with at most 5 % of the hypotheses left out.  Returns the largest share of the bound."""
    want, (tol, tol_px) = case.ref64(), case.bounds()
    worst = 0.0
    for k, bound in (("add", tol), ("adds", tol), ("mssd", tol), ("mspd", tol_px)):
        g, w = got[k].astype(np.float64), want[k]
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isinf(g), np.isinf(w)), (what, k)
        ok = np.isfinite(w)
        dev = float(np.abs(g[ok] - w[ok]).max())
        worst = max(worst, dev / bound)
        print("%s %s: %.3e from float64 at the worst, bound %.3e (%d values)" % (what, k, dev, bound, int(ok.sum())))
        assert dev <= bound, (what, k)
    for k, gap, bound in (("mssd_sym", "mssd_gap", tol), ("mspd_sym", "mspd_gap", tol_px)):
        defined = want[k] >= 0
        clear = defined & (want[gap] >= 2 * bound)
        assert (got[k][~defined] == -1).all(), (what, k)
        left_out = int((defined & ~clear).sum())
        print("%s %s: %d of %d hypotheses left out as near-ties" % (what, k, left_out, int(defined.sum())))
        assert left_out <= 0.05 * max(1, int(defined.sum())), (what, k)
        assert np.array_equal(got[k][clear], want[k][clear]), (what, k)
    return worst


CASES = {"Hy1": lambda: hypotheses_case(1), "Hy3": lambda: hypotheses_case(3), "Hy33": lambda: hypotheses_case(33),
         "N4096": large_class_case, "diff": diff_shape_case}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_against_float64(name):
    """the restatement alone, then the host twin: bit for bit against the restatement, both within the bound of float64"""
    case = CASES[name]()
    want = case.ref32()
    share = check_against_float64(want, case, name + " restatement")
    print("%s: the restatement uses %.3f of the bound" % (name, share))
    assert share <= 0.25                                                      # room to spare, or the rule is poor
    got = host_errors(case)
    for k in want:
        assert same_bits(got[k], want[k]), (name, k)
    check_against_float64(got, case, name + " host twin")


def test_class_without_points_nan_and_behind_the_camera():
    case = hypotheses_case(3)
    got = host_errors(case)
    for k in ("add", "adds", "mssd", "mspd"):
        assert np.isposinf(got[k][0, 2]).all() and np.isposinf(got[k][1, 2]).all(), k      # outside the bank; count 0: never 0
        assert np.isnan(got[k][0, 0, 1]) and np.isfinite(got[k][0, 0, [0, 2]]).all(), k      # the NaN estimate, its neighbours
    for k in ("mssd_sym", "mspd_sym"):
        assert (got[k][0, 2] == -1).all() and (got[k][1, 2] == -1).all() and got[k][0, 0, 1] == -1
    assert np.isposinf(got["mspd"][1, 0, 0]) and got["mspd_sym"][1, 0, 0] == -1                # behind the camera: mspd alone
    assert np.isfinite(got["mssd"][1, 0, 0]) and got["mssd_sym"][1, 0, 0] >= 0 and np.isfinite(got["add"][1, 0, 0])
    assert np.isfinite(got["mspd"][1, 0, 1:]).all()


def test_only_the_outputs_asked_for():
    case = hypotheses_case(3)
    full = host_errors(case)
    for names in (("add",), ("adds",), ("mssd",), ("mspd",), ("add", "mspd")):
        got = host_errors(case, names)
        assert set(got) == {k for n in names for k in ((n,) if n in ("add", "adds") else (n, n + "_sym"))}
        for k in got:
            assert same_bits(got[k], full[k]), (names, k)


# ---- known answers by hand -------------------------------------------------------------------------------------------------------
def one_object(points, syms, gt, est, outputs=("add", "adds", "mssd", "mspd"), K=K4):
    points = np.asarray(points, np.float64)
    pts = np.ones((1, len(points), 4), F)
    pts[0, :, :3] = points
    syms = np.asarray(syms, F)[None]
    got = pe.evaluate_host(np.asarray(gt, F)[None, None], np.asarray(est, F)[None, None, None], [[0]], pts, [len(points)], syms,
                           [syms.shape[1]], K, outputs)
    return {k: v[0, 0, 0] for k, v in got.items()}


def test_two_points_turned_by_pi():
    a = 0.125
    model = [[a, 0, 0], [-a, 0, 0]]
    gt = np.array([[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 1.0]])
    est = compose(gt, np.array([[-1.0, 0, 0, 0], [0, -1, 0, 0], [0, 0, 1, 0]]))
    alone = one_object(model, [EYE], gt, est)
    assert alone["add"] == 2 * a and alone["adds"] == 0 and alone["mssd"] == 2 * a and alone["mssd_sym"] == 0
    both = one_object(model, [EYE, rot([0, 0, 1], np.pi)[:3]], gt, est)
    assert both["add"] == 2 * a and both["adds"] == 0
    assert both["mssd"] <= R.tol(1.2) and both["mssd_sym"] == 1 and both["mspd_sym"] == 1


def test_pure_translation():
    rng = np.random.default_rng(5)
    model = rng.uniform(-0.1, 0.1, (40, 3))
    gt = random_poses(rng, ())
    d = np.array([0.03, -0.04, 0.12])                                         # |d| = 0.13
    est = gt.copy()
    est[:, 3] += d
    got = one_object(model, [EYE], gt, est)
    tol = R.tol(float(np.abs(gt[:, 3]).max()) + 0.3)
    assert abs(got["add"] - 0.13) <= tol and abs(got["mssd"] - 0.13) <= tol and got["adds"] <= 0.13 + tol


def test_translation_along_x_in_pixels():
    model = [[0.0625, 0.03125, 0], [-0.125, 0.0625, 0], [0, -0.09375, 0]]     # flat and dyadic: every product below is exact
    gt = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.0]])
    est = gt.copy()
    est[0, 3] = 0.25
    got = one_object(model, [EYE], gt, est, K=(64.0, 48.0, 31.5, 23.5))
    assert got["mspd"] == 64.0 * 0.25 / 2.0 and got["mspd_sym"] == 0           # fx |d| / Z


def test_cube_diameter():
    s = 0.5
    corners = np.ones((1, 8, 4), F)
    corners[0, :, :3] = [[x, y, z] for x in (0, s) for y in (0, s) for z in (0, s)]
    got = pe.diameter_host(corners, [8])
    assert abs(float(got[0]) - s * np.sqrt(3.0)) <= 2.0 ** -24 and same_bits(got, R.diameter32(corners, [8]))


def test_diameter_of_the_five_classes():
    points, count, _, _ = five_class_bank()
    got, want, exact = pe.diameter_host(points, count), R.diameter32(points, count), R.diameter64(points, count)
    assert same_bits(got, want) and got[0] == 0 and got[1] == 0
    assert np.abs(got - exact).max() <= R.tol(0.2)


# ---- ties ------------------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_index():
    rng = np.random.default_rng(9)
    model = rng.uniform(-0.1, 0.1, (70, 3))
    M = rot([0.3, -0.2, 1.0], 2.1)[:3]
    syms = np.stack([EYE, M, M, EYE]).astype(F)
    gt = random_poses(rng, ())
    pts = np.ones((1, 70, 4), F)
    pts[0, :, :3] = model
    for S, want_idx in ((syms[1].astype(np.float64), 1), (EYE.astype(np.float64), 0)):
        est = compose(compose(gt, S), np.array([[1.0, 0, 0, 0.004], [0, 1, 0, -0.002], [0, 0, 1, 0.003]]))
        got = one_object(model, syms, gt, est)
        assert got["mssd_sym"] == want_idx and got["mspd_sym"] == want_idx
        want = R.errors32(pts, [70], syms[None], [4], np.zeros((1, 1), np.int32), gt.astype(F)[None, None], est.astype(F)[None, None, None], K4)
        for k, v in want.items():
            assert same_bits(np.asarray(got[k]).reshape(1, 1, 1), v), k


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def good():
    return pe.make_params(K4, 3, 5)


def test_a_good_record_passes():
    rec = pe.check_params(good())
    assert rec.dtype == _abi.POSE_ERROR_PARAMS_DTYPE and rec.itemsize == 32
    for name, v in (("n_objects", 1), ("n_objects", 64), ("n_hypotheses", 1), ("n_hypotheses", 100000), ("outputs", 1), ("outputs", 8),
                    ("cx", -3.5)):
        p = good()
        p[name] = v
        pe.check_params(p)


@pytest.mark.parametrize("name,value,word", [
    ("fx", 0.0, "fx"), ("fy", -1.0, "fx"), ("fx", np.inf, "finite"), ("cx", np.nan, "finite"), ("cy", -np.inf, "finite"),
    ("n_objects", 0, "n_objects"), ("n_objects", 65, "n_objects"), ("n_hypotheses", 0, "n_hypotheses"),
    ("outputs", 0, "outputs"), ("outputs", 16, "outputs"),
])
def test_check_params_refuses_each_broken_rule(name, value, word):
    p = good()
    p[name] = value
    with pytest.raises(_abi.SlhipError) as e:
        pe.check_params(p)
    assert word in str(e.value)
    assert _abi.lib().slhip_pose_error_check_params(None) < 0
    with pytest.raises(ValueError):
        pe.make_params(K4, 3, 5, outputs=("vsd",))


def host_call(null=None, misalign=None, n_points=None, n_symmetries=None, n_assets=None, stride=1, Hy=2, outputs=R.ALL, diameter=False):
    """slhip_pose_error_host (or _diameter_host) on a small good call with one thing wrong"""
    pts = np.ones((2, 9, 4), F)
    raw = np.zeros(2 * 9 * 16 + 32, np.uint8)                                 # room to place the points 4 bytes off
    at = raw.ctypes.data + (-raw.ctypes.data) % 16 + (4 if misalign == "points" else 0)
    C.memmove(at, pts.ctypes.data, pts.nbytes)
    count, n_sym = np.array([9, 4], np.int32), np.array([1, 1], np.int32)
    syms = np.tile(EYE, (2, 2, 1, 1)).astype(F)
    sym_at = syms.ctypes.data + (8 if misalign == "symmetries" else 0)
    ptrs = dict(points=at, count=count.ctypes.data, symmetries=sym_at, n_sym=n_sym.ctypes.data)
    if null in ptrs:
        ptrs[null] = None
    rec = _abi.PoseBank(ptrs["points"], ptrs["count"], ptrs["symmetries"], ptrs["n_sym"], 2 if n_assets is None else n_assets,
                        9 if n_points is None else n_points, 2 if n_symmetries is None else n_symmetries, 0)
    L = _abi.lib()
    if diameter:
        d = np.full(2, 7.0, F)
        st = L.slhip_pose_error_diameter_host(None if null == "bank" else C.byref(rec), None if null == "out" else d.ctypes.data)
        return st, d
    p = pe.make_params(K4, 3, Hy, outputs).reshape(1)
    cls, gt, est = np.zeros((1, 3), np.int32), np.tile(EYE, (1, 3, 1, 1)), np.tile(EYE, (1, 3, max(Hy, 1), 1, 1))
    outs = {k: np.full((1, 3, max(Hy, 1)), 7, F if "sym" not in k else np.int32) for k in ("add", "adds", "mssd", "mssd_sym", "mspd", "mspd_sym")}
    o = _abi.PoseErrorOut(*(None if null == k else outs[k].ctypes.data for k in ("add", "adds", "mssd", "mssd_sym", "mspd", "mspd_sym")))
    st = L.slhip_pose_error_host(None if null == "params" else p.ctypes.data, None if null == "bank" else C.byref(rec),
                                 None if null == "classes" else cls.ctypes.data, stride, None if null == "gt" else gt.ctypes.data,
                                 None if null == "est" else est.ctypes.data, 1, None if null == "record" else C.byref(o))
    return st, outs


REFUSALS = [dict(null="params"), dict(null="bank"), dict(null="points"), dict(null="count"), dict(null="symmetries"), dict(null="n_sym"),
            dict(null="classes"), dict(null="gt"), dict(null="est"), dict(null="record"), dict(null="add"), dict(null="adds"),
            dict(null="mssd"), dict(null="mssd_sym"), dict(null="mspd"), dict(null="mspd_sym"), dict(misalign="points"),
            dict(misalign="symmetries"), dict(n_points=0), dict(n_points=4097), dict(n_symmetries=0), dict(n_symmetries=1025),
            dict(n_assets=0), dict(n_assets=1025), dict(stride=0), dict(Hy=0), dict(outputs=0), dict(outputs=32)]


def test_the_entries_refuse_each_bad_argument():
    st, outs = host_call()
    assert st == 0 and all((v != 7).all() for v in outs.values())
    st, outs = host_call(null="add", outputs=R.ALL & ~R.ADD)                   # an output that is not named may be null ...
    assert st == 0 and (outs["add"] == 7).all() and (outs["adds"] != 7).all()  # ... and is not touched
    for kw in REFUSALS:
        st, outs = host_call(**kw)
        assert st < 0, kw
        assert all((v == 7).all() for v in outs.values()), kw
        assert _abi.lib().slhip_last_error(), kw
    for kw in (dict(null="bank"), dict(null="points"), dict(null="count"), dict(null="out"), dict(misalign="points"), dict(n_points=0),
               dict(n_points=4097), dict(n_symmetries=1025), dict(n_assets=0)):
        st, d = host_call(diameter=True, **kw)
        assert st < 0 and (d == 7).all(), kw
    st, d = host_call(diameter=True)
    assert st == 0 and d[0] == 0 and d[1] == 0                                 # all points equal


# ---- the Python surface on CPU tensors -----------------------------------------------------------------------------------------------
def cpu_bank():
    points, count, syms, n_sym = (torch.from_numpy(np.ascontiguousarray(a)) for a in five_class_bank())
    bank = pe.ModelBank(points, count, syms, n_sym)
    bank.diameter = torch.from_numpy(pe.diameter_host(points.numpy(), count.numpy()))
    return bank


def test_add_auto_closest_gt_and_recall():
    case, bank = hypotheses_case(3), cpu_bank()
    got = {k: torch.from_numpy(v) for k, v in host_errors(case).items()}
    err = pe.PoseErrors(torch.from_numpy(case.classes), **got)
    auto = err.add_auto(bank)
    sym = np.array([[True, True, False], [True, False, False]])              # n_sym > 1; the class outside the bank is not
    assert same_bits(auto[torch.from_numpy(sym)].numpy(), err.adds[torch.from_numpy(sym)].numpy())
    assert same_bits(auto[torch.from_numpy(~sym)].numpy(), err.add[torch.from_numpy(~sym)].numpy())
    gt = torch.from_numpy(case.gt)
    near = err.closest_gt(gt, bank).numpy()
    assert near.shape == (2, 3, 3, 3, 4)
    tol, _ = case.bounds()
    for b in range(2):
        for o in range(3):
            for h in range(3):
                s = int(got["mssd_sym"][b, o, h])
                S = case.syms[case.classes[b, o], s].astype(np.float64) if s >= 0 else EYE.astype(np.float64)
                assert np.abs(near[b, o, h] - compose(case.gt[b, o].astype(np.float64), S)).max() <= tol, (b, o, h)
    assert same_bits(near[0, 2], np.broadcast_to(case.gt[0, 2], (3, 3, 4)).copy())      # index -1: the ground truth itself
    # the estimate was gt * S * (a small motion): the closest ground truth is at most that motion away from it
    assert np.abs(near[1, 0, 1:, :, 3] - case.est[1, 0, 1:, :, 3]).max() < 0.05
    finite = np.isfinite(host_errors(case)["add"])
    r = err.recall("add", [0.0, 0.01, 1e9])
    add = got["add"].numpy()
    assert r.tolist() == pytest.approx([0.0, float((add[finite] <= 0.01).sum()) / finite.sum(), 1.0])
    rd = err.recall("mssd", [0.1, 1e9], bank)
    d = bank.diameter.numpy()[np.clip(case.classes, 0, 4)][..., None]
    mssd = got["mssd"].numpy()
    ok = np.isfinite(mssd)
    assert rd.tolist() == pytest.approx([float(((mssd <= np.float32(0.1) * d) & ok).sum()) / ok.sum(), float((ok & (d > 0)).sum()) / ok.sum()])
    with pytest.raises(RuntimeError):
        pe.PoseErrors(err.classes, add=err.add).recall("mspd", [1.0])
    one = pe.PoseErrors(err.classes, **{k: v[:, :, 0] for k, v in got.items()})      # without the hypothesis axis
    assert tuple(one.add_auto(bank).shape) == (2, 3) and tuple(one.closest_gt(gt, bank).shape) == (2, 3, 3, 4)


def test_bank_symmetry_dictionaries():
    from stillleben_amd.pose_error import _symmetry_tensor

    flip = rot([1, 0, 0], np.pi)
    sym, n_sym = _symmetry_tensor(3, {1: [flip]}, None, 0.01, 1.0, torch.device("cpu"))
    assert n_sym.tolist() == [1, 2, 1] and tuple(sym.shape) == (3, 2, 3, 4)
    assert same_bits(sym[0].numpy(), np.tile(EYE, (2, 1, 1))) and same_bits(sym[1, 0].numpy(), EYE)
    info = {"5": {"diameter": 100.0, "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]},
            "9": {"symmetries_discrete": [list(flip.reshape(-1))]}}
    sym, n_sym = _symmetry_tensor(3, info, {0: 9, 2: 5}, 0.01, 0.001, torch.device("cpu"))
    assert n_sym.tolist() == [2, 1, 315] and tuple(sym.shape) == (3, 315, 3, 4)
    with pytest.raises(ValueError) as e:
        _symmetry_tensor(3, info, {0: 9, 2: 5}, 0.001, 0.001, torch.device("cpu"))
    assert "2 (object 5)" in str(e.value)


def test_host_tensors_are_refused():
    bank = cpu_bank()
    o2c = torch.zeros((1, 2, 3, 4))
    with pytest.raises(_abi.SlhipError) as e:
        pe.evaluate(o2c, torch.zeros((1, 2, 3, 4)), torch.zeros((1, 2), dtype=torch.int32), bank, K4)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError) as e:
        pe.diameters(bank)
    assert "no CPU path" in str(e.value)
    with pytest.raises(TypeError):
        pe.evaluate(o2c, o2c, torch.zeros((1, 2), dtype=torch.int32), bank.points, K4)
    with pytest.raises(ValueError):
        pe.ModelBank(bank.points, bank.count, bank.symmetries[:, :, :2], bank.n_sym)


def test_header_declares_the_entries_and_the_version_stays():
    import os

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "slhip.h")).read()
    for name in ("_check_params", "_diameter", "_diameter_host", "", "_host", "_timing_enable", "_timings"):
        assert "int slhip_pose_error%s(" % name in text, name
        assert hasattr(_abi.lib(), "slhip_pose_error%s" % name), name
    assert "#define SLHIP_ABI_VERSION 5 " in text and _abi.ABI_VERSION == 5
    import stillleben_amd as sl

    assert sl.pose_error is pe and sl.ModelBank is pe.ModelBank and sl.PoseErrors is pe.PoseErrors
