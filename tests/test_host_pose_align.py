"""The robust alignment on the host (slhip_pose_align_host, slhip_pose_align_check_params, sl.pose_align) against the independent
float64 implementation tests/pose_align_ref.py and against answers known by hand.  Needs no device.

The tolerance.  Correspondences are exact rigid motions rounded to float32 (an object of 0.1 m about a metre from the camera),
so even a float64 fit of the untouched rows misses the exact motion by what that rounding leaves.  That miss -- the reference's
own deviation -- is computed here on every run over all 640 damaged sets of FAMILIES, and a pose of the library must lie within
four times the worst of them (the convention of tests/test_host_pose_fit.py: one bound over all sizes), of the exact motion and
of the reference's pose alike.  Nothing here is a constant taken from the library's output.  One run gives
    the float64 fit against the exact motion, worst of 640:  6.5e-6 rad, 2.4e-7 m  (the sets of K = 5 with three untouched rows)
    the library against the exact motion, worst per family (K, damaged):  (256, 102) 3.7e-7 rad, 2.4e-7 m;  (9, 2) 1.1e-6 rad,
    1.3e-7 m;  (9, 3) 1.3e-6 rad, 1.7e-7 m;  (5, 2) 2.0e-5 rad, 4.9e-7 m  (bound 2.6e-5 rad, 9.8e-7 m)
A bound per family does not serve: the float64 fit of the 154 untouched rows of K = 256 lies 5.7e-9 m from the exact translation,
and four times that is below the half unit in the last place (6e-8 m) to which float32 stores a translation of a metre -- no
float32 pose can meet it.  DESIGN.md "Robust alignment" records the figures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_align_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_align as pa
from stillleben_amd import pose_fit as pf

F = np.float32
NAMES = ("pose", "n_inliers", "rms", "inliers", "best", "flags")
POISON = 0x5A5A5A5A
THR = 1e-3      # m: far above the rounding of the coordinates (6e-8 m at 1 m), 50 times below the smallest damage


def points4(xyz, w=1.0):
    out = np.full((len(xyz), 4), w, F)
    out[:, :3] = xyz
    return out


def moved(src, Rm, t):
    """dst of src [K, 4] under (Rm, t), rounded to float32"""
    return points4(np.asarray(src, np.float64)[:, :3] @ np.asarray(Rm, np.float64).T + t)


def damaged_case(K, n_bad, seed):
    """(src, dst float32 [K, 4], pose float64 [3, 4], clean bool [K]): an object of 0.1 m about a metre from the camera, exact
    correspondences rounded to float32; then the object coordinates of n_bad rows moved by 0.05 to 0.3 m in a random direction"""
    rng = np.random.default_rng(seed)
    Rm, t = R.random_rotation(rng), np.array([0.1, -0.05, 1.0]) + rng.normal(size=3) * 0.1
    src = points4((rng.random((K, 3)) - 0.5) * 0.1)
    dst = moved(src, Rm, t)
    clean = np.ones(K, bool)
    bad = rng.permutation(K)[:n_bad]
    d = rng.normal(size=(n_bad, 3))
    src[bad, :3] += (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.05, 0.3, (n_bad, 1))).astype(F)
    clean[bad] = False
    return src, dst, np.concatenate([Rm, t[:, None]], 1), clean


def solve_one(src, dst, init=None, **kw):
    kw.setdefault("threshold", THR)
    return pa.solve_host(src[None], dst[None], None if init is None else np.asarray(init, F)[None], **kw)


def deviation(pose, exact):
    return np.array([R.rotation_angle(pose, exact), R.translation_distance(pose, exact)])


def reference_deviation(src, dst, clean, exact):
    """(rad, m): how far the float64 fit of the untouched rows lies from the exact motion -- the float32 inputs' share"""
    return deviation(R.kabsch(src[clean, :3], dst[clean, :3]), exact)


def assert_none(r, flag, m=0):
    """NaN, never an identity and never the initial pose"""
    assert r.flags[m] == flag and r.n_inliers[m] == 0 and r.best[m] == -2 and not r.found[m]
    assert np.isnan(r.pose[m]).all() and np.isnan(r.rms[m]) and not r.inliers[m].any() and not r.inlier_mask()[m].any()


def same_bytes(a, b, names=NAMES):
    for k in names:
        assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), k


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------
CUBE = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]) * 0.25      # exact in float32


def test_identity():
    src = points4(CUBE)
    r = solve_one(src, src, seed=1)
    assert np.array_equal(r.pose[0], np.eye(4, dtype=F)[:3]) and r.rms[0] == 0.0 and r.n_inliers[0] == 8 and r.flags[0] == 0
    assert r.best[0] >= 0 and r.inlier_mask()[0].all() and r.found[0]


def test_pure_translation():
    src = points4(CUBE)
    r = solve_one(src, moved(src, np.eye(3), [0.5, -0.25, 2.0]), seed=2)
    assert np.array_equal(r.pose[0], F([[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 2.0]])) and r.rms[0] == 0.0 and r.n_inliers[0] == 8


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_quarter_turn_about_an_axis(axis):
    Rm = np.eye(3)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    Rm[i, i], Rm[i, j], Rm[j, i], Rm[j, j] = 0, -1, 1, 0
    src = points4(CUBE + [0.125, 0.25, -0.0625])
    dst = moved(src, Rm, [0.5, -0.25, 2.0])
    r = solve_one(src, dst, seed=3)
    exact = np.concatenate([Rm, [[0.5], [-0.25], [2.0]]], 1)
    # the correspondences are exact in float32, so the float64 fit is exact too: the bound is the float32 arithmetic's, a few
    # roundings of numbers of size 1 (rotation) and 2 (translation)
    assert r.flags[0] == 0 and r.n_inliers[0] == 8 and r.inlier_mask()[0].all()
    assert np.abs(r.pose[0] - exact).max() <= 8 * np.finfo(F).eps * 2.0, r.pose[0]
    # all eight are inliers, so the refit is the plain fit of the same eight, to the bit
    assert np.array_equal(r.pose[0], pf.solve_host(src[None], dst[None]).pose[0])


def test_four_coplanar_points_give_a_proper_rotation():
    """the third singular value of the moments is 0, so an SVD route without the determinant correction returns a reflection for
    about every other motion; Horn's quaternion, in the samples and in the refit, cannot"""
    flat = np.array([[-0.1, -0.05, 0.0], [0.1, -0.05, 0.0], [0.1, 0.05, 0.0], [-0.1, 0.07, 0.0]])
    cases = []
    for seed in range(12):
        rng = np.random.default_rng(seed)
        Rm, t = R.random_rotation(rng), np.array([0.0, 0.0, 1.0])
        src = points4(flat)
        cases.append((src, moved(src, Rm, t), np.concatenate([Rm, t[:, None]], 1)))
    # four times the float64 fit's own deviation, plus what storing a pose in float32 costs at best: half a unit in the last
    # place of each of nine entries up to 1 and of three translations up to 1 m (the deviation alone is below that here)
    half_ulp = float(np.finfo(F).eps) / 2.0
    bound = 4 * np.max([reference_deviation(s, d, np.ones(4, bool), e) for s, d, e in cases], 0) + [3.0 * half_ulp, np.sqrt(3.0) * half_ulp]
    for seed, (src, dst, exact) in enumerate(cases):
        r = solve_one(src, dst, seed=seed)
        assert r.flags[0] == 0 and r.n_inliers[0] == 4
        Rg = r.pose[0, :, :3].astype(np.float64)
        assert abs(np.linalg.det(Rg) - 1.0) <= 1e-5 and np.abs(Rg @ Rg.T - np.eye(3)).max() <= 1e-5, seed
        assert (deviation(r.pose[0], exact) <= bound).all(), (seed, deviation(r.pose[0], exact), bound)


# ---- 2. damaged sets: exactly the untouched rows, and the pose of the float64 fit of them -----------------------------------------
FAMILIES = [(256, 102, 40), (9, 2, 200), (9, 3, 200), (5, 2, 200)]      # K, damaged rows (40 % of 256), seeded cases


@pytest.fixture(scope="module")
def families():
    """({(K, n_bad): cases}, the bound: 4 x the worst deviation of the float64 fit of the untouched rows from the exact motion
    over all cases, (rad, m))"""
    out, worst = {}, np.zeros(2)
    for K, n_bad, n in FAMILIES:
        out[K, n_bad] = cases = [damaged_case(K, n_bad, 1000 * K + 10 * n_bad + s) for s in range(n)]
        dev = np.max([reference_deviation(s, d, c, e) for s, d, e, c in cases], 0)
        print("pose_align K %d, %d damaged: the float64 fit of the untouched rows lies %.3g rad, %.3g m from the exact motion at worst"
              % (K, n_bad, dev[0], dev[1]))
        worst = np.maximum(worst, dev)
    return out, 4 * worst


@pytest.mark.parametrize("K,n_bad,n", FAMILIES)
def test_damaged_sets_recover_the_untouched_rows(families, K, n_bad, n):
    cases, bound = families[0][K, n_bad], families[1]
    worst = np.zeros(2)
    for i, (src, dst, exact, clean) in enumerate(cases):
        r = solve_one(src, dst, seed=7, set_id_base=i)
        assert r.found[0] and np.array_equal(r.inlier_mask()[0], clean), "case %d: %d inliers, %d untouched rows" % (i, r.n_inliers[0], clean.sum())
        assert r.n_inliers[0] == clean.sum() and r.best[0] >= 0
        worst = np.maximum(worst, deviation(r.pose[0], exact))
    print("pose_align K %d, %d damaged: worst %.3g rad, %.3g m from the exact motion (bound %.3g rad, %.3g m)" % (K, n_bad, *worst, *bound))
    assert (worst <= bound).all(), (worst, bound)


@pytest.mark.parametrize("K,n_bad,n", FAMILIES)
def test_least_squares_is_ruined_by_the_same_sets(families, K, n_bad, n):
    """the contrast: pose_fit on the damaged sets is more than 100 bounds off, pose_align (above) inside one"""
    cases, bound = families[0][K, n_bad], families[1]
    for src, dst, exact, clean in cases[:20]:
        fit = pf.solve_host(src[None], dst[None])
        assert fit.flags[0] == 0 and (deviation(fit.pose[0], exact) > 100 * bound).all(), deviation(fit.pose[0], exact)


# ---- 3. the pipeline against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n_bad", [(3, 0), (4, 1), (257, 77), (1024, 307)])
def test_pipeline_against_the_reference(families, K, n_bad):
    cases, bound = [damaged_case(K, n_bad, 77 * K + s) for s in range(4)], families[1]
    for i, (src, dst, exact, clean) in enumerate(cases):
        kw = dict(n_hypotheses=48, refine_iters=2, seed=0x1234567812345678 + i, set_id_base=5 * i)
        r = solve_one(src, dst, **kw)
        ref = R.solve(src, dst, THR, n_hypotheses=48, refine_iters=2, seed=kw["seed"], set_id=5 * i)
        assert r.flags[0] == ref.flags == 0 and r.best[0] == ref.best, (K, i, r.best[0], ref.best)
        assert np.array_equal(r.inlier_mask()[0], ref.inliers) and np.array_equal(ref.inliers, clean) and r.n_inliers[0] == ref.n_inliers
        assert (deviation(r.pose[0], ref.pose) <= bound).all(), (K, i, deviation(r.pose[0], ref.pose), bound)
        # two poses a bound apart move a residual by at most the translations' distance plus the angle times the object's 0.1 m
        assert abs(float(r.rms[0]) - ref.rms) <= bound[1] + 0.1 * bound[0], (K, i, float(r.rms[0]), ref.rms)


# ---- 4. failures -----------------------------------------------------------------------------------------------------------------
def test_fewer_than_three_valid_is_insufficient():
    src, dst, _, _ = damaged_case(9, 0, 1)
    for keep in (0, 1, 2):
        s2 = src.copy()
        s2[keep:, 3] = 0.0
        assert_none(solve_one(s2, dst), _abi.ALIGN_INSUFFICIENT)
        assert R.solve(s2, dst, THR).flags == R.INSUFFICIENT
    ident = np.eye(4, dtype=F)[:3]
    s2 = src.copy()
    s2[2:, 0] = np.nan
    assert_none(solve_one(s2, dst, init=ident), _abi.ALIGN_INSUFFICIENT)      # never the initial pose


def test_collinear_points_have_no_model():
    rng = np.random.default_rng(2)
    Rm, t = R.random_rotation(rng), np.array([0.1, 0.0, 1.0])
    line = points4(np.outer(np.linspace(-0.1, 0.1, 9), [0.6, 0.0, 0.8]) + [0.01, 0.02, 0.03])
    assert_none(solve_one(line, moved(line, Rm, t)), _abi.ALIGN_NO_MODEL)
    assert R.solve(line, moved(line, Rm, t), THR).flags == R.NO_MODEL
    spot = points4(np.tile([0.01, 0.02, 0.03], (5, 1)))
    assert_none(solve_one(spot, spot), _abi.ALIGN_NO_MODEL)


def test_min_inliers_above_what_exists_has_no_model():
    src, dst, exact, clean = damaged_case(9, 3, 4)
    assert solve_one(src, dst, min_inliers=6).n_inliers[0] == 6
    assert_none(solve_one(src, dst, min_inliers=7), _abi.ALIGN_NO_MODEL)
    assert_none(solve_one(src, dst, min_inliers=7, init=exact), _abi.ALIGN_NO_MODEL)      # 6 inliers: never the initial pose
    assert R.solve(src, dst, THR, min_inliers=7).flags == R.NO_MODEL


@pytest.mark.parametrize("K", [40, 200])
def test_invalid_rows_are_left_out_of_the_list(K):
    """NaN and w = 0 rows scattered through the set: the list, hence the picks, the winner and the refit, are those of the set
    without them (the sums of the final pass run in other lanes, so the rms may differ in its last bits)"""
    src, dst, exact, clean = damaged_case(K, K // 4, 5)
    rng = np.random.default_rng(6)
    slots = np.sort(rng.permutation(K + 12)[:K])
    s2, d2 = np.ones((K + 12, 4), F), np.ones((K + 12, 4), F)
    s2[slots], d2[slots] = src, dst
    gaps = np.setdiff1d(np.arange(K + 12), slots)
    kinds = [(s2, 3, 0.0), (s2, 3, -1.0), (d2, 3, 0.0), (s2, 0, np.nan), (d2, 1, np.nan), (d2, 2, np.inf)]
    for n, j in enumerate(gaps):
        a, col, v = kinds[n % len(kinds)]
        a[j, col] = v
    r, want = solve_one(s2, d2, seed=9), solve_one(src, dst, seed=9)
    same_bytes(r, want, ("pose", "n_inliers", "best", "flags"))
    assert want.flags[0] == 0 and np.array_equal(r.inlier_mask()[0][slots], clean) and not r.inlier_mask()[0][gaps].any()
    assert abs(float(r.rms[0]) - float(want.rms[0])) <= 1e-6 * float(want.rms[0]) + 1e-12
    ref = R.solve(s2, d2, THR, seed=9)
    assert ref.best == r.best[0] and np.array_equal(ref.inliers, r.inlier_mask()[0])


# ---- 5. the initial pose ---------------------------------------------------------------------------------------------------------
def test_initial_pose_wins_a_tie_and_a_nan_one_is_ignored():
    src, dst, exact, clean = damaged_case(64, 20, 11)
    plain = solve_one(src, dst, seed=3)
    assert plain.best[0] >= 0 and plain.n_inliers[0] == 44
    r = solve_one(src, dst, init=exact, seed=3)      # 44 inliers as well: the lowest slot wins
    assert r.best[0] == -1 and r.n_inliers[0] == 44 and r.flags[0] == 0 and np.array_equal(r.inlier_mask()[0], clean)
    assert R.solve(src, dst, THR, seed=3, init=exact).best == -1
    bad = exact.copy()
    bad[1, 2] = np.nan
    same_bytes(solve_one(src, dst, init=bad, seed=3), plain)
    far = exact.copy()
    far[:, 3] += 0.5      # a finite pose without inliers competes and loses
    same_bytes(solve_one(src, dst, init=far, seed=3), plain)


def test_no_hypotheses_is_a_pure_refit():
    src, dst, exact, clean = damaged_case(64, 20, 12)
    near = exact.copy()
    near[:, 3] += [4e-4, -3e-4, 2e-4]      # inside the threshold: the untouched rows are its inliers
    r = solve_one(src, dst, init=near, n_hypotheses=0)
    assert r.best[0] == -1 and r.flags[0] == 0 and np.array_equal(r.inlier_mask()[0], clean)
    # the refit is the plain fit of the inliers in their lanes: pose_fit with the damaged rows' weights at 0, to the bit
    masked = src.copy()
    masked[~clean, 3] = 0.0
    fit = pf.solve_host(masked[None], dst[None])
    assert np.array_equal(r.pose[0], fit.pose[0]) and r.rms[0] == fit.rms[0] and r.n_inliers[0] == fit.n_used[0] == 44
    kept = solve_one(src, dst, init=near, n_hypotheses=0, refine_iters=0)
    assert np.array_equal(kept.pose[0], near.astype(F)) and kept.best[0] == -1 and kept.rms[0] > 4e-4
    far = exact.copy()
    far[:, 3] += 0.5
    assert_none(solve_one(src, dst, init=far, n_hypotheses=0), _abi.ALIGN_NO_MODEL)
    far[0, 0] = np.nan
    assert_none(solve_one(src, dst, init=far, n_hypotheses=0), _abi.ALIGN_NO_MODEL)


def test_a_refit_that_loses_inliers_is_rejected():
    """ten rows under the identity: seven exact, two 0.99 thresholds off along +x, one 0.99 along -x.  All ten are inliers of the
    identity; their least-squares fit moves about 0.1 threshold along +x, which puts the last row outside: nine inliers, fewer
    than the ten the identity scored, so the identity is returned with REFINE_REJECTED"""
    rng = np.random.default_rng(13)
    src = points4((rng.random((10, 3)) - 0.5) * 0.25)
    dst = src.copy()
    thr = 0.125
    dst[7:9, 0] += F(0.99 * thr)
    dst[9, 0] -= F(0.99 * thr)
    ident = np.eye(4, dtype=F)[:3]
    for iters in (1, 4):
        r = solve_one(src, dst, init=ident, n_hypotheses=0, threshold=thr, refine_iters=iters)
        assert r.flags[0] == _abi.ALIGN_REFINE_REJECTED and r.best[0] == -1 and r.n_inliers[0] == 10 and r.inlier_mask()[0].all()
        assert np.array_equal(r.pose[0], ident)
        ref = R.solve(src, dst, thr, n_hypotheses=0, refine_iters=iters, init=ident)
        assert ref.flags == R.REFINE_REJECTED and ref.n_inliers == 10
    assert solve_one(src, dst, init=ident, n_hypotheses=0, threshold=thr, refine_iters=0).flags[0] == 0


def test_a_refit_without_three_inliers_stops():
    """an initial pose with min_inliers = 3 inliers that are collinear: the refit is degenerate, the pose stays"""
    line = points4(np.outer([-0.1, 0.0, 0.1], [1.0, 0.0, 0.0]))
    src = np.concatenate([line, points4([[0.0, 0.1, 0.0], [0.0, -0.1, 0.05]])])
    dst = src.copy()
    dst[3:, :3] += 0.5
    ident = np.eye(4, dtype=F)[:3]
    r = solve_one(src, dst, init=ident, n_hypotheses=0)
    assert r.flags[0] == _abi.ALIGN_REFINE_STOPPED and np.array_equal(r.pose[0], ident) and r.n_inliers[0] == 3 and r.best[0] == -1
    assert R.solve(src, dst, THR, n_hypotheses=0, init=ident).flags == R.REFINE_STOPPED


# ---- 6. parameters, arguments, outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,word", [
    ("n_points", 2, "n_points"), ("n_points", 4097, "n_points"), ("n_hypotheses", 4097, "n_hypotheses"), ("threshold", 0.0, "threshold"),
    ("threshold", -1.0, "threshold"), ("threshold", np.nan, "threshold"), ("threshold", np.inf, "threshold"), ("min_gap", -1e-6, "min_gap"),
    ("min_gap", 1.0, "min_gap"), ("min_gap", np.nan, "min_gap"), ("refine_iters", 17, "refine_iters"), ("min_inliers", 2, "min_inliers"),
    ("outputs", 0, "outputs"), ("outputs", 64, "outputs")])
def test_check_params_names_the_broken_rule(field, value, word):
    p = pa.make_params(1, 16, THR)
    pa.check_params(p)
    p[field] = value
    with pytest.raises(_abi.SlhipError, match=word):
        pa.check_params(p)


def test_threshold_has_no_default():
    with pytest.raises(TypeError, match="threshold"):
        pa.make_params(1, 16)
    src, dst, _, _ = damaged_case(9, 0, 1)
    with pytest.raises(TypeError, match="threshold"):
        pa.solve_host(src[None], dst[None])


def host_call(null=None, misalign=None, mask=63, init=True, **fields):
    M, K = 2, 16
    src, dst, exact, _ = damaged_case(M * K, 4, 5)
    raw = {"src": np.zeros(M * K * 4 + 8, F), "dst": np.zeros(M * K * 4 + 8, F), "init": np.zeros(M * 12 + 8, F)}
    ptr = {}
    for k, a in (("src", src), ("dst", dst), ("init", np.stack([exact, exact]).astype(F))):
        shift = ((-raw[k].ctypes.data) % 16) // 4      # 16-byte aligned
        raw[k][shift:shift + a.size] = a.reshape(-1)
        ptr[k] = None if null == k else raw[k].ctypes.data + 4 * shift + ((2 if k == "init" else 4) if misalign == k else 0)
    if not init:
        ptr["init"] = None
    outs = {k: np.full(64, POISON, np.uint32) for k in NAMES}
    o = _abi.PoseAlignOut(*(None if null == k else outs[k].ctypes.data + (2 if misalign == k else 0) for k in NAMES))
    p = pa.make_params(M, K, THR, outputs=mask).reshape(1)
    for k, v in fields.items():
        p[k] = v
    st = _abi.lib().slhip_pose_align_host(None if null == "params" else p.ctypes.data, ptr["src"], ptr["dst"], ptr["init"],
                                          None if null == "record" else C.byref(o))
    return st, outs


REFUSALS = [(dict(null="params"), "null parameter record"), (dict(null="src"), "null argument"), (dict(null="dst"), "null argument"),
            (dict(null="record"), "null argument"), (dict(null="pose"), "null pointer"), (dict(null="inliers"), "null pointer"),
            (dict(null="flags"), "null pointer"), (dict(misalign="src"), "16-byte aligned"), (dict(misalign="dst"), "16-byte aligned"),
            (dict(misalign="init"), "initial poses 4-byte"), (dict(misalign="rms"), "4-byte aligned"),
            (dict(init=False, n_hypotheses=0), "needs an initial pose"), (dict(n_points=2), "n_points"), (dict(n_points=4097), "n_points"),
            (dict(n_hypotheses=4097), "n_hypotheses"), (dict(threshold=0.0), "threshold"), (dict(min_gap=1.0), "min_gap"),
            (dict(refine_iters=17), "refine_iters"), (dict(min_inliers=2), "min_inliers"), (dict(mask=0), "outputs"), (dict(mask=64), "outputs")]


@pytest.mark.parametrize("kw,text", REFUSALS)
def test_entries_refuse_bad_arguments(kw, text):
    st, outs = host_call(**kw)
    assert st < 0 and text in _abi.lib().slhip_last_error().decode(), _abi.lib().slhip_last_error()
    for k in NAMES:
        assert (outs[k] == POISON).all(), k
    assert host_call()[0] == 0 and host_call(init=False)[0] == 0 and host_call(null="init")[0] == 0


def test_no_sets_succeed_and_write_nothing():
    st, outs = host_call(n_sets=0)
    assert st == 0 and all((o == POISON).all() for o in outs.values())


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 1 | 32, 2 | 8])
def test_outputs_not_named_stay_poison(mask):
    st, outs = host_call(mask=mask)
    assert st == 0
    sizes = dict(pose=24, n_inliers=2, rms=2, inliers=2, best=2, flags=2)      # the words of two sets of 16 points
    for i, k in enumerate(NAMES):
        if not mask & (1 << i):
            assert (outs[k] == POISON).all(), k
        else:
            assert (outs[k][:sizes[k]] != POISON).all() and (outs[k][sizes[k]:] == POISON).all(), k
    st, full = host_call()
    for i, k in enumerate(NAMES):      # what one output holds does not depend on which others were asked for
        if mask & (1 << i):
            assert np.array_equal(outs[k], full[k]), k
    src, dst, _, _ = damaged_case(8, 0, 6)
    r = solve_one(src, dst, outputs=("pose",))
    assert r.rms is None and r.flags is None and r.best is None and r.found[0]
    with pytest.raises(RuntimeError, match="inliers"):
        r.inlier_mask()
    assert solve_one(src, dst, outputs=("best",)).found[0]


def test_failing_sets_inside_a_batch():
    src, dst, exact, clean = damaged_case(32, 8, 21)
    few, line = src.copy(), src.copy()
    few[2:, 3] = 0.0
    line[:, :3] = np.outer(np.linspace(-0.1, 0.1, 32), [0.6, 0.0, 0.8])
    S, D = np.stack([src, few, src, line, src]), np.stack([dst, dst, dst, moved(line, exact[:, :3], exact[:, 3]), dst])
    r = pa.solve_host(S, D, threshold=THR, seed=4)
    assert list(r.flags) == [0, _abi.ALIGN_INSUFFICIENT, 0, _abi.ALIGN_NO_MODEL, 0] and list(r.found) == [True, False, True, False, True]
    assert_none(r, _abi.ALIGN_INSUFFICIENT, 1)
    assert_none(r, _abi.ALIGN_NO_MODEL, 3)
    for m in (0, 2, 4):      # set m draws as set m: the same rows, other samples, the same inliers
        assert np.array_equal(r.inlier_mask()[m], clean)
        same_bytes(pa.solve_host(S[m:m + 1], D[m:m + 1], threshold=THR, seed=4, set_id_base=m), pa.PoseAlign(32, **{k: getattr(r, k)[m:m + 1] for k in NAMES}))
    d = r.dense(2, 3, [0, 0, 0, 1, 1], [1, 2, 3, 1, 2])
    assert np.array_equal(d[0, 0], r.pose[0]) and np.isnan(d[0, 1]).all() and np.array_equal(d[1, 1], r.pose[4]) and np.isnan(d[1, 2]).all()


def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5" in text and _abi.ABI_VERSION == 5 and _abi.lib().slhip_abi_version() == 5
    for name in ("slhip_pose_align_check_params", "slhip_pose_align", "slhip_pose_align_host", "slhip_pose_align_timing_enable",
                 "slhip_pose_align_timings"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name), name
    assert _abi.POSE_ALIGN_PARAMS_DTYPE.itemsize == 64 and "} slhip_pose_align_params; /* 64 bytes */" in text
    for name, value in (("POINTS_MAX", _abi.ALIGN_POINTS_MAX), ("HYPOTHESES_MAX", _abi.ALIGN_HYPOTHESES_MAX), ("REFINE_MAX", _abi.ALIGN_REFINE_MAX)):
        assert re.search(r"#define SLHIP_ALIGN_%s\s+%du\b" % (name, value), text), name
    for name, bit in pa.OUTPUTS.items():
        assert re.search(r"#define SLHIP_ALIGN_OUT_%s\s+%du\b" % (name.upper(), bit), text), name
    for name, bit in pa.FLAGS.items():
        assert re.search(r"#define SLHIP_ALIGN_%s\s+%d\b" % (name.upper(), bit), text), name
    assert pa.PoseAlign.FAILED == _abi.ALIGN_INSUFFICIENT | _abi.ALIGN_NO_MODEL
    rules = open(os.path.join(root, "stillleben_amd", "csrc", "slhip_align_rules.h")).read()
    assert "constexpr uint32_t STREAM = %du;" % R.STREAM in rules and _abi.SYNTH_STREAM_ALIGN == R.STREAM and "Stream 9, alignment samples" in text
    import stillleben as alias
    import stillleben_amd as sl
    assert sl.pose_align is pa and alias.pose_align is pa and sl.PoseAlign is pa.PoseAlign and "pose_align" in sl.__all__
    assert alias.PoseAlign is pa.PoseAlign and hasattr(sl.SceneBatch, "pose_align")


def test_cpu_tensors_are_refused():
    import torch

    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        pa.solve(torch.ones((1, 8, 4)), torch.ones((1, 8, 4)), threshold=THR)
