"""The rigid fit on the host (slhip_pose_fit_host, slhip_pose_fit_check_params, sl.pose_fit) against two float64 references
(tests/pose_fit_ref.py: Kabsch by SVD with the determinant correction as the independent answer, the 4 x 4 route of the rules in
float64) and against answers known by hand.  Needs no device.

The tolerance.  T_ROT bounds the angle between the float32 twin's rotation and fit_svd's, T_TRANS the distance of the
translations: each is four times the worst difference over the random rigid motions of test_random_motions_against_svd (N in
3, 4, 9, 64, 65, 1024; points of an object's size, 0.1 m, about a metre from the camera, exact correspondences rounded to
float32), measured there on every run and printed; the constants below record it.
    measured worst:  rotation 1.2e-6 rad,  translation 2.1e-7 m  (fit_svd against the exact motions: 2.4e-6 rad)
The rotation error is the data's: three points 0.1 m apart whose float32 coordinates near 1 m carry 6e-8 m of rounding determine
a rotation to about 1e-6 rad, whatever solves for it (the float64 SVD on the same float32 inputs lies further from the exact
motion than the twin lies from the SVD).  With 8 sweeps nothing measurable is left off the diagonal: test_eight_sweeps_leave_nothing_off_the_diagonal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_fit_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_fit as pf

F = np.float32
T_ROT = 4 * 1.2e-6           # rad; 4 x the measured worst 1.2e-6
T_TRANS = 4 * 2.1e-7         # m; 4 x the measured worst 2.1e-7
NAMES = ("pose", "n_used", "rms", "flags")
POISON = 0x5A5A5A5A
SIZES = (3, 4, 9, 64, 65, 1024)


def points4(xyz, w=1.0):
    out = np.full((len(xyz), 4), w, F)
    out[:, :3] = xyz
    return out


def moved(src, Rm, t):
    """dst of src [N, 4] under (Rm, t), rounded to float32"""
    return points4(np.asarray(src, np.float64)[:, :3] @ np.asarray(Rm, np.float64).T + t)


def motion_case(N, seed):
    """(src, dst float32 [N, 4], R float64 [3, 3], t float64 [3]): an object of 0.1 m about a metre from the camera"""
    rng = np.random.default_rng(seed)
    Rm, t = R.random_rotation(rng), np.array([0.1, -0.05, 1.0]) + rng.normal(size=3) * 0.1
    src = points4(rng.normal(size=(N, 3)) * 0.05)
    return src, moved(src, Rm, t), Rm, t


def solve_one(src, dst, **kw):
    return pf.solve_host(src[None], dst[None], **kw)


def assert_pose(r, Rm, t, what, t_rot=T_ROT, t_trans=T_TRANS):
    assert r.flags[0] == 0 and r.found[0], what
    ang, dist = R.rotation_angle(r.pose[0, :, :3], Rm), float(np.linalg.norm(r.pose[0, :, 3].astype(np.float64) - t))
    assert ang <= t_rot and dist <= t_trans, "%s: rotation %.3g rad, translation %.3g m from the answer" % (what, ang, dist)
    return ang, dist


def assert_none(r, flag, n_used, m=0):
    """NaN, never an identity"""
    assert r.flags[m] == flag and r.n_used[m] == n_used and not r.found[m] and np.isnan(r.pose[m]).all() and np.isnan(r.rms[m])


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------
CUBE = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]) * 0.25      # exact in float32


def test_identity():
    src = points4(CUBE)
    r = solve_one(src, src)
    assert np.array_equal(r.pose[0], np.eye(4, dtype=F)[:3]) and r.rms[0] == 0.0 and r.n_used[0] == 8 and r.flags[0] == 0


def test_pure_translation():
    src = points4(CUBE)
    r = solve_one(src, moved(src, np.eye(3), [0.5, -0.25, 2.0]))
    assert np.array_equal(r.pose[0], F([[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 2.0]])) and r.rms[0] == 0.0


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("turns", [1, 2, 3])
def test_quarter_turns_about_an_axis(axis, turns):
    a = turns * np.pi / 2.0
    c, s = round(np.cos(a)), round(np.sin(a))
    Rm = np.eye(3)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    Rm[i, i], Rm[i, j], Rm[j, i], Rm[j, j] = c, -s, s, c
    src = points4(CUBE + [0.125, 0.25, -0.0625])
    r = solve_one(src, moved(src, Rm, [0.5, -0.25, 2.0]))
    assert_pose(r, Rm, np.array([0.5, -0.25, 2.0]), "%d quarter turns about axis %d" % (turns, axis))
    assert r.rms[0] <= T_TRANS


def test_flat_points_give_a_proper_rotation():
    """four coplanar points: the third singular value of the moments is 0 and its singular vectors are free in sign, so Kabsch
    without the determinant correction returns a reflection for about every other motion; the quaternion cannot"""
    flat = np.array([[-0.1, -0.05, 0.0], [0.1, -0.05, 0.0], [0.1, 0.05, 0.0], [-0.1, 0.07, 0.0]])
    reflections = 0
    for seed in range(12):
        rng = np.random.default_rng(seed)
        Rm, t = R.random_rotation(rng), np.array([0.0, 0.0, 1.0])
        src = points4(flat)
        dst = moved(src, Rm, t)
        reflections += np.linalg.det(R.naive_svd_rotation(src, dst)) < 0
        r = solve_one(src, dst)
        assert_pose(r, Rm, t, "flat, motion %d" % seed)
        Rg = r.pose[0, :, :3].astype(np.float64)
        assert abs(np.linalg.det(Rg) - 1.0) <= T_ROT and np.abs(Rg @ Rg.T - np.eye(3)).max() <= T_ROT
    assert reflections >= 1, "the naive SVD route returned no reflection on 12 flat motions: the case shows nothing"


def test_fewer_than_three_is_insufficient():
    src, dst, _, _ = motion_case(9, 1)
    for keep in (0, 1, 2):
        s2 = src.copy()
        s2[keep:, 3] = 0.0
        assert_none(solve_one(s2, dst), _abi.FIT_INSUFFICIENT, keep)
        assert R.fit_rules(s2, dst).flags == R.INSUFFICIENT and R.fit_svd(s2, dst)[0] is None
    assert_none(pf.solve_host(src[None, :2], dst[None, :2]), _abi.FIT_INSUFFICIENT, 2)


def test_collinear_and_coincident_points_are_degenerate():
    rng = np.random.default_rng(2)
    Rm, t = R.random_rotation(rng), np.array([0.1, 0.0, 1.0])
    line = points4(np.outer(np.linspace(-0.1, 0.1, 9), [0.6, 0.0, 0.8]) + [0.01, 0.02, 0.03])
    assert_none(solve_one(line, moved(line, Rm, t)), _abi.FIT_DEGENERATE, 9)
    assert R.fit_rules(line, moved(line, Rm, t)).flags == R.DEGENERATE
    spot = points4(np.tile([0.01, 0.02, 0.03], (5, 1)))
    assert_none(solve_one(spot, moved(spot, Rm, t)), _abi.FIT_DEGENERATE, 5)
    # min_gap = 0 accepts whatever the eigenvalues say but for an exact tie; the coincident points are one
    assert_none(solve_one(spot, spot, min_gap=0.0), _abi.FIT_DEGENERATE, 5)


def test_a_zero_weight_on_either_side_removes_a_correspondence():
    src, dst, Rm, t = motion_case(12, 3)
    clean = solve_one(src, dst)
    src2, dst2 = np.concatenate([src, src[:4]]), np.concatenate([dst, dst[:4]])
    dst2[12:, :3] += 0.5                      # four correspondences that would ruin the fit
    src2[12, 3], src2[13, 3], dst2[14, 3], src2[15, 0] = 0.0, -1.0, 0.0, np.nan
    r = solve_one(src2, dst2)
    assert r.n_used[0] == 12
    for k in NAMES:      # they sit in lanes of their own: the sums are the clean ones to the bit
        assert np.array_equal(getattr(r, k).view(np.int32), getattr(clean, k).view(np.int32)), k
    dst2[14, 3] = 1.0
    assert solve_one(src2, dst2).rms[0] > 0.05
    # dst.w needs only to differ from 0 (the camera points' w is a depth); src.w must be positive
    dst3 = dst.copy()
    dst3[:, 3] = -2.5
    assert np.array_equal(solve_one(src, dst3).pose, clean.pose)


# ---- 2. the twin against the references ------------------------------------------------------------------------------------------
def test_random_motions_against_svd():
    worst = np.zeros(3)
    for N in SIZES:
        for seed in range(8):
            src, dst, Rm, t = motion_case(N, 100 * N + seed)
            r = solve_one(src, dst)
            pose, n, rms = R.fit_svd(src, dst)
            what = "N %d, motion %d" % (N, seed)
            ang, dist = assert_pose(r, pose[:, :3], pose[:, 3], what)
            rules = R.fit_rules(src, dst)
            assert rules.flags == 0 and R.rotation_angle(rules.pose[:, :3], pose[:, :3]) < 1e-12, what      # the two references agree
            assert r.n_used[0] == n == N and abs(float(r.rms[0]) - rms) <= T_TRANS, what
            worst = np.maximum(worst, [ang, dist, R.rotation_angle(pose[:, :3], Rm)])
    print("pose_fit twin against the float64 SVD: worst rotation %.3g rad, worst translation %.3g m (the SVD against the exact "
          "motion: %.3g rad)" % tuple(worst))
    assert worst[0] * 4 <= T_ROT * 1.0001 and worst[1] * 4 <= T_TRANS * 1.0001, worst      # the constants are 4 x what is measured


def test_eight_sweeps_leave_nothing_off_the_diagonal():
    """the rules in float32 (pose_fit_ref.fit_rules with dtype float32: the same rotations in NumPy): after the 8 sweeps of
    slhip_fit_rules.h the off-diagonal mass lies below float32 rounding of the diagonal's, for every case of this file's
    comparisons; 2 sweeps do not manage that, so the check can fail"""
    eps = float(np.finfo(F).eps)
    short = 0
    cases = [motion_case(N, 100 * N + seed)[:2] for N in SIZES for seed in range(8)]
    flat = points4(np.array([[-0.1, -0.05, 0.0], [0.1, -0.05, 0.0], [0.1, 0.05, 0.0], [-0.1, 0.07, 0.0]]))
    cases += [(flat, moved(flat, R.random_rotation(np.random.default_rng(s)), [0.0, 0.0, 1.0])) for s in range(12)]
    for src, dst in cases:
        f = R.fit_rules(src, dst, dtype=F)
        assert f.flags == 0 and f.off_diagonal <= eps * f.trace, (f.off_diagonal, f.trace)
        got = solve_one(src, dst)
        assert R.rotation_angle(got.pose[0, :, :3], f.pose[:, :3]) <= T_ROT      # NumPy's sums differ in order, not in kind
        g = R.fit_rules(src, dst, dtype=F, sweeps=2)
        short += g.off_diagonal > eps * g.trace
    assert short >= 1


# ---- 3. parameters, arguments, outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,word", [
    ("n_points", 0, "n_points"), ("n_points", 4097, "n_points"), ("min_gap", -1e-6, "min_gap"), ("min_gap", 1.0, "min_gap"),
    ("min_gap", np.nan, "min_gap"), ("outputs", 0, "outputs"), ("outputs", 16, "outputs")])
def test_check_params_names_the_broken_rule(field, value, word):
    p = pf.make_params(1, 16)
    pf.check_params(p)
    p[field] = value
    with pytest.raises(_abi.SlhipError, match=word):
        pf.check_params(p)


def host_call(null=None, misalign=None, mask=15, **fields):
    M, N = 2, 16
    src, dst, _, _ = motion_case(M * N, 5)
    raw = {"src": np.zeros(M * N * 4 + 8, F), "dst": np.zeros(M * N * 4 + 8, F)}
    ptr = {}
    for k, a in (("src", src), ("dst", dst)):
        shift = ((-raw[k].ctypes.data) % 16) // 4      # 16-byte aligned
        raw[k][shift:shift + M * N * 4] = a.reshape(-1)
        ptr[k] = None if null == k else raw[k].ctypes.data + 4 * shift + (4 if misalign == k else 0)
    outs = {k: np.full(64, POISON, np.uint32) for k in NAMES}
    o = _abi.PoseFitOut(*(None if null == k else outs[k].ctypes.data + (2 if misalign == k else 0) for k in NAMES))
    p = pf.make_params(M, N, outputs=mask).reshape(1)
    for k, v in fields.items():
        p[k] = v
    st = _abi.lib().slhip_pose_fit_host(None if null == "params" else p.ctypes.data, ptr["src"], ptr["dst"],
                                        None if null == "record" else C.byref(o))
    return st, outs


REFUSALS = [dict(null="params"), dict(null="src"), dict(null="dst"), dict(null="record"), dict(null="pose"), dict(null="flags"),
            dict(misalign="src"), dict(misalign="dst"), dict(misalign="rms"), dict(n_points=0), dict(n_points=4097), dict(min_gap=-1.0),
            dict(min_gap=1.0), dict(mask=0), dict(mask=16)]


@pytest.mark.parametrize("kw", REFUSALS)
def test_entries_refuse_bad_arguments(kw):
    st, outs = host_call(**kw)
    assert st < 0 and _abi.lib().slhip_last_error()
    for k in NAMES:
        assert (outs[k] == POISON).all(), k
    assert host_call()[0] == 0


def test_no_sets_succeed_and_write_nothing():
    st, outs = host_call(n_sets=0)
    assert st == 0 and all((o == POISON).all() for o in outs.values())


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 1 | 8, 2 | 4])
def test_outputs_not_named_stay_poison(mask):
    st, outs = host_call(mask=mask)
    assert st == 0
    for i, k in enumerate(NAMES):
        if not mask & (1 << i):
            assert (outs[k] == POISON).all(), k
        else:
            assert (outs[k][:2] != POISON).all(), k
    src, dst, _, _ = motion_case(8, 6)
    r = solve_one(src, dst, outputs=("pose",))
    assert r.rms is None and r.flags is None and r.found[0]
    with pytest.raises(RuntimeError):
        pf.PoseFit(rms=r.pose).dense(1, 1, [0], [1])


def test_dense_places_the_poses():
    src, dst, _, _ = motion_case(8, 7)
    r = pf.solve_host(np.stack([src, src]), np.stack([dst, src]))
    d = r.dense(2, 3, [1, 0], [3, 1])
    assert d.shape == (2, 3, 3, 4) and np.array_equal(d[1, 2], r.pose[0]) and np.array_equal(d[0, 0], r.pose[1])
    assert np.isnan(d[0, 1:]).all() and np.isnan(d[1, :2]).all()


def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5" in text and _abi.ABI_VERSION == 5 and _abi.lib().slhip_abi_version() == 5
    for name in ("slhip_pose_fit_check_params", "slhip_pose_fit", "slhip_pose_fit_host", "slhip_pose_fit_timing_enable",
                 "slhip_pose_fit_timings"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name), name
    assert _abi.POSE_FIT_PARAMS_DTYPE.itemsize == 64 and "} slhip_pose_fit_params; /* 64 bytes */" in text
    for name, bit in pf.OUTPUTS.items():
        assert re.search(r"#define SLHIP_FIT_OUT_%s\s+%du\b" % (name.upper(), bit), text), name
    for name, bit in pf.FLAGS.items():
        assert re.search(r"#define SLHIP_FIT_%s\s+%d\b" % (name.upper(), bit), text), name
    rules = open(os.path.join(root, "stillleben_amd", "csrc", "slhip_fit_rules.h")).read()
    assert "constexpr int SWEEPS = %d;" % R.SWEEPS in rules
    import stillleben as alias
    import stillleben_amd as sl
    assert sl.pose_fit is pf and alias.pose_fit is pf and sl.PoseFit is pf.PoseFit and "pose_fit" in sl.__all__
    assert alias.PoseFit is pf.PoseFit and hasattr(sl.SceneBatch, "pose_fit")


def test_cpu_tensors_are_refused():
    import torch

    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        pf.solve(torch.ones((1, 8, 4)), torch.ones((1, 8, 4)))
