"""Pose PnP on the host (slhip_pose_pnp_host, slhip_pose_pnp_p3p_host, slhip_pose_pnp_check_params, sl.pose_pnp) against the
independent float64 implementation tests/pose_pnp_ref.py and against answers known by hand.  Needs no device.

The tolerances.  T_PX, T_ROT and T_T are four times the worst deviation of the float32 solver from the float64 reference over the
1000 triples of test_p3p (measured there on every run and printed; the constants below record it): rounding grows with the
conditioning of the image triangle, not with the seed, so the margin is a factor and not an offset.
    measured worst (seed 1):  reprojection 1.3e-4 px,  rotation 2.7e-5 rad,  translation 1.8e-5 m
The true pose lies within the same tolerances of the nearest solution (worst 5.3e-5 rad, 1.9e-5 m, the float32 pixels' share included)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pose_pnp_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_pnp as pnp

F = np.float32
K4 = (572.4, 572.4, 320.0, 240.0)      # a 640 x 480 camera
T_PX = 4 * 1.3e-4                      # px;   4 x the measured worst 1.3e-4
T_ROT = 4 * 2.7e-5                     # rad;  4 x the measured worst 2.7e-5
T_T = 4 * 1.8e-5                       # m;    4 x the measured worst 1.8e-5
P3P_SEED = 1
NAMES = ("pose", "n_inliers", "rms", "inliers", "best", "flags")


def rotation(rng):
    q = rng.normal(size=4)
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def random_pose(rng):
    """a random rotation at 0.4 to 1.5 m in front of the camera, inside its field of view"""
    z = 0.4 + 1.1 * rng.random()
    t = np.array([(rng.random() - 0.5) * 0.8 * z, (rng.random() - 0.5) * 0.6 * z, z])
    return np.concatenate([rotation(rng), t[:, None]], 1)


def make_set(K, outliers, seed, flat=False):
    """K exact correspondences of a random pose, points uniform in a 0.1 m cube (z = 0 with `flat`); the xyz of `outliers` of
    them replaced by another uniform point of the cube.  (uv float32 [K, 2], xyz float32 [K, 4], pose, clean bool [K])"""
    rng = np.random.default_rng(seed)
    pose = random_pose(rng)
    P = ((rng.random((K, 3)) - 0.5) * 0.1).astype(F)
    if flat:
        P[:, 2] = 0
    uv, _ = R.project(pose, K4, P)
    xyz = np.ones((K, 4), F)
    xyz[:, :3] = P
    clean = np.ones(K, bool)
    bad = rng.permutation(K)[:outliers]
    xyz[bad, :3] = ((rng.random((len(bad), 3)) - 0.5) * 0.1).astype(F)
    clean[bad] = False
    return uv.astype(F), xyz, pose, clean


def nearest(poses, pose):
    """(rotation angle, translation distance) of the entry of `poses` nearest `pose` by angle"""
    d = [(R.rotation_angle(m, pose), R.translation_distance(m, pose)) for m in poses]
    return min(d) if d else (np.inf, np.inf)


# ---- 1. the minimal solver -------------------------------------------------------------------------------------------------------
def test_p3p():
    rng = np.random.default_rng(P3P_SEED)
    left = ref_failed = 0
    worst = np.zeros(3)
    for i in range(1000):
        P = ((rng.random((3, 3)) - 0.5) * 0.1).astype(F)
        pose = random_pose(rng)
        uv = R.project(pose, K4, P)[0].astype(F)
        e1, e2 = uv[1] - uv[0], uv[2] - uv[0]
        area = 0.5 * abs(float(e1[0]) * float(e2[1]) - float(e1[1]) * float(e2[0]))
        ref = R.p3p(uv, P, K4)
        ref_ok = nearest(ref, pose) < (1e-3, 1e-3) and nearest(ref, pose)[1] < 1e-3
        ref_failed += not ref_ok
        if area < 4.0 or not ref_ok:
            left += 1
            continue
        got = pnp.p3p_host(uv, P, K4)
        assert 1 <= len(got) <= 4, i
        for m in got.astype(np.float64):
            px = np.abs(R.project(m, K4, P)[0] - uv).max()
            worst[0] = max(worst[0], px)
            assert px <= T_PX, "triple %d: a solution reprojects %.3g px off" % (i, px)
        rot, t = nearest(got, pose)
        assert rot <= T_ROT and t <= T_T, "triple %d (area %.1f px^2): the true pose is %.3g rad, %.3g m from the nearest solution" % (i, area, rot, t)
        # the deviation from the reference: the reference's solution nearest the truth against ours nearest the truth
        truth = min(ref, key=lambda m: R.rotation_angle(m, pose))
        rot, t = nearest(got, truth)
        worst[1:] = np.maximum(worst[1:], (rot, t))
    print("p3p: %d of 1000 left out (%d by the reference), worst against float64: %.3g px, %.3g rad, %.3g m" % ((left, ref_failed) + tuple(worst)))
    assert ref_failed <= 20 and left <= 20, "more than 2 %% of the triples left out: %d (the reference alone: %d)" % (left, ref_failed)
    assert worst[0] * 4 <= T_PX * 1.0001 and worst[1] * 4 <= T_ROT * 1.0001 and worst[2] * 4 <= T_T * 1.0001, worst      # the constants are 4 x what is measured


# ---- 2. known answers ------------------------------------------------------------------------------------------------------------
def square(d, shift=(0, 0)):
    P = np.array([[-0.05, -0.05, 0], [0.05, -0.05, 0], [0.05, 0.05, 0], [-0.05, 0.05, 0]], F)
    xyz = np.ones((4, 4), F)
    xyz[:, :3] = P
    uv = np.stack([K4[0] * P[:, 0] / d + K4[2] + shift[0], K4[1] * P[:, 1] / d + K4[3] + shift[1]], -1).astype(F)
    return uv[None], xyz[None]


@pytest.mark.parametrize("shift", [(0, 0), (7, -3), (-40, 25)])
def test_square_facing_the_camera(shift):
    """four corners of a square at depth d: the identity rotation and the translation the pixel shift implies at d"""
    d = 0.8
    uv, xyz = square(d, shift)
    r = pnp.solve_host(uv, xyz, K4, n_hypotheses=64, seed=3)
    want = np.concatenate([np.eye(3), [[shift[0] * d / K4[0]], [shift[1] * d / K4[1]], [d]]], 1)
    assert r.flags[0] == 0 and r.n_inliers[0] == 4 and r.best[0] >= 0 and r.inlier_mask()[0].all()
    assert R.rotation_angle(r.pose[0], want) <= T_ROT and R.translation_distance(r.pose[0], want) <= T_T, r.pose[0]
    assert r.rms[0] <= T_PX


def test_pure_refinement_returns_the_true_pose():
    uv, xyz, pose, _ = make_set(300, 0, 11)
    for iters in (0, 4):
        r = pnp.solve_host(uv[None], xyz[None], K4, init=pose[None], n_hypotheses=0, refine_iters=iters)
        assert r.best[0] == -1 and r.n_inliers[0] == 300 and r.flags[0] == 0 and r.inlier_mask().all()
        assert R.rotation_angle(r.pose[0], pose) <= T_ROT and R.translation_distance(r.pose[0], pose) <= T_T
        if iters == 0:
            assert np.array_equal(r.pose[0], pose.astype(F))


def test_initial_pose_wins_ties():
    uv, xyz, pose, _ = make_set(64, 0, 12)
    r = pnp.solve_host(uv[None], xyz[None], K4, init=pose[None], n_hypotheses=64, refine_iters=0)
    assert r.best[0] == -1 and r.n_inliers[0] == 64
    assert pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=64, refine_iters=0).best[0] >= 0


# ---- 3. the whole pipeline against the reference ---------------------------------------------------------------------------------
PIPELINE = [(K, frac) for K in (4, 5, 257, 1024) for frac in (0.0, 0.4)]
_pipeline = {}


def pipeline_case(K, frac):
    """(inputs, the library's result, the reference's), computed once and shared with tests/test_gpu_pose_pnp.py"""
    if (K, frac) not in _pipeline:
        uv, xyz, pose, clean = make_set(K, int(frac * K), 100 + K)
        kw = dict(n_hypotheses=48, threshold_px=2.0, refine_iters=3, min_inliers=4, seed=5 + K)
        got = pnp.solve_host(uv[None], xyz[None], K4, **kw)
        ref = R.solve(uv, xyz, K4, set_id=0, **kw)
        _pipeline[(K, frac)] = (uv, xyz, pose, clean, kw, got, ref)
    return _pipeline[(K, frac)]


def compare_with_reference(got, ref, K, what, i=0):
    """best equal; inliers equal but for those the reference sees within 1e-3 px of the threshold; the pose within T_ROT, T_T"""
    assert got.best[i] == ref.best, "%s: best %d, the reference %d" % (what, got.best[i], ref.best)
    assert (got.flags[i] & 3) == (ref.flags & 3), what
    if ref.best == -2:
        assert np.isnan(got.pose[i]).all() and got.n_inliers[i] == 0 and np.isnan(got.rms[i]) and not got.inlier_mask()[i].any()
        return
    near = np.abs(np.sqrt(ref.err2) - 2.0) <= 1e-3
    differ = got.inlier_mask()[i] != ref.inliers
    assert not (differ & ~near).any(), "%s: %d inlier bits differ away from the threshold" % (what, int((differ & ~near).sum()))
    assert abs(int(got.n_inliers[i]) - ref.n_inliers) <= int(near.sum()) and got.n_inliers[i] == got.inlier_mask()[i].sum()
    rot, t = R.rotation_angle(got.pose[i], ref.pose), R.translation_distance(got.pose[i], ref.pose)
    print("%s: %.3g rad, %.3g m from the reference, rms %.3g against %.3g" % (what, rot, t, got.rms[i], ref.rms))
    assert rot <= T_ROT and t <= T_T, "%s: %.3g rad, %.3g m from the reference" % (what, rot, t)
    assert abs(got.rms[i] - ref.rms) <= T_PX


@pytest.mark.parametrize("K,frac", PIPELINE)
def test_pipeline_against_float64(K, frac):
    uv, xyz, pose, clean, kw, got, ref = pipeline_case(K, frac)
    compare_with_reference(got, ref, K, "K %d, %d %% outliers" % (K, round(100 * frac)))
    if K >= 257:      # (a replaced point may land within the threshold by chance: it is then an inlier of both, and pulls the pose)
        assert ref.best >= 0 and ref.inliers[clean].all() and (ref.inliers & ~clean).sum() <= 0.05 * K
        if frac == 0.0:
            assert R.rotation_angle(got.pose[0], pose) <= T_ROT and R.translation_distance(got.pose[0], pose) <= T_T


# ---- 4. edge cases ---------------------------------------------------------------------------------------------------------------
def assert_none(r, flag, i=0):
    assert r.flags[i] == flag and r.best[i] == -2 and r.n_inliers[i] == 0
    assert np.isnan(r.pose[i]).all() and np.isnan(r.rms[i]) and not r.inliers[i].any()


def test_three_valid_of_eight_is_insufficient():
    uv, xyz, _, _ = make_set(8, 0, 21)
    xyz[3:, 3] = 0
    assert_none(pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=16), _abi.PNP_INSUFFICIENT)


def test_identical_correspondences_have_no_model():
    uv, xyz, _, _ = make_set(8, 0, 22)
    uv[:], xyz[:] = uv[0], xyz[0]
    assert_none(pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=64), _abi.PNP_NO_MODEL)


def test_points_behind_the_camera():
    """a pose that puts every point behind the camera counts nothing, as the initial pose or as the only candidate"""
    uv, xyz, pose, _ = make_set(32, 0, 23)
    behind = -pose      # (X, Y, Z) -> (-X, -Y, -Z): the same pixels from Z < 0
    assert (R.project(behind, K4, xyz)[1] < 0).all() and np.allclose(R.project(behind, K4, xyz)[0], uv, atol=1e-2)
    assert_none(pnp.solve_host(uv[None], xyz[None], K4, init=behind[None], n_hypotheses=0), _abi.PNP_NO_MODEL)
    r = pnp.solve_host(uv[None], xyz[None], K4, init=behind[None], n_hypotheses=32)
    assert r.best[0] >= 0 and r.n_inliers[0] == 32 and (R.project(r.pose[0].astype(np.float64), K4, xyz)[1] > 0).all()


def test_invalid_entries_are_skipped():
    uv, xyz, pose, _ = make_set(40, 0, 24)
    clean = pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=32, seed=9)
    bad = np.zeros(48, bool)
    bad[[0, 5, 17, 33, 34, 40, 46, 47]] = True
    uv2, xyz2 = np.zeros((48, 2), F), np.ones((48, 4), F)
    uv2[~bad], xyz2[~bad] = uv, xyz
    poison = [(0, np.nan, None), (5, None, np.inf), (17, None, -np.inf), (33, np.inf, None)]
    for j, u, x in poison:
        if u is not None:
            uv2[j, j % 2] = u
        if x is not None:
            xyz2[j, j % 3] = x
    xyz2[[34, 40], 3] = [0.0, -1.0]
    xyz2[46, 3], xyz2[47, 3] = np.nan, -np.inf
    r = pnp.solve_host(uv2[None], xyz2[None], K4, n_hypotheses=32, seed=9)
    # the valid list is the clean set in the same order: the same picks, the same pose to the bit
    assert np.array_equal(r.pose, clean.pose) and r.best[0] == clean.best[0] and r.n_inliers[0] == 40
    assert np.array_equal(r.inlier_mask()[0], ~bad)


def test_coplanar_object_still_solves():
    uv, xyz, pose, _ = make_set(100, 0, 25, flat=True)
    r = pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=32)
    assert r.n_inliers[0] == 100 and R.rotation_angle(r.pose[0], pose) <= T_ROT and R.translation_distance(r.pose[0], pose) <= T_T


def test_seed_changes_best_and_repeats():
    uv, xyz, _, _ = make_set(257, 100, 26)
    a = pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=64, seed=1)
    b = pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=64, seed=1)
    for k in NAMES:
        assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), k
    bests = {int(pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=64, seed=s).best[0]) for s in range(1, 6)}
    assert len(bests) > 1, bests
    # the set id enters the counter like the seed: set 1 of two equal sets draws differently, and as set_id_base 1 draws
    two = pnp.solve_host(np.stack([uv, uv]), np.stack([xyz, xyz]), K4, n_hypotheses=64, seed=1)
    one = pnp.solve_host(uv[None], xyz[None], K4, n_hypotheses=64, seed=1, set_id_base=1)
    assert two.best[0] == a.best[0] and two.best[1] == one.best[0] and np.array_equal(two.pose[1], one.pose[0])


def test_per_set_intrinsics():
    """a crop has its own camera: the pixels of set 1 under K' = (2 fx, 2 fy, 2 cx - 100, 2 cy - 60) give the pose of set 0"""
    uv, xyz, pose, _ = make_set(50, 0, 27)
    k2 = np.array([[K4[0], K4[1], K4[2], K4[3]], [2 * K4[0], 2 * K4[1], 2 * K4[2] - 100, 2 * K4[3] - 60]], F)
    uv2 = np.stack([uv, uv * 2 - F([100, 60])])
    r = pnp.solve_host(uv2, np.stack([xyz, xyz]), (1.0, 1.0, 0.0, 0.0), per_set_intrinsics=k2, n_hypotheses=32)
    for i in range(2):
        assert r.n_inliers[i] == 50 and R.rotation_angle(r.pose[i], pose) <= T_ROT and R.translation_distance(r.pose[i], pose) <= T_T


def test_refinement_flags():
    uv, xyz, pose, _ = make_set(64, 0, 28)
    # four copies of one correspondence and nothing else valid: the initial pose holds them, the normal equations are singular
    uv1, xyz1 = np.repeat(uv[:1], 4, 0), np.repeat(xyz[:1], 4, 0)
    r = pnp.solve_host(uv1[None], xyz1[None], K4, init=pose[None], n_hypotheses=0, refine_iters=2)
    assert r.flags[0] == _abi.PNP_REFINE_STOPPED and r.n_inliers[0] == 4 and np.array_equal(r.pose[0], pose.astype(F))


# ---- 5. parameters, arguments, outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,word", [
    ("fx", 0.0, "intrinsics"), ("cy", np.nan, "intrinsics"), ("n_points", 3, "n_points"), ("n_points", 4097, "n_points"),
    ("n_hypotheses", 4097, "n_hypotheses"), ("threshold_px", 0.0, "threshold_px"), ("threshold_px", np.inf, "threshold_px"),
    ("refine_iters", 17, "refine_iters"), ("min_inliers", 3, "min_inliers"), ("outputs", 0, "outputs"), ("outputs", 64, "outputs")])
def test_check_params_names_the_broken_rule(field, value, word):
    p = pnp.make_params(K4, 1, 16)
    pnp.check_params(p)
    p[field] = value
    with pytest.raises(_abi.SlhipError, match=word):
        pnp.check_params(p)


def host_call(null=None, misalign=None, Hy=8, init=True, mask=63):
    M, K = 2, 16
    uv, xyz, k4, t0 = np.zeros((M * K * 2 + 4), F), np.zeros((M * K * 4 + 4), F), np.zeros(M * 4 + 4, F), np.zeros(M * 12 + 4, F)
    outs = {k: np.full(64, 0x5A5A5A5A, np.uint32) for k in NAMES}
    ptr = {"uv": uv.ctypes.data, "xyz": xyz.ctypes.data, "intrinsics": k4.ctypes.data, "init": t0.ctypes.data if init else None}
    if misalign in ptr:
        ptr[misalign] += 4
    for k in ("uv", "xyz"):
        if null == k:
            ptr[k] = None
    o = _abi.PosePnpOut(*(None if null == k else outs[k].ctypes.data + (2 if misalign == k else 0) for k in NAMES))
    p = pnp.make_params(K4, M, K, n_hypotheses=Hy, outputs=mask).reshape(1)
    st = _abi.lib().slhip_pose_pnp_host(None if null == "params" else p.ctypes.data, ptr["uv"], ptr["xyz"], ptr["intrinsics"], ptr["init"],
                                        None if null == "record" else C.byref(o))
    return st, outs


@pytest.mark.parametrize("kw", [dict(null="params"), dict(null="uv"), dict(null="xyz"), dict(null="record"), dict(null="pose"),
                                dict(null="inliers"), dict(null="flags"), dict(misalign="uv"), dict(misalign="xyz"),
                                dict(misalign="intrinsics"), dict(misalign="rms"), dict(Hy=0, init=False)])
def test_entries_refuse_bad_arguments(kw):
    st, outs = host_call(**kw)
    assert st < 0 and _abi.lib().slhip_last_error()
    if kw == dict(misalign="rms"):
        assert "4-byte aligned" in _abi.lib().slhip_last_error().decode()
    for k in NAMES:
        assert (outs[k] == 0x5A5A5A5A).all(), k
    assert host_call()[0] == 0


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 1 | 8, 2 | 4 | 32])
def test_outputs_not_named_stay_poison(mask):
    st, outs = host_call(mask=mask)
    assert st == 0
    for i, k in enumerate(NAMES):
        if not mask & (1 << i):
            assert (outs[k] == 0x5A5A5A5A).all(), k
        else:
            assert (outs[k][:2] != 0x5A5A5A5A).all(), k
    r = pnp.solve_host(np.zeros((1, 8, 2), F), np.ones((1, 8, 4), F), K4, outputs=("pose", "best"))
    assert r.rms is None and r.inliers is None and r.pose is not None
    with pytest.raises(RuntimeError):
        r.inlier_mask()


def test_p3p_host_refuses_null():
    assert _abi.lib().slhip_pose_pnp_p3p_host(None, None, None, None) < 0


def test_dense_scatters():
    r = pnp.PosePnP(8, pose=np.arange(36, dtype=F).reshape(3, 3, 4))
    d = r.dense(2, 3, scene=[0, 1, 1], slot=[2, 1, 3])
    assert d.shape == (2, 3, 3, 4) and np.array_equal(d[0, 1], r.pose[0]) and np.array_equal(d[1, 0], r.pose[1]) and np.array_equal(d[1, 2], r.pose[2])
    assert np.isnan(d[0, 0]).all() and np.isnan(d[0, 2]).all() and np.isnan(d[1, 1]).all()


def test_inlier_mask_bit_order():
    r = pnp.PosePnP(40, inliers=np.array([[1 | (1 << 31), 1 << 7]], np.uint32))
    m = r.inlier_mask()
    assert m.shape == (1, 40) and m[0].nonzero()[0].tolist() == [0, 31, 39]


def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5" in text and _abi.ABI_VERSION == 5
    for name in ("slhip_pose_pnp_check_params", "slhip_pose_pnp", "slhip_pose_pnp_host", "slhip_pose_pnp_p3p_host",
                 "slhip_pose_pnp_timing_enable", "slhip_pose_pnp_timings"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name), name
    assert "Stream 7" in text and _abi.SYNTH_STREAM_PNP == R.STREAM == 7
    import stillleben as alias
    import stillleben_amd as sl
    assert sl.pose_pnp is pnp and alias.pose_pnp is pnp and sl.PosePnP is pnp.PosePnP and "pose_pnp" in sl.__all__


def test_cpu_tensors_are_refused():
    import torch

    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        pnp.solve(torch.zeros((1, 8, 2)), torch.ones((1, 8, 4)), intrinsics=K4)
