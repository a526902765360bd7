"""Keypoint voting on the host (slhip_keypoint_vote_host, slhip_keypoint_vote_check_params, sl.keypoint_vote) against the
independent float64 implementation tests/keypoint_vote_ref.py and against answers known by hand.  Needs no device.

The tolerance.  T_UV is four times the worst distance of the float32 twin's position from the float64 reference's over the sets of
test_twin_against_float64 (measured there on every run and printed; the constant below records it), the 4 x rule of
tests/test_host_pose_pnp.py: rounding grows with the conditioning of the sampled pair and of the fit, not with the seed, so the
margin is a factor and not an offset.  T_STAT is the same for the distribution's mean and the square roots of its variances.
    measured worst:  uv 1.1e-5 px,  mean and sqrt(cov) 7.6e-5 px
Every seed below is chosen so that the reference finds every keypoint and picks the hypothesis the twin picks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keypoint_vote_ref as R
from stillleben_amd import _abi
from stillleben_amd import keypoint_vote as kv

F = np.float32
SIZE = (160, 120)
T_UV = 4 * 1.1e-5        # px; 4 x the measured worst 1.1e-5
T_STAT = 4 * 7.6e-5      # px; 4 x the measured worst 7.6e-5
NEAR = 1e-4              # inlier sets may differ from the reference's only at voters this near the cosine bound
COS = 0.99
NAMES = ("uv", "n_inliers", "best", "flags", "mean", "cov", "inliers")
POISON = 0x5A5A5A5A


def make_sets(M, K, Kp, frac, seed, noise_deg=0.5, size=SIZE):
    """M sets of K distinct pixels of a window of the picture, each with unit vectors towards Kp keypoints in and round the
    window, `noise_deg` of Gaussian angular noise, `frac` of the vectors of every keypoint replaced by uniform directions.
    (pixel int16 [M, K, 2], vectors float32 [M, K, Kp, 2], keypoints float64 [M, Kp, 2], clean bool [M, K, Kp])"""
    rng = np.random.default_rng(seed)
    side = max(8, int(np.ceil(np.sqrt(2.0 * K))))
    pixel, vec = np.zeros((M, K, 2), np.int16), np.zeros((M, K, Kp, 2), F)
    kps, clean = np.zeros((M, Kp, 2)), np.ones((M, K, Kp), bool)
    for m in range(M):
        x0, y0 = rng.integers(0, size[0] - side + 1), rng.integers(0, size[1] - side + 1)
        cells = rng.permutation(side * side)[:K]
        pixel[m, :, 0], pixel[m, :, 1] = x0 + cells % side, y0 + cells // side
        kps[m] = np.array([x0, y0]) + (rng.random((Kp, 2)) * 1.4 - 0.2) * side
        to = kps[m][None] - (pixel[m].astype(np.float64) + 0.5)[:, None]                 # [K, Kp, 2]
        ang = np.arctan2(to[..., 1], to[..., 0]) + np.deg2rad(noise_deg) * rng.normal(size=(K, Kp))
        for k in range(Kp):
            bad = rng.permutation(K)[:int(frac * K)]
            ang[bad, k] = rng.random(len(bad)) * 2.0 * np.pi
            clean[m, bad, k] = False
        vec[m] = np.stack([np.cos(ang), np.sin(ang)], -1).astype(F)
    return pixel, vec, kps, clean


def exact_vectors(pixel, target):
    """the unnormalised vectors from the centres of pixel [K, 2] to target (x, y): exact in float32 for half-integers"""
    return (np.asarray(target, np.float64)[None] - (np.asarray(pixel, np.float64) + 0.5)).astype(F)


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", [(1, 1), (40, 17), (159, 119), (64, 64)])
def test_lattice_round_an_integer_point(corner):
    """the 2 x 2 lattice of pixels round the lattice point (cx, cy), every vector pointing exactly at it: all four directions
    are (+-c, +-c) with one float32 c, every meeting point of two neighbours is the lattice point to the bit, the fit's right
    side is 0, and so uv and mean equal it exactly, every voter is an inlier and cov is 0"""
    cx, cy = corner
    pixel = np.array([[cx - 1, cy - 1], [cx, cy - 1], [cx - 1, cy], [cx, cy]], np.int16)
    vec = exact_vectors(pixel, (cx, cy))
    r = kv.vote_host(pixel[None], vectors=vec[None, :, None], size=SIZE, n_hypotheses=64, seed=3)
    assert r.flags[0, 0] == 0 and r.best[0, 0] >= 0 and r.n_inliers[0, 0] == 4 and r.inlier_mask()[0, 0].all()
    assert np.array_equal(r.uv[0, 0], F([cx, cy])) and np.array_equal(r.mean[0, 0], F([cx, cy]))
    assert np.array_equal(r.cov[0, 0], F([0, 0, 0]))


def test_keypoint_at_a_voters_centre():
    """voters of one row and one column, vectors along the axes towards the centre of pixel (10, 7): every product is exact,
    so uv is that centre to the bit, and the voter AT the centre is an inlier whatever its vector says (n2 == 0)"""
    pixel = np.array([[2, 7], [5, 7], [14, 7], [30, 7], [10, 0], [10, 3], [10, 20], [10, 7]], np.int16)
    vec = exact_vectors(pixel, (10.5, 7.5))
    vec[7] = (-3.0, 0.0)      # the voter at the centre points away along its row
    r = kv.vote_host(pixel[None], vectors=vec[None, :, None], size=SIZE, n_hypotheses=64, seed=1)
    assert r.flags[0, 0] == 0 and np.array_equal(r.uv[0, 0], F([10.5, 7.5])) and np.array_equal(r.mean[0, 0], F([10.5, 7.5]))
    assert r.n_inliers[0, 0] == 8 and r.inlier_mask()[0, 0].all() and np.array_equal(r.cov[0, 0], F([0, 0, 0]))
    ref = R.solve(pixel, vec, SIZE, n_hypotheses=64, seed=1)
    assert ref.inliers.all() and np.abs(ref.uv - [10.5, 7.5]).max() < 1e-12


def test_two_voters_only():
    pixel = np.array([[20, 30], [60, 35]], np.int16)
    vec = exact_vectors(pixel, (43.25, 71.5))
    r = kv.vote_host(pixel[None], vectors=vec[None, :, None], size=SIZE, n_hypotheses=32, seed=2)
    assert r.flags[0, 0] == 0 and r.n_inliers[0, 0] == 2 and r.best[0, 0] >= 0 and r.inlier_mask()[0, 0].all()
    assert np.abs(r.uv[0, 0] - [43.25, 71.5]).max() <= T_UV and np.abs(r.mean[0, 0] - [43.25, 71.5]).max() <= T_STAT
    # one pair at most: with a single hypothesis that draws the same voter twice there is nothing
    lone = [s for s in range(40) if R.picks(s, 0, 0, 1, 2)[0, 0] == R.picks(s, 0, 0, 1, 2)[0, 1]][0]
    assert_none(kv.vote_host(pixel[None], vectors=vec[None, :, None], size=SIZE, n_hypotheses=1, seed=lone), _abi.VOTE_NO_MODEL)


def assert_none(r, flag, m=0, k=0):
    """NaN, never zeros"""
    assert r.flags[m, k] == flag and r.best[m, k] == -2 and r.n_inliers[m, k] == 0 and not r.found[m, k]
    assert np.isnan(r.uv[m, k]).all() and np.isnan(r.mean[m, k]).all() and np.isnan(r.cov[m, k]).all() and not r.inliers[m, k].any()


def test_parallel_vectors_have_no_model():
    pixel, vec, _, _ = make_sets(1, 65, 2, 0.0, 4)
    vec[:] = F([0.6, 0.8])
    r = kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=64)
    assert_none(r, _abi.VOTE_NO_MODEL, 0, 0)
    assert_none(r, _abi.VOTE_NO_MODEL, 0, 1)
    assert R.solve(pixel[0], vec[0, :, 0], SIZE, n_hypotheses=64).flags == R.NO_MODEL


def test_keypoint_outside_the_picture_is_found():
    pixel, vec, _, _ = make_sets(1, 257, 1, 0.0, 5, noise_deg=0.0)
    target = np.array([-30.0, 200.0])
    vec[0, :, 0] = exact_vectors(pixel[0], target)
    r = kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=32, seed=6)
    assert r.found[0, 0] and r.flags[0, 0] == 0 and r.n_inliers[0, 0] == 257
    ref = R.solve(pixel[0], vec[0, :, 0], SIZE, n_hypotheses=32, seed=6)
    assert np.abs(ref.uv - target).max() < 1e-5      # (the float32 vectors are the exact ones rounded once)
    # T_UV is measured on keypoints within 60 px of their voters; here every intermediate is of the size of 256 px, so the bound
    # is stated in float32 spacings of that size: 64 of them, a few for each of the dozen rounded operations behind a position
    assert np.linalg.norm(r.uv[0, 0] - ref.uv) <= 64 * float(np.spacing(F(256.0)))


# ---- 2. the twin against the reference -------------------------------------------------------------------------------------------
PIPELINE = [(K, frac) for K in (2, 3, 65, 257, 1024) for frac in (0.0, 0.4)]
KW = dict(n_hypotheses=48, inlier_cos=COS, min_inliers=2, min_sin=1e-3)
_pipeline = {}


def pipeline_case(K, frac):
    """(inputs, the library's result, the reference's), computed once and shared with tests/test_gpu_keypoint_vote.py"""
    if (K, frac) not in _pipeline:
        pixel, vec, kps, clean = make_sets(2, K, 3, frac, 200 + K)
        kw = dict(KW, seed=11 + K)
        got = kv.vote_host(pixel, vectors=vec, size=SIZE, **kw)
        ref = R.solve_sets(pixel, vec, SIZE, **kw)
        _pipeline[(K, frac)] = (pixel, vec, kps, clean, kw, got, ref)
    return _pipeline[(K, frac)]


def compare_with_reference(got, ref, what, m=0, k=0, t_uv=T_UV, t_stat=T_STAT):
    """best and flags equal; inliers equal but for those the reference sees within NEAR of the cosine bound; uv within t_uv,
    mean and the standard deviations within t_stat.  Returns (distance of uv, the worst of the statistics)."""
    assert got.best[m, k] == ref.best, "%s: best %d, the reference %d" % (what, got.best[m, k], ref.best)
    assert got.flags[m, k] == ref.flags, "%s: flags %d, the reference %d" % (what, got.flags[m, k], ref.flags)
    if ref.best == -2:
        assert_none(got, ref.flags, m, k)
        return 0.0, 0.0
    near = np.abs(ref.cos - float(F(COS))) <= NEAR
    differ = got.inlier_mask()[m, k] != ref.inliers
    assert not (differ & ~near).any(), "%s: %d inlier bits differ away from the bound" % (what, int((differ & ~near).sum()))
    assert got.n_inliers[m, k] == got.inlier_mask()[m, k].sum() and abs(int(got.n_inliers[m, k]) - ref.n_inliers) <= int(near.sum())
    d_uv = float(np.linalg.norm(got.uv[m, k].astype(np.float64) - ref.uv))
    sd = np.sqrt(np.maximum(got.cov[m, k].astype(np.float64)[[0, 2]], 0.0)) - np.sqrt(ref.cov[[0, 2]])
    d_stat = float(max(np.abs(got.mean[m, k].astype(np.float64) - ref.mean).max(), np.abs(sd).max()))
    assert d_uv <= t_uv, "%s: uv %.3g px from the reference" % (what, d_uv)
    assert d_stat <= t_stat, "%s: mean or standard deviation %.3g px from the reference" % (what, d_stat)
    return d_uv, d_stat


def test_twin_against_float64():
    worst = np.zeros(2)
    for K, frac in PIPELINE:
        pixel, vec, kps, clean, kw, got, ref = pipeline_case(K, frac)
        for m in range(len(pixel)):
            for k in range(vec.shape[2]):
                what = "K %d, %d %% replaced, set %d, keypoint %d" % (K, round(100 * frac), m, k)
                assert ref[m][k].best >= 0 and ref[m][k].flags & 3 == 0, what + ": the reference finds no keypoint"
                worst = np.maximum(worst, compare_with_reference(got, ref[m][k], what, m, k))
                if K >= 65:
                    # the keypoint itself: half a degree over <= 60 px is 0.5 px per voter, averaged over the inliers (with
                    # replaced vectors those inside the 8.1 degree cone pull a keypoint seen from one side along the view:
                    # there the inlier sets are the check)
                    assert frac > 0.0 or np.linalg.norm(ref[m][k].uv - kps[m, k]) < 0.5, what
                    assert ref[m][k].inliers[clean[m, :, k]].mean() > 0.95 and (ref[m][k].inliers & ~clean[m, :, k]).mean() < 0.1, what
    print("keypoint_vote twin against float64: worst uv %.3g px, worst mean / sqrt(cov) %.3g px" % tuple(worst))
    assert worst[0] * 4 <= T_UV * 1.0001 and worst[1] * 4 <= T_STAT * 1.0001, worst      # the constants are 4 x what is measured


# ---- 3. cases that do not count --------------------------------------------------------------------------------------------------
def test_voters_that_do_not_count_are_skipped():
    pixel, vec, _, _ = make_sets(1, 40, 2, 0.2, 7)
    clean = kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=32, seed=9)
    bad = np.zeros(48, bool)
    bad[[0, 5, 17, 33, 34, 40, 46, 47]] = True
    pixel2, vec2 = np.zeros((1, 48, 2), np.int16), np.ones((1, 48, 2, 2), F)
    pixel2[0, ~bad], vec2[0, ~bad] = pixel[0], vec[0]
    vec2[0, 0] = np.nan
    vec2[0, 5, :, 1] = np.inf
    vec2[0, 17] = 0.0
    vec2[0, 33, :, 0] = -np.inf
    pixel2[0, [34, 40, 46, 47]] = [[-1, 5], [SIZE[0], 5], [5, SIZE[1]], [5, -32768]]
    r = kv.vote_host(pixel2, vectors=vec2, size=SIZE, n_hypotheses=32, seed=9)
    # the valid list is the clean set in the same order: the same picks, the same position to the bit
    for k in ("uv", "mean", "cov", "best", "n_inliers", "flags"):
        assert np.array_equal(getattr(r, k).view(np.int32), getattr(clean, k).view(np.int32)), k
    assert np.array_equal(r.inlier_mask()[0][:, ~bad], clean.inlier_mask()[0]) and not r.inlier_mask()[0][:, bad].any()
    # a vector that counts for one keypoint only
    vec3 = vec2.copy()
    vec3[0, 0, 1] = vec[0, 0, 1]
    r3 = kv.vote_host(pixel2, vectors=vec3, size=SIZE, n_hypotheses=32, seed=9)
    assert np.array_equal(r3.uv[0, 0].view(np.int32), r.uv[0, 0].view(np.int32)) and not r3.inlier_mask()[0, 0, 0]


def test_dense_field_reads_what_the_gathered_vectors_hold():
    """both input modes give the same bits; a scene outside the field reads nothing and leaves its set without voters"""
    rng = np.random.default_rng(8)
    pixel, vec, _, _ = make_sets(3, 65, 2, 0.3, 8)
    field = rng.normal(size=(2, SIZE[1], SIZE[0], 2, 2)).astype(F)
    scene = np.array([1, 0, 1], np.int32)
    for m in range(3):
        field[scene[m], pixel[m, :, 1], pixel[m, :, 0]] = vec[m]
    pixel[2, 7] = (-4, 3)      # outside the picture: not read in either mode
    a = kv.vote_host(pixel, field=field, scene=scene, n_hypotheses=32, seed=4)
    b = kv.vote_host(pixel, vectors=R.gather(field, scene, pixel), size=SIZE, n_hypotheses=32, seed=4)
    for k in NAMES:
        assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), k
    assert a.found.all()
    for bad in (-1, 2, 2 ** 31 - 1):
        scene2 = scene.copy()
        scene2[1] = bad
        c = kv.vote_host(pixel, field=field, scene=scene2, n_hypotheses=32, seed=4)
        assert_none(c, _abi.VOTE_INSUFFICIENT, 1, 0)
        assert_none(c, _abi.VOTE_INSUFFICIENT, 1, 1)
        assert np.array_equal(c.uv[[0, 2]].view(np.int32), a.uv[[0, 2]].view(np.int32))


def test_one_valid_voter_is_insufficient():
    pixel, vec, _, _ = make_sets(1, 8, 1, 0.0, 9)
    vec[0, 1:] = 0.0
    assert_none(kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=16), _abi.VOTE_INSUFFICIENT)
    assert R.solve(pixel[0], vec[0, :, 0], SIZE).flags == R.INSUFFICIENT


def test_seed_set_and_keypoint_enter_the_counter():
    pixel, vec, _, _ = make_sets(1, 257, 1, 0.4, 10)
    a = kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=64, seed=1)
    b = kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=64, seed=1)
    for k in NAMES:
        assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), k
    assert len({int(kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=64, seed=s).best[0, 0]) for s in range(1, 6)}) > 1
    # set 1 of two equal sets draws differently, and as set_id_base 1 draws; keypoint 1 of two equal keypoints draws differently
    two = kv.vote_host(np.concatenate([pixel, pixel]), vectors=np.concatenate([vec, vec]), size=SIZE, n_hypotheses=64, seed=1)
    one = kv.vote_host(pixel, vectors=vec, size=SIZE, n_hypotheses=64, seed=1, set_id_base=1)
    assert np.array_equal(two.uv[0], a.uv[0]) and np.array_equal(two.uv[1], one.uv[0]) and two.best[1, 0] == one.best[0, 0]
    twice = kv.vote_host(pixel, vectors=np.concatenate([vec, vec], 2), size=SIZE, n_hypotheses=64, seed=1)
    ref = R.solve(pixel[0], vec[0, :, 0], SIZE, k=1, n_hypotheses=64, seed=1)
    assert twice.best[0, 0] == a.best[0, 0] and twice.best[0, 1] == ref.best


# ---- 4. parameters, arguments, outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,word", [
    ("W", 0, "picture"), ("H", 32769, "picture"), ("n_points", 1, "n_points"), ("n_points", 4097, "n_points"),
    ("n_keypoints", 0, "n_keypoints"), ("n_keypoints", 33, "n_keypoints"), ("n_hypotheses", 0, "n_hypotheses"),
    ("n_hypotheses", 1025, "n_hypotheses"), ("inlier_cos", 0.0, "inlier_cos"), ("inlier_cos", 1.0, "inlier_cos"),
    ("inlier_cos", np.nan, "inlier_cos"), ("min_inliers", 1, "min_inliers"), ("min_sin", -1e-3, "min_sin"), ("min_sin", np.inf, "min_sin"),
    ("min_sin", np.nan, "min_sin"), ("outputs", 0, "outputs"), ("outputs", 128, "outputs")])
def test_check_params_names_the_broken_rule(field, value, word):
    p = kv.make_params(SIZE, 1, 16, 9)
    kv.check_params(p)
    p[field] = value
    with pytest.raises(_abi.SlhipError, match=word):
        kv.check_params(p)


def host_call(null=None, misalign=None, mask=127, dense=True, n_field=2, **fields):
    M, K, Kp = 2, 16, 3
    pixel = np.zeros(M * K * 2 + 4, np.int16)
    pixel[:M * K * 2] = np.arange(M * K * 2) % 8
    vec = np.ones((2 * 8 * 8 * Kp * 2 if dense else M * K * Kp * 2) + 4, F)
    vec[1::4] = -0.5
    vec[2::6] = 0.25
    scene = np.zeros(M + 2, np.int32)
    outs = {k: np.full(256, POISON, np.uint32) for k in NAMES}
    ptr = {"pixel": pixel.ctypes.data, "vectors": vec.ctypes.data, "scene": scene.ctypes.data if dense else None}
    if misalign in ptr:
        ptr[misalign] += 4 if misalign == "vectors" else 2
    for k in ("pixel", "vectors"):
        if null == k:
            ptr[k] = None
    o = _abi.KeypointVoteOut(*(None if null == k else outs[k].ctypes.data + (2 if misalign == k else 0) for k in NAMES))
    p = kv.make_params((8, 8), M, K, Kp, n_hypotheses=8, outputs=mask).reshape(1)
    for k, v in fields.items():
        p[k] = v
    st = _abi.lib().slhip_keypoint_vote_host(None if null == "params" else p.ctypes.data, ptr["pixel"], ptr["vectors"], ptr["scene"],
                                             n_field, None if null == "record" else C.byref(o))
    return st, outs


REFUSALS = [dict(null="params"), dict(null="pixel"), dict(null="vectors"), dict(null="record"), dict(null="uv"), dict(null="cov"),
            dict(null="inliers"), dict(misalign="pixel"), dict(misalign="vectors"), dict(misalign="scene"), dict(misalign="mean"),
            dict(n_field=0), dict(W=0), dict(H=40000), dict(n_points=1), dict(n_points=4097), dict(n_keypoints=0), dict(n_keypoints=33),
            dict(n_hypotheses=0), dict(n_hypotheses=1025), dict(inlier_cos=1.0), dict(inlier_cos=0.0), dict(min_inliers=1),
            dict(min_sin=-1.0), dict(mask=0), dict(mask=128)]


@pytest.mark.parametrize("kw", REFUSALS)
def test_entries_refuse_bad_arguments(kw):
    st, outs = host_call(**kw)
    assert st < 0 and _abi.lib().slhip_last_error()
    for k in NAMES:
        assert (outs[k] == POISON).all(), k
    assert host_call()[0] == 0 and host_call(dense=False)[0] == 0 and host_call(dense=False, n_field=0)[0] == 0


def test_no_sets_succeed_and_write_nothing():
    st, outs = host_call(n_sets=0)
    assert st == 0 and all((o == POISON).all() for o in outs.values())


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 64, 1 | 64, 2 | 16 | 32])
def test_outputs_not_named_stay_poison(mask):
    st, outs = host_call(mask=mask)
    assert st == 0
    for i, k in enumerate(NAMES):
        if not mask & (1 << i):
            assert (outs[k] == POISON).all(), k
        else:
            assert (outs[k][:6] != POISON).all(), k
    pixel, vec, _, _ = make_sets(1, 8, 1, 0.0, 12)
    r = kv.vote_host(pixel, vectors=vec, size=SIZE, outputs=("uv", "best"))
    assert r.cov is None and r.inliers is None and r.uv is not None and r.found.all()
    with pytest.raises(RuntimeError):
        r.inlier_mask()
    with pytest.raises(RuntimeError):
        r.cov2x2()


def test_inlier_mask_bit_order_and_cov2x2():
    r = kv.KeypointVotes(40, inliers=np.array([[[1 | (1 << 31), 1 << 7]]], np.uint32), cov=np.array([[[1.0, 2.0, 3.0]]], F))
    m = r.inlier_mask()
    assert m.shape == (1, 1, 40) and m[0, 0].nonzero()[0].tolist() == [0, 31, 39]
    assert r.cov2x2().shape == (1, 1, 2, 2) and r.cov2x2()[0, 0].tolist() == [[1.0, 2.0], [2.0, 3.0]]


def test_correspondences_carry_the_found_flag():
    bank = np.arange(2 * 3 * 4, dtype=F).reshape(2, 3, 4)
    r = kv.KeypointVotes(8, uv=np.zeros((2, 3, 2), F), flags=np.array([[0, 2, 4], [1, 0, 8]], np.int32))
    uv, xyz = r.correspondences(bank, classes=[1, 0])
    assert uv is r.uv and xyz.shape == (2, 3, 4) and np.array_equal(xyz[..., :3], bank[[1, 0]][..., :3])
    assert xyz[..., 3].tolist() == [[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]
    with pytest.raises(TypeError):
        r.correspondences(bank)


def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5" in text and _abi.ABI_VERSION == 5 and _abi.lib().slhip_abi_version() == 5
    for name in ("slhip_keypoint_vote_check_params", "slhip_keypoint_vote", "slhip_keypoint_vote_host",
                 "slhip_keypoint_vote_timing_enable", "slhip_keypoint_vote_timings"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name), name
    assert "Stream 8" in text and _abi.SYNTH_STREAM_VOTE == R.STREAM == 8
    assert _abi.KEYPOINT_VOTE_PARAMS_DTYPE.itemsize == 64 and "} slhip_keypoint_vote_params; /* 64 bytes */" in text
    for name, bit in kv.OUTPUTS.items():
        assert re.search(r"#define SLHIP_VOTE_OUT_%s\s+%du\b" % (name.upper(), bit), text), name
    import stillleben as alias
    import stillleben_amd as sl
    assert sl.keypoint_vote is kv and alias.keypoint_vote is kv and sl.KeypointVotes is kv.KeypointVotes and "keypoint_vote" in sl.__all__
    assert alias.KeypointVotes is kv.KeypointVotes and hasattr(sl.SceneBatch, "keypoint_votes")


def test_cpu_tensors_are_refused():
    import torch

    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        kv.vote(torch.zeros((1, 8, 2), dtype=torch.int16), vectors=torch.ones((1, 8, 1, 2)))
