"""Keypoint voting in 3D on the host (slhip_keypoint_vote3d_host, slhip_keypoint_vote3d_check_params, sl.keypoint_vote3d) against
the independent float64 implementation tests/keypoint_vote3d_ref.py and against answers known by hand.  Needs no device.

The tolerance.  T_XYZ bounds the distance, per component, of the float32 twin's xyz and mean from the float64 reference's, T_COV
the same for the six covariance terms: each is four times the worst difference over the cases of test_twin_against_float64
(measured there on every run and printed; the constants below record it), rounded up to a power of two.  Both lie far below
tol = 1e-4 m, as they must: a twin that strayed from the reference by as much as a seed may still move would not be the same
mean shift.
    measured worst:  xyz and mean 7.2e-8 m (candidates about 1 m from the camera: under one float32 spacing),  cov 9.7e-12 m^2
The inputs of that test are built with a margin -- every cluster within 0.4 h of its centre, the centres 4 h apart, every outlier
at least 2 h from every cluster point, the sizes of the clusters at least 2 apart -- so that no discrete decision (who supports
whom, which seed wins) rests on rounding and no case is left out.  test_noisy_twin_against_float64 has no margin and may skip
a (set, keypoint) only where the float64 reference itself reports a near tie (keypoint_vote3d_ref.Result.near_tie)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keypoint_vote3d_ref as R
from stillleben_amd import _abi
from stillleben_amd import keypoint_vote3d as kv

F = np.float32
H = 0.05                     # the bandwidth of every test, metres
TOL = 1e-4
T_XYZ = 2.0 ** -21           # 4.8e-7 m: 4 x the measured worst 7.2e-8, up to a power of two
T_COV = 2.0 ** -34           # 5.8e-11 m^2: 4 x the measured worst 9.7e-12, up to a power of two
NAMES = ("xyz", "n_support", "best", "iters", "flags", "mean", "cov", "support")
POISON = 0x5A5A5A5A
KW = dict(bandwidth=H, tol=TOL, max_iters=32, min_support=1)


def in_ball(rng, n, radius):
    """n points uniform in a ball"""
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius * rng.random((n, 1)) ** (1.0 / 3.0)


def voters(rng, targets):
    """(camera float32 [K, 4], offsets float32 [K, 3]) whose candidates are `targets` [K, 3] up to float32 rounding: camera
    points scattered over an object's size about a metre from the camera"""
    K = len(targets)
    cam = np.ones((K, 4), F)
    cam[:, :3] = np.array([0.1, -0.05, 1.0]) + (rng.random((K, 3)) - 0.5) * 0.3
    return cam, (np.asarray(targets, np.float64) - cam[:, :3]).astype(F)


def make_clusters(M, K, Kp, seed, share_out=0.2, invalid=True, empty_set=None, h=H):
    """M sets of K voters, for each of Kp keypoints two clusters of 60 % and 40 % of the voters that are no outliers (radius
    0.4 h, centres 4 h apart, the sizes at least 2 apart) and `share_out` outliers at least 2 h from every cluster point, in a
    shuffled order; with `invalid` a sprinkle of voters that do not count (w == 0, a NaN or an infinite offset); set `empty_set`
    has no valid voter.  (camera [M, K, 4], offsets [M, K, Kp, 3], centres float64 [M, Kp, 3] of the large cluster,
    member bool [M, K, Kp] of the large cluster)"""
    rng = np.random.default_rng(seed)
    cam, off = np.zeros((M, K, 4), F), np.zeros((M, K, Kp, 3), F)
    centres, member = np.zeros((M, Kp, 3)), np.zeros((M, K, Kp), bool)
    for m in range(M):
        for k in range(Kp):
            n_out = int(share_out * K) if K >= 10 else 0
            big = max((6 * (K - n_out) + 9) // 10, 1)
            small = K - n_out - big
            if small > big - 2:      # the sizes at least 2 apart
                n_out += small - max(big - 2, 0)
                small = max(big - 2, 0)
            c0 = np.array([0.1, -0.05, 1.0]) + (rng.random(3) - 0.5) * 0.2
            axis = rng.normal(size=3)
            c1 = c0 + axis / np.linalg.norm(axis) * 4.0 * h
            pts = [c0 + in_ball(rng, big, 0.4 * h), c1 + in_ball(rng, small, 0.4 * h)]
            out = np.zeros((0, 3))
            while len(out) < n_out:
                cand = c0 + (rng.random((4 * n_out, 3)) - 0.5) * 40.0 * h
                far = np.linalg.norm(cand[:, None] - np.concatenate(pts)[None], axis=2).min(1) >= 2.2 * h
                out = np.concatenate([out, cand[far]])[:n_out]
            targets = np.concatenate(pts + [out])
            order = rng.permutation(K)
            targets, is_big = targets[order], (np.arange(K) < big)[order]
            if k == 0:
                cam[m], _ = voters(rng, targets)
            off[m, :, k] = (targets - cam[m, :, :3]).astype(F)
            centres[m, k], member[m, :, k] = c0, is_big
        if invalid and K >= 16:
            j = rng.permutation(K)[:max(3, K // 20)]
            cam[m, j[0::3], 3] = 0.0
            off[m, j[1::3], :, 1] = np.nan
            off[m, j[2::3], rng.integers(0, Kp)] = np.inf
    if empty_set is not None:
        cam[empty_set, :, 3] = 0.0
    valid = (cam[..., 3] != 0)[..., None] & np.isfinite(off).all(-1)
    return cam, off, centres, member & valid


def assert_none(r, flag, m=0, k=0):
    """NaN, never zeros"""
    assert r.flags[m, k] == flag and r.best[m, k] == -2 and r.n_support[m, k] == 0 and r.iters[m, k] == 0 and not r.found[m, k]
    assert np.isnan(r.xyz[m, k]).all() and np.isnan(r.mean[m, k]).all() and np.isnan(r.cov[m, k]).all() and not r.support[m, k].any()


def same_bits(a, b, names=NAMES):
    for k in names:
        assert np.array_equal(getattr(a, k).view(np.int32), getattr(b, k).view(np.int32)), k


# ---- 1. known answers ------------------------------------------------------------------------------------------------------------
def test_one_voter():
    cam = np.array([[[0.25, -0.5, 1.5, 1.0]]], F)
    off = np.array([[[[0.125, 0.25, -0.5]]]], F)
    r = kv.vote_host(cam, off, **KW)
    assert np.array_equal(r.xyz[0, 0], F([0.375, -0.25, 1.0])) and np.array_equal(r.mean[0, 0], r.xyz[0, 0])
    assert r.n_support[0, 0] == 1 and r.iters[0, 0] == 1 and r.best[0, 0] == 0 and r.flags[0, 0] == 0
    assert np.array_equal(r.cov[0, 0], np.zeros(6, F)) and r.support_mask()[0, 0].tolist() == [True]


def test_identical_candidates_give_the_candidate_exactly():
    """every d is 0, every w is 1: the shift is 0 / n = 0 and the seed stops where it started, at any tol.  (32 voters: the plain
    mean's sum, one voter a lane, doubles at every stage of the butterfly and is exact too)"""
    target = F([0.1234567, -0.7654321, 1.0101])
    cam = np.ones((1, 32, 4), F)
    cam[0, :, :3] = target      # offsets of zero: the sums are exact
    off = np.zeros((1, 32, 2, 3), F)
    r = kv.vote_host(cam, off, n_seeds=8, bandwidth=H, tol=0.0)
    for k in range(2):
        assert np.array_equal(r.xyz[0, k], target) and np.array_equal(r.mean[0, k], target) and np.array_equal(r.cov[0, k], np.zeros(6, F))
        assert r.n_support[0, k] == 32 and r.iters[0, k] == 1 and r.best[0, k] == 0 and r.flags[0, k] == 0 and r.support_mask()[0, k].all()


def test_large_cluster_wins_and_its_members_are_the_supporters():
    cam, off, centres, member = make_clusters(2, 100, 3, 2, share_out=0.0, invalid=False)
    r = kv.vote_host(cam, off, n_seeds=32, **KW)
    assert (r.flags == 0).all() and (r.n_support == 60).all() and member.sum(1).tolist() == [[60] * 3] * 2
    assert np.array_equal(r.support_mask(), member.transpose(0, 2, 1))
    assert np.abs(r.xyz - centres).max() < 0.4 * H and np.abs(r.mean - centres).max() < 0.4 * H


def test_equal_clusters_the_lower_seed_wins():
    """two clusters of 20 voters each, 4 h apart: with 8 seeds (ranks 2, 7, ..., 37) seeds 0-3 start in whichever cluster comes
    first, and seed 0 wins the tie"""
    rng = np.random.default_rng(3)
    a, b = np.array([0.0, 0.0, 1.0]) + in_ball(rng, 20, 0.4 * H), np.array([4 * H, 0.0, 1.0]) + in_ball(rng, 20, 0.4 * H)
    for first, second, centre in ((a, b, [0.0, 0.0, 1.0]), (b, a, [4 * H, 0.0, 1.0])):
        cam, off = voters(rng, np.concatenate([first, second]))
        r = kv.vote_host(cam[None], off[None, :, None], n_seeds=8, **KW)
        assert r.best[0, 0] == 0 and r.n_support[0, 0] == 20 and r.flags[0, 0] == 0
        assert np.abs(r.xyz[0, 0] - centre).max() < 0.4 * H and r.support_mask()[0, 0].tolist() == [True] * 20 + [False] * 20


def test_voters_that_do_not_count_are_skipped_and_the_ranks_move():
    cam, off, _, _ = make_clusters(1, 40, 2, 4, invalid=False)
    clean = kv.vote_host(cam, off, n_seeds=8, **KW)
    bad = np.zeros(48, bool)
    bad[[0, 5, 17, 33, 34, 40, 46, 47]] = True
    cam2, off2 = np.ones((1, 48, 4), F), np.ones((1, 48, 2, 3), F)
    cam2[0, ~bad], off2[0, ~bad] = cam[0], off[0]
    cam2[0, [0, 5], 3] = 0.0
    off2[0, 17] = np.nan
    off2[0, 33, :, 2] = np.inf
    off2[0, 34, :, 0] = -np.inf
    cam2[0, 40, 1] = np.nan
    cam2[0, [46, 47], 3] = [0.0, -0.0]
    r = kv.vote_host(cam2, off2, n_seeds=8, **KW)
    # the valid list is the clean set in the same order: the same seeds, the same position to the bit
    same_bits(r, clean, ("xyz", "mean", "cov", "best", "n_support", "iters", "flags"))
    assert np.array_equal(r.support_mask()[0][:, ~bad], clean.support_mask()[0]) and not r.support_mask()[0][:, bad].any()
    # an offset that counts for one keypoint only: voter 17 votes for keypoint 0 where clean voter 3 (voter 4 here) does, so
    # they support the same mode or neither; keypoint 1 does not notice
    off3 = off2.copy()
    off3[0, 17, 0] = off[0, 3, 0] + (cam[0, 3, :3] - cam2[0, 17, :3])
    r3 = kv.vote_host(cam2, off3, n_seeds=8, **KW)
    assert np.array_equal(r3.xyz[0, 1].view(np.int32), r.xyz[0, 1].view(np.int32)) and not r3.support_mask()[0, 1, 17]
    assert r3.support_mask()[0, 0, 17] == r3.support_mask()[0, 0, 4]


def test_no_valid_voter_is_insufficient():
    cam, off, _, _ = make_clusters(2, 20, 2, 5, empty_set=1)
    r = kv.vote_host(cam, off, **KW)
    for k in range(2):
        assert_none(r, _abi.VOTE3D_INSUFFICIENT, 1, k)
        assert R.solve(cam[1], off[1, :, k]).flags == R.INSUFFICIENT
    assert r.found[0].all()


def test_min_support_above_the_best_is_no_model():
    cam, off, _, member = make_clusters(1, 50, 1, 6, invalid=False)
    size = int(member.sum())
    assert kv.vote_host(cam, off, **dict(KW, min_support=size)).n_support[0, 0] == size
    assert_none(kv.vote_host(cam, off, **dict(KW, min_support=size + 1)), _abi.VOTE3D_NO_MODEL)
    assert R.solve(cam[0], off[0, :, 0], min_support=size + 1, bandwidth=H).flags == R.NO_MODEL


def test_one_step_on_a_spread_cluster_is_not_converged():
    rng = np.random.default_rng(7)
    cam, off = voters(rng, np.array([0.0, 0.0, 1.0]) + in_ball(rng, 80, 0.45 * H))
    r = kv.vote_host(cam[None], off[None, :, None], n_seeds=16, **dict(KW, max_iters=1))
    assert r.flags[0, 0] == _abi.VOTE3D_NOT_CONVERGED and r.iters[0, 0] == 1 and r.found[0, 0] and r.best[0, 0] >= 0
    assert np.isfinite(r.xyz[0, 0]).all() and r.n_support[0, 0] == 80 and np.isfinite(r.cov[0, 0]).all()
    assert kv.vote_host(cam[None], off[None, :, None], n_seeds=16, **KW).flags[0, 0] == 0


def test_more_seeds_than_voters_makes_every_candidate_a_seed():
    """five candidates more than h apart: each is its own mode; with S >= 5 seed s IS candidate s, with S = 1 the seed is the
    candidate of rank n_valid / 2"""
    rng = np.random.default_rng(8)
    targets = np.array([[0.0, 0.0, 1.0], [3 * H, 0.0, 1.0], [0.0, 3 * H, 1.0], [0.0, 0.0, 1.0 + 3 * H], [3 * H, 3 * H, 1.0]])
    cam, off = voters(rng, targets)
    cand = cam[:, :3] + off
    for S in (5, 64, 1024):
        r = kv.vote_host(cam[None], off[None, :, None], n_seeds=S, **KW)
        assert r.best[0, 0] == 0 and r.n_support[0, 0] == 1 and np.array_equal(r.xyz[0, 0], cand[0])
    # the pair (1, 4) is the only one within h once candidate 4 moves next to candidate 1: seed 1 finds both, seed 4 too -- 1 wins
    targets[4] = targets[1] + [0.2 * H, 0.0, 0.0]
    cam, off = voters(rng, targets)
    r = kv.vote_host(cam[None], off[None, :, None], n_seeds=64, **KW)
    assert r.best[0, 0] == 1 and r.n_support[0, 0] == 2 and r.support_mask()[0, 0].tolist() == [False, True, False, False, True]
    one = kv.vote_host(cam[None], off[None, :, None], n_seeds=1, **KW)
    assert one.best[0, 0] == 0 and one.n_support[0, 0] == 1 and np.array_equal(one.xyz[0, 0], (cam[:, :3] + off)[2])


# ---- 2. the twin against the reference -------------------------------------------------------------------------------------------
MARGIN = [(1, 2, 4), (2, 3, 4), (9, 2, 16), (65, 3, 32), (257, 2, 300), (1024, 2, 128)]      # K, Kp, S
_margin = {}


def margin_case(K, Kp, S):
    """(inputs, the library's result, the reference's), computed once"""
    if (K, Kp, S) not in _margin:
        cam, off, centres, member = make_clusters(2, K, Kp, 300 + K)
        kw = dict(KW, n_seeds=S)
        _margin[(K, Kp, S)] = (cam, off, member, kw, kv.vote_host(cam, off, **kw), R.solve_sets(cam, off, **kw))
    return _margin[(K, Kp, S)]


def compare_with_reference(got, ref, what, m, k):
    """every discrete output equal, the support sets equal; xyz and mean within T_XYZ, cov within T_COV per component.
    Returns (the worst of xyz and mean, the worst of cov)."""
    for name in ("best", "flags", "n_support", "iters"):
        assert getattr(got, name)[m, k] == getattr(ref, name), "%s: %s %d, the reference %d" % (what, name, getattr(got, name)[m, k], getattr(ref, name))
    if ref.best == -2:
        assert_none(got, ref.flags, m, k)
        return 0.0, 0.0
    assert np.array_equal(got.support_mask()[m, k], ref.support), "%s: the support sets differ" % what
    d_xyz = float(max(np.abs(got.xyz[m, k] - ref.xyz).max(), np.abs(got.mean[m, k] - ref.mean).max()))
    d_cov = float(np.abs(got.cov[m, k] - ref.cov).max())
    assert d_xyz <= T_XYZ, "%s: xyz or mean %.3g m from the reference" % (what, d_xyz)
    assert d_cov <= T_COV, "%s: cov %.3g m^2 from the reference" % (what, d_cov)
    return d_xyz, d_cov


def test_twin_against_float64():
    worst = np.zeros(2)
    for K, Kp, S in MARGIN:
        cam, off, member, kw, got, ref = margin_case(K, Kp, S)
        for m in range(len(cam)):
            for k in range(Kp):
                what = "K %d, S %d, set %d, keypoint %d" % (K, S, m, k)
                assert not ref[m][k].near_tie, what + ": the margin left a near tie"      # cap 0: no case is left out
                worst = np.maximum(worst, compare_with_reference(got, ref[m][k], what, m, k))
                assert np.array_equal(ref[m][k].support, member[m, :, k]), what      # the winner is the large cluster, whole
    print("keypoint_vote3d twin against float64: worst xyz / mean %.3g m, worst cov %.3g m^2" % tuple(worst))
    assert T_XYZ < TOL and 4 * worst[0] <= T_XYZ and 4 * worst[1] <= T_COV, worst      # the constants are >= 4 x what is measured


NOISY_SEED = 11      # chosen so that the float64 reference alone reports near ties in under 2 % of the cases (checked below)


def test_noisy_twin_against_float64():
    """no margin: Gaussian offsets of 0.3 h round the keypoint and 30 % of the voters anywhere in a box of 10 h.  A case may be
    skipped only where the float64 reference reports a near tie, and at most 2 % of them"""
    rng = np.random.default_rng(NOISY_SEED)
    M, K, Kp = 8, 200, 9
    cam = np.ones((M, K, 4), F)
    cam[..., :3] = np.array([0.1, -0.05, 1.0]) + (rng.random((M, K, 3)) - 0.5) * 0.3
    kp = np.array([0.1, -0.05, 1.0]) + (rng.random((M, Kp, 3)) - 0.5) * 0.2
    targets = kp[:, None] + rng.normal(size=(M, K, Kp, 3)) * 0.3 * H
    wild = rng.random((M, K, Kp)) < 0.3
    targets[wild] = (kp[:, None] + (rng.random((M, K, Kp, 3)) - 0.5) * 10.0 * H)[wild]
    off = (targets - cam[:, :, None, :3]).astype(F)
    kw = dict(KW, n_seeds=32)
    got, ref = kv.vote_host(cam, off, **kw), R.solve_sets(cam, off, **kw)
    skipped = 0
    for m in range(M):
        for k in range(Kp):
            if ref[m][k].near_tie:
                skipped += 1
                continue
            compare_with_reference(got, ref[m][k], "noisy set %d keypoint %d" % (m, k), m, k)
            assert np.linalg.norm(ref[m][k].xyz - kp[m, k]) < 0.3 * H
    print("keypoint_vote3d noisy twin: %d of %d cases skipped as near ties of the reference" % (skipped, M * Kp))
    assert skipped <= 0.02 * M * Kp


# ---- 3. parameters, arguments, outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,word", [
    ("n_points", 0, "n_points"), ("n_points", 4097, "n_points"), ("n_keypoints", 0, "n_keypoints"), ("n_keypoints", 33, "n_keypoints"),
    ("n_seeds", 0, "n_seeds"), ("n_seeds", 1025, "n_seeds"), ("bandwidth", 0.0, "bandwidth"), ("bandwidth", -1.0, "bandwidth"),
    ("bandwidth", np.nan, "bandwidth"), ("bandwidth", np.inf, "bandwidth"), ("bandwidth", 1e-30, "bandwidth"), ("max_iters", 0, "max_iters"),
    ("max_iters", 65, "max_iters"), ("tol", -1e-6, "tol"), ("tol", np.nan, "tol"), ("tol", np.inf, "tol"), ("min_support", 0, "min_support"),
    ("outputs", 0, "outputs"), ("outputs", 256, "outputs")])
def test_check_params_names_the_broken_rule(field, value, word):
    p = kv.make_params(1, 16, 9)
    kv.check_params(p)
    p[field] = value
    with pytest.raises(_abi.SlhipError, match=word):
        kv.check_params(p)


def host_call(null=None, misalign=None, mask=255, **fields):
    M, K, Kp = 2, 16, 3
    rng = np.random.default_rng(9)
    cam = np.ones(M * K * 4 + 8, F)
    cam[:M * K * 4] = np.concatenate([rng.random((M * K, 3)) * 0.02, np.ones((M * K, 1))], 1).astype(F).reshape(-1)
    off = np.zeros(M * K * Kp * 3 + 4, F)
    outs = {k: np.full(256, POISON, np.uint32) for k in NAMES}
    base = cam.ctypes.data + (-cam.ctypes.data) % 16      # the camera points 16-byte aligned
    ptr = {"camera": base, "offsets": off.ctypes.data}
    if misalign in ptr:
        ptr[misalign] += 4 if misalign == "camera" else 2
    for k in ("camera", "offsets"):
        if null == k:
            ptr[k] = None
    o = _abi.KeypointVote3dOut(*(None if null == k else outs[k].ctypes.data + (2 if misalign == k else 0) for k in NAMES))
    p = kv.make_params(M, K, Kp, n_seeds=8, outputs=mask).reshape(1)
    for k, v in fields.items():
        p[k] = v
    st = _abi.lib().slhip_keypoint_vote3d_host(None if null == "params" else p.ctypes.data, ptr["camera"], ptr["offsets"],
                                               None if null == "record" else C.byref(o))
    return st, outs


REFUSALS = [dict(null="params"), dict(null="camera"), dict(null="offsets"), dict(null="record"), dict(null="xyz"), dict(null="cov"),
            dict(null="support"), dict(null="iters"), dict(misalign="camera"), dict(misalign="offsets"), dict(misalign="mean"),
            dict(n_points=0), dict(n_points=4097), dict(n_keypoints=0), dict(n_keypoints=33), dict(n_seeds=0), dict(n_seeds=1025),
            dict(bandwidth=0.0), dict(max_iters=0), dict(max_iters=65), dict(tol=-1.0), dict(min_support=0), dict(mask=0), dict(mask=256)]


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


@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 64, 128, 1 | 128, 2 | 32 | 64])
def test_outputs_not_named_stay_poison(mask):
    st, outs = host_call(mask=mask)
    assert st == 0
    for i, k in enumerate(NAMES):
        if not mask & (1 << i):
            assert (outs[k] == POISON).all(), k
        else:
            assert (outs[k][:6] != POISON).all(), k
    cam, off, _, _ = make_clusters(1, 12, 1, 12, invalid=False)
    r = kv.vote_host(cam, off, outputs=("xyz", "best"), **KW)
    assert r.cov is None and r.support is None and r.xyz is not None and r.found.all()
    with pytest.raises(RuntimeError):
        r.support_mask()
    with pytest.raises(RuntimeError):
        r.cov3x3()


def test_support_mask_bit_order_and_cov3x3():
    r = kv.KeypointVotes3D(40, support=np.array([[[1 | (1 << 31), 1 << 7]]], np.uint32), cov=np.array([[[1.0, 2.0, 3.0, 4.0, 5.0, 6.0]]], F))
    m = r.support_mask()
    assert m.shape == (1, 1, 40) and m[0, 0].nonzero()[0].tolist() == [0, 31, 39]
    assert r.cov3x3().shape == (1, 1, 3, 3) and r.cov3x3()[0, 0].tolist() == [[1.0, 2.0, 3.0], [2.0, 4.0, 5.0], [3.0, 5.0, 6.0]]


def test_correspondences_carry_the_found_flag():
    bank = np.arange(2 * 3 * 4, dtype=F).reshape(2, 3, 4)
    xyz = np.arange(2 * 3 * 3, dtype=F).reshape(2, 3, 3)
    r = kv.KeypointVotes3D(8, xyz=xyz, flags=np.array([[0, 2, 4], [1, 0, 0]], np.int32))
    src, dst = r.correspondences(bank, classes=[1, 0])
    assert src.shape == (2, 3, 4) and np.array_equal(src, bank[[1, 0]]) and dst.shape == (2, 3, 4) and np.array_equal(dst[..., :3], xyz)
    assert dst[..., 3].tolist() == [[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]]
    with pytest.raises(TypeError):
        r.correspondences(bank)


def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5" in text and _abi.ABI_VERSION == 5 and _abi.lib().slhip_abi_version() == 5
    for name in ("slhip_keypoint_vote3d_check_params", "slhip_keypoint_vote3d", "slhip_keypoint_vote3d_host",
                 "slhip_keypoint_vote3d_timing_enable", "slhip_keypoint_vote3d_timings"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name), name
    assert _abi.KEYPOINT_VOTE3D_PARAMS_DTYPE.itemsize == 64 and "} slhip_keypoint_vote3d_params; /* 64 bytes */" in text
    for name, bit in kv.OUTPUTS.items():
        assert re.search(r"#define SLHIP_VOTE3D_OUT_%s\s+%du\b" % (name.upper(), bit), text), name
    for name, bit in kv.FLAGS.items():
        assert re.search(r"#define SLHIP_VOTE3D_%s\s+%d\b" % (name.upper(), bit), text), name
    import stillleben as alias
    import stillleben_amd as sl
    assert sl.keypoint_vote3d is kv and alias.keypoint_vote3d is kv and sl.KeypointVotes3D is kv.KeypointVotes3D
    assert "keypoint_vote3d" in sl.__all__ and alias.KeypointVotes3D is kv.KeypointVotes3D and hasattr(sl.SceneBatch, "keypoint_votes3d")


def test_cpu_tensors_are_refused():
    import torch

    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        kv.vote(torch.ones((1, 8, 4)), torch.zeros((1, 8, 1, 3)))
