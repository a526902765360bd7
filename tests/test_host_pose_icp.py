"""ICP on the host (slhip_pose_icp_host, slhip_pose_icp_check_params, sl.pose_icp) against tests/pose_icp_ref.py: bit for bit on
every output against the float32 restatement of the rules, and on known answers against the float64 loop with an SVD fit.  Needs
no device.

Known answers.  The camera points are R_gt p + t_gt (rounded to float32) of a subset of the bank's own points, so the fixed point
of the loop pairs every camera point with the bank point it came from and has a residual of float32 rounding only.  The initial
pose is the truth turned about a random axis and shifted by 2 mm per degree (pose_icp_ref.perturbed).  The turn is the largest step
of the ladder 1, 2, 5, 10 degrees for which the float64 reference ends in that fixed point -- every camera point paired with its own
bank point -- in every case: the clouds of KNOWN here and the rendered point sets of tests/test_gpu_pose_icp.py.
  * The clouds (64 to 600 points of a 0.05 m normal cloud, about 0.015 m apart) are recovered from every step, 10 degrees
    included: CLOUD_STEP = 10, which test_the_ladder_step_is_the_largest_that_the_reference_recovers checks on every run.
  * The rendered sets are not: their points are pixels, a lattice of a few millimetres on faces that are flat or round, and a
    shift of a lattice step along such a face is a fixed point of point-to-point ICP in any precision.  There the float64
    reference ends at the float64 SVD fit of the true correspondences for all 16 sets from 1 degree (2 mm), for 15 from 2 degrees
    and for 13 from 5 and from 10 (rendered coordinates repeat, so the criterion is the pose, not the indices); the GPU test
    prints the ladder on its data on every run and asserts the step.
So LADDER_STEP = 1 degree is the step of the known-answer checks of both files; the clouds are checked from CLOUD_STEP as well.

The tolerance of the twin against the float64 reference is the larger of
  * four times the reference's own worst pose difference from the truth (the margin of tests/test_gpu_pose_fit.py), and
  * the float32 floor of the data: a float32 coordinate of magnitude m carries eps m of rounding through every operation, points
    of RMS radius r about their centroid fix a rotation to eps m / r, and the pose difference is a norm over twelve entries:
    sqrt(12) eps m / r, m the largest |coordinate| of the camera points, r the bank's RMS radius (float32_floor).
Every figure is printed on every run."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import pose_fit_ref as RF
import pose_icp_ref as R
from stillleben_amd import _abi
from stillleben_amd import pose_icp as pi

F = np.float32
NAMES = ("pose", "n_pairs", "rms", "iters", "flags", "nearest")
POISON = 0x5A5A5A5A
LADDER = (1, 2, 5, 10)
LADDER_STEP = 1       # degrees: the largest step of LADDER that the float64 reference recovers in every case (the docstring)
CLOUD_STEP = 10       # degrees: the largest that it recovers on the clouds of KNOWN alone
KNOWN = [(200, 128, s) for s in range(6)] + [(64, 64, 10), (500, 256, 11), (600, 512, 12)]      # (bank points, K, seed)


def points4(xyz, w=1.0):
    out = np.full((len(xyz), 4), w, F)
    out[:, :3] = xyz
    return out


def pose_difference(poses, gt):
    d = np.asarray(poses, np.float64) - np.asarray(gt, np.float64)
    return np.sqrt((d * d).sum((-2, -1)))


def float32_floor(camera, bank_xyz):
    """sqrt(12) eps m / r (the docstring)"""
    ok = R.counts(camera)
    m = float(np.abs(camera[ok, :3]).max())
    p = np.asarray(bank_xyz, np.float64)
    r = float(np.sqrt(((p - p.mean(0)) ** 2).sum(1).mean()))
    return float(np.sqrt(12.0) * np.finfo(F).eps * m / r)


def make_case(K, count, seed, N=None, A=2, degrees=2.0, poison=True):
    """One set of class 1 of a bank of A classes: `count` points of a 0.05 m normal cloud, K camera points = the truth applied to
    bank points chosen at random.  `poison`: the rows past `count` are points at the origin, camera point 0 is the object's origin
    itself and bank point 0 lies 5 mm from it.  Returns (camera [1, K, 4], init [1, 3, 4], classes [1],
    points [A, N, 4], count [A], truth [3, 4], picks [K])."""
    rng = np.random.default_rng(seed)
    N = count + 3 if N is None else N
    points = np.zeros((A, N, 4), F)
    counts = np.zeros(A, np.int32)
    for a in range(A):
        n = count if a == 1 else min(N, 7)
        points[a, :n] = points4(rng.normal(size=(n, 3)) * 0.05)
        counts[a] = n
    if poison:
        points[1, 0, :3] = [0.004, -0.003, 0.002]
        points[:, :, 3] = 1.0      # the rows past count: (0, 0, 0, 1), nearer a query at the origin than any point of the class
    Rm, t = RF.random_rotation(rng), np.array([0.1, -0.05, 1.0]) + rng.normal(size=3) * 0.1
    picks = rng.permutation(count)[:K] if K <= count else np.concatenate([rng.permutation(count), rng.integers(0, count, K - count)])
    picks = picks.astype(np.int64)
    camera = points4(points[1, picks, :3].astype(np.float64) @ Rm.T + t)
    if poison:
        camera[0, :3] = t      # the object's origin itself
    init = R.perturbed(Rm, t, degrees, seed + 1000).astype(F)
    truth = np.concatenate([Rm, t[:, None]], 1)
    return camera[None], init[None], np.array([1], np.int32), points, counts, truth, picks


def same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got, F).view(np.int32), np.ascontiguousarray(want, F).view(np.int32))


def assert_same(host, refs, what, names=NAMES):
    """every output of the host twin against the restatement's Results, bit for bit (NaN against NaN by position)"""
    for m, r in enumerate(refs):
        w = "%s, set %d" % (what, m)
        if "flags" in names:
            assert host.flags[m] == r.flags, "%s: flags %d against %d" % (w, host.flags[m], r.flags)
        if "iters" in names:
            assert host.iters[m] == r.iters, "%s: iters %d against %d" % (w, host.iters[m], r.iters)
        if "n_pairs" in names:
            assert host.n_pairs[m] == r.n_pairs, "%s: n_pairs %d against %d" % (w, host.n_pairs[m], r.n_pairs)
        if "nearest" in names:
            assert np.array_equal(host.nearest[m], r.nearest), "%s: nearest differs at %r" % (w, np.flatnonzero(host.nearest[m] != r.nearest)[:8])
        if "pose" in names:
            if np.isnan(r.pose).all():
                assert np.isnan(host.pose[m]).all(), "%s: the pose must be NaN" % w
            else:
                assert same_bits(host.pose[m], r.pose), "%s: pose\n%r\nagainst\n%r" % (w, host.pose[m], r.pose)
        if "rms" in names:
            assert (np.isnan(r.rms) and np.isnan(host.rms[m])) or same_bits(host.rms[m], F(r.rms)), "%s: rms %r against %r" % (w, host.rms[m], r.rms)


def both(camera, init, classes, points, count, **kw):
    return pi.solve_host(camera, init, classes, (points, count), **kw), R.solve_rules(camera, init, classes, points, count, **kw)


# ---- 1. the twin against the float32 restatement, bit for bit --------------------------------------------------------------------
# K: one to five points, either side of the 256 stride and of the tile of 1024
@pytest.mark.parametrize("K", [1, 2, 3, 5, 255, 256, 257, 1023, 1024, 1025])
def test_camera_point_counts_bit_for_bit(K):
    camera, init, classes, points, count, truth, picks = make_case(K, 61, 20 + K)
    host, refs = both(camera, init, classes, points, count, max_iters=6, min_pairs=3)
    assert_same(host, refs, "K %d" % K)
    assert (host.nearest < 61).all()
    if K < 3:
        assert host.flags[0] == _abi.ICP_INSUFFICIENT and host.iters[0] == 0 and host.n_pairs[0] == K and np.isnan(host.pose).all()
    if K >= 255:
        assert host.found[0] and host.iters[0] >= 2


# count: a single point, the fewest that fit, either side of the 16-byte read and of the 256 stride; always count < N, the rows
# past count poisoned by points at the origin and camera point 0 at the object's origin
@pytest.mark.parametrize("count", [1, 3, 4, 5, 255, 256, 257])
def test_bank_counts_bit_for_bit_and_padding_is_never_matched(count):
    camera, init, classes, points, cnt, truth, picks = make_case(70, count, 40 + count)
    assert points.shape[1] > count and (points[1, count:, :3] == 0).all() and np.array_equal(camera[0, 0, :3], F(truth[:, 3]))
    host, refs = both(camera, init, classes, points, cnt, max_iters=6, min_pairs=3)
    assert_same(host, refs, "count %d" % count)
    assert (host.nearest < count).all() and host.n_pairs[0] == 70
    if count == 1:
        assert host.flags[0] == _abi.ICP_DEGENERATE and np.isnan(host.pose).all() and np.isnan(host.rms[0]) and host.iters[0] == 0
    if count >= 255:      # the case can fail: with the padded rows as candidates the query at the origin takes one of them
        assert host.found[0]
        cnt2 = cnt.copy()
        cnt2[1] = points.shape[1]
        assert pi.solve_host(camera, init, classes, (points, cnt2), max_iters=6, min_pairs=3).nearest[0, 0] >= count


def test_equidistant_bank_points_the_lowest_index_wins():
    cube = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)]) * 0.25      # exact in float32
    points = np.zeros((1, 12, 4), F)
    points[0, :8] = points4(cube)
    points[0, 8:10] = points4(cube[[3, 5]])      # copies of points 3 and 5 at higher indices
    eye = np.eye(4, dtype=F)[None, :3]
    camera = points4(np.concatenate([cube, [[0, 0, 0], [0.125, 0, 0], [0, 0.125, 0.125]]]))[None]      # centre, a face, an edge
    host, refs = both(camera, eye, np.zeros(1, np.int32), points, np.array([10], np.int32), max_iters=1, min_pairs=3)
    assert_same(host, refs, "ties")
    assert host.nearest[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 4, 3]


def test_points_that_do_not_count_are_skipped():
    camera, init, classes, points, count, truth, picks = make_case(300, 200, 3)
    clean, _ = both(camera, init, classes, points, count, max_iters=4, min_pairs=3)
    cam2 = camera.copy()
    cam2[0, 5::7, 3] = 0.0
    cam2[0, 6::7, 0] = np.nan
    cam2[0, 7::7, 2] = np.inf
    cam2[0, 8::7, 1] = -np.inf
    host, refs = both(cam2, init, classes, points, count, max_iters=4, min_pairs=3)
    assert_same(host, refs, "interleaved")
    ok = R.counts(cam2[0])
    assert host.n_pairs[0] == ok.sum() < 300 and (host.nearest[0][~ok] == -1).all() and (host.nearest[0][ok] >= 0).all()
    assert host.found[0]
    cam3 = cam2.copy()
    cam3[0, :, 3] = np.where(ok, -2.5, cam2[0, :, 3])      # w needs only to differ from 0
    assert same_bits(pi.solve_host(cam3, init, classes, (points, count), max_iters=4, min_pairs=3).pose, host.pose)


def test_the_gate():
    camera, init, classes, points, count, truth, picks = make_case(300, 200, 4, degrees=5.0)
    # rejects every pair: insufficient at iteration 0
    host, refs = both(camera, init, classes, points, count, max_dist=0.0, min_pairs=3)
    assert_same(host, refs, "gate 0")
    assert host.flags[0] == _abi.ICP_INSUFFICIENT and host.iters[0] == 0 and host.n_pairs[0] == 0 and (host.nearest == -1).all()
    assert np.isnan(host.pose).all() and np.isnan(host.rms[0]) and not host.found[0]
    # rejects some
    host, refs = both(camera, init, classes, points, count, max_dist=0.004, max_iters=1, min_pairs=3)
    assert_same(host, refs, "gate 4 mm")
    assert 3 <= host.n_pairs[0] < 300 and (host.nearest[0] == -1).sum() == 300 - host.n_pairs[0]
    # shrinks by dist_scale down to min_dist: the pairs of the last association lie inside the last gate
    kw = dict(max_dist=0.02, dist_scale=0.5, min_dist=0.003, max_iters=5, tol_rot=0.0, tol_trans=0.0, min_pairs=3)
    host, refs = both(camera, init, classes, points, count, **kw)
    assert_same(host, refs, "shrinking gate")
    assert host.iters[0] >= 2 and host.found[0]
    wide, _ = both(camera, init, classes, points, count, **dict(kw, dist_scale=1.0))
    assert not same_bits(wide.pose, host.pose)
    # +inf: no gate
    host, refs = both(camera, init, classes, points, count, max_dist=np.inf, max_iters=3, min_pairs=3)
    assert_same(host, refs, "no gate")
    assert host.n_pairs[0] == 300


def test_one_iteration_and_convergence():
    camera, init, classes, points, count, truth, picks = make_case(128, 200, 5, poison=False)
    host, refs = both(camera, init, classes, points, count, max_iters=1)
    assert_same(host, refs, "max_iters 1")
    assert host.iters[0] == 1 and host.found[0] and not host.converged[0] and np.isfinite(host.rms[0])
    host, refs = both(camera, init, classes, points, count, max_iters=30)
    assert_same(host, refs, "max_iters 30")
    assert host.converged[0] and host.found[0] and 2 <= host.iters[0] < 30 and host.flags[0] == _abi.ICP_CONVERGED
    assert np.array_equal(host.nearest[0], picks) and host.rms[0] < 1e-6


def test_a_collinear_bank_is_degenerate():
    line = np.outer(np.linspace(-0.1, 0.1, 9), [0.6, 0.0, 0.8]) + [0.01, 0.02, 0.03]
    points = points4(line)[None]
    camera = points4(line + [0.0, 0.0, 1.0])[None]
    init = F([[1, 0, 0, 0.001], [0, 1, 0, 0], [0, 0, 1, 1.0]])[None]
    host, refs = both(camera, init, np.zeros(1, np.int32), points, np.array([9], np.int32), min_pairs=3)
    assert_same(host, refs, "line")
    assert host.flags[0] == _abi.ICP_DEGENERATE and host.n_pairs[0] == 9 and host.iters[0] == 0 and (host.nearest >= 0).all()
    assert np.isnan(host.pose).all() and np.isnan(host.rms[0]) and not host.found[0]


def test_sets_that_cannot_start_and_mixed_classes():
    """one call: classes 1, 0, -1, A, 1 with a NaN init, 0 with an inf init, a class without points, 1 again"""
    camera, init, classes, points, count, truth, picks = make_case(40, 30, 6, A=3)
    count[2] = 0
    cls = np.array([1, 0, -1, 3, 1, 0, 2, 1], np.int32)
    cam = np.repeat(camera, 8, 0)
    ini = np.repeat(init, 8, 0)
    ini[4, 1, 2], ini[5, 2, 3] = np.nan, np.inf
    host, refs = both(cam, ini, cls, points, count, max_iters=4, min_pairs=3)
    assert_same(host, refs, "mixed")
    want = [0, None, _abi.ICP_BAD_CLASS, _abi.ICP_BAD_CLASS, _abi.ICP_NO_INIT, _abi.ICP_NO_INIT, _abi.ICP_BAD_CLASS, 0]
    for m, f in enumerate(want):
        if f:
            assert host.flags[m] == f and np.isnan(host.pose[m]).all() and np.isnan(host.rms[m]) and host.iters[m] == 0, m
            assert host.n_pairs[m] == 0 and (host.nearest[m] == -1).all() and not host.found[m], m
    assert host.found[0] and host.found[7] and same_bits(host.pose[0], host.pose[7])
    assert (host.nearest[1][host.nearest[1] >= 0] < count[0]).all()      # class 0 has its own, shorter row
    count[0] = points.shape[1] + 1      # a count past the row: the class is outside the bank
    assert pi.solve_host(cam[1:2], ini[1:2], cls[1:2], (points, count), min_pairs=3).flags[0] == _abi.ICP_BAD_CLASS


# ---- 2. known answers against the float64 reference ------------------------------------------------------------------------------
def known_case(n_bank, K, seed, degrees):
    return make_case(K, n_bank, 300 + seed, degrees=degrees, poison=False)


def recovered(res, picks):
    return res.flags in (0, R.CONVERGED) and np.array_equal(res.nearest, picks)


def test_the_ladder_step_is_the_largest_that_the_reference_recovers():
    best = 0
    for step in LADDER:
        got = []
        for n_bank, K, seed in KNOWN:
            camera, init, classes, points, count, truth, picks = known_case(n_bank, K, seed, step)
            got.append(recovered(R.icp_svd(camera[0], init[0], 1, points, count, max_iters=40), picks))
        print("ladder step %2d degrees: the float64 reference recovers %d of %d cases" % (step, sum(got), len(got)))
        if all(got) and best == LADDER.index(step):
            best += 1
    assert best >= 1 and LADDER[best - 1] == CLOUD_STEP and LADDER_STEP in LADDER[:best]


@pytest.mark.parametrize("step", [LADDER_STEP, CLOUD_STEP])
def test_known_answers_against_the_float64_reference(step):
    worst_ref = worst_twin = 0.0
    rows = []
    for n_bank, K, seed in KNOWN:
        camera, init, classes, points, count, truth, picks = known_case(n_bank, K, seed, step)
        ref = R.icp_svd(camera[0], init[0], 1, points, count, max_iters=40)
        assert recovered(ref, picks), (n_bank, K, seed)
        host = pi.solve_host(camera, init, classes, (points, count), max_iters=40)
        assert host.found[0] and np.array_equal(host.nearest[0], picks) and host.n_pairs[0] == K
        rows.append((pose_difference(ref.pose, truth), pose_difference(host.pose[0], ref.pose), float32_floor(camera[0], points[1, :n_bank, :3])))
        worst_ref, worst_twin = max(worst_ref, rows[-1][0]), max(worst_twin, rows[-1][1])
    for (n_bank, K, seed), (r, h, fl) in zip(KNOWN, rows):
        bound = max(4.0 * worst_ref, fl)
        print("bank %4d, K %4d, seed %2d: reference from the truth %.3g, twin from the reference %.3g, 4 x worst reference %.3g, "
              "float32 floor %.3g" % (n_bank, K, seed, r, h, 4.0 * worst_ref, fl))
        assert h <= bound, (n_bank, K, seed, h, bound)
    assert worst_ref < 1e-5      # the reference returns R_gt, t_gt up to the float32 rounding of the camera points


# ---- 3. surface_points -----------------------------------------------------------------------------------------------------------
def surface_of(verts, tris, begin, count):
    import torch

    from stillleben_amd import pose_vsd

    v = np.concatenate([np.asarray(verts, F), np.ones((len(verts), 1), F)], 1)
    return pose_vsd.surface(vertices=torch.from_numpy(v), triangles=torch.from_numpy(np.asarray(tris, np.int32)),
                            tri_begin=torch.tensor(begin, dtype=torch.int32), tri_count=torch.tensor(count, dtype=torch.int32))


def sphere_mesh(n_lat=9, n_lon=14):
    """a lumpy UV sphere: many triangles of very different areas"""
    v, t = [], []
    for i in range(n_lat + 1):
        for j in range(n_lon):
            th, ph = np.pi * i / n_lat, 2 * np.pi * j / n_lon
            r = 0.05 * (1.0 + 0.3 * np.sin(3 * ph) * np.sin(th))
            v.append([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), 1.7 * r * np.cos(th)])
    for i in range(n_lat):
        for j in range(n_lon):
            a, b, c, d = i * n_lon + j, i * n_lon + (j + 1) % n_lon, (i + 1) * n_lon + j, (i + 1) * n_lon + (j + 1) % n_lon
            t += [[a, c, b], [b, c, d]]
    return np.array(v), np.array(t)


def drawn_triangles(verts, tris, n):
    """the triangle of every sample by the documented rule, and n area / total per triangle"""
    v = np.asarray(verts, np.float64)[tris]
    area = 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    cum = np.cumsum(area)
    return np.searchsorted(cum, (np.arange(n) + 0.5) / n * cum[-1], side="right"), n * area / area.sum()


def check_samples(verts, tris, pts, n):
    """the counts per triangle sit within 1 of n area / total; every sample lies in its triangle's plane and inside it (float64;
    the samples are float32: 8 eps of the mesh's size off the plane, and as much relative to the triangle's size outside it)"""
    drawn, want = drawn_triangles(verts, tris, n)
    got = np.bincount(drawn, minlength=len(tris))
    assert (np.abs(got - want) <= 1.0).all(), (got, want)
    v = np.asarray(verts, np.float64)[tris][drawn]      # [n, 3, 3]
    p = np.asarray(pts, np.float64)
    e1, e2, d = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0], p - v[:, 0]
    cross = np.cross(e1, e2)
    size = np.sqrt(np.linalg.norm(cross, axis=1))
    tol = 8 * np.finfo(F).eps * float(np.abs(verts).max())
    off = np.abs((d * cross).sum(1)) / np.linalg.norm(cross, axis=1)
    assert (off <= tol).all(), "samples %r lie off their triangle's plane (%.3g)" % (np.flatnonzero(off > tol)[:8], off.max())
    d11, d12, d22, c1, c2 = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1), (d * e1).sum(1), (d * e2).sum(1)
    den = d11 * d22 - d12 * d12
    b1, b2 = (d22 * c1 - d12 * c2) / den, (d11 * c2 - d12 * c1) / den
    b = np.stack([1 - b1 - b2, b1, b2], 1)
    assert (b >= -(tol / size)[:, None]).all(), "samples %r lie outside their triangle" % np.flatnonzero((b < -(tol / size)[:, None]).any(1))[:8]
    assert len(np.unique(np.round(p / tol).astype(np.int64), axis=0)) == n      # no two samples coincide
    return got, want


def test_surface_points_two_triangles():
    verts = np.array([[0, 0, 0], [0.3, 0, 0], [0, 0.1, 0], [0, 0, 0.05], [0.02, 0, 0.05], [0, 0.05, 0.07]], float)
    tris = np.array([[0, 1, 2], [3, 4, 5]])
    surf = surface_of(verts, tris, [0], [2])
    n = 100
    pts, cnt = pi.surface_points(surf, n)
    assert tuple(pts.shape) == (1, n, 4) and pts.dtype.is_floating_point and int(cnt[0]) == n and (pts[0, :, 3] == 1).all()
    got, want = check_samples(verts, tris, pts[0, :, :3].numpy(), n)
    print("two triangles: %r samples for %r expected" % (got.tolist(), np.round(want, 2).tolist()))
    again, _ = pi.surface_points(surf, n)
    assert np.array_equal(pts.numpy().view(np.int32), again.numpy().view(np.int32))      # the same on every call


def test_surface_points_many_triangles_and_classes():
    sv, st = sphere_mesh()
    box = np.array([[x, y, z] for x in (-0.1, 0.1) for y in (-0.05, 0.05) for z in (-0.02, 0.02)], float)
    bt = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])
    verts = np.concatenate([sv, box])
    tris = np.concatenate([st, bt + len(sv)])
    surf = surface_of(verts, tris, [0, len(st), 0], [len(st), len(bt), 0])      # the third class has no triangles
    n = 700
    pts, cnt = pi.surface_points(surf, n)
    assert cnt.tolist() == [n, n, 0] and (pts[2] == 0).all()
    for c, t in ((0, st), (1, bt + len(sv))):
        got, want = check_samples(verts, t, pts[c, :, :3].numpy(), n)
        print("class %d: %d triangles, counts within %.2f of n area / total" % (c, len(t), np.abs(got - want).max()))
    again, _ = pi.surface_points(surf, n)
    assert np.array_equal(pts.numpy().view(np.int32), again.numpy().view(np.int32))
    with pytest.raises(ValueError):
        pi.surface_points(surf, 0)
    with pytest.raises(ValueError):
        pi.surface_points(surf, 4097)


# ---- 4. parameters, arguments, outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value,word", [
    ("n_points", 0, "n_points"), ("n_points", 4097, "n_points"), ("max_iters", 0, "max_iters"), ("max_iters", 65, "max_iters"),
    ("min_pairs", 2, "min_pairs"), ("max_dist", -1.0, "max_dist"), ("max_dist", np.nan, "max_dist"), ("dist_scale", 0.0, "dist_scale"),
    ("dist_scale", 1.5, "dist_scale"), ("dist_scale", np.nan, "dist_scale"), ("min_dist", -1e-3, "min_dist"), ("min_dist", np.nan, "min_dist"),
    ("min_gap", -1e-6, "min_gap"), ("min_gap", 1.0, "min_gap"), ("min_gap", np.nan, "min_gap"), ("tol_rot", -1.0, "tol_rot"),
    ("tol_rot", np.nan, "tol_rot"), ("tol_trans", -1.0, "tol_trans"), ("tol_trans", np.nan, "tol_trans"), ("outputs", 0, "outputs"),
    ("outputs", 64, "outputs")])
def test_check_params_names_the_broken_rule(field, value, word):
    p = pi.make_params(1, 16)
    pi.check_params(p)
    p[field] = value
    with pytest.raises(_abi.SlhipError, match=word):
        pi.check_params(p)


def test_defaults_and_limits_pass():
    p = pi.make_params(3, 4096, max_iters=64, dist_scale=1.0, max_dist=np.inf)
    pi.check_params(p)
    assert p["max_iters"] == 64 and p["min_pairs"] == 6 and np.isinf(p["max_dist"]) and p["outputs"] == 63
    d = pi.make_params(1, 1)
    assert (d["max_iters"], d["dist_scale"], d["min_dist"], d["tol_rot"], d["tol_trans"]) == (20, 1.0, 0.0, F(1e-6), F(1e-6))
    assert "not measured" in pi.make_params.__doc__ or "not a measured" in pi.make_params.__doc__


def aligned(a):
    """a 16-byte aligned copy of a float32 / int32 array (and what keeps it alive)"""
    raw = np.zeros(a.size + 8, a.dtype)
    shift = ((-raw.ctypes.data) % 16) // 4
    raw[shift:shift + a.size] = a.reshape(-1)
    return raw, raw.ctypes.data + 4 * shift


def host_call(null=None, misalign=None, mask=63, bank=None, **fields):
    M, K = 2, 16
    camera, init, classes, points, count, truth, picks = make_case(K, 12, 7)
    arrays = {"camera": np.repeat(camera, M, 0), "init": np.repeat(init, M, 0), "classes": np.repeat(classes, M), "points": points, "count": count}
    keep, ptr = {}, {}
    for k, a in arrays.items():
        keep[k], at = aligned(a)
        ptr[k] = None if null == k else at + ((4 if a.dtype == F else 2) if misalign == k else 0)
    outs = {k: np.full(64, POISON, np.uint32) for k in NAMES}
    o = _abi.PoseIcpOut(*(None if null == k else outs[k].ctypes.data + (2 if misalign == k else 0) for k in NAMES))
    b = dict(n_assets=points.shape[0], n_points=points.shape[1])
    b.update(bank or {})
    brec = _abi.PoseBank(ptr["points"], ptr["count"], None, None, b["n_assets"], b["n_points"], 1, 0)
    p = pi.make_params(M, K, min_pairs=3, outputs=mask).reshape(1)
    for k, v in fields.items():
        p[k] = v
    st = _abi.lib().slhip_pose_icp_host(None if null == "params" else p.ctypes.data, ptr["camera"], ptr["init"], ptr["classes"],
                                        None if null == "bank" else C.byref(brec), None if null == "record" else C.byref(o))
    return st, outs


REFUSALS = [dict(null=k) for k in ("params", "camera", "init", "classes", "bank", "points", "count", "record") + NAMES] + \
           [dict(misalign=k) for k in ("camera", "init", "classes", "points", "count") + NAMES] + \
           [dict(n_points=0), dict(n_points=4097), dict(max_iters=0), dict(max_iters=65), dict(min_pairs=2), dict(dist_scale=0.0),
            dict(dist_scale=1.0001), dict(max_dist=-1.0), dict(max_dist=np.nan), dict(min_dist=-1.0), dict(min_dist=np.nan),
            dict(tol_rot=-1.0), dict(tol_rot=np.nan), dict(tol_trans=-1.0), dict(tol_trans=np.nan), dict(min_gap=-1.0), dict(min_gap=1.0),
            dict(mask=0), dict(mask=64), dict(bank=dict(n_assets=0)), dict(bank=dict(n_points=0)), dict(bank=dict(n_points=4097))]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_entries_refuse_bad_arguments(kw):
    st, outs = host_call(**kw)
    assert st < 0 and _abi.lib().slhip_last_error()
    for k in NAMES:
        assert (outs[k] == POISON).all(), k
    assert host_call()[0] == 0


def test_no_sets_succeed_and_write_nothing():
    st, outs = host_call(n_sets=0)
    assert st == 0 and all((o == POISON).all() for o in outs.values())


def test_every_output_mask_subset():
    full, outs_full = host_call()
    assert full == 0
    width = dict(pose=24, n_pairs=2, rms=2, iters=2, flags=2, nearest=32)
    for r in range(1, 7):
        for names in itertools.combinations(range(6), r):
            mask = sum(1 << i for i in names)
            st, outs = host_call(mask=mask)
            assert st == 0, mask
            for i, k in enumerate(NAMES):
                if mask & (1 << i):      # named: the same words as with every output
                    assert np.array_equal(outs[k], outs_full[k]) and (outs[k][:width[k]] != POISON).all(), (mask, k)
                else:
                    assert (outs[k] == POISON).all(), (mask, k)
    camera, init, classes, points, count, truth, picks = make_case(16, 12, 7)
    r = pi.solve_host(camera, init, classes, (points, count), min_pairs=3, outputs=("pose",))
    assert r.rms is None and r.flags is None and r.nearest is None and r.found[0] and len(r) == 1
    with pytest.raises(RuntimeError):
        r.converged
    with pytest.raises(RuntimeError):
        pi.PoseICP(rms=r.pose).dense(1, 1, [0], [1])
    with pytest.raises(ValueError):
        pi.make_params(1, 1, outputs=("poses",))


def test_dense_places_the_poses():
    camera, init, classes, points, count, truth, picks = make_case(16, 12, 8)
    r = pi.solve_host(np.repeat(camera, 2, 0), np.stack([init[0], truth.astype(F)]), np.repeat(classes, 2), (points, count), min_pairs=3)
    d = r.dense(2, 3, [1, 0], [3, 1])
    assert d.shape == (2, 3, 3, 4) and np.array_equal(d[1, 2], r.pose[0]) and np.array_equal(d[0, 0], r.pose[1])
    assert np.isnan(d[0, 1:]).all() and np.isnan(d[1, :2]).all()


def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5" in text and _abi.ABI_VERSION == 5 and _abi.lib().slhip_abi_version() == 5
    for name in ("slhip_pose_icp_check_params", "slhip_pose_icp", "slhip_pose_icp_host", "slhip_pose_icp_timing_enable",
                 "slhip_pose_icp_timings"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name), name
    assert _abi.POSE_ICP_PARAMS_DTYPE.itemsize == 64 and "} slhip_pose_icp_params; /* 64 bytes */" in text
    for name, bit in pi.OUTPUTS.items():
        assert re.search(r"#define SLHIP_ICP_OUT_%s\s+%du\b" % (name.upper(), bit), text), name
    for name, bit in pi.FLAGS.items():
        assert re.search(r"#define SLHIP_ICP_%s\s+%d\b" % (name.upper(), bit), text), name
    assert re.search(r"#define SLHIP_ICP_FAILED\s+%d\b" % pi.FAILED, text) and pi.FAILED == sum(pi.FLAGS.values()) - pi.FLAGS["converged"]
    import stillleben as alias
    import stillleben_amd as sl
    assert sl.pose_icp is pi and alias.pose_icp is pi and sl.PoseICP is pi.PoseICP and "pose_icp" in sl.__all__
    assert alias.PoseICP is pi.PoseICP and hasattr(sl.SceneBatch, "pose_icp")


def test_cpu_tensors_are_refused():
    import torch

    from stillleben_amd import pose_error

    bank = pose_error.ModelBank(torch.ones((1, 8, 4)), torch.full((1,), 8, dtype=torch.int32), torch.eye(4)[None, None, :3].contiguous(),
                                torch.ones((1,), dtype=torch.int32))
    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        pi.solve(torch.ones((1, 8, 4)), torch.eye(4)[None, :3].contiguous(), torch.zeros((1,), dtype=torch.int32), bank)
    with pytest.raises(TypeError):
        pi.solve(torch.ones((1, 8, 4)), torch.eye(4)[None, :3].contiguous(), torch.zeros((1,), dtype=torch.int32), (None, None))
