"""Point k-NN on the host (slhip_point_knn_host, slhip_point_knn_check_params, sl.point_knn) against known answers worked out by
hand and against tests/point_knn_ref.py, the NumPy statement of the rules (masks and a lexsort, no scan).  Every comparison is bit
for bit, floats as their int32 views: the rules leave nothing to a tolerance.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import point_knn_ref as R
from stillleben_amd import _abi
from stillleben_amd import point_knn as pk

F = np.float32
NAMES = ("idx", "dist2", "count")
ALL = ("idx", "dist2", "count")
POISON = 0x5A5A5A5A
TILE = _abi.KNN_TILE
# (Q, R, k): a single pair; fewer references than k; a query block with one live lane over a tile and one reference; three tiles
# that end unevenly at the top of the ladder
SHAPES = [(1, 1, 1), (5, 3, 4), (257, TILE + 1, 16), (64, 2 * TILE + 3, 32)]


def lattice():
    """the 3 x 3 x 3 integer lattice, point x + 3 y + 9 z: [1, 27, 4]"""
    p = np.ones((1, 27, 4), F)
    for i in range(27):
        p[0, i, :3] = [i % 3, (i // 3) % 3, i // 9]
    return p


def cloud(n, P, seed, dirty=True):
    """[n, P, 4]: coordinates that are multiples of 1/8 in a cube of side 2 (exact ties abound), w of 1 or -2.5, and with `dirty`
    a sprinkle of points that do not count: w = 0, a NaN, a +inf and a -inf coordinate"""
    rng = np.random.default_rng(seed)
    p = np.empty((n, P, 4), F)
    p[..., :3] = rng.integers(0, 17, (n, P, 3)) / 8.0
    p[..., 3] = np.where(rng.random((n, P)) < 0.5, 1.0, -2.5)
    if dirty and P >= 5:
        for i in range(n):
            j = rng.permutation(P)[:max(4, P // 12)]
            p[i, j[0::4], 3] = 0.0
            p[i, j[1::4], 0] = np.nan
            p[i, j[2::4], 2] = np.inf
            p[i, j[3::4], 1] = -np.inf
    return p


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.int32), want.view(np.int32))


def assert_same(res, ref, what):
    """a PointNeighbours against the reference's (idx, dist2, count), bit for bit (NaN against NaN by its bits' position)"""
    idx, d2, count = ref
    if res.idx is not None:
        assert np.array_equal(res.idx, idx), "%s: idx differs at %r" % (what, np.argwhere(res.idx != idx)[:4].tolist())
    if res.dist2 is not None:
        assert np.array_equal(np.isnan(res.dist2), np.isnan(d2)), "%s: the NaN slots of dist2 differ" % what
        ok = ~np.isnan(d2)
        assert same_bits(res.dist2[ok], d2[ok]), "%s: dist2 differs" % what
    if res.count is not None:
        assert np.array_equal(res.count, count), "%s: count differs" % what


def both(queries, refs=None, **kw):
    return pk.search_host(queries, refs, outputs=ALL, **kw), R.search(queries, refs, **kw)


# ---- 1. known answers by hand ----------------------------------------------------------------------------------------------------
def test_lattice_centre_and_corner():
    p = lattice()
    r = pk.search_host(p, k=7, outputs=ALL)
    assert r.idx[0, 13].tolist() == [13, 4, 10, 12, 14, 16, 22] and r.dist2[0, 13].tolist() == [0, 1, 1, 1, 1, 1, 1] and r.count[0, 13] == 7
    r = pk.search_host(p, k=4, outputs=ALL)
    assert r.idx[0, 0].tolist() == [0, 1, 3, 9] and r.dist2[0, 0].tolist() == [0, 1, 1, 1]
    assert_same(r, R.search(p, k=4), "lattice")


def test_lattice_skip_same_drops_the_self_and_closes_with_the_next_candidate():
    p = lattice()
    r = pk.search_host(p, k=7, skip_same=True, outputs=ALL)
    assert r.idx[0, 13].tolist() == [4, 10, 12, 14, 16, 22, 1] and r.dist2[0, 13].tolist() == [1, 1, 1, 1, 1, 1, 2]      # 1: the first at distance^2 2
    r = pk.search_host(p, k=4, skip_same=True, outputs=ALL)
    assert r.idx[0, 0].tolist() == [1, 3, 9, 4] and r.dist2[0, 0].tolist() == [1, 1, 1, 2]      # 4 = (1, 1, 0)
    assert_same(r, R.search(p, k=4, skip_same=True), "lattice, skip_same")


def test_lattice_gate_is_inclusive_and_empty_slots_hold_minus_one_and_nan():
    p = lattice()
    r = pk.search_host(p, k=8, max_dist=1.0, outputs=ALL)
    assert r.count[0, 13] == 7 and r.idx[0, 13].tolist() == [13, 4, 10, 12, 14, 16, 22, -1]
    assert r.dist2[0, 13, :7].tolist() == [0, 1, 1, 1, 1, 1, 1] and np.isnan(r.dist2[0, 13, 7])
    assert r.count[0, 0] == 4 and r.idx[0, 0].tolist() == [0, 1, 3, 9, -1, -1, -1, -1] and np.isnan(r.dist2[0, 0, 4:]).all()
    assert r.found[0, 13].tolist() == [True] * 7 + [False]
    assert r.filled()[0, 13].tolist() == [13, 4, 10, 12, 14, 16, 22, 13] and r.filled()[0, 0].tolist() == [0, 1, 3, 9, 0, 0, 0, 0]
    assert_same(r, R.search(p, k=8, max_dist=1.0), "lattice, gate 1")
    assert pk.search_host(p, k=8, max_dist=np.nextafter(F(1), F(0)), outputs=ALL).count[0, 13] == 1      # just under: the self alone
    assert pk.search_host(p, k=8, max_dist=0.0, skip_same=True, outputs=ALL).count.max() == 0


def test_duplicates_are_told_apart_by_index():
    p = np.ones((1, 6, 4), F)
    p[0, :, :3] = [[1, 1, 1], [2, 2, 2], [1, 1, 1], [1, 1, 1], [2, 2, 2], [0, 0, 0]]
    r, ref = both(p, k=3)
    assert_same(r, ref, "duplicates")
    assert r.idx[0].tolist() == [[0, 2, 3], [1, 4, 0], [0, 2, 3], [0, 2, 3], [1, 4, 0], [5, 0, 2]]
    r, ref = both(p, k=3, skip_same=True)
    assert_same(r, ref, "duplicates, skip_same")
    assert r.idx[0].tolist() == [[2, 3, 1], [4, 0, 2], [0, 3, 1], [0, 2, 1], [1, 0, 2], [0, 2, 3]]      # the other copies stay
    assert (r.dist2[0, [0, 2, 3], :2] == 0).all()


# ---- 2. the twin against the NumPy reference, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("Q,Rn,k", SHAPES)
def test_host_twin_against_numpy(Q, Rn, k):
    q, r = cloud(2, Q, 10 + Q), cloud(2, Rn, 20 + Rn)
    res, ref = both(q, r, k=k)
    assert_same(res, ref, "Q %d, R %d, k %d" % (Q, Rn, k))
    assert (res.count <= min(k, Rn)).all() and ((res.idx >= 0).sum(-1) == res.count).all()
    if Rn > k:
        assert (res.count[R.counts(q)] == k).all() and (res.count[~R.counts(q)] == 0).all()
        srt = np.sort(res.idx, -1)
        assert ((srt[..., 1:] != srt[..., :-1]) | (srt[..., 1:] < 0)).all()      # never a repeated neighbour
    if Rn > 100:      # exact ties abound: some list holds equal distances, in rising index order
        tie = res.dist2[..., 1:] == res.dist2[..., :-1]
        assert tie.any() and (res.idx[..., 1:][tie] > res.idx[..., :-1][tie]).all()


@pytest.mark.parametrize("Q,Rn,k", SHAPES)
def test_host_twin_with_a_finite_gate(Q, Rn, k):
    q, r = cloud(2, Q, 30 + Q), cloud(2, Rn, 40 + Rn)
    res, ref = both(q, r, k=k, max_dist=0.375)      # 0.375^2 = 9/64 = (3/8)^2 of the lattice: reached exactly
    assert_same(res, ref, "gate, Q %d, R %d, k %d" % (Q, Rn, k))
    with np.errstate(invalid="ignore"):
        assert not (res.dist2 > F(0.375) * F(0.375)).any()
    if Rn > 100:
        assert (res.dist2 == F(0.375) * F(0.375)).any() and (res.count < k).any()


@pytest.mark.parametrize("Q,Rn,k", SHAPES)
def test_host_twin_on_prefixes_of_longer_rows(Q, Rn, k):
    q, r = cloud(2, Q + 9, 50 + Q), cloud(2, Rn + 5, 60 + Rn)
    res, ref = both(q, r, k=k, n_queries=Q, n_refs=Rn)
    assert_same(res, ref, "strides, Q %d, R %d, k %d" % (Q, Rn, k))
    assert res.idx.shape == (2, Q, k) and res.idx.max() < Rn
    whole = pk.search_host(q, r, k=k, outputs=ALL)
    assert whole.idx.shape == (2, Q + 9, k)
    assert_same(pk.search_host(np.ascontiguousarray(q[:, :Q]), np.ascontiguousarray(r[:, :Rn]), k=k, outputs=ALL), ref, "copied prefixes")


def test_self_search_with_skip_same():
    p = cloud(2, 300, 7)
    res, ref = both(p, k=3, skip_same=True)
    assert_same(res, ref, "self, skip_same")
    assert (res.idx != np.arange(300)[None, :, None]).all()
    res, ref = both(p, k=3)
    assert_same(res, ref, "self")
    ok = R.counts(p)
    assert (res.idx[..., 0][ok] <= np.broadcast_to(np.arange(300), (2, 300))[ok]).all() and (res.dist2[..., 0][ok] == 0).all()
    res, ref = both(p, k=3, skip_same=True, max_dist=0.125)
    assert_same(res, ref, "self, skip_same, gate")


def test_the_list_does_not_depend_on_k():
    q, r = cloud(1, 40, 3), cloud(1, 700, 4)
    full = pk.search_host(q, r, k=32, outputs=ALL)
    for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 31):
        res = pk.search_host(q, r, k=k, outputs=ALL)
        assert np.array_equal(res.idx, full.idx[..., :k]) and same_bits(res.dist2, full.dist2[..., :k]), k
        assert np.array_equal(res.count, np.minimum(full.count, k)), k


def test_points_that_do_not_count():
    q, r = cloud(1, 64, 5, dirty=False), cloud(1, 200, 6, dirty=False)
    clean = pk.search_host(q, r, k=8, outputs=ALL)
    q2, r2 = q.copy(), r.copy()
    q2[0, 3, 3], q2[0, 4, 1], q2[0, 5, 2] = 0.0, np.nan, np.inf
    bad = clean.idx[0, 10, :3].copy()      # the three nearest references of query 10 stop counting
    r2[0, bad[0], 3], r2[0, bad[1], 0], r2[0, bad[2], 2] = 0.0, np.nan, -np.inf
    res, ref = both(q2, r2, k=8)
    assert_same(res, ref, "non-counting")
    assert res.count[0, 3:6].tolist() == [0, 0, 0] and (res.idx[0, 3:6] == -1).all() and np.isnan(res.dist2[0, 3:6]).all()
    assert not np.isin(res.idx, bad).any() and res.count[0, 10] == 8
    big = np.ones((1, 2, 4), F)
    big[0, :, 0] = [3e38, -3e38]      # finite points at a distance of +inf: no neighbours of each other
    res, ref = both(big, k=2)
    assert_same(res, ref, "overflow")
    assert res.idx[0].tolist() == [[0, -1], [1, -1]]


# ---- 3. the pyramid --------------------------------------------------------------------------------------------------------------
def test_pyramid_through_the_host_twin():
    p = cloud(3, 64, 8)
    pyr = pk.pyramid_host(p, k=5, ratios=(2, 2))
    sizes, nei, up = R.pyramid(p, 5, (2, 2))
    assert pyr.sizes == [64, 32, 16] == sizes and pyr.levels == 2 and len(pyr.neighbours) == 2 and len(pyr.interp) == 2
    for l in range(2):
        assert pyr.neighbours[l].shape == (3, sizes[l], 5) and pyr.neighbours[l].dtype == np.int32
        assert pyr.interp[l].shape == (3, sizes[l], 1) and pyr.interp[l].dtype == np.int32
        assert np.array_equal(pyr.neighbours[l], nei[l]) and np.array_equal(pyr.interp[l], up[l]), l
        assert pyr.interp[l].max() < sizes[l + 1] and pyr.neighbours[l].max() < sizes[l]
        assert pyr.xyz(l).shape == (3, sizes[l], 4) and np.shares_memory(pyr.xyz(l), pyr.points)
        assert np.array_equal(pyr.sub(l), nei[l][:, :sizes[l + 1]])
    assert pyr.xyz(2).shape == (3, 16, 4)
    ok = R.counts(p)
    first = np.broadcast_to(np.arange(32), (3, 32))
    assert (pyr.interp[0][:, :32, 0][ok[:, :32]] <= first[ok[:, :32]]).all()      # a point of the next level is its own nearest, or an earlier copy
    assert pk.pyramid_host(p, k=5, ratios=(2, 2), interp=False).interp is None
    assert pk.pyramid_host(p, k=5, ratios=(64,)).sizes == [64, 1]
    for ratios in ((3,), (2, 2, 2, 2, 2, 2, 2), (0,), ()):
        with pytest.raises(ValueError):
            pk.pyramid_host(p, k=5, ratios=ratios)
    assert "valid-depth" in pk.pyramid.__doc__ and "r2p" in pk.pyramid.__doc__ and "p2r" in pk.pyramid.__doc__


# ---- 4. parameters, arguments, outputs -------------------------------------------------------------------------------------------
BROKEN = [
    (dict(n_sets=0x80000000), "n_sets"), (dict(n_queries=0), "n_queries"), (dict(n_refs=0), "n_refs"), (dict(query_stride=15), "query_stride"),
    (dict(ref_stride=19), "ref_stride"), (dict(k=0), "k"), (dict(k=33), "k"), (dict(max_dist=np.nan), "max_dist"), (dict(max_dist=-1.0), "max_dist"),
    (dict(skip_same=2), "skip_same"), (dict(skip_same=1), "skip_same"), (dict(outputs=0), "outputs"), (dict(outputs=8), "outputs"),
    (dict(n_sets=1 << 20, n_queries=1 << 10, query_stride=1 << 10, k=2), "2\\^31"),      # 2^31 list elements
    (dict(n_sets=1 << 16, ref_stride=1 << 13), "2\\^31"),                                 # 2^31 floats of an input
]


@pytest.mark.parametrize("fields,word", BROKEN, ids=lambda v: "-".join("%s=%s" % i for i in v.items()) if isinstance(v, dict) else None)
def test_check_params_names_the_broken_rule(fields, word):
    p = pk.make_params(2, 16, 20, k=4)      # (strides 16 and 20: skip_same alone breaks the equal strides)
    pk.check_params(p)
    for f, v in fields.items():
        p[f] = v
    with pytest.raises(_abi.SlhipError, match=word):
        pk.check_params(p)


def test_limits_pass():
    pk.check_params(pk.make_params(1, 1, 1, k=1))
    pk.check_params(pk.make_params(0, 1, 1, k=1))
    pk.check_params(pk.make_params(1, 8, 8, k=32, skip_same=True, max_dist=0.0, outputs=ALL))
    pk.check_params(pk.make_params((1 << 31) // (1024 * 16) - 1, 1024, 1024, k=16))
    pk.check_params(pk.make_params(1, (1 << 29) - 1, 1, k=1))      # 2^31 - 4 floats
    p = pk.make_params(3, 5, 7)
    assert (p["k"], p["query_stride"], p["ref_stride"], p["skip_same"], p["outputs"]) == (16, 5, 7, 0, 5) and np.isinf(p["max_dist"])
    with pytest.raises(ValueError):
        pk.make_params(1, 1, 1, outputs=("index",))


def aligned(a):
    """a 16-byte aligned copy of a float32 array (and what keeps it alive)"""
    raw = np.zeros(a.size + 8, a.dtype)
    shift = ((-raw.ctypes.data) % 16) // 4
    raw[shift:shift + a.size] = a.reshape(-1)
    return raw, raw.ctypes.data + 4 * shift


def host_call(null=None, misalign=None, mask=7, other_refs=False, **fields):
    n, P, k = 2, 12, 3
    pts = cloud(n, P, 9)
    keep_q, q = aligned(pts)
    keep_r, r = aligned(pts) if other_refs else (keep_q, q)
    ptr = {"queries": q, "refs": r}
    for name in ptr:
        ptr[name] = None if null == name else ptr[name] + (4 if misalign == name else 0)
    outs = {name: np.full(n * P * k + 8, POISON, np.uint32) for name in NAMES}
    o = _abi.PointKnnOut(*(None if null == name else outs[name].ctypes.data + (2 if misalign == name else 0) for name in NAMES))
    p = pk.make_params(n, P, P, k=k, outputs=mask).reshape(1)
    for f, v in fields.items():
        p[f] = v
    st = _abi.lib().slhip_point_knn_host(None if null == "params" else p.ctypes.data, ptr["queries"], ptr["refs"],
                                         None if null == "record" else C.byref(o))
    return st, outs


REFUSALS = [dict(null=name) for name in ("params", "queries", "refs", "record") + NAMES] + \
           [dict(misalign=name) for name in ("queries", "refs") + NAMES] + \
           [dict(skip_same=1, other_refs=True), dict(k=0), dict(k=33), dict(n_queries=13), dict(n_refs=13), dict(max_dist=np.nan), dict(mask=0),
            dict(mask=8)]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_entries_refuse_bad_arguments(kw):
    st, outs = host_call(**kw)
    assert st < 0 and _abi.lib().slhip_last_error()
    for name in NAMES:
        assert (outs[name] == POISON).all(), name
    assert host_call()[0] == 0 and host_call(skip_same=1)[0] == 0 and host_call(other_refs=True)[0] == 0


def test_no_sets_succeed_and_write_nothing():
    st, outs = host_call(n_sets=0)
    assert st == 0 and all((o == POISON).all() for o in outs.values())
    assert pk.search_host(np.zeros((0, 4, 4), F), k=2).idx.shape == (0, 4, 2)


def test_every_output_mask_subset():
    st, full = host_call()
    assert st == 0
    width = dict(idx=2 * 12 * 3, dist2=2 * 12 * 3, count=2 * 12)
    for mask in range(1, 8):
        st, outs = host_call(mask=mask)
        assert st == 0, mask
        for i, name in enumerate(NAMES):
            if mask & (1 << i):
                assert np.array_equal(outs[name], full[name]) and (outs[name][width[name]:] == POISON).all(), (mask, name)
            else:
                assert (outs[name] == POISON).all(), (mask, name)
    r = pk.search_host(cloud(1, 9, 1), k=2)
    assert r.dist2 is None and r.idx is not None and r.count is not None and len(r) == 1
    r = pk.search_host(cloud(1, 9, 1), k=2, outputs=("dist2",))
    with pytest.raises(RuntimeError):
        r.found
    with pytest.raises(RuntimeError):
        r.filled()


def test_python_arguments():
    p = cloud(2, 9, 2)
    for bad in (dict(refs=cloud(3, 9, 2)), dict(refs=cloud(2, 9, 3), skip_same=True), dict(n_queries=10), dict(n_refs=0), dict(n_queries=0)):
        with pytest.raises(ValueError):
            pk.search_host(p, **{"k": 2, **bad})
    with pytest.raises(ValueError):
        pk.search_host(p[..., :3], k=2)
    with pytest.raises(_abi.SlhipError, match="k"):
        pk.search_host(p, k=33)
    assert_same(pk.search_host(p, p, k=2, skip_same=True, outputs=ALL), R.search(p, k=2, skip_same=True), "refs is queries")


def test_header_declares_the_entries_and_abi_stays_5():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    text = open(os.path.join(root, "include", "slhip.h")).read()
    assert "#define SLHIP_ABI_VERSION 5" in text and _abi.ABI_VERSION == 5 and _abi.lib().slhip_abi_version() == 5
    for name in ("slhip_point_knn_check_params", "slhip_point_knn", "slhip_point_knn_host", "slhip_point_knn_timing_enable",
                 "slhip_point_knn_timings"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert hasattr(_abi.lib(), name), name
    assert _abi.POINT_KNN_PARAMS_DTYPE.itemsize == 48 and "} slhip_point_knn_params; /* 48 bytes */" in text
    fields = re.search(r"typedef struct \{([^}]*)\} slhip_point_knn_params;", text).group(1)
    assert re.findall(r"(?:uint32_t|float) (\w+)", fields) == list(_abi.POINT_KNN_PARAMS_DTYPE.names)
    for name, value in (("K_MAX", _abi.KNN_K_MAX), ("BLOCK", _abi.KNN_BLOCK), ("TILE", _abi.KNN_TILE)):
        assert re.search(r"#define SLHIP_KNN_%s\s+%du\b" % (name, value), text), name
    assert _abi.KNN_K_MAX == 32 and _abi.KNN_BLOCK == 256 and _abi.KNN_TILE % _abi.KNN_BLOCK == 0
    for name, bit in pk.OUTPUTS.items():
        assert re.search(r"#define SLHIP_KNN_OUT_%s\s+%du\b" % (name.upper(), bit), text), name
    assert [f[0] for f in _abi.PointKnnOut._fields_] == list(pk.OUTPUTS) == list(NAMES)
    import stillleben as alias
    import stillleben_amd as sl
    assert sl.point_knn is pk and alias.point_knn is pk and sl.PointNeighbours is pk.PointNeighbours and "point_knn" in sl.__all__
    assert alias.PointPyramid is pk.PointPyramid and hasattr(sl.SceneBatch, "point_graph")


def test_cpu_tensors_are_refused():
    import torch

    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        pk.search(torch.ones((1, 8, 4)), k=2)
    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        pk.pyramid(torch.ones((1, 8, 4)), k=2, ratios=(2,))
    with pytest.raises(ValueError):
        pk.search(np.ones((1, 8, 4), F), k=2)
