"""Point k-NN on the device (slhip_point_knn, sl.point_knn, SceneBatch.point_graph) against the library's host twin of the same
rules (slhip_point_knn_host), bit for bit on every output -- floats as their int32 views --, and end to end on a placed batch
against tests/point_knn_ref.py, the NumPy statement of the rules.  Every output lies between 256 poisoned guard bytes that must
stay poison, an output that `outputs` does not name stays poison throughout, and every run is on a stream that is not the
default one.  No tolerance appears: the order (distance, index) is total, so the answer is unique.

The shapes are the smallest at which something can go wrong: Q = 257 leaves the second query block of a set one live lane;
R = TILE + 1 and 2 TILE + 3 end a tile unevenly with barriers on two and three tiles; R = 3 < k = 4 leaves empty slots; k = 1, 4,
7, 16, 32 run every instantiation of the kernel, k = 3 and 7 lie between the rungs of its ladder.  TILE is read from _abi."""
import ctypes as C

import numpy as np
import pytest
import torch

import point_knn_ref as R
from stillleben_amd import _abi
from stillleben_amd import point_knn as pk
from test_gpu_keypoint_vote3d import placed3d  # noqa: F401  (a fixture)
from test_gpu_object_keypoints import Guarded, bits, to_dev
from test_host_point_knn import ALL, NAMES, SHAPES, cloud

pytestmark = pytest.mark.gpu

F = np.float32
TILE = _abi.KNN_TILE
DTYPES = dict(idx=np.int32, dist2=F, count=np.int32)
N_SETS = 3


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


@pytest.fixture(scope="module")
def side(dev):
    """a stream that is not the default one"""
    return torch.cuda.Stream(device=dev)


def run_device(dev, side, queries, refs, k, mask=7, null=None, misalign=None, n_queries=None, n_refs=None, fields=None, **kw):
    """slhip_point_knn on uploaded copies of `queries` and `refs` (None: the queries' own buffer): (status, guarded outputs)"""
    n, qs = queries.shape[:2]
    rs = qs if refs is None else refs.shape[1]
    Q, Rn = qs if n_queries is None else n_queries, rs if n_refs is None else n_refs
    d_q = to_dev(queries, dev)
    d_r = d_q if refs is None else to_dev(refs, dev)
    ptr = {"queries": d_q.data_ptr(), "refs": d_r.data_ptr()}
    for name in ptr:
        ptr[name] = None if null == name else ptr[name] + (4 if misalign == name else 0)
    width = dict(idx=Q * k, dist2=Q * k, count=Q)
    outs = {name: Guarded(n * width[name] * 4, dev) for name in NAMES}
    o = _abi.PointKnnOut(*(None if null == name else outs[name].ptr().value + (2 if misalign == name else 0) for name in NAMES))
    p = pk.make_params(n, Q, Rn, k=k, query_stride=qs, ref_stride=rs, outputs=mask, **kw).reshape(1)
    for f, v in (fields or {}).items():
        p[f] = v
    torch.cuda.synchronize()
    with torch.cuda.device(dev), torch.cuda.stream(side):
        st = _abi.lib().slhip_point_knn(None if null == "params" else p.ctypes.data, C.c_void_p(ptr["queries"]), C.c_void_p(ptr["refs"]),
                                        None if null == "record" else C.byref(o), C.c_void_p(side.cuda_stream))
    side.synchronize()
    return st, outs, (d_q, d_r)


def read(outs, n, Q, k, mask=7):
    got = {}
    for i, name in enumerate(NAMES):
        if mask & (1 << i):
            got[name] = outs[name].host(DTYPES[name], (n, Q) if name == "count" else (n, Q, k)).copy()
        else:
            assert outs[name].untouched(), name
    return got


def assert_same(got, want, what):
    for name, v in got.items():
        w = getattr(want, name)
        assert v.shape == w.shape, (what, name, v.shape, w.shape)
        diff = bits(v).reshape(-1, 4).view(np.int32) != bits(w).reshape(-1, 4).view(np.int32)
        first = int(np.argwhere(diff.reshape(-1))[0][0]) if diff.any() else 0
        assert not diff.any(), "%s %s: %d of %d words differ, the first at %d: %r against %r" % (
            what, name, int(diff.sum()), diff.size, first, v.reshape(-1)[first], w.reshape(-1)[first])


CASES = SHAPES + [(257, TILE + 1, k) for k in (1, 3, 7, 32)] + [(5, 3, 1)]


@pytest.mark.parametrize("Q,Rn,k", CASES)
def test_device_against_host_twin_bit_for_bit(dev, side, Q, Rn, k):
    q, r = cloud(N_SETS, Q, 100 + Q + k), cloud(N_SETS, Rn, 200 + Rn + k)
    want = pk.search_host(q, r, k=k, outputs=ALL)
    st, outs, keep = run_device(dev, side, q, r, k)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, N_SETS, Q, k), want, "Q %d, R %d, k %d" % (Q, Rn, k))
    assert (want.count == min(k, Rn)).any() and (want.count == 0).any() or Q < 5


@pytest.mark.parametrize("Q,Rn,k", [(257, TILE + 1, 16), (64, 2 * TILE + 3, 32)])
def test_device_against_host_twin_with_a_gate(dev, side, Q, Rn, k):
    q, r = cloud(N_SETS, Q, 300 + Q), cloud(N_SETS, Rn, 400 + Rn)
    want = pk.search_host(q, r, k=k, max_dist=0.375, outputs=ALL)
    st, outs, keep = run_device(dev, side, q, r, k, max_dist=0.375)
    assert st == 0
    assert_same(read(outs, N_SETS, Q, k), want, "gate")
    assert (want.dist2 == F(0.375) * F(0.375)).any() and (want.count < k).any() and (want.count > 0).any()


@pytest.mark.parametrize("skip", [True, False])
def test_self_search(dev, side, skip):
    p = cloud(N_SETS, 300, 11)
    want = pk.search_host(p, k=3, skip_same=skip, outputs=ALL)
    st, outs, keep = run_device(dev, side, p, None, 3, skip_same=skip)
    assert st == 0, _abi.lib().slhip_last_error()
    assert_same(read(outs, N_SETS, 300, 3), want, "self, skip_same %r" % skip)
    assert (want.idx == np.arange(300)[None, :, None]).any() != skip


def test_prefix_of_the_same_tensor(dev, side):
    """the queries are all 64 points, the references the first 16 of the same tensor (ref_stride = 64), k = 1: the up-sampling
    index of the pyramid"""
    p = cloud(N_SETS, 64, 12)
    want = pk.search_host(p, p, k=1, n_refs=16, outputs=ALL)
    st, outs, keep = run_device(dev, side, p, None, 1, n_refs=16)
    assert st == 0
    assert_same(read(outs, N_SETS, 64, 1), want, "prefix")
    assert want.idx.max() < 16
    ref = R.search(p, None, 1, n_refs=16)
    assert np.array_equal(want.idx, ref[0]) and np.array_equal(want.count, ref[2])
    # and a prefix of the queries over a longer row of references, through the wrapper
    d_p = torch.from_numpy(p).to(dev)
    with torch.cuda.stream(side):
        nb = pk.search(d_p, k=4, n_queries=20, n_refs=33, outputs=ALL)
    side.synchronize()
    assert_same({name: getattr(nb, name).cpu().numpy() for name in NAMES}, pk.search_host(p, k=4, n_queries=20, n_refs=33, outputs=ALL), "wrapper prefix")


def test_two_runs_give_the_same_bytes(dev, side):
    q, r = cloud(N_SETS, 257, 13), cloud(N_SETS, TILE + 1, 14)
    a = read(run_device(dev, side, q, r, 16)[1], N_SETS, 257, 16)
    b = read(run_device(dev, side, q, r, 16)[1], N_SETS, 257, 16)
    for name in NAMES:
        assert np.array_equal(bits(a[name]), bits(b[name])), name


@pytest.mark.parametrize("mask", [1, 2, 4, 3, 5, 6])
def test_outputs_not_named_stay_poison(dev, side, mask):
    q, r = cloud(N_SETS, 70, 15), cloud(N_SETS, 90, 16)
    st, outs, keep = run_device(dev, side, q, r, 5, mask=mask)
    assert st == 0
    assert_same(read(outs, N_SETS, 70, 5, mask), pk.search_host(q, r, k=5, outputs=ALL), "mask %d" % mask)


def test_refusals_leave_the_device_untouched(dev, side):
    q, r = cloud(2, 16, 17), cloud(2, 20, 18)
    refusals = [dict(null=name) for name in ("params", "queries", "refs", "record") + NAMES]
    refusals += [dict(misalign=name) for name in ("queries", "refs") + NAMES]
    refusals += [dict(fields=f) for f in (dict(k=0), dict(k=33), dict(n_queries=0), dict(n_refs=0), dict(n_queries=17), dict(n_refs=21),
                                          dict(max_dist=np.nan), dict(max_dist=-1.0), dict(skip_same=1), dict(skip_same=2), dict(outputs=0),
                                          dict(outputs=8))]
    for kw in refusals:
        st, outs, keep = run_device(dev, side, q, r, 4, **kw)
        assert st < 0, kw
        assert all(o.untouched() for o in outs.values()), kw
    st, outs, keep = run_device(dev, side, q, q.copy(), 4, fields=dict(skip_same=1))      # equal strides, two buffers
    assert st < 0 and all(o.untouched() for o in outs.values())
    st, outs, keep = run_device(dev, side, q, r, 4, fields=dict(n_sets=0))      # no sets: fine, and writes nothing
    assert st == 0 and all(o.untouched() for o in outs.values())
    assert run_device(dev, side, q, r, 4)[0] == 0


def test_step_timer(dev, side):
    q, r = cloud(2, 64, 19), cloud(2, 61, 20)
    L = _abi.lib()
    ms = (C.c_float * 1)()
    try:
        assert L.slhip_point_knn_timing_enable(1) == 0
        assert run_device(dev, side, q, r, 4, mask=0)[0] < 0                        # a refused call records no event
        assert L.slhip_point_knn_timings(C.byref(ms)) == 0 and list(ms) == [-1.0]
        assert run_device(dev, side, q, r, 4)[0] == 0
        assert L.slhip_point_knn_timings(C.byref(ms)) == 0 and np.isfinite(ms[0]) and ms[0] >= 0.0
        assert L.slhip_point_knn_timings(None) < 0
    finally:
        L.slhip_point_knn_timing_enable(0)


# ---- end to end on a placed batch ------------------------------------------------------------------------------------------------
def test_point_graph_of_a_render(placed3d, side):  # noqa: F811
    sl, batch, _, kbank, kps, off, mbank = placed3d
    bufs = batch.render(0, object_masks=True)
    points = batch.points(bufs, n_points=64, outputs=("camera", "coord"))
    torch.cuda.synchronize()
    n = len(points)
    assert n >= 4
    repeats = 0
    for space in ("camera", "coord"):
        with torch.cuda.stream(side):
            graph = batch.point_graph(points, k=8, space=space)
            pyr = batch.point_graph(points, k=8, space=space, ratios=(2, 2))
        side.synchronize()
        cloud_h = getattr(points, space).cpu().numpy()
        idx, d2, count = R.search(cloud_h, None, 8)
        assert graph.dist2 is None and np.array_equal(graph.idx.cpu().numpy(), idx) and np.array_equal(graph.count.cpu().numpy(), count), space
        sizes, nei, up = R.pyramid(cloud_h, 8, (2, 2))
        assert pyr.sizes == [64, 32, 16] == sizes
        for l in range(2):
            assert np.array_equal(pyr.neighbours[l].cpu().numpy(), nei[l]) and np.array_equal(pyr.interp[l].cpu().numpy(), up[l]), (space, l)
            assert pyr.xyz(l).data_ptr() == getattr(points, space).data_ptr() and tuple(pyr.xyz(l).shape) == (n, sizes[l], 4)
        assert count.max() == 8 and int(pyr.interp[1].max()) < 16
        repeats += int((d2[..., 1] == 0).sum())
        filled = graph.filled().cpu().numpy()
        assert (filled[count > 0] >= 0).all() and np.array_equal(filled[idx >= 0], idx[idx >= 0])
    print("point_graph: %d sets of 64 points, %d points with a copy of themselves as second neighbour" % (n, repeats))
    only = batch.points(bufs, n_points=64, outputs=("camera",))
    with pytest.raises(RuntimeError, match="coord"):
        batch.point_graph(only, k=8, space="coord")
    with pytest.raises(ValueError):
        batch.point_graph(points, k=8, space="world")
    with pytest.raises(ValueError):
        batch.point_graph(points, k=8, ratios=(3,))
    with pytest.raises(_abi.SlhipError, match="no CPU path"):
        pk.search(points.camera.cpu(), k=8)
