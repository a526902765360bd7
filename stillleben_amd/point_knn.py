"""Point neighbours -- this project's addition (the reference has no counterpart): for every query point of a set its k nearest
reference points of the same set, as lists sorted by (distance, index), and the RandLA pyramid composed from them -- what the
data loaders of FFB6D and PVN3D-with-RandLA build per frame with a CPU kd-tree (cld_nei_idx, cld_sub_idx, cld_interp_idx,
r2p_ds_nei_idx, p2r_ds_nei_idx), and the k-NN grouping of PointNet++ / DGCNN style refiners on the point sets of ObjectPoints.
Everything stays on the device, through one entry of include/slhip.h: slhip_point_knn, one workgroup per set and 256 queries with
the references passing through LDS.  There is no CPU path; `search_host` and `pyramid_host` run the library's host twin of the same
rules for tests and need no device.

    nb = sl.point_knn.search(points.camera, k=16)                         # self-search: .idx [n, K, 16] .count [n, K] (.dist2 on request)
    nb = sl.point_knn.search(points.camera, k=16, skip_same=True, max_dist=0.01)      # DGCNN / normals: without the point itself, gated
    nb.filled()                                                            # -1 replaced by the row's nearest: what a gather wants
    pyr = sl.point_knn.pyramid(cloud, k=16, ratios=(4, 4, 4, 4))           # .sizes .neighbours[l] .interp[l] .xyz(l)
    graph = batch.point_graph(points, k=16, space="coord")                 # the same on the ObjectPoints of a render

DESIGN.md "Point neighbours" states the rules operation by operation."""
import ctypes as C

import numpy as np
import torch

from . import _abi, _device, _record_set

__all__ = ["OUTPUTS", "PointNeighbours", "PointPyramid", "make_params", "check_params", "search", "search_host", "pyramid", "pyramid_host"]

NAME = "point_knn"


class PointNeighbours(_record_set.OutputSet):
    """The neighbour lists of every query (torch tensors on the device from `search`, numpy arrays from `search_host`; those not
    asked for are None):
        idx    int32 [n, Q, k] the references of every query, nearest first, among equal distances the lower index first; -1 in a
               slot without a neighbour (fewer candidates than k)
        dist2  float32 [n, Q, k] their squared distances, NaN in such a slot
        count  int32 [n, Q] the filled slots; 0 for a query that does not count (w == 0, or a coordinate that is not finite)
        found  bool [n, Q, k]: the slot holds a neighbour"""
    NAME, RECORD = NAME, _abi.PointKnnOut
    TABLE = (("idx", _abi.KNN_OUT_IDX, ("k",), np.int32), ("dist2", _abi.KNN_OUT_DIST2, ("k",), np.float32),
             ("count", _abi.KNN_OUT_COUNT, (), np.int32))

    def __init__(self, idx=None, dist2=None, count=None):
        super().__init__(idx=idx, dist2=dist2, count=count)

    @property
    def found(self):
        if self.idx is None:
            raise RuntimeError("point_knn: `found` reads the `idx` output, which was not asked for")
        return self.idx >= 0

    def filled(self):
        """`idx` with every -1 replaced by the row's slot 0, the nearest neighbour -- the index tensor a gather takes (RandLA
        repeats a neighbour where a point has fewer than k).  A row without any neighbour stays -1 throughout.  Plain tensor
        work, no kernel."""
        if self.idx is None:
            raise RuntimeError("point_knn: `filled` reads the `idx` output, which was not asked for")
        where = np.where if isinstance(self.idx, np.ndarray) else torch.where
        return where(self.idx >= 0, self.idx, self.idx[..., :1])


OUTPUTS = PointNeighbours.OUTPUTS


def make_params(n_sets, n_queries, n_refs, k=16, max_dist=float("inf"), skip_same=False, query_stride=None, ref_stride=None,
                outputs=("idx", "count")):
    """One slhip_point_knn_params record (numpy).
        n_queries, n_refs        Q and R, the points of a set that are searched from and among
        query_stride, ref_stride the points from one set to the next in memory (default: Q and R); larger ones make a prefix
                                 of every row the set
        k                        1..32 neighbours per query
        max_dist                 a reference farther than this is no neighbour (the distance itself passes); +inf: no gate
        skip_same                a self-search without the query's own index
    `outputs`: names or the bit mask."""
    p = np.zeros((), _abi.POINT_KNN_PARAMS_DTYPE)
    p["n_sets"], p["n_queries"], p["n_refs"], p["k"] = int(n_sets), int(n_queries), int(n_refs), int(k)
    p["query_stride"] = int(n_queries if query_stride is None else query_stride)
    p["ref_stride"] = int(n_refs if ref_stride is None else ref_stride)
    p["max_dist"], p["skip_same"] = np.float32(max_dist), 1 if skip_same else 0
    p["outputs"] = outputs if isinstance(outputs, int) else _record_set.output_bits(outputs, OUTPUTS)
    return p


def check_params(params):
    """Raises SlhipError when the record breaks a rule of slhip_point_knn_check_params.  Needs no device."""
    rec = np.ascontiguousarray(np.asarray(params, dtype=_abi.POINT_KNN_PARAMS_DTYPE).reshape(1))
    _abi.check(_abi.lib().slhip_point_knn_check_params(rec.ctypes.data), "slhip_point_knn")
    return rec


def _shapes(queries, refs, n_queries, n_refs, skip_same):
    """(refs, n, Q, R, query stride, ref stride) of [n, *, 4] arrays or tensors"""
    same = refs is None or refs is queries
    refs = queries if same else refs
    for name, a in (("queries", queries), ("refs", refs)):
        if len(a.shape) != 3 or a.shape[2] != 4:
            raise ValueError("point_knn: `%s` must be [n, points, 4]" % name)
    if refs.shape[0] != queries.shape[0]:
        raise ValueError("point_knn: queries and refs must hold the same number of sets")
    if skip_same and not same:
        raise ValueError("point_knn: skip_same is for a self-search (refs=None)")
    n, qs, rs = int(queries.shape[0]), int(queries.shape[1]), int(refs.shape[1])
    Q, R = qs if n_queries is None else int(n_queries), rs if n_refs is None else int(n_refs)
    if not 1 <= Q <= qs or not 1 <= R <= rs:
        raise ValueError("point_knn: n_queries %d and n_refs %d must lie in [1, %d] and [1, %d], the points of the rows" % (Q, R, qs, rs))
    return refs, n, Q, R, qs, rs


def search_host(queries, refs=None, k=16, max_dist=float("inf"), skip_same=False, n_queries=None, n_refs=None, outputs=("idx", "count")):
    """slhip_point_knn_host on host arrays: a PointNeighbours of numpy arrays.  The arguments of `search`, as float32 arrays
    [n, points, 4].  Needs no device: the CPU tests' handle."""
    queries = np.ascontiguousarray(queries, np.float32)
    refs = None if refs is None else np.ascontiguousarray(refs, np.float32)
    refs, n, Q, R, qs, rs = _shapes(queries, refs, n_queries, n_refs, skip_same)
    rec = check_params(make_params(n, Q, R, k, max_dist, skip_same, qs, rs, outputs))
    res = PointNeighbours(**PointNeighbours.empty((n, Q), int(rec["outputs"][0]), k=int(k)))
    if n:
        _abi.check(_abi.lib().slhip_point_knn_host(rec.ctypes.data, queries.ctypes.data, refs.ctypes.data, C.byref(res.record())),
                   "slhip_point_knn_host")
    return res


def search(queries, refs=None, k=16, max_dist=float("inf"), skip_same=False, n_queries=None, n_refs=None, outputs=("idx", "count")):
    """The k nearest references of every query: a PointNeighbours.

    queries    float32 [n, Pq, 4] on the device, the layout of ObjectPoints.camera and .coord: a point counts when its w != 0
               and x, y, z are finite
    refs       float32 [n, Pr, 4] on the device, or None: the queries themselves (a self-search)
    k          1..32
    max_dist   the gate, in the points' unit; +inf: none
    skip_same  self-search only: the query's own index is no candidate (DGCNN, normal estimation: on; RandLA: off).  Decided
               by index, so a duplicate of the query at another index stays a neighbour
    n_queries, n_refs   fewer than Pq, Pr: the first so many points of every row are the set (nothing is copied)
    outputs    of "idx", "dist2", "count"

    Among equal distances the lower index comes first, so the answer is unique whatever the coordinates repeat.  Asynchronous
    on the current stream; the result keeps its inputs alive."""
    same = refs is None or refs is queries
    dev = _device.require_cuda(NAME, (queries,) if same else (queries, refs), "queries and refs", "queries and refs must be torch tensors")
    for name, t in (("queries", queries),) if same else (("queries", queries), ("refs", refs)):
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 4 or not t.is_contiguous():
            raise ValueError("point_knn: `%s` must be a contiguous float32 [n, points, 4] tensor" % name)
    refs, n, Q, R, qs, rs = _shapes(queries, refs, n_queries, n_refs, skip_same)
    rec = check_params(make_params(n, Q, R, k, max_dist, skip_same, qs, rs, outputs))
    res = PointNeighbours(**PointNeighbours.empty((n, Q), int(rec["outputs"][0]), dev, k=int(k)))
    if n:
        out = res.record()
        with torch.cuda.device(dev):
            st = _abi.lib().slhip_point_knn(rec.ctypes.data, C.c_void_p(queries.data_ptr()), C.c_void_p(refs.data_ptr()), C.byref(out),
                                            _device.stream_ptr(dev))
        _abi.check(st, "slhip_point_knn")
    res._keepalive = (queries, refs)      # the launch is asynchronous: its inputs live as long as its outputs
    return res


class PointPyramid:
    """The neighbourhood graph of a cloud at every level of a RandLA-style encoder, level l + 1 being the first N_l / ratio_l
    points of level l (the clouds arrive in random order, so a prefix is a random sub-sample):
        sizes          [N_0, N_1, ..., N_L], L = the number of ratios
        neighbours[l]  int32 [n, N_l, k], l < L: for every point of level l its k nearest among the level's points, itself
                       included (cld_nei_idx); -1 where a point has fewer -- PointNeighbours(idx=...).filled() for a gather
        interp[l]      int32 [n, N_l, 1], l < L: for every point of level l the nearest of the N_l+1 points of the next level
                       (cld_interp_idx); None without `interp`
        xyz(l)         the level's points, a view of `points`
    cld_sub_idx, the neighbours of the points that survive to the next level, is neighbours[l][:, :N_l+1]: a view as well."""

    def __init__(self, points, sizes, neighbours, interp):
        self.points, self.sizes, self.neighbours, self.interp = points, sizes, neighbours, interp

    @property
    def levels(self):
        return len(self.sizes) - 1

    def xyz(self, level):
        return self.points[:, :self.sizes[level]]

    def sub(self, level):
        """neighbours[level] of the points that are level + 1: int32 [n, N_level+1, k], a view"""
        return self.neighbours[level][:, :self.sizes[level + 1]]


def _pyramid(points, find, k, ratios, interp):
    if len(points.shape) != 3 or points.shape[2] != 4:
        raise ValueError("point_knn: `points` must be [n, N, 4]")
    sizes = [int(points.shape[1])]
    for r in ratios:
        r = int(r)
        if r < 1 or sizes[-1] % r or sizes[-1] // r < 1:
            raise ValueError("point_knn: level %d of %d points does not divide by its ratio %d" % (len(sizes) - 1, sizes[-1], r))
        sizes.append(sizes[-1] // r)
    if len(sizes) < 2:
        raise ValueError("point_knn: a pyramid needs at least one ratio")
    kept = [find(points, None, k, n_queries=N, n_refs=N, outputs=("idx",)) for N in sizes[:-1]]
    ups = [find(points, points, 1, n_queries=N, n_refs=M, outputs=("idx",)) for N, M in zip(sizes[:-1], sizes[1:])] if interp else []
    pyr = PointPyramid(points, sizes, [nb.idx for nb in kept], [nb.idx for nb in ups] if interp else None)
    pyr._keepalive = (kept, ups)
    return pyr


def pyramid(points, k=16, ratios=(4, 4, 4, 4), interp=True):
    """The PointPyramid of clouds float32 [n, N, 4] on the device: 2 * len(ratios) launches of the one kernel on the current
    stream (len(ratios) without `interp`), every level read in place as a prefix of `points` -- no copy of the points, no host
    synchronisation.  Every N_l must divide by its ratio exactly (ValueError).

    A whole-scene cloud is fed in as any [B, N, 4] tensor with a validity w: for FFB6D, N (12 288 there) randomly chosen
    valid-depth pixels of every picture, back-projected -- x, y, z in the camera frame and w = 1, w = 0 for a pixel that must not
    count; the random choice is what makes the prefix a random sub-sample.  The pixel-to-point and point-to-pixel indices of
    FFB6D's fusion are the two plain searches between the down-sampled picture's points and the cloud:
        r2p = sl.point_knn.search(pixel_xyz, cloud, k)          # for every pixel the k nearest cloud points
        p2r = sl.point_knn.search(cloud, pixel_xyz, 1)          # for every cloud point the nearest pixel
    with n_queries / n_refs selecting the level's prefix of the cloud."""
    return _pyramid(points, search, int(k), ratios, interp)


def pyramid_host(points, k=16, ratios=(4, 4, 4, 4), interp=True):
    """`pyramid` on a host array through `search_host`: a PointPyramid of numpy arrays.  Needs no device."""
    return _pyramid(np.ascontiguousarray(points, np.float32), search_host, int(k), ratios, interp)
