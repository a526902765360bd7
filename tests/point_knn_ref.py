"""The rules of the point k-NN (include/slhip.h "Point neighbours") stated in NumPy, independently of the library's scan: all
distances of a set at once in float32 with the contract's parenthesisation, the candidates by boolean masks, the order by
np.lexsort((index, d)).  No list is built, nothing is inserted, nothing is tiled: it shares no code and no method with
csrc/slhip_knn_rules.h."""
import numpy as np

F = np.float32


def counts(p):
    """rule 1: bool [..., P] of points [..., P, 4]"""
    with np.errstate(invalid="ignore"):
        return (p[..., 3] != 0) & np.isfinite(p[..., :3]).all(-1)


def dist2(q, r):
    """rule 2: float32 [Q, R] of q [Q, 4] and r [R, 4]: (dx*dx + dy*dy) + dz*dz, every operation rounded to float32"""
    q, r = np.asarray(q, F), np.asarray(r, F)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (q[:, None, i] - r[None, :, i] for i in range(3))
        return ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F) + (dz * dz).astype(F)


def search(queries, refs=None, k=16, max_dist=np.inf, skip_same=False, n_queries=None, n_refs=None):
    """(idx int32 [n, Q, k], dist2 float32 [n, Q, k], count int32 [n, Q]) of queries [n, Pq, 4] and refs [n, Pr, 4] (None: the
    queries), the first n_queries and n_refs points of every row"""
    queries = np.asarray(queries, F)
    refs = queries if refs is None else np.asarray(refs, F)
    n = queries.shape[0]
    Q = queries.shape[1] if n_queries is None else n_queries
    R = refs.shape[1] if n_refs is None else n_refs
    idx, dd, count = np.full((n, Q, k), -1, np.int32), np.full((n, Q, k), np.nan, F), np.zeros((n, Q), np.int32)
    with np.errstate(over="ignore"):
        g2 = F(max_dist) * F(max_dist)
    index = np.arange(R)
    for i in range(n):
        q, r = queries[i, :Q], refs[i, :R]
        d = dist2(q, r)
        with np.errstate(invalid="ignore"):
            cand = counts(q)[:, None] & counts(r)[None, :] & np.isfinite(d) & (d <= g2)      # rule 3
        if skip_same:
            cand &= np.arange(Q)[:, None] != index[None, :]
        for j in range(Q):
            c = index[cand[j]]
            order = c[np.lexsort((c, d[j, c]))][:k]      # rule 4: by distance, among equals by index
            m = len(order)
            idx[i, j, :m], dd[i, j, :m], count[i, j] = order, d[j, order], m      # rule 5: the rest stays -1 / NaN
    return idx, dd, count


def pyramid(points, k, ratios):
    """(sizes, neighbours, interp) of the RandLA pyramid: level l is the first N_l points; neighbours[l] the self-search of the
    level, interp[l] the nearest of the next level's points for every point of level l"""
    sizes = [points.shape[1]]
    for r in ratios:
        assert sizes[-1] % r == 0
        sizes.append(sizes[-1] // r)
    nei = [search(points, None, k, n_queries=N, n_refs=N)[0] for N in sizes[:-1]]
    up = [search(points, None, 1, n_queries=N, n_refs=M)[0] for N, M in zip(sizes[:-1], sizes[1:])]
    return sizes, nei, up
