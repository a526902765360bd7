"""An independent float64 NumPy implementation of the keypoint voting (include/slhip.h "Keypoint voting"): the yardstick of
tests/test_host_keypoint_vote.py and tests/test_gpu_keypoint_vote.py.  It is not a restatement of the library's float32
operations: two voters' lines are intersected by numpy.linalg.solve on the 2 x 2 system p_a + s d_a = p_b + t d_b, a voter agrees
when the angle arccos(cos) between its vector and its view of the position is at most arccos(inlier_cos), the distribution is
numpy's weighted mean and outer products, and the refinement is numpy.linalg.lstsq on the inliers' line equations.  Shared with
the library are only the rules a user can observe: which voters count, the Philox picks (tests/sensor_rng_ref.py has the
generator; the pick is formed in float32 as the rule says), the score, the ties and the flags."""
import numpy as np

import sensor_rng_ref as RNG

F = np.float32
STREAM = 8
INSUFFICIENT, NO_MODEL, REFINE_STOPPED, REFINE_REJECTED = 1, 2, 4, 8


def valid_mask(pixel, vec, size):
    """rule 1 for voters pixel [K, 2] (x, y), vec float32 [K, 2]; the length is formed in float32, as the rule says"""
    pixel, v = np.asarray(pixel, np.int64), np.asarray(vec, F)
    inside = (pixel[:, 0] >= 0) & (pixel[:, 1] >= 0) & (pixel[:, 0] < size[0]) & (pixel[:, 1] < size[1])
    with np.errstate(all="ignore"):
        length = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])
        return inside & np.isfinite(v).all(-1) & (length > 0)


def picks(seed, set_id, k, n_hypotheses, n_valid):
    """the two picks of every hypothesis of keypoint k (rule 2): int64 [Hy, 2]"""
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    ctr = np.zeros((n_hypotheses, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = set_id & 0xFFFFFFFF, STREAM, np.arange(n_hypotheses), k
    words = RNG.philox4x32_10(ctr, key)[:, :2]
    return np.minimum(n_valid - 1, (RNG.uniform_of(words) * F(n_valid)).astype(np.uint32).astype(np.int64))


def cosines(q, p, d):
    """the cosine of the angle between d and q - p per voter (1 where q is the voter's own centre); q [.., 1, 2] or [2]"""
    e = np.asarray(q, np.float64) - p
    n = np.linalg.norm(e, axis=-1)
    with np.errstate(all="ignore"):
        return np.where(n == 0, 1.0, (e * d).sum(-1) / n)


def agree(cos, inlier_cos):
    """angles by arccos against the bound's"""
    with np.errstate(all="ignore"):
        return np.arccos(np.clip(cos, -1.0, 1.0)) <= np.arccos(float(F(inlier_cos)))


class Result:
    pass


def solve(pixel, vec, size, k=0, n_hypotheses=128, inlier_cos=0.99, min_inliers=2, min_sin=1e-3, seed=0, set_id=0):
    """one (set, keypoint): pixel [K, 2], vec float32 [K, 2].  A Result with uv, mean (float64 [2] or NaN), cov (float64 [3]:
    xx, xy, yy), n_inliers, best, flags, inliers (bool [K]) and cos (float64 [K], the cosine of every voter under the position
    returned; NaN: not valid)"""
    pixel, v32 = np.asarray(pixel, np.int64), np.asarray(vec, F)
    K = len(pixel)
    ok = valid_mask(pixel, v32, size)
    res = Result()
    res.uv, res.mean, res.cov = np.full(2, np.nan), np.full(2, np.nan), np.full(3, np.nan)
    res.n_inliers, res.best, res.flags = 0, -2, 0
    res.inliers, res.cos = np.zeros(K, bool), np.full(K, np.nan)
    n = int(ok.sum())
    if n < 2:
        res.flags = INSUFFICIENT
        return res
    p = pixel[ok].astype(np.float64) + 0.5
    v = v32[ok].astype(np.float64)
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    ab = picks(seed, set_id, k, n_hypotheses, n)
    a, b = ab[:, 0], ab[:, 1]
    det = d[a, 0] * d[b, 1] - d[a, 1] * d[b, 0]
    have = (a != b) & ~(p[a] == p[b]).all(-1) & (np.abs(det) > float(F(min_sin)))
    Q = np.full((n_hypotheses, 2), np.nan)
    if have.any():
        A = np.stack([d[a[have]], -d[b[have]]], -1)                      # columns d_a, -d_b: A (s, t) = p_b - p_a
        st = np.linalg.solve(A, (p[b[have]] - p[a[have]])[..., None])[..., 0]
        Q[have] = p[a[have]] + st[:, :1] * d[a[have]]
    have &= np.isfinite(Q).all(-1)
    counts = np.zeros(n_hypotheses, np.int64)
    for h in np.nonzero(have)[0]:
        counts[h] = int(agree(cosines(Q[h], p, d), inlier_cos).sum())
    best = int(np.argmax(counts))                                        # the first of the highest: ties to the lowest h
    if not have.any() or counts[best] < min_inliers:
        res.flags = NO_MODEL
        return res
    w = counts[have] / n
    res.mean = (w[:, None] * Q[have]).sum(0) / w.sum()
    g = Q[have] - res.mean
    C = (w[:, None, None] * g[:, :, None] * g[:, None, :]).sum(0) / w.sum()
    res.cov = np.array([C[0, 0], C[0, 1], C[1, 1]])
    q = Q[best]
    inl = agree(cosines(q, p, d), inlier_cos)
    N = np.stack([-d[inl, 1], d[inl, 0]], -1)                            # the normal of every inlier's line
    delta, _, rank, _ = np.linalg.lstsq(N, (N * (p[inl] - q)).sum(-1), rcond=None)      # N (x - q) = N . (p - q)
    uv = q + delta
    if rank < 2:
        res.flags |= REFINE_STOPPED
        uv = q
    cos = cosines(uv, p, d)
    if int(agree(cos, inlier_cos).sum()) < counts[best]:
        res.flags |= REFINE_REJECTED
        uv = q
        cos = cosines(uv, p, d)
    res.uv, res.best = uv, best
    res.cos[ok] = cos
    res.inliers[ok] = agree(cos, inlier_cos)
    res.n_inliers = int(res.inliers.sum())
    return res


def solve_sets(pixel, vectors, size, seed=0, set_id_base=0, **kw):
    """every (set, keypoint) of pixel [M, K, 2], vectors float32 [M, K, Kp, 2]: a list of M lists of Kp Results"""
    return [[solve(pixel[m], vectors[m, :, k], size, k=k, seed=seed, set_id=set_id_base + m, **kw) for k in range(vectors.shape[2])]
            for m in range(len(pixel))]


def gather(field, scene, pixel):
    """the vectors of voters pixel [M, K, 2] in a dense field [B, H, W, Kp, 2]: [M, K, Kp, 2], zeros where nothing is read"""
    B, H, W = field.shape[:3]
    pixel = np.asarray(pixel, np.int64)
    x, y = pixel[..., 0], pixel[..., 1]
    s = np.broadcast_to(np.asarray(scene, np.int64)[:, None], x.shape)
    ok = (x >= 0) & (y >= 0) & (x < W) & (y < H) & (s >= 0) & (s < B)
    out = field[np.where(ok, s, 0), np.where(ok, y, 0), np.where(ok, x, 0)].copy()
    out[~ok] = 0
    return out
