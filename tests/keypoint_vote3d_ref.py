"""Keypoint voting in 3D in NumPy float64: an independent statement of the rules of include/slhip.h "Keypoint voting in 3D" for
tests/test_host_keypoint_vote3d.py and tests/test_gpu_keypoint_vote3d.py.  Same rules, other arithmetic: float64 throughout and
NumPy's own summation order, so what it shares with the library is the rule and not the rounding."""
import numpy as np

INSUFFICIENT, NO_MODEL, NOT_CONVERGED = 1, 2, 4


class Result:
    """xyz, mean float64 [3] (NaN: none); cov float64 [6] xx xy xz yy yz zz; n_support, best (-2: none), iters, flags;
    support bool [K]; near_tie: two seeds of equal top support whose modes lie more than tol apart, or a candidate within
    1e-4 h of the band's edge round the winner -- a discrete decision that rounding may take the other way"""

    def __init__(self, K):
        self.xyz, self.mean, self.cov = np.full(3, np.nan), np.full(3, np.nan), np.full(6, np.nan)
        self.n_support, self.best, self.iters, self.flags = 0, -2, 0, 0
        self.support = np.zeros(K, bool)
        self.near_tie = False


def candidates(camera, offsets):
    """(c float64 [n_valid, 3], index int [n_valid]) of camera float32 [K, 4] and offsets float32 [K, 3]: the float32 sums, as
    the rule forms them, of the voters that count"""
    c = (np.asarray(camera, np.float32)[:, :3] + np.asarray(offsets, np.float32)).astype(np.float32)
    ok = (np.asarray(camera)[:, 3] != 0) & np.isfinite(c).all(1)
    return c[ok].astype(np.float64), np.nonzero(ok)[0]


def solve(camera, offsets, n_seeds=128, bandwidth=0.05, max_iters=32, tol=1e-4, min_support=1):
    """one (set, keypoint): camera [K, 4], offsets [K, 3]"""
    K = len(camera)
    res = Result(K)
    c, index = candidates(camera, offsets)
    n = len(c)
    if n == 0:
        res.flags = INSUFFICIENT
        return res
    h = float(np.float32(bandwidth))
    tol = float(np.float32(tol))
    S = min(int(n_seeds), n)
    modes, supports, iters, stopped = [], [], [], []
    for s in range(S):
        x = c[((2 * s + 1) * n) // (2 * S)].copy()
        it, done = 0, False
        while it < max_iters and not done:
            d = c - x
            t = (d * d).sum(1) / (h * h)
            w = np.where(t < 1.0, 1.0 - t, 0.0)
            m = (w[:, None] * d).sum(0) / w.sum()
            x = x + m
            done = bool((m * m).sum() <= tol * tol)
            it += 1
        modes.append(x)
        supports.append(int((((c - x) ** 2).sum(1) <= h * h).sum()))
        iters.append(it)
        stopped.append(done)
    supports = np.array(supports)
    best = int(np.argmax(supports))      # the first of the largest
    if supports[best] < min_support:
        res.flags = NO_MODEL
        return res
    x = modes[best]
    d2 = ((c - x) ** 2).sum(1)
    sup = d2 <= h * h
    res.xyz, res.n_support, res.best, res.iters = x, int(supports[best]), best, iters[best]
    res.flags = 0 if stopped[best] else NOT_CONVERGED
    res.support[index[sup]] = True
    res.mean = c[sup].mean(0)
    g = c[sup] - res.mean
    res.cov = np.array([(g[:, a] * g[:, b]).mean() for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
    rivals = [s for s in range(S) if s != best and supports[s] == supports[best] and np.linalg.norm(modes[s] - x) > tol]
    res.near_tie = bool(rivals) or bool((np.abs(np.sqrt(d2) - h) <= 1e-4 * h).any())
    return res


def solve_sets(camera, offsets, **kw):
    """camera [M, K, 4], offsets [M, K, Kp, 3]: a list of lists of Results"""
    return [[solve(camera[m], offsets[m, :, k], **kw) for k in range(offsets.shape[2])] for m in range(len(camera))]
