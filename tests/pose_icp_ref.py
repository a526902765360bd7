"""ICP in NumPy: two statements for tests/test_host_pose_icp.py and tests/test_gpu_pose_icp.py.
`icp_rules` restates the rules of include/slhip.h "ICP" in float32, operation by operation and sum by sum in the library's order
(lane j % 256 upwards, the wave's butterfly, ((w0 + w1) + w2) + w3), with pose_fit_ref's Horn matrix and Jacobi sweeps: the host
twin must give its outputs bit for bit.  `icp_svd` is the same loop in float64 with Kabsch by SVD as the fit (pose_fit_ref.fit_svd)
and a brute-force nearest neighbour: the independent reference, which shares nothing with the library but the problem."""
import numpy as np

import pose_fit_ref as RF

F = np.float32
BLOCK, WAVE = 256, 64
BAD_CLASS, NO_INIT, INSUFFICIENT, DEGENERATE, CONVERGED = 1, 2, 4, 8, 16
FAILED = 15
DEFAULTS = dict(max_iters=20, max_dist=np.inf, dist_scale=1.0, min_dist=0.0, min_pairs=6, min_gap=1e-6, tol_rot=1e-6, tol_trans=1e-6)


class Result:
    def __init__(self, K):
        self.pose, self.n_pairs, self.rms, self.iters, self.flags = np.full((3, 4), np.nan), 0, np.nan, 0, 0
        self.nearest = np.full(K, -1, np.int32)


def class_points(points, count, cls):
    """the [n, 3] points of class cls, or None when the set cannot start for its class"""
    A, N = points.shape[:2]
    if not 0 <= cls < A or not 1 <= count[cls] <= N:
        return None
    return points[cls, :count[cls], :3]


def counts(camera):
    return (camera[:, 3] != 0) & np.isfinite(camera[:, :3]).all(1)


def block_sum(terms):
    """lane l of 256 adds its terms l, l + 256, ... upwards from 0; the wave's butterfly; ((w0 + w1) + w2) + w3.  A term that
    does not count comes in as +0.0, which adds exactly."""
    n = len(terms)
    rows = -(-n // BLOCK)
    padded = np.zeros(rows * BLOCK, F)
    padded[:n] = terms
    acc = np.zeros(BLOCK, F)
    for k in range(rows):
        acc = (acc + padded[k * BLOCK:(k + 1) * BLOCK]).astype(F)
    v = acc.reshape(BLOCK // WAVE, WAVE)
    lanes = np.arange(WAVE)
    off = WAVE // 2
    while off:
        v = (v + v[:, lanes ^ off]).astype(F)
        off //= 2
    w = v[:, 0]
    return F(F(F(w[0] + w[1]) + w[2]) + w[3])


def to_object(pose, xyz):
    """rule 3: q = R^T (c - t), in the dtype of pose"""
    d0, d1, d2 = xyz[:, 0] - pose[0, 3], xyz[:, 1] - pose[1, 3], xyz[:, 2] - pose[2, 3]
    return np.stack([(pose[0, k] * d0 + pose[1, k] * d1) + pose[2, k] * d2 for k in range(3)], 1)


def nearest(q, p):
    """rule 4: (best squared distance [K], index [K] or -1): the smallest dist2, among equals the lowest index; a NaN and a
    +inf never win"""
    K = len(q)
    best, at = np.full(K, np.inf, q.dtype), np.full(K, -1, np.int64)
    for a in range(0, K, 256):
        dx, dy, dz = (q[a:a + 256, None, i] - p[None, :, i] for i in range(3))
        d = (dx * dx + dy * dy) + dz * dz
        d = np.where(np.isnan(d), np.inf, d)
        idx = d.argmin(1)      # the first of the smallest
        val = d[np.arange(len(idx)), idx]
        best[a:a + 256] = val
        at[a:a + 256] = np.where(val < np.inf, idx, -1)
    return best, at


def pose_of32(e, V, c, min_gap):
    """rules 4 to 6 of "Rigid fit" in float32 scalars: the pose [3, 4], or None when degenerate"""
    best, largest = 0, e[0]
    for i in range(1, 4):
        if e[i] > largest:
            largest, best = e[i], i
    second = F(-np.inf)
    for i in range(4):
        if i != best and e[i] > second:
            second = e[i]
    scale = F(F(F(abs(e[0]) + abs(e[1])) + abs(e[2])) + abs(e[3]))
    if not F(largest - second) > F(F(min_gap) * scale):
        return None
    q = V[:, best]
    n = np.sqrt(F(F(F(q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
    sgn = F(-1) if q[0] < 0 else F(1)
    w, x, y, z = (F(F(q[k] / n) * sgn) for k in range(4))
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    one, two = F(1), F(2)
    R = np.array([[one - two * (yy + zz), two * (xy - wz), two * (xz + wy)],
                  [two * (xy + wz), one - two * (xx + zz), two * (yz - wx)],
                  [two * (xz - wy), two * (yz + wx), one - two * (xx + yy)]], F)
    t = np.array([c[3 + i] - F(F(R[i, 0] * c[0] + R[i, 1] * c[1]) + R[i, 2] * c[2]) for i in range(3)], F)
    return np.concatenate([R, t[:, None]], 1).astype(F)


def fit32(s, d, pair, min_gap):
    """rule 6: Horn's fit of the pairs in float32, every sum in the library's order: (pose or None, n_pairs)"""
    n = F(int(pair.sum()))
    z = F(0)
    c = np.array([block_sum(np.where(pair, s[:, i], z)) / n for i in range(3)] +
                 [block_sum(np.where(pair, d[:, i], z)) / n for i in range(3)], F)
    a, b = (s - c[:3]).astype(F), (d - c[3:]).astype(F)
    M = np.array([[block_sum(np.where(pair, a[:, i] * b[:, j], z)) for j in range(3)] for i in range(3)], F)
    e, V, _ = RF.jacobi(RF.horn(M))
    return pose_of32(e, V, c, min_gap), c


def residual2(pose, s, d):
    """rule 7 of "Rigid fit": |R s + t - d|^2, rows ((R0 x + R1 y) + R2 z) + t"""
    r = [(((pose[i, 0] * s[:, 0] + pose[i, 1] * s[:, 1]) + pose[i, 2] * s[:, 2]) + pose[i, 3]) - d[:, i] for i in range(3)]
    return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]


def moved(before, after, tol_rot, tol_trans):
    """rule 8: True when an entry moved by more than its tolerance (or is NaN)"""
    tol = np.array([tol_rot, tol_rot, tol_rot, tol_trans], before.dtype)
    return not bool((np.abs(after - before) <= tol[None, :]).all())


def _loop(camera, init, cls, points, count, dtype, fit, kw):
    """the loop both statements share: rules 1, 2, 5, 8 and the bookkeeping; `fit(s, d, pair)` -> pose or None"""
    p = dict(DEFAULTS)
    p.update(kw)
    K = len(camera)
    res = Result(K)
    bank = class_points(points, count, cls)
    if bank is None:
        res.flags = BAD_CLASS
        return res
    if not np.isfinite(np.asarray(init, F)).all():
        res.flags = NO_INIT
        return res
    ok = counts(camera)
    bank = bank.astype(dtype)
    d = np.where(ok[:, None], camera[:, :3], 0).astype(dtype)      # (what does not count is never read by a sum)
    pose = np.asarray(init, dtype).reshape(3, 4).copy()
    as_t = dtype if dtype is F else np.float64
    gate = as_t(F(p["max_dist"]))
    with np.errstate(all="ignore"):
        for it in range(int(p["max_iters"])):
            best, at = nearest(to_object(pose, d), bank)
            pair = ok & (at >= 0) & (best <= as_t(gate * gate))
            res.nearest = np.where(pair, at, -1).astype(np.int32)
            res.n_pairs = int(pair.sum())
            if res.n_pairs < int(p["min_pairs"]):
                res.flags, res.pose, res.rms = INSUFFICIENT, np.full((3, 4), np.nan), np.nan
                return res
            s = bank[np.where(pair, at, 0)]
            new = fit(s, d, pair)
            if new is None:
                res.flags, res.pose, res.rms = DEGENERATE, np.full((3, 4), np.nan), np.nan
                return res
            still = not moved(pose, new, as_t(F(p["tol_rot"])), as_t(F(p["tol_trans"])))
            pose, res.iters = new, it + 1
            g = as_t(gate * as_t(F(p["dist_scale"])))
            gate = g if g > as_t(F(p["min_dist"])) else as_t(F(p["min_dist"]))
            if still or res.iters == int(p["max_iters"]):
                res.flags = CONVERGED if still else 0
                r2 = residual2(pose, s, d)
                if dtype is F:
                    res.rms = np.sqrt(F(block_sum(np.where(pair, r2, F(0))) / F(res.n_pairs)))
                else:
                    res.rms = float(np.sqrt(r2[pair].mean()))
                break
    res.pose = pose
    return res


def icp_rules(camera, init, cls, points, count, **kw):
    """the rules in float32, bit for bit what slhip_pose_icp_host gives: a Result"""
    min_gap = F(kw.get("min_gap", DEFAULTS["min_gap"]))
    camera, points = np.asarray(camera, F), np.asarray(points, F)
    return _loop(camera, init, int(cls), points, np.asarray(count), F, lambda s, d, pair: fit32(s, d, pair, min_gap)[0], kw)


def icp_svd(camera, init, cls, points, count, **kw):
    """the same loop in float64 with the SVD fit: a Result with a float64 pose"""
    def fit(s, d, pair):
        w = pair.astype(np.float64)[:, None]
        pose, n, _ = RF.fit_svd(np.concatenate([s, w], 1), np.concatenate([d, w], 1))
        return pose

    camera, points = np.asarray(camera, F), np.asarray(points, F)
    return _loop(camera, init, int(cls), points, np.asarray(count), np.float64, fit, kw)


def solve_rules(camera, init, classes, points, count, **kw):
    return [icp_rules(camera[i], init[i], classes[i], points, count, **kw) for i in range(len(camera))]


def solve_svd(camera, init, classes, points, count, **kw):
    return [icp_svd(camera[i], init[i], classes[i], points, count, **kw) for i in range(len(camera))]


def perturbed(Rm, t, degrees, seed):
    """the pose (Rm, t) turned by `degrees` about a random axis through the object's origin and shifted by 2 % of a 0.1 m object
    per degree: float64 [3, 4]"""
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = np.radians(degrees)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    dR = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)
    shift = rng.normal(size=3)
    shift *= 0.002 * degrees / np.linalg.norm(shift)
    return np.concatenate([np.asarray(Rm) @ dR, (np.asarray(t) + shift)[:, None]], 1)
