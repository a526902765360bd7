"""An independent float64 NumPy implementation of the pose from correspondences (include/slhip.h "Pose PnP"): the yardstick of
tests/test_host_pose_pnp.py and tests/test_gpu_pose_pnp.py.  It is not a restatement of the library's float32 operations: the
minimal solver is the classical cosine form of the three distance equations with numpy.roots on its quartic and an SVD alignment
of the two triangles, the refinement solves its normal equations with numpy.linalg.  Shared with the library are only the rules a
user can observe: which correspondences count, the Philox picks (tests/sensor_rng_ref.py has the generator; the pick is formed in
float32 as the rule says), the score, the ties, the Cayley update and the flags."""
import numpy as np

import sensor_rng_ref as RNG

F = np.float32
STREAM = 7
INSUFFICIENT, NO_MODEL, REFINE_STOPPED, REFINE_REJECTED = 1, 2, 4, 8


def valid_mask(uv, xyz):
    uv, xyz = np.asarray(uv, F), np.asarray(xyz, F)
    return np.isfinite(uv).all(-1) & np.isfinite(xyz[..., :3]).all(-1) & (xyz[..., 3] > 0)


def picks(seed, set_id, h, n_valid):
    """the four picks of hypothesis h (rule 2), None when two coincide"""
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    words = RNG.philox4x32_10(np.array([set_id & 0xFFFFFFFF, STREAM, h, 0x51DE5EED], np.uint32), key)
    idx = np.minimum(n_valid - 1, (RNG.uniform_of(words) * F(n_valid)).astype(np.uint32).astype(np.int64))
    return None if len(set(idx.tolist())) < 4 else idx


def project(pose, K4, xyz):
    """(pixels [n, 2], Z [n]) of object points under a 3 x 4 pose, float64"""
    fx, fy, cx, cy = (float(v) for v in K4)
    X = np.asarray(xyz, np.float64)[..., :3] @ pose[:, :3].T + pose[:, 3]
    with np.errstate(all="ignore"):
        return np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], -1), X[..., 2]


def errors2(pose, K4, uv, xyz):
    """squared pixel error per correspondence, +inf where the point is not in front"""
    px, Z = project(pose, K4, xyz)
    with np.errstate(all="ignore"):
        e = ((px - np.asarray(uv, np.float64)) ** 2).sum(-1)
    return np.where(Z > 0, e, np.inf)


def align(P, X):
    """the rigid motion that takes the three points P onto X (Kabsch by SVD): a 3 x 4 pose"""
    pc, xc = P.mean(0), X.mean(0)
    U, _, Vt = np.linalg.svd((X - xc).T @ (P - pc))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return np.concatenate([R, (xc - R @ pc)[:, None]], 1)


def p3p(uv, xyz, K4):
    """every pose that sees the three points xyz [3, 3] at the pixels uv [3, 2]: a list of 3 x 4 float64 poses"""
    fx, fy, cx, cy = (float(v) for v in K4)
    uv, P = np.asarray(uv, np.float64), np.asarray(xyz, np.float64)[:, :3]
    f = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(3)], -1)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    a2, b2, c2 = float(((P[1] - P[2]) ** 2).sum()), float(((P[0] - P[2]) ** 2).sum()), float(((P[0] - P[1]) ** 2).sum())
    ca, cb, cg = float(f[1] @ f[2]), float(f[0] @ f[2]), float(f[0] @ f[1])      # (plain floats: numpy scalars would broadcast a poly1d away)
    if not (a2 > 0 and b2 > 0 and c2 > 0):
        return []
    # x = s1 / s3, y = s2 / s3:  b2 (y^2 + 1 - 2 y ca) = a2 q,  b2 (x^2 + y^2 - 2 x y cg) = c2 q,  q = x^2 + 1 - 2 x cb
    q = np.poly1d([1.0, -2.0 * cb, 1.0])
    N = b2 * np.poly1d([-1.0, 0.0, 1.0]) - (a2 - c2) * q
    D = 2.0 * b2 * np.poly1d([-cg, ca])
    quartic = b2 * (N * N + D * D - 2.0 * ca * N * D) - a2 * q * D * D
    out = []
    cos, d2 = np.array([cg, cb, ca]), np.array([c2, b2, a2])      # the pairs (0, 1), (0, 2), (1, 2)
    pairs = ((0, 1), (0, 2), (1, 2))
    for r in np.roots(quartic.coeffs):
        if abs(r.imag) > 1e-4 * max(1.0, abs(r.real)) or r.real <= 0:      # (a near-double root leaves the eigenvalue solve complex)
            continue
        x = r.real
        if D(x) == 0 or q(x) <= 0:
            continue
        y = N(x) / D(x)
        s3 = np.sqrt(b2 / q(x))
        s = np.array([x * s3, y * s3, s3])
        for _ in range(8):      # Newton on si^2 + sj^2 - 2 si sj cos = d^2: numpy.roots is only an eigenvalue solve
            res = np.array([s[i] ** 2 + s[j] ** 2 - 2.0 * s[i] * s[j] * cos[k] - d2[k] for k, (i, j) in enumerate(pairs)])
            J = np.zeros((3, 3))
            for k, (i, j) in enumerate(pairs):
                J[k, i], J[k, j] = 2.0 * s[i] - 2.0 * s[j] * cos[k], 2.0 * s[j] - 2.0 * s[i] * cos[k]
            if not np.isfinite(J).all() or abs(np.linalg.det(J)) < 1e-300:
                break
            s = s - np.linalg.solve(J, res)
        if not (np.isfinite(s).all() and (s > 0).all()):
            continue
        X = s[:, None] * f
        side = np.array([((X[0] - X[1]) ** 2).sum() - c2, ((X[0] - X[2]) ** 2).sum() - b2, ((X[1] - X[2]) ** 2).sum() - a2])
        if (np.abs(side) > 1e-9 * np.array([c2, b2, a2])).any():
            continue
        m = align(P, X)
        if any(np.abs(m - o).max() < 1e-9 for o in out):      # two starts that met in one solution
            continue
        out.append(m)
    return out


def hypothesis(uv, xyz, K4, idx):
    """rule 3: the solution of the first three picks that sees the fourth best, None when there is none"""
    best, pose = None, None
    for m in p3p(uv[idx[:3]], xyz[idx[:3]], K4):
        e = errors2(m, K4, uv[idx[3]], xyz[idx[3]])
        e = float(e) if np.isfinite(e) else np.inf
        if best is None or e < best:
            best, pose = e, m
    return pose


def cayley(c):
    cx_ = np.array([[0, -c[2], c[1]], [c[2], 0, -c[0]], [-c[1], c[0], 0]], np.float64)
    cc = c @ c
    return ((1.0 - cc) * np.eye(3) + 2.0 * np.outer(c, c) + 2.0 * cx_) / (1.0 + cc)


def gauss_newton_step(pose, K4, uv, xyz):
    """one step on the correspondences given (the inliers), increment on the left; None when the normal matrix is not
    positive definite"""
    fx, fy = float(K4[0]), float(K4[1])
    X = xyz[:, :3] @ pose[:, :3].T + pose[:, 3]
    px, _ = project(pose, K4, xyz)
    r = (px - uv).reshape(-1)
    J = np.zeros((len(X), 2, 6))
    for i, (x, y, z) in enumerate(X):
        du = np.array([fx / z, 0.0, -fx * x / z ** 2])
        dv = np.array([0.0, fy / z, -fy * y / z ** 2])
        dX = np.concatenate([-np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]], np.float64), np.eye(3)], 1)      # d(w x X + t)
        J[i, 0], J[i, 1] = du @ dX, dv @ dX
    J = J.reshape(-1, 6)
    A = J.T @ J
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    d = np.linalg.solve(A, -J.T @ r)
    R = cayley(d[:3] / 2.0)
    return np.concatenate([R @ pose[:, :3], (R @ pose[:, 3] + d[3:])[:, None]], 1)


class Result:
    pass


def solve(uv, xyz, K4, n_hypotheses=256, threshold_px=2.0, refine_iters=4, min_inliers=4, seed=0, set_id=0, init=None):
    """one set: uv [K, 2], xyz [K, 4].  A Result with pose (3 x 4 float64 or NaN), n_inliers, rms, inliers (bool [K]), best,
    flags, and err2 (float64 [K], the squared pixel error of every correspondence under the pose returned; inf: not valid)"""
    uv32, xyz32 = np.asarray(uv, F), np.asarray(xyz, F)
    uv, xyz = uv32.astype(np.float64), xyz32.astype(np.float64)
    ok = valid_mask(uv32, xyz32)
    res = Result()
    res.pose, res.n_inliers, res.rms, res.best, res.flags = np.full((3, 4), np.nan), 0, np.nan, -2, 0
    res.inliers, res.err2 = np.zeros(len(uv), bool), np.full(len(uv), np.inf)
    vu, vx = uv[ok], xyz[ok]
    if len(vu) < 4:
        res.flags = INSUFFICIENT
        return res
    thr2 = float(F(threshold_px)) ** 2
    best_count, best_h, best_pose = -1, None, None
    if init is not None:
        m = np.asarray(init, np.float64)
        best_count, best_h, best_pose = (int((errors2(m, K4, vu, vx) <= thr2).sum()) if np.isfinite(m).all() else 0), -1, m
    for h in range(n_hypotheses):
        idx = picks(seed, set_id, h, len(vu))
        m = None if idx is None else hypothesis(vu, vx, K4, idx)
        count = 0 if m is None else int((errors2(m, K4, vu, vx) <= thr2).sum())
        if count > best_count:
            best_count, best_h, best_pose = count, h, m
    if best_h is None or best_count < min_inliers or best_pose is None:
        res.flags = NO_MODEL
        return res
    pose = best_pose
    for _ in range(refine_iters):
        inl = errors2(pose, K4, vu, vx) <= thr2
        new = gauss_newton_step(pose, K4, vu[inl], vx[inl])
        if new is None:
            res.flags |= REFINE_STOPPED
            break
        pose = new
    e = np.where(ok, errors2(pose, K4, uv, xyz), np.inf)
    if int((e <= thr2).sum()) < best_count:
        res.flags |= REFINE_REJECTED
        pose = best_pose
        e = np.where(ok, errors2(pose, K4, uv, xyz), np.inf)
    res.pose, res.err2, res.inliers, res.best = pose, e, e <= thr2, best_h
    res.n_inliers = int(res.inliers.sum())
    res.rms = float(np.sqrt(e[res.inliers].sum() / res.n_inliers))
    return res


# ---- distances between two poses ------------------------------------------------------------------------------------------------
def rotation_angle(a, b):
    """the angle (radians) of the rotation that takes pose a's rotation to pose b's"""
    R = np.asarray(a, np.float64)[:, :3].T @ np.asarray(b, np.float64)[:, :3]
    skew = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(skew) / 2.0, (np.trace(R) - 1.0) / 2.0))


def translation_distance(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64)[:, 3] - np.asarray(b, np.float64)[:, 3]))
