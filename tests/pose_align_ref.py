"""An independent float64 NumPy implementation of the robust alignment (include/slhip.h "Robust alignment"): the yardstick of
tests/test_host_pose_align.py and tests/test_gpu_pose_align.py.  It is not a restatement of the library's float32 operations:
every fit, the minimal one included, is Kabsch by numpy.linalg.svd with the determinant correction, the score is
numpy.linalg.norm against the threshold, and a degenerate sample is told by the singular values of its moments.  Shared with the
library are only the rules a user can observe: which correspondences count, the Philox picks of stream 9
(tests/sensor_rng_ref.py has the generator; the pick is formed in float32 as the rule says), the score, the ties and the flags."""
import numpy as np

import sensor_rng_ref as RNG

F = np.float32
STREAM = 9
INSUFFICIENT, NO_MODEL, REFINE_STOPPED, REFINE_REJECTED = 1, 2, 4, 8


def valid_mask(src, dst):
    src, dst = np.asarray(src, F), np.asarray(dst, F)
    return (src[..., 3] > 0) & (dst[..., 3] != 0) & np.isfinite(src[..., :3]).all(-1) & np.isfinite(dst[..., :3]).all(-1)


def picks(seed, set_id, h, n_valid):
    """the three picks of hypothesis h (rule 2), None when two coincide"""
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    words = RNG.philox4x32_10(np.array([set_id & 0xFFFFFFFF, STREAM, h, 0x51DE5EED], np.uint32), key)[:3]
    idx = np.minimum(n_valid - 1, (RNG.uniform_of(words) * F(n_valid)).astype(np.uint32).astype(np.int64))
    return None if len(set(idx.tolist())) < 3 else idx


def kabsch(a, b, min_gap=1e-6):
    """the rigid motion that takes the points a [n, 3] onto b [n, 3] in the least-squares sense: a 3 x 4 float64 pose, None
    when the points are collinear or coincident.  With the singular values s0 >= s1 >= s2 of the moments and d the sign of the
    determinant, the two largest eigenvalues of Horn's matrix differ by 2 (s1 + d s2) and the four absolute ones sum to at
    most 4 s0: that is the library's min_gap test, said with what an SVD gives"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ca, cb = a.mean(0), b.mean(0)
    H = (a - ca).T @ (b - cb)
    if not np.isfinite(H).all():
        return None
    U, s, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    lam = np.array([s[0] + s[1] + d * s[2], s[0] - s[1] - d * s[2], -s[0] + s[1] - d * s[2], -s[0] - s[1] + d * s[2]])
    if not 2.0 * (s[1] + d * s[2]) > float(F(min_gap)) * np.abs(lam).sum():
        return None
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return np.concatenate([R, (cb - R @ ca)[:, None]], 1)


def residuals(pose, src, dst):
    """|R s + t - d| per correspondence, float64; NaN under a NaN pose"""
    with np.errstate(all="ignore"):
        return np.linalg.norm(np.asarray(src, np.float64)[..., :3] @ pose[:, :3].T + pose[:, 3] - np.asarray(dst, np.float64)[..., :3], axis=-1)


class Result:
    pass


def solve(src, dst, threshold, n_hypotheses=256, refine_iters=4, min_gap=1e-6, min_inliers=3, seed=0, set_id=0, init=None):
    """one set: src, dst [K, 4].  A Result with pose (3 x 4 float64 or NaN), n_inliers, rms, inliers (bool [K]), best, flags"""
    src32, dst32 = np.asarray(src, F), np.asarray(dst, F)
    ok = valid_mask(src32, dst32)
    res = Result()
    res.pose, res.n_inliers, res.rms, res.best, res.flags = np.full((3, 4), np.nan), 0, np.nan, -2, 0
    res.inliers = np.zeros(len(src32), bool)
    a, b = src32[ok, :3].astype(np.float64), dst32[ok, :3].astype(np.float64)
    if len(a) < 3:
        res.flags = INSUFFICIENT
        return res
    thr = float(F(threshold))

    def count(m):
        with np.errstate(invalid="ignore"):
            return int((residuals(m, a, b) <= thr).sum())

    best_count, best_h, best_pose = -1, None, None
    if init is not None:
        m = np.asarray(init, np.float64)
        best_count, best_h, best_pose = (count(m) if np.isfinite(m).all() else 0), -1, (m if np.isfinite(m).all() else None)
    for h in range(n_hypotheses):
        idx = picks(seed, set_id, h, len(a))
        m = None if idx is None else kabsch(a[idx], b[idx], min_gap)
        c = 0 if m is None else count(m)
        if c > best_count:
            best_count, best_h, best_pose = c, h, m
    if best_h is None or best_count < min_inliers or best_pose is None:
        res.flags = NO_MODEL
        return res
    pose = best_pose
    for _ in range(refine_iters):
        inl = residuals(pose, a, b) <= thr
        new = kabsch(a[inl], b[inl], min_gap) if inl.sum() >= 3 else None
        if new is None:
            res.flags |= REFINE_STOPPED
            break
        pose = new
    with np.errstate(invalid="ignore"):
        e = np.where(ok, residuals(pose, src32, dst32), np.inf)
        if int((e <= thr).sum()) < best_count:
            res.flags |= REFINE_REJECTED
            pose = best_pose
            e = np.where(ok, residuals(pose, src32, dst32), np.inf)
        res.inliers = e <= thr
    res.pose, res.best, res.n_inliers = pose, best_h, int(res.inliers.sum())
    res.rms = float(np.sqrt((e[res.inliers] ** 2).sum() / res.n_inliers))
    return res


# ---- distances between two poses ------------------------------------------------------------------------------------------------
def rotation_angle(a, b):
    """the angle in radians between the rotations of two poses, well conditioned near 0: from the norm of the difference"""
    d = np.linalg.norm(np.asarray(a, np.float64)[:, :3] - np.asarray(b, np.float64)[:, :3])
    return float(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0)))))


def translation_distance(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64)[:, 3] - np.asarray(b, np.float64)[:, 3]))


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
