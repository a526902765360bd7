"""The rigid fit in NumPy: two independent statements for tests/test_host_pose_fit.py and tests/test_gpu_pose_fit.py.
`fit_svd` is the textbook answer -- Kabsch by a float64 SVD with the determinant correction -- and shares nothing with the
library but the problem.  `fit_rules` restates the rules of include/slhip.h "Rigid fit" (Horn's 4 x 4, cyclic Jacobi with a fixed
number of sweeps) in a chosen precision: in float64 it is the reference of the route, in float32 it shows what the sweeps leave
off the diagonal."""
import numpy as np

INSUFFICIENT, DEGENERATE = 1, 2
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def used(src, dst):
    src, dst = np.asarray(src), np.asarray(dst)
    return (src[:, 3] > 0) & (dst[:, 3] != 0) & np.isfinite(src[:, :3]).all(1) & np.isfinite(dst[:, :3]).all(1)


def fit_svd(src, dst):
    """(pose float64 [3, 4], n_used, rms) of src, dst [N, 4]; None as the pose with fewer than 3 correspondences"""
    ok = used(src, dst)
    n = int(ok.sum())
    if n < 3:
        return None, n, np.nan
    a, b = np.asarray(src, np.float64)[ok, :3], np.asarray(dst, np.float64)[ok, :3]
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((a - ca).T @ (b - cb))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    t = cb - R @ ca
    rms = float(np.sqrt((((a @ R.T + t) - b) ** 2).sum(1).mean()))
    return np.concatenate([R, t[:, None]], 1), n, rms


def naive_svd_rotation(src, dst):
    """Kabsch WITHOUT the determinant correction: what a plain batched SVD route returns"""
    a, b = np.asarray(src, np.float64)[:, :3], np.asarray(dst, np.float64)[:, :3]
    U, _, Vt = np.linalg.svd((a - a.mean(0)).T @ (b - b.mean(0)))
    return Vt.T @ U.T


def jacobi(A, sweeps=SWEEPS):
    """(eigenvalues [4], eigenvector columns [4, 4], the matrix as the sweeps left it) in A's dtype"""
    A = A.copy()
    dt = A.dtype.type
    V = np.eye(4, dtype=A.dtype)
    for _ in range(sweeps):
        for p, q in PAIRS:
            apq = A[p, q]
            if apq == 0:
                continue
            with np.errstate(over="ignore", divide="ignore"):
                theta = (A[q, q] - A[p, p]) / (dt(2) * apq)
                t = (dt(-1) if theta < 0 else dt(1)) / (abs(theta) + np.sqrt(theta * theta + dt(1)))
            c = dt(1) / np.sqrt(t * t + dt(1))
            s = t * c
            A[p, p], A[q, q] = A[p, p] - t * apq, A[q, q] + t * apq
            A[p, q] = A[q, p] = 0
            for k in range(4):
                if k != p and k != q:
                    akp, akq = A[k, p], A[k, q]
                    A[k, p] = A[p, k] = c * akp - s * akq
                    A[k, q] = A[q, k] = s * akp + c * akq
                vkp, vkq = V[k, p], V[k, q]
                V[k, p], V[k, q] = c * vkp - s * vkq, s * vkp + c * vkq
    return np.diag(A).copy(), V, A


def horn(M):
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, Syy - Sxx - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, Szz - Sxx - Syy]], M.dtype)


class Fit:
    def __init__(self):
        self.pose, self.n_used, self.rms, self.flags = None, 0, np.nan, 0
        self.off_diagonal, self.trace = 0.0, 0.0      # what the sweeps left: sum |a_pq|, p < q; sum |a_pp|


def fit_rules(src, dst, min_gap=1e-6, dtype=np.float64, sweeps=SWEEPS):
    """the 4 x 4 route in `dtype`: a Fit"""
    res = Fit()
    ok = used(src, dst)
    res.n_used = n = int(ok.sum())
    if n < 3:
        res.flags = INSUFFICIENT
        return res
    a, b = np.asarray(src, dtype)[ok, :3], np.asarray(dst, dtype)[ok, :3]
    ca, cb = a.sum(0, dtype=dtype) / dtype(n), b.sum(0, dtype=dtype) / dtype(n)
    M = ((a - ca).T @ (b - cb)).astype(dtype)
    e, V, A = jacobi(horn(M), sweeps)
    res.off_diagonal = float(sum(abs(A[p, q]) for p, q in PAIRS))
    res.trace = float(np.abs(e).sum())
    best = int(np.argmax(e))
    second = max(e[i] for i in range(4) if i != best)
    if not e[best] - second > dtype(np.float32(min_gap)) * np.abs(e).sum():
        res.flags = DEGENERATE
        return res
    q = V[:, best] / np.sqrt((V[:, best] ** 2).sum())
    w, x, y, z = q if q[0] >= 0 else -q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype)
    t = cb - R @ ca
    res.pose = np.concatenate([R, t[:, None]], 1)
    res.rms = float(np.sqrt((((a @ R.T + t) - b) ** 2).sum(1).mean()))
    return res


def rotation_angle(Ra, Rb):
    """the angle in radians between two rotations [3, 3] (float64), well conditioned near 0: from the norm of the difference"""
    return float(2.0 * np.arcsin(min(1.0, np.linalg.norm(np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64)) / (2.0 * np.sqrt(2.0)))))


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
