"""Two NumPy restatements of the pose errors (include/slhip.h "Pose errors"):
  errors32 / diameter32   the float32 rules of csrc/slhip_pose_rules.h operation by operation, the sums' order included: the
                          tests compare the library with these bit for bit
  errors64 / diameter64   the definitions in float64 in the camera frame, knowing nothing of the rules: the tests compare both
                          the library and the restatement with these within the bound tol()"""
import numpy as np

from object_keypoints_ref import row_point

F = np.float32
ADD, ADDS, MSSD, MSPD = 1, 2, 4, 8
ALL = ADD | ADDS | MSSD | MSPD
BLOCK, WAVE = 256, 64
INF, NAN = F(np.inf), F(np.nan)


def apply(m, p):
    """the rows of a 3 x 4 row-major m applied to the points p [n, >= 3], float32: [n, 3]"""
    m = np.asarray(m, F).reshape(3, 4)
    x, y, z = (np.ascontiguousarray(p[..., i], F) for i in range(3))
    return np.stack([row_point(m[r], x, y, z) for r in range(3)], axis=-1).astype(F)


def dist2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return ((dx * dx + dy * dy) + dz * dz).astype(F)


def move_points(g, e, p):
    """D = e - g; w = D p (rows); add2 = (w0^2 + w1^2) + w2^2; v_c = (g[0][c] w0 + g[1][c] w1) + g[2][c] w2; q = p + v.
    Returns (D, q [n, 3], add2 [n])"""
    g, e = np.asarray(g, F).reshape(3, 4), np.asarray(e, F).reshape(3, 4)
    D = (e - g).astype(F)
    w = apply(D, p)
    add2 = ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]).astype(F)
    v = np.stack([(g[0, c] * w[:, 0] + g[1, c] * w[:, 1]) + g[2, c] * w[:, 2] for c in range(3)], axis=1).astype(F)
    return D, (np.asarray(p, F)[:, :3] + v).astype(F), add2


def block_mean(terms, count):
    """lane l of 256 adds its terms l, l + 256, ... upwards from 0; the wave's butterfly; ((w0 + w1) + w2) + w3; / count"""
    n = len(terms)
    rows = -(-n // BLOCK)
    padded = np.zeros(rows * BLOCK, F)      # a lane without a term in a row adds +0.0: exact
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
    total = F(F(F(w[0] + w[1]) + w[2]) + w[3])
    return F(total / F(count))


def pixels(m, p, K4):
    """(u, v, Z > 0) of the points p under the 3 x 4 m"""
    fx, fy, cx, cy = (F(v) for v in K4)
    X = apply(m, p)
    u = ((fx * X[..., 0]) / X[..., 2] + cx).astype(F)
    v = ((fy * X[..., 1]) / X[..., 2] + cy).astype(F)
    return u, v, X[..., 2] > 0


def lowest_min(vals):
    """(min, its lowest index)"""
    m = vals.min()
    return m, int(np.flatnonzero(vals == m)[0])


def pair32(p, syms, g, e, K4, mask):
    """one pose pair: p [n, 3] the class's points, syms [S, 3, 4]; a dict of scalars"""
    out = {}
    with np.errstate(all="ignore"):
        D, q, add2 = move_points(g, e, p)
        if not np.isfinite(D).all():
            vals = {"add": NAN, "adds": NAN, "mssd": NAN, "mssd_sym": -1, "mspd": NAN, "mspd_sym": -1}
            return vals
        n = len(p)
        if mask & ADD:
            out["add"] = block_mean(np.sqrt(add2).astype(F), n)
        if mask & ADDS:
            best = np.full(n, INF, F)
            for a in range(0, n, 512):
                best[a:a + 512] = dist2(q[a:a + 512, None, :], p[None, :, :]).min(axis=1)
            out["adds"] = block_mean(np.sqrt(best).astype(F), n)
        if mask & (MSSD | MSPD):
            y = np.stack([apply(s, p) for s in syms])                      # [S, n, 3]
        if mask & MSSD:
            m3 = dist2(q[None], y).max(axis=1)
            v, i = lowest_min(m3)
            out["mssd"], out["mssd_sym"] = F(np.sqrt(v)), i
        if mask & MSPD:
            ue, ve, front_e = pixels(e, p, K4)
            ug, vg, front_g = pixels(g, y, K4)
            du, dv = (ue[None] - ug).astype(F), (ve[None] - vg).astype(F)
            m2 = np.fmax.reduce((du * du + dv * dv).astype(F), axis=1, initial=F(0))
            v, i = lowest_min(m2)
            if front_e.all() and front_g.all():
                out["mspd"], out["mspd_sym"] = F(np.sqrt(v)), i
            else:
                out["mspd"], out["mspd_sym"] = INF, -1
    return out


def _empty(shape):
    out = {k: np.zeros(shape, F) for k in ("add", "adds", "mssd", "mspd")}
    out.update({k: np.zeros(shape, np.int32) for k in ("mssd_sym", "mspd_sym")})
    return out


def _class(points, count, symmetries, n_sym, cls):
    """(p [n, 3], syms [S, 3, 4]) of class cls, or None when it has no points"""
    A, N = points.shape[:2]
    if not 0 <= cls < A:
        return None
    n, S = int(count[cls]), int(n_sym[cls])
    if not (1 <= n <= N and 1 <= S <= symmetries.shape[1]):
        return None
    return points[cls, :n, :3], symmetries[cls, :S]


def _keep(out, mask):
    names = {ADD: ("add",), ADDS: ("adds",), MSSD: ("mssd", "mssd_sym"), MSPD: ("mspd", "mspd_sym")}
    return {k: out[k] for bit, ks in names.items() if mask & bit for k in ks}


def errors32(points, count, symmetries, n_sym, classes, gt, est, K4, mask=ALL):
    """points [A, N, 4], count [A], symmetries [A, S, 3, 4], n_sym [A], classes [B, O], gt [B, O, 3, 4], est [B, O, Hy, 3, 4]"""
    points, symmetries = np.asarray(points, F), np.asarray(symmetries, F)
    B, O, Hy = est.shape[:3]
    out = _empty((B, O, Hy))
    for b in range(B):
        for o in range(O):
            c = _class(points, count, symmetries, n_sym, int(classes[b, o]))
            for h in range(Hy):
                if c is None:
                    vals = {"add": INF, "adds": INF, "mssd": INF, "mssd_sym": -1, "mspd": INF, "mspd_sym": -1}
                else:
                    vals = pair32(c[0], c[1], gt[b, o], est[b, o, h], K4, mask)
                for k, v in vals.items():
                    out[k][b, o, h] = v
    return _keep(out, mask)


def diameter32(points, count):
    points = np.asarray(points, F)
    A, N = points.shape[:2]
    out = np.zeros(A, F)
    for a in range(A):
        n = int(count[a])
        if not 1 <= n <= N:
            continue
        p = points[a, :n, :3]
        best = F(0)
        for s in range(0, n, 512):
            best = max(best, dist2(p[s:s + 512, None, :], p[None, :, :]).max())
        out[a] = np.sqrt(F(best))
    return out


# ---- the definitions, float64, camera frame ----------------------------------------------------------------------------------------
def move(m, p):
    m = np.asarray(m, np.float64).reshape(3, 4)
    return p @ m[:, :3].T + m[:, 3]


def errors64(points, count, symmetries, n_sym, classes, gt, est, K4):
    """The formulas of the errors in float64.  Also `mssd_gap` / `mspd_gap`: runner-up minus best over the symmetries (+inf with
    one symmetry), for the tests to leave near-ties out of the index comparison."""
    fx, fy, cx, cy = (float(F(v)) for v in K4)
    B, O, Hy = est.shape[:3]
    out = {k: np.full((B, O, Hy), np.inf) for k in ("add", "adds", "mssd", "mspd", "mssd_gap", "mspd_gap")}
    out.update({k: np.full((B, O, Hy), -1, np.int32) for k in ("mssd_sym", "mspd_sym")})

    def proj(X):
        return np.stack([fx * X[..., 0] / X[..., 2] + cx, fy * X[..., 1] / X[..., 2] + cy], axis=-1)

    def best_and_gap(v):
        order = np.sort(v)
        return float(order[0]), int(np.argmin(v)), float(order[1] - order[0]) if len(v) > 1 else np.inf

    with np.errstate(all="ignore"):
        for b in range(B):
            for o in range(O):
                c = _class(np.asarray(points), count, np.asarray(symmetries), n_sym, int(classes[b, o]))
                if c is None:
                    continue
                p = c[0].astype(np.float64)
                xg = move(gt[b, o], p)
                xs = np.stack([move(gt[b, o], move(s, p)) for s in c[1]])      # [S, n, 3]
                for h in range(Hy):
                    at = (b, o, h)
                    if not np.isfinite(est[b, o, h]).all():
                        for k in ("add", "adds", "mssd", "mspd"):
                            out[k][at] = np.nan
                        continue
                    xe = move(est[b, o, h], p)
                    out["add"][at] = np.linalg.norm(xe - xg, axis=1).mean()
                    out["adds"][at] = sum(np.linalg.norm(xe[i:i + 512, None] - xg[None], axis=2).min(axis=1).sum()
                                          for i in range(0, len(p), 512)) / len(p)
                    out["mssd"][at], out["mssd_sym"][at], out["mssd_gap"][at] = best_and_gap(np.linalg.norm(xe[None] - xs, axis=2).max(axis=1))
                    if (xe[:, 2] > 0).all() and (xs[..., 2] > 0).all():
                        v = np.linalg.norm(proj(xe)[None] - proj(xs), axis=2).max(axis=1)
                        out["mspd"][at], out["mspd_sym"][at], out["mspd_gap"][at] = best_and_gap(v)
    return out


def diameter64(points, count):
    out = np.zeros(len(count))
    for a in range(len(count)):
        n = int(count[a])
        if 1 <= n <= points.shape[1]:
            p = np.asarray(points[a, :n, :3], np.float64)
            out[a] = max(np.linalg.norm(p[i:i + 1] - p, axis=1).max() for i in range(n))
    return out


def largest_coordinate(points, count, symmetries, n_sym, classes, gt, est):
    """M: the largest absolute camera-frame coordinate of the inputs -- every point of every object under its ground truth and
    under each of its finite estimates"""
    M = 0.0
    B, O, Hy = est.shape[:3]
    for b in range(B):
        for o in range(O):
            c = _class(np.asarray(points), count, np.asarray(symmetries), n_sym, int(classes[b, o]))
            if c is None:
                continue
            p = c[0].astype(np.float64)
            for T in [gt[b, o]] + [est[b, o, h] for h in range(Hy)]:
                if np.isfinite(T).all():
                    M = max(M, float(np.abs(move(T, p)).max()))
    return M


def tol(M):
    """64 * 2^-24 * M: a float32 coordinate of magnitude <= M through k roundings is off by at most k 2^-24 M; k is about 8 per
    coordinate and a distance combines three."""
    return 64.0 * 2.0 ** -24 * M


def tol_px(M, K4, z_min):
    """the same factor times fx M / Z_min + max(|cx|, |cy|)"""
    fx, fy, cx, cy = (float(v) for v in K4)
    return 64.0 * 2.0 ** -24 * (max(fx, fy) * M / z_min + max(abs(cx), abs(cy)))
