"""NumPy restatement of the pose VSD (include/slhip.h "Pose VSD", csrc/slhip_vsd_rules.h), operation by operation: float32
throughout, every NumPy operation on float32 arrays is one rounded IEEE operation and the parentheses are those of the header;
the coverage is int64 arithmetic on the snapped vertices.  `dtype=np.float64` runs the same rules in float64 over the same
snapped integers (the snap itself stays float32) and also counts the pixels that sit within 64 * 2^-24 * (the largest distance)
of a threshold -- the cases of the tests must have none.

A bank is (vertices float32 [V, 4], triangles uint32 [N, 3], tri_begin [A], tri_count [A], diameter float32 [A] or None)."""
import numpy as np

F = np.float32
ABSENT = np.uint32(0xFFFFFFFF)
VSD, COUNTS, COST, FLAGS = 1, 2, 4, 8
ALL = 15
CLIPPED = 1
TAUS = tuple(0.05 * k for k in range(1, 11))
EDGE = 64.0 * 2.0 ** -24
CHUNK = 1 << 21      # (triangle, pixel) pairs evaluated at once


def row_point(m, x, y, z):
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]


def snap(c):
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.floor(c * F(256.0) + F(0.5))
    s = np.where(np.isnan(s), F(0.0), s)
    return np.minimum(np.maximum(s, F(-67108864.0)), F(67108864.0)).astype(np.int64)


def class_triangles(bank, cls):
    """the triangles of class `cls` with every index inside the table, or None when the class has no surface"""
    vertices, triangles, tri_begin, tri_count = bank[:4]
    if not 0 <= cls < len(tri_begin):
        return None
    b, n = int(tri_begin[cls]), int(tri_count[cls])
    if n < 1 or b + n > len(triangles):
        return None
    t = np.asarray(triangles[b:b + n], np.int64)
    return t[(t < len(vertices)).all(axis=1)]


def raster(bank, cls, M, K, size, z_near, dtype=F):
    """One pose of a class: (bits uint32 [H, W] of the depth, ABSENT where nothing is covered -- float64 depths with +inf when
    dtype is float64 --, clipped).  The class must have a surface."""
    T = dtype
    fx, fy, cx, cy = (F(v) for v in K)
    W, H = size
    tris = class_triangles(bank, cls)
    M = np.asarray(M, F).reshape(3, 4)
    v = np.asarray(bank[0], F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        X, Y, Z = (row_point(M[r], v[:, 0], v[:, 1], v[:, 2]) for r in range(3))
        ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z > F(z_near))
        Xs, Ys = snap((fx * X) / Z + cx), snap((fy * Y) / Z + cy)
        Mt, vt = M.astype(T), v.astype(T)
        iz = T(1.0) / (row_point(Mt[2], vt[:, 0], vt[:, 1], vt[:, 2]) if T is not F else Z)
    plane = np.full((H, W), ABSENT, np.uint32) if T is F else np.full((H, W), np.inf, T)
    tri_ok = ok[tris].all(axis=1)
    clipped = bool((~tri_ok).any())
    tris = tris[tri_ok]
    TX, TY, TI = Xs[tris], Ys[tris], iz[tris]                                 # [n, 3]
    area2 = (TX[:, 1] - TX[:, 0]) * (TY[:, 2] - TY[:, 0]) - (TY[:, 1] - TY[:, 0]) * (TX[:, 2] - TX[:, 0])
    x0 = np.maximum((TX.min(axis=1) - 128 + 255) >> 8, 0)
    x1 = np.minimum((TX.max(axis=1) - 128) >> 8, W - 1)
    y0 = np.maximum((TY.min(axis=1) - 128 + 255) >> 8, 0)
    y1 = np.minimum((TY.max(axis=1) - 128) >> 8, H - 1)
    keep = (area2 != 0) & (x0 <= x1) & (y0 <= y1)
    if not keep.any():
        return plane, clipped
    TX, TY, TI, area2 = TX[keep], TY[keep], TI[keep], area2[keep]
    wx0, wx1, wy0, wy1 = int(x0[keep].min()), int(x1[keep].max()), int(y0[keep].min()), int(y1[keep].max())
    sign = np.where(area2 < 0, -1, 1).astype(np.int64)[:, None]
    fa = np.abs(area2).astype(T)[:, None]
    py, px = np.mgrid[wy0:wy1 + 1, wx0:wx1 + 1]
    pcx, pcy = (256 * px + 128).reshape(1, -1).astype(np.int64), (256 * py + 128).reshape(1, -1).astype(np.int64)
    best = plane[wy0:wy1 + 1, wx0:wx1 + 1].reshape(-1).copy()
    step = max(1, CHUNK // pcx.size)
    for s in range(0, len(TX), step):
        sl = slice(s, s + step)
        e = []
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            e.append(sign[sl] * ((TX[sl, b] - TX[sl, a])[:, None] * (pcy - TY[sl, a][:, None]) - (TY[sl, b] - TY[sl, a])[:, None] * (pcx - TX[sl, a][:, None])))
        inside = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
        b0, b1, b2 = (e[i].astype(T) / fa[sl] for i in range(3))
        with np.errstate(divide="ignore"):
            z = T(1.0) / ((b0 * TI[sl, 0][:, None] + b1 * TI[sl, 1][:, None]) + b2 * TI[sl, 2][:, None])
        if T is F:
            best = np.minimum(best, np.where(inside, z.view(np.uint32), ABSENT).min(axis=0))
        else:
            best = np.minimum(best, np.where(inside, z, np.inf).min(axis=0))
    plane[wy0:wy1 + 1, wx0:wx1 + 1] = best.reshape(wy1 - wy0 + 1, wx1 - wx0 + 1)
    return plane, clipped


def depth32(bank, classes, poses, K, size, z_near=1e-3):
    """slhip_pose_depth: (float32 [B, O, Hy, H, W], uint32 flags [B, O, Hy])"""
    B, O, Hy = poses.shape[:3]
    W, H = size
    out, flags = np.zeros((B, O, Hy, H, W), F), np.zeros((B, O, Hy), np.uint32)
    for b in range(B):
        for o in range(O):
            cls = int(classes[b, o])
            if class_triangles(bank, cls) is None:
                continue
            for h in range(Hy):
                if not np.isfinite(poses[b, o, h]).all():
                    continue
                plane, clipped = raster(bank, cls, poses[b, o, h], K, size, z_near)
                out[b, o, h] = np.where(plane == ABSENT, F(0.0), plane.view(F))
                flags[b, o, h] = CLIPPED if clipped else 0
    return out, flags


def ray_length(K, size, T=F):
    fx, fy, cx, cy = (T(v) for v in (F(k) for k in K))
    W, H = size
    py, px = np.mgrid[0:H, 0:W]
    xn, yn = ((px.astype(T) + T(0.5)) - cx) / fx, ((py.astype(T) + T(0.5)) - cy) / fy
    return np.sqrt((xn * xn + yn * yn) + T(1.0))


def compare(zg, ze, present_g, present_e, t, ray, delta, thr, T=F):
    """the counts of one hypothesis: (n_visib_gt, n_visib_est, n_inter, n_union), n_cost [len(thr)], near-threshold pixels"""
    with np.errstate(invalid="ignore", over="ignore"):
        absent_t = ~(t > 0) | ~(t - t == 0)
        D_g, D_e, D_t = zg * ray, ze * ray, t * ray
        near_g, near_e = (D_g - D_t) <= T(delta), (D_e - D_t) <= T(delta)
        vg = present_g & (absent_t | near_g)
        ve = (present_e & (absent_t | near_e)) | (vg & present_e)
        inter, uni = vg & ve, vg | ve
        diff = np.abs(D_g - D_e)
        cost = [int((inter & (diff >= T(th))).sum()) for th in thr]
        edge = 0
        if T is not F:
            largest = max([float(np.abs(d[m]).max()) for d, m in ((D_g, present_g), (D_e, present_e), (D_t, ~absent_t & (present_g | present_e)))
                           if m.any()] + [0.0])
            bound = EDGE * largest
            for D, present in ((D_g, present_g), (D_e, present_e)):
                edge += int((present & ~absent_t & (np.abs((D - D_t) - T(delta)) < bound)).sum())
            for th in thr:
                edge += int((inter & (np.abs(diff - T(th)) < bound)).sum())
    return (int(vg.sum()), int(ve.sum()), int(inter.sum()), int(uni.sum())), cost, edge


def evaluate(bank, classes, gt, est, depth, K, taus=TAUS, delta=0.015, normalized=True, z_near=1e-3, mask=ALL, dtype=F):
    """slhip_pose_vsd on host arrays: classes [B, O], gt [B, O, 3, 4], est [B, O, Hy, 3, 4], depth [B, H, W] (the plane the
    entry reads through its stride).  A dict of the outputs named in `mask`; with dtype float64 the same rules in float64 and
    `edge`, the number of pixels within EDGE * (the largest distance) of a threshold."""
    T = dtype
    B, O, Hy = est.shape[:3]
    H, W = depth.shape[1:3]
    size = (W, H)
    taus = np.asarray(taus, F)
    nt = len(taus)
    vsd, counts = np.zeros((B, O, Hy, nt), F), np.zeros((B, O, Hy, 4), np.int32)
    n_cost, flags = np.zeros((B, O, Hy, nt), np.int32), np.zeros((B, O, Hy), np.uint32)
    ray = ray_length(K, size, T)
    edge = 0
    for b in range(B):
        t = np.asarray(depth[b], F).astype(T)
        for o in range(O):
            cls = int(classes[b, o])
            if class_triangles(bank, cls) is None:
                vsd[b, o], counts[b, o], n_cost[b, o] = np.inf, -1, -1
                continue
            if normalized:
                d = F(bank[4][cls])
                thr = [T(taus[k] * d) if T is F else T(taus[k]) * T(d) for k in range(nt)]
            else:
                thr = [T(taus[k]) for k in range(nt)]
            g_plane = None
            for h in range(Hy):
                if not (np.isfinite(gt[b, o]).all() and np.isfinite(est[b, o, h]).all()):
                    vsd[b, o, h], counts[b, o, h], n_cost[b, o, h] = np.nan, -1, -1
                    continue
                if g_plane is None:
                    g_plane, g_clipped = raster(bank, cls, gt[b, o], K, size, z_near, T)
                e_plane, e_clipped = raster(bank, cls, est[b, o, h], K, size, z_near, T)
                if T is F:
                    args = (g_plane.view(F), e_plane.view(F), g_plane != ABSENT, e_plane != ABSENT)
                else:
                    args = (g_plane, e_plane, np.isfinite(g_plane), np.isfinite(e_plane))
                n, cost, near = compare(*args, t, ray, delta, thr, T)
                edge += near
                counts[b, o, h], n_cost[b, o, h] = n, cost
                flags[b, o, h] = CLIPPED if (g_clipped or e_clipped) else 0
                for k in range(nt):
                    vsd[b, o, h, k] = F(1.0) if n[3] == 0 else F(cost[k] + (n[3] - n[2])) / F(n[3])
    out = {"vsd": vsd, "counts": counts, "n_cost": n_cost, "flags": flags}
    out = {k: v for k, v in out.items() if mask & {"vsd": VSD, "counts": COUNTS, "n_cost": COST, "flags": FLAGS}[k]}
    if T is not F:
        out["edge"] = edge
    return out
