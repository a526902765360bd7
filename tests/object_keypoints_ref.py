"""NumPy restatement of the object keypoint rules (include/slhip.h "Object keypoints", csrc/slhip_keypoint_rules.h): farthest
point sampling per class, the projection and the per-pixel field, every float32 operation rounded on its own and parenthesised
as the header writes it.  The tests compare the library with these bit for bit."""
import numpy as np

F = np.float32
IN_FRONT, INSIDE, UNOCCLUDED = 1, 2, 4
OFFSET, UNIT = 0, 1


def row_point(m, x, y, z):
    """((m0*x + m1*y) + m2*z) + m3 in float32; m: 4 floats, x, y, z: float32 arrays"""
    m = np.asarray(m, F)
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]


def object_points(mesh_to_object, pos):
    """pos [n, >=3] float32 -> [n, 3]: rows 0..2 of the row-major 4 x 4 applied to (x, y, z, 1)"""
    m = np.asarray(mesh_to_object, F).reshape(4, 4)
    x, y, z = (np.ascontiguousarray(pos[:, i], F) for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([row_point(m[r], x, y, z) for r in range(3)], axis=1).astype(F)


def d2(p, q):
    dx, dy, dz = p[..., 0] - q[0], p[..., 1] - q[1], p[..., 2] - q[2]
    return (dx * dx + dy * dy) + dz * dz


def class_vertices(asset, templates, n_vertices):
    if int(asset["draw_count"]) == 0 or int(asset["n_verts"]) == 0 or int(asset["draw_begin"]) >= len(templates):
        return 0, 0
    base, n = int(templates[int(asset["draw_begin"])]["vtx_base"]), int(asset["n_verts"])
    return (base, n) if base + n <= n_vertices else (0, 0)


def fps_class(points, o, n_fps):
    """points [n, 3] float32 in the object frame, o [3] float32: (keypoints [n_fps, 4], vertex [n_fps]) by a plain scan"""
    kps, idx = np.zeros((n_fps, 4), F), np.full(n_fps, -1, np.int32)
    kps[:, 3] = 1
    if len(points) == 0:
        kps[:, :3] = o
        return kps, idx
    with np.errstate(invalid="ignore", over="ignore"):
        dmin = d2(points, o).astype(F)
        for k in range(n_fps):
            best, i = F(-np.inf), 0
            # the lowest index of the maximum, NaNs never winning: a strict > scanning upwards
            ok = dmin > best
            if ok.any():
                m = dmin[ok].max()
                i = int(np.flatnonzero(dmin == m)[0])
            kps[k, :3], idx[k] = points[i], i
            d = d2(points, points[i]).astype(F)
            dmin = np.where(d < dmin, d, dmin)
    return kps, idx


def fps_class_scan(points, o, n_fps):
    """fps_class written as the literal sequential scan (slow: the check of the vectorised form on small inputs)"""
    kps, idx = np.zeros((n_fps, 4), F), np.full(n_fps, -1, np.int32)
    kps[:, 3] = 1
    if len(points) == 0:
        kps[:, :3] = o
        return kps, idx
    with np.errstate(invalid="ignore", over="ignore"):
        dmin = d2(points, o).astype(F)
        for k in range(n_fps):
            best, i = F(-np.inf), 0
            for v in range(len(points)):
                if dmin[v] > best:
                    best, i = dmin[v], v
            kps[k, :3], idx[k] = points[i], i
            d = d2(points, points[i]).astype(F)
            dmin = np.where(d < dmin, d, dmin)
    return kps, idx


def fps(pos, assets, templates, n_fps, scan=False):
    """(keypoints float32 [A, n_fps, 4], vertex int32 [A, n_fps]) of every class of the table"""
    pos = np.asarray(pos, F).reshape(-1, 4)
    A = len(assets)
    kps, idx = np.zeros((A, n_fps, 4), F), np.zeros((A, n_fps), np.int32)
    for c in range(A):
        a = assets[c]
        base, n = class_vertices(a, templates, len(pos))
        o = ((a["bbox_min"][:3].astype(F) + a["bbox_max"][:3].astype(F)) * F(0.5)).astype(F)
        pts = object_points(a["mesh_to_object"], pos[base:base + n]) if n else np.zeros((0, 3), F)
        kps[c], idx[c] = (fps_class_scan if scan else fps_class)(pts, o, n_fps)
    return kps, idx


def project(bank, asset_ids, o2c, intrinsics, size, depth=None, depth_stride=1, depth_tol=0.005):
    """bank [A, Kp, 4], asset_ids [B, O] (uint32), o2c [B, O, 3, 4] -> camera [B, O, Kp, 4], uv [B, O, Kp, 2], flags u8 [B, O, Kp].
    depth: a flat float32 array read at ((b * H + y) * W + x) * depth_stride, or None."""
    bank, o2c = np.asarray(bank, F), np.asarray(o2c, F)
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    W, H = int(size[0]), int(size[1])
    B, O = asset_ids.shape
    A, Kp = bank.shape[:2]
    camera, uv, flags = np.zeros((B, O, Kp, 4), F), np.zeros((B, O, Kp, 2), F), np.zeros((B, O, Kp), np.uint8)
    tol = F(depth_tol)
    with np.errstate(all="ignore"):
        for b in range(B):
            for o in range(O):
                a = int(asset_ids[b, o])
                if a >= A:
                    continue
                x, y, z = bank[a, :, 0], bank[a, :, 1], bank[a, :, 2]
                X, Y, Z = (row_point(o2c[b, o, r], x, y, z).astype(F) for r in range(3))
                for k in range(Kp):
                    if not (np.isfinite(X[k]) and np.isfinite(Y[k]) and np.isfinite(Z[k]) and Z[k] > 0):
                        continue
                    f = IN_FRONT
                    u = F(F(F(fx * X[k]) / Z[k]) + cx)
                    v = F(F(F(fy * Y[k]) / Z[k]) + cy)
                    if u >= 0 and u < F(W) and v >= 0 and v < F(H):
                        f |= INSIDE
                        if depth is not None:
                            zp = depth[((b * H + int(np.floor(v))) * W + int(np.floor(u))) * depth_stride]
                            if np.isfinite(zp) and zp > 0 and Z[k] <= F(zp + tol):
                                f |= UNOCCLUDED
                    camera[b, o, k] = (X[k], Y[k], Z[k], 1)
                    uv[b, o, k] = (u, v)
                    flags[b, o, k] = f
    return camera, uv, flags


def field(instance, uv, flags, mode, first=0, count=None):
    """instance int16 [B, H, W], uv [B, O, Kp, 2], flags [B, O, Kp] -> float32 [count, H, W, Kp, 2]"""
    B, H, W = instance.shape
    O, Kp = flags.shape[1:]
    count = B - first if count is None else count
    out = np.zeros((count, H, W, Kp, 2), F)
    xc = (np.arange(W).astype(F) + F(0.5))[None, :, None]
    yc = (np.arange(H).astype(F) + F(0.5))[:, None, None]
    with np.errstate(all="ignore"):
        for s in range(count):
            inst = instance[first + s].astype(np.int64)
            own = (inst >= 1) & (inst <= O)
            obj = np.where(own, inst - 1, 0)
            at = np.asarray(uv[first + s], F)[obj]                        # [H, W, Kp, 2]
            live = own[..., None] & ((flags[first + s][obj] & IN_FRONT) != 0)
            dx, dy = (at[..., 0] - xc).astype(F), (at[..., 1] - yc).astype(F)
            if mode == UNIT:
                l = np.sqrt((dx * dx + dy * dy).astype(F)).astype(F)
                zero = l == 0
                safe = np.where(zero, F(1), l)
                dx, dy = np.where(zero, F(0), dx / safe).astype(F), np.where(zero, F(0), dy / safe).astype(F)
            out[s, ..., 0] = np.where(live, dx, F(0))
            out[s, ..., 1] = np.where(live, dy, F(0))
    return out
