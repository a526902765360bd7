"""NumPy restatement of the render flow (include/slhip.h "Render flow", DESIGN.md "Render flow", csrc/slhip_flow_rules.h): the
motion of a rigid frame and every per-pixel output, operation for operation.  One body serves two number types: with
T = np.float32 it is the restatement the library is compared with bit for bit (every intermediate is asserted to be float32);
with T = np.float64 it is the same definitions in double precision, the reference of the known answers."""
import numpy as np

from stillleben_amd import _abi

F = np.float32
VALID, INSIDE, VISIBLE = _abi.FLOW_VALID, _abi.FLOW_INSIDE, _abi.FLOW_VISIBLE


def _is(T, *arrays):
    for a in arrays:
        assert a.dtype == T, (a.dtype, T)


def row_point(m, x, y, z):
    """m [..., 4]: ((m0 * x + m1 * y) + m2 * z) + m3"""
    return ((m[..., 0] * x + m[..., 1] * y) + m[..., 2] * z) + m[..., 3]


def dot3(a, b, c, d, e, f):
    return (a * b + c * d) + e * f


def motion(from_, to, T=F):
    """to o inv_rigid(from_) on [..., 3, 4] (rows 0-2 of [..., 4, 4] taken); 12 NaNs where any of the 24 entries is not finite"""
    f = np.asarray(from_, T)[..., :3, :]
    t = np.asarray(to, T)[..., :3, :]
    out = np.zeros(f.shape, T)
    with np.errstate(invalid="ignore", over="ignore"):
        Ri = np.swapaxes(f[..., :3], -1, -2)                                   # Ri[r][c] = R[c][r]
        ti = np.stack([-dot3(f[..., 0, r], f[..., 0, 3], f[..., 1, r], f[..., 1, 3], f[..., 2, r], f[..., 2, 3]) for r in range(3)], axis=-1)
        for r in range(3):
            m = t[..., r, :]
            for c in range(3):
                out[..., r, c] = dot3(m[..., 0], Ri[..., 0, c], m[..., 1], Ri[..., 1, c], m[..., 2], Ri[..., 2, c])
            out[..., r, 3] = row_point(m, ti[..., 0], ti[..., 1], ti[..., 2])
    _is(T, Ri, ti, out)
    bad = ~(np.isfinite(f).all(axis=(-1, -2)) & np.isfinite(t).all(axis=(-1, -2)))
    out[bad] = np.nan
    return out


def depth_plane(d):
    d = np.asarray(d)
    return d[..., 3] if d.ndim == 4 else d


def flow(p, depth_a, instance_a, table, depth_b=None, instance_b=None, T=F):
    """p: a slhip_render_flow_params record.  depth_* f32 [B, H, W] or the coord target [B, H, W, 4]; instance_* int16 / uint16
    [B, H, W]; table [B, S, 3, 4].  Returns (flow [B, H, W, 2], scene_flow [B, H, W, 3], flags u8 [B, H, W], counts i32
    [B, S, 4]) -- all four whatever p["outputs"] says."""
    fx, fy, cx, cy = (T(p[k]) for k in ("fx", "fy", "cx", "cy"))
    W, H, S = int(p["W"]), int(p["H"]), int(p["n_slots"])
    z = depth_plane(depth_a).astype(T)
    B = z.shape[0]
    assert z.shape == (B, H, W)
    i = np.ascontiguousarray(instance_a).reshape(B, H, W).view(np.uint16).astype(np.int64)
    table = np.asarray(table, T)
    assert table.shape == (B, S, 3, 4)
    bb = np.arange(B)[:, None, None]
    M = table[bb, np.minimum(i, S - 1)]                                        # [B, H, W, 3, 4]
    ok = np.isfinite(z) & (z > 0) & (z < T(p["max_depth"])) & (i < S) & np.isfinite(M).all(axis=(-1, -2))
    px = (np.arange(W).astype(T) + T(0.5))[None, None, :]
    py = (np.arange(H).astype(T) + T(0.5))[None, :, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        X = ((px - cx) * z) / fx
        Y = ((py - cy) * z) / fy
        Xp, Yp, Zp = (row_point(M[..., r, :], X, Y, z) for r in range(3))
        front = np.isfinite(Xp) & np.isfinite(Yp) & np.isfinite(Zp) & (Zp > 0)
        valid = ok & front
        u = (fx * Xp) / Zp + cx
        v = (fy * Yp) / Zp + cy
        inside = valid & (u >= 0) & (u < T(W)) & (v >= 0) & (v < T(H))
        fl = np.stack([u - px, v - py], axis=-1)
        sf = np.stack([Xp - X, Yp - Y, Zp - z], axis=-1)
        _is(T, X, Y, Xp, Yp, Zp, u, v, fl, sf)
        visible = np.zeros_like(valid)
        if depth_b is not None:
            zb = depth_plane(depth_b).astype(T)
            ib = None
            if instance_b is not None and (int(p["flags"]) & _abi.FLOW_MATCH_INSTANCE):
                ib = np.ascontiguousarray(instance_b).reshape(B, H, W).view(np.uint16).astype(np.int64)
            x0 = np.where(inside, np.floor(u - T(0.5)), 0).astype(np.int64)
            y0 = np.where(inside, np.floor(v - T(0.5)), 0).astype(np.int64)
            tol = T(p["depth_tol"]) + T(p["depth_rel"]) * Zp
            _is(T, tol)
            for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
                xx, yy = x0 + dx, y0 + dy
                inb = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                xc, yc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
                zp = zb[bb, yc, xc]
                passes = inb & np.isfinite(zp) & (zp > 0) & (Zp <= zp + tol)
                if ib is not None:
                    passes &= ib[bb, yc, xc] == i
                visible |= inside & passes
    zero = T(0.0)
    fl = np.where(valid[..., None], fl, zero).astype(T)
    sf = np.where(valid[..., None], sf, zero).astype(T)
    flags = (valid * VALID + inside * INSIDE + visible * VISIBLE).astype(np.uint8)
    counts = np.zeros((B, S, 4), np.int32)
    for b in range(B):
        mine = i[b] < S
        for col, which in enumerate((np.ones_like(valid[b]), valid[b], inside[b], visible[b])):
            counts[b, :, col] = np.bincount(i[b][mine & which], minlength=S)
    return fl, sf, flags, counts
