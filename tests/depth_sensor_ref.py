"""CPU restatement of the depth sensor model (DESIGN.md "Depth sensor model"; slhip_depth_sensor of include/slhip.h): NumPy,
float32 throughout, the operation order of the kernels, so that everything but the normal draws of the RNG is comparable bit
for bit.  Also the small scenes the host and the GPU tests share.  One image at a time; `p` is one make_params record."""
import numpy as np

F = np.float32
RANGE, GRAZING, SHADOW, SUPPORT, DROPOUT = 1, 2, 4, 8, 16


def dmax_of(p):
    return int(np.ceil(F(p["fb"]) / F(p["z_min"])))


def project(z, p, c=None):
    """Pass 1: (disparity f32 [H,W], flags u8 [H,W]) with RANGE, GRAZING and SHADOW."""
    z = np.asarray(z, F)
    H, W = z.shape
    fb, dmax = F(p["fb"]), dmax_of(p)
    with np.errstate(invalid="ignore"):
        inr = (z >= F(p["z_min"])) & (z <= F(p["z_max"]))          # NaN: out of range
    d = np.zeros((H, W), F)
    d[inr] = fb / z[inr]
    flags = np.where(inr, 0, RANGE).astype(np.uint8)
    if c is not None and F(p["cos_min"]) > 0:
        flags[inr & (np.abs(np.asarray(c, F)) < F(p["cos_min"]))] = GRAZING
    xs = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    k = np.clip(np.floor(xs - d + F(0.5)).astype(np.int64) + dmax, 0, W + dmax - 1)
    rows = np.broadcast_to(np.arange(H)[:, None], (H, W))
    line = np.zeros((H, W + dmax), F)
    np.maximum.at(line, (rows[inr], k[inr]), d[inr])              # grazing pixels block the projector too
    flags[inr & (line[rows, k] > d + F(p["shadow_margin"]))] |= SHADOW
    return d, flags


def measure(d, flags, p, ex=None, ey=None, u=None, en=None):
    """Pass 2 on the planes of pass 1 with the given draws ([H,W] f32 each; None: ex = ey = en = 0, u = 1, the model with its
    noise off).  Returns (depth f32, depth u16, flags u8)."""
    H, W = d.shape
    zero = np.zeros((H, W), F)
    ex, ey, en = (zero if a is None else np.asarray(a, F) for a in (ex, ey, en))
    u = np.ones((H, W), F) if u is None else np.asarray(u, F)
    fb, r = F(p["fb"]), int(p["window_radius"])
    jx = np.clip(np.floor(F(p["sigma_lateral"]) * ex + F(0.5)), -2, 2).astype(np.int64)
    jy = np.clip(np.floor(F(p["sigma_lateral"]) * ey + F(0.5)), -2, 2).astype(np.int64)
    ys, xs = np.mgrid[0:H, 0:W]
    sx, sy = np.clip(xs + jx, 0, W - 1), np.clip(ys + jy, 0, H - 1)
    fs, ds = flags[sy, sx], d[sy, sx]
    padded = np.full((H + 2 * r, W + 2 * r), np.nan, F)              # NaN: outside the image, or flagged
    padded[r:r + H, r:r + W] = np.where(flags == 0, d, F(np.nan))
    support = np.zeros((H, W), np.int64)
    with np.errstate(invalid="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                support += np.abs(padded[sy + r + dy, sx + r + dx] - ds) <= F(p["window_tol"])
        ok = fs == 0
        out = fs.copy()
        out[ok & (support < int(p["min_support"]))] |= SUPPORT
        out[ok & (u < F(p["dropout_p"]))] |= DROPOUT
        dn = ds + F(p["sigma_disparity"]) * en
        dq = dn
        if int(p["subpixel"]):
            q = F(int(p["subpixel"]))
            dq = np.floor(dn * q + F(0.5)) / q
        pos = dq > 0
        out[ok & ~pos] |= RANGE
        z_out = np.where(pos, fb / np.where(pos, dq, F(1)), F(0)).astype(F)
        valid = out == 0
        u16 = np.minimum(F(65535), np.floor(z_out * F(1000) / F(p["depth_scale"]) + F(0.5)))
    return (np.where(valid, z_out, F(0)).astype(F), np.where(valid, u16, F(0)).astype(np.uint16), out.astype(np.uint8))


def reference(z, p, c=None, **draws):
    d, flags = project(z, p, c)
    return measure(d, flags, p, **draws)


def reference_batch(z, params, c=None):
    """The noise-free model on [n,H,W]: stacked (depth f32, depth u16, flags u8)."""
    res = [reference(z[i], params[i], None if c is None else c[i]) for i in range(len(params))]
    return tuple(np.stack([r[k] for r in res]) for k in range(3))


# ---- shared scenes ---------------------------------------------------------------------------------------------------
def known_answer_params(make_params, **kw):
    """fb = 512 * 0.0625 = 32: every disparity of the two known-answer scenes is an exact integer."""
    a = dict(baseline=0.0625, z_min=0.25, z_max=10.0, shadow_margin=1.0, cos_min=0.0, window_radius=1, window_tol=1.0,
             min_support=6, sigma_lateral=0.0, sigma_disparity=0.0, subpixel=8, dropout_p=0.0, depth_scale=1.0, seed=0)
    a.update(kw)
    return make_params(512.0, **a)


def rectangle_scene():
    """24 x 96, z = 2 everywhere, a rectangle at z = 1 over rows 6..17 and columns 40..63; n.v = 1."""
    z = np.full((24, 96), 2.0, F)
    z[6:18, 40:64] = 1.0
    return z, np.ones((24, 96), F)


def ramp_scene():
    return np.broadcast_to(F(1.0) + F(0.01) * np.arange(96, dtype=F), (24, 96)).copy()


def synthetic_batch(make_params):
    """3 images of 64 x 160 from a fixed seed: a plane, 6 boxes at random depths, a ramp, out-of-range pixels, a random n.v
    plane; all noise off; r = 0, 2, 4; subpixel 0, 8, 8; W + Dmax = 288, 285 (uneven), 280."""
    rng = np.random.default_rng(20261018)
    n, H, W = 3, 64, 160
    z = np.empty((n, H, W), F)
    for i in range(n):
        z[i] = F(2.5) + F(0.002) * np.arange(H, dtype=F)[:, None]
        z[i, 44:] = F(0.9) + F(0.01) * np.arange(W, dtype=F)                      # the ramp
        for _ in range(6):
            y0, x0 = int(rng.integers(0, H - 4)), int(rng.integers(0, W - 4))
            h, w = int(rng.integers(3, 30)), int(rng.integers(3, 50))
            z[i, y0:y0 + h, x0:x0 + w] = F(rng.uniform(0.6, 2.0))
        bad = rng.random((H, W)) < 0.01
        z[i][bad] = rng.choice(np.array([3000.0, np.nan, 0.0, 0.1, -1.0], F), int(bad.sum()))
        z[i, 0, 0], z[i, H - 1, W - 1] = 3000.0, np.nan                           # (every kind at least once)
    c = rng.uniform(-1.0, 1.0, (n, H, W)).astype(F)
    common = dict(sigma_lateral=0.0, sigma_disparity=0.0, dropout_p=0.0, seed=0)
    params = [
        make_params(512.0, baseline=0.0625, z_min=0.25, z_max=10.0, shadow_margin=1.0, cos_min=0.0, window_radius=0,
                    window_tol=0.5, min_support=1, subpixel=0, depth_scale=1.0, **common),
        make_params(500.0, baseline=0.075, z_min=0.3, z_max=2.6, shadow_margin=0.5, cos_min=0.2, window_radius=2,
                    window_tol=1.0, min_support=12, subpixel=8, depth_scale=0.1, **common),
        make_params(600.0, baseline=0.1, z_min=0.5, z_max=5.0, shadow_margin=2.0, cos_min=0.1, window_radius=4,
                    window_tol=2.0, min_support=40, subpixel=8, depth_scale=0.02, **common),
    ]
    return z, c, params
