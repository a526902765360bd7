"""NumPy restatement of the object crops (include/slhip.h "Object crops", DESIGN.md "Object crops"): eligibility, box, jitter,
window and intrinsics, the nearest and the bilinear sampler, the two mask bits -- operation for operation in np.float32, so that
the device's records and windows can be compared bit for bit.  The amodal bit is read from dense masks here, where the device
reads the bit tiles."""
import numpy as np

from stillleben_amd import _abi
from test_host_environment import philox4x32_10, u01

F = np.float32
STREAM_CROP = 5


def uniforms(p, scene, slot):
    """u0, u1, u2 of (scene, slot): key (seed_lo, seed_hi), counter (scene_id_base + scene, 5, slot, 0x51DE5EED)."""
    x = philox4x32_10(((int(p["scene_id_base"]) + int(scene)) & 0xFFFFFFFF, STREAM_CROP, int(slot), 0x51DE5EED),
                      (int(p["seed_lo"]), int(p["seed_hi"])))
    return u01(x[0]), u01(x[1]), u01(x[2])


def eligible(p, s):
    b = s["bbox_obj"] if int(p["box"]) else s["bbox_visib"]
    return bool(b[2] > 0 and b[3] > 0 and int(s["px_visib"]) >= int(p["min_px"])
                and F(s["px_visib"]) >= F(p["min_visib_fract"]) * F(s["px_all"]))


def record(p, s, scene, slot):
    b = s["bbox_obj"] if int(p["box"]) else s["bbox_visib"]
    x, y, w, h = (int(v) for v in b)
    u0, u1, u2 = uniforms(p, scene, slot)
    fw, fh = F(w), F(h)
    side0 = F(max(w, h)) * F(p["pad"])
    side = side0 * (F(1.0) + F(p["jitter_scale"]) * (F(2.0) * u0 - F(1.0)))
    cxb = (F(x) + F(0.5) * fw) + F(p["jitter_shift"]) * fw * (F(2.0) * u1 - F(1.0))
    cyb = (F(y) + F(0.5) * fh) + F(p["jitter_shift"]) * fh * (F(2.0) * u2 - F(1.0))
    r = np.zeros((), _abi.OBJECT_CROP_DTYPE)
    r["scene"], r["slot"] = scene, slot
    r["x0"] = cxb - F(0.5) * side
    r["y0"] = cyb - F(0.5) * side
    r["side"] = side
    step = side / F(int(p["size"]))
    r["step"] = step
    r["K"] = [F(p["fx"]) / step, F(p["fy"]) / step, (F(p["cx"]) - F(r["x0"])) / step, (F(p["cy"]) - F(r["y0"])) / step]
    for v in (side0, side, cxb, cyb, step):
        assert type(v) is np.float32
    return r


def select(p, stats):
    """stats: [B, S] of _abi.OBJECT_STATS_DTYPE.  The records of all eligible (scene, slot >= 1) in ascending order."""
    B, S = stats.shape
    out = [record(p, stats[b, i], b, i) for b in range(B) for i in range(1, S) if eligible(p, stats[b, i])]
    return np.array(out, dtype=_abi.OBJECT_CROP_DTYPE).reshape(-1)


def _centres(origin, step, N):
    return F(origin) + (np.arange(N, dtype=F) + F(0.5)) * F(step)


def gather(p, recs, rgb=None, coord=None, normals=None, instance=None, dense_all=None):
    """rgb u8 [B,H,W,4], coord / normals f32 [B,H,W,4], instance u16 [B,H,W], dense_all bool [B,S,H,W] or None.  Returns a
    dict of the outputs named in p["outputs"]."""
    N, bits, isolate = int(p["size"]), int(p["outputs"]), bool(p["isolate"])
    n = len(recs)
    H, W = next(t for t in (rgb, coord, normals, instance) if t is not None).shape[1:3]
    out = {}
    if bits & _abi.CROP_RGB:
        out["rgb"] = np.zeros((n, N, N, 4), np.uint8)
    if bits & _abi.CROP_COORD:
        out["coord"] = np.zeros((n, N, N, 4), F)
    if bits & _abi.CROP_NORMALS:
        out["normals"] = np.zeros((n, N, N, 4), F)
    if bits & _abi.CROP_INSTANCE:
        out["instance"] = np.zeros((n, N, N), np.int16)
    if bits & _abi.CROP_MASK:
        out["mask"] = np.zeros((n, N, N), np.uint8)
    for k, r in enumerate(recs):
        b, slot = int(r["scene"]), int(r["slot"])
        sx = _centres(r["x0"], r["step"], N)[None, :] + np.zeros((N, 1), F)      # [v, u]
        sy = _centres(r["y0"], r["step"], N)[:, None] + np.zeros((1, N), F)
        assert sx.dtype == F and sy.dtype == F
        if "rgb" in out:
            tx, ty = sx - F(0.5), sy - F(0.5)
            bx, by = np.floor(tx), np.floor(ty)
            ax, ay = (tx - bx)[..., None], (ty - by)[..., None]
            jx, jy = bx.astype(np.int64), by.astype(np.int64)

            def tap(x, y):
                ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                t = rgb[b, np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(F)
                return np.where(ok[..., None], t, F(0.0))

            top = (F(1.0) - ax) * tap(jx, jy) + ax * tap(jx + 1, jy)
            bot = (F(1.0) - ax) * tap(jx, jy + 1) + ax * tap(jx + 1, jy + 1)
            val = (F(1.0) - ay) * top + ay * bot
            assert val.dtype == F
            out["rgb"][k] = np.minimum(F(255.0), np.floor(val + F(0.5))).astype(np.uint8)
        ix, iy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        cx, cy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
        inst = np.where(inside, instance[b, cy, cx], 0).astype(np.uint16) if instance is not None else np.zeros((N, N), np.uint16)
        visible = inside & (inst == slot) & (instance is not None)
        keep = inside & (visible | (not isolate))
        if "coord" in out:
            out["coord"][k] = np.where(keep[..., None], coord[b, cy, cx], F(0.0))
        if "normals" in out:
            out["normals"][k] = np.where(keep[..., None], normals[b, cy, cx], F(0.0))
        if "instance" in out:
            out["instance"][k] = inst.view(np.int16)
        if "mask" in out:
            amodal = inside & dense_all[b, slot, cy, cx] if dense_all is not None else np.zeros((N, N), bool)
            out["mask"][k] = visible.astype(np.uint8) | (amodal.astype(np.uint8) << 1)
    return out


def reaches_outside(recs, W, H):
    """(left, top, right, bottom): does any window reach beyond that border of the picture?"""
    x1 = recs["x0"].astype(np.float64) + recs["side"]
    y1 = recs["y0"].astype(np.float64) + recs["side"]
    return bool((recs["x0"] < 0).any()), bool((recs["y0"] < 0).any()), bool((x1 > W).any()), bool((y1 > H).any())
