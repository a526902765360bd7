"""NumPy restatement of the object points (include/slhip.h "Object points", DESIGN.md "Object points"): eligibility, tile order,
the stratified ranks (Python ints: exact) and every output, the camera point operation for operation in np.float32 -- so that the
device's records and points can be compared bit for bit.  The visible pixels are listed from dense masks or from host words here,
where the device searches the bit tiles."""
import numpy as np

from stillleben_amd import _abi
from test_host_environment import philox4x32_10

F = np.float32
STREAM_POINTS = 6


def draws(p, scene, slot):
    """x_0 .. x_{K-1} of (scene, slot): word j & 3 of key (seed_lo, seed_hi), counter (scene_id_base + scene, 6,
    (slot << 12) | (j >> 2), 0x51DE5EED)."""
    K = int(p["n_points"])
    out = []
    for q in range((K + 3) // 4):
        out += list(philox4x32_10(((int(p["scene_id_base"]) + int(scene)) & 0xFFFFFFFF, STREAM_POINTS, (int(slot) << 12) | q, 0x51DE5EED),
                                  (int(p["seed_lo"]), int(p["seed_hi"]))))
    return [int(x) for x in out[:K]]


def rank(j, n, K, x):
    lo, hi = j * n // K, (j + 1) * n // K
    return lo + ((x * (hi - lo)) >> 32)


def ranks(p, scene, slot, n):
    K = int(p["n_points"])
    return [rank(j, int(n), K, x) for j, x in enumerate(draws(p, scene, slot))]


def tile_order(dense):
    """The set pixels of a dense mask [H, W] in tile order, int64 [m, 2] (x, y): tiles row-major, a tile's pixels by rising bit
    (y & 7) * 8 + (x & 7).  (Every set pixel lies inside the tile box, so the box does not enter.)"""
    ys, xs = np.nonzero(dense)
    order = np.lexsort((xs & 7, ys & 7, xs >> 3, ys >> 3))
    return np.stack([xs[order], ys[order]], axis=1).astype(np.int64).reshape(-1, 2)


def words_order(tile_box, words):
    """The same list from the kind-1 words of a slot (word 0 = the box's first tile)."""
    tx0, ty0, tx1, ty1 = (int(v) for v in tile_box)
    out = []
    if tx0 <= tx1:
        tw = tx1 - tx0 + 1
        for t in range(tw * (ty1 - ty0 + 1)):
            w = int(words[t])
            for bit in range(64):
                if (w >> bit) & 1:
                    out.append((8 * (tx0 + t % tw) + (bit & 7), 8 * (ty0 + t // tw) + (bit >> 3)))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def eligible(p, s, m):
    return bool(int(s["px_visib"]) >= int(p["min_px"]) and F(s["px_visib"]) >= F(p["min_visib_fract"]) * F(s["px_all"])
                and int(m["tile_box"][0]) <= int(m["tile_box"][2]))


def select(p, stats, mask_records):
    """stats [B, S] of OBJECT_STATS_DTYPE, mask_records [B, S] of OBJECT_MASK_DTYPE.  The sets of all eligible (scene,
    slot >= 1) in ascending order."""
    B, S = stats.shape
    out = [(b, i, int(stats[b, i]["px_visib"]), 0) for b in range(B) for i in range(1, S) if eligible(p, stats[b, i], mask_records[b, i])]
    return np.array(out, dtype=_abi.OBJECT_POINT_SET_DTYPE).reshape(-1)


def pixels(p, sets, visible):
    """int16 [n, K, 2] and found bool [n, K].  visible: {(scene, slot): [m, 2] pixels in tile order}; a set without an entry,
    or a rank >= m, gives (0, 0) / False."""
    K = int(p["n_points"])
    xy, found = np.zeros((len(sets), K, 2), np.int16), np.zeros((len(sets), K), bool)
    for k, r in enumerate(sets):
        lst = visible.get((int(r["scene"]), int(r["slot"])))
        if lst is None:
            continue
        for j, rk in enumerate(ranks(p, r["scene"], r["slot"], r["n_visib"])):
            if rk < len(lst):
                xy[k, j], found[k, j] = lst[rk], True
    return xy, found


def gather(p, sets, visible, coord=None, normals=None, rgb=None, depth=None):
    """coord / normals f32 [B,H,W,4], rgb u8 [B,H,W,4], depth f32 [B,H,W] (default: the w of coord).  A dict of the outputs
    named in p["outputs"]."""
    bits = int(p["outputs"])
    xy, found = pixels(p, sets, visible)
    n, K = found.shape
    b = np.broadcast_to(sets["scene"].astype(np.int64)[:, None], (n, K))
    b = np.where(found, b, 0)
    x, y = xy[..., 0].astype(np.int64), xy[..., 1].astype(np.int64)
    out = {}
    if bits & _abi.POINTS_PIXEL:
        out["pixel"] = xy
    if bits & _abi.POINTS_CAMERA:
        plane = coord[..., 3] if depth is None else depth
        z = plane[b, y, x].astype(F)
        with np.errstate(invalid="ignore", over="ignore"):
            X = (((x.astype(F) + F(0.5)) - F(p["cx"])) * z) / F(p["fx"])
            Y = (((y.astype(F) + F(0.5)) - F(p["cy"])) * z) / F(p["fy"])
        assert X.dtype == F and Y.dtype == F
        ok = found & np.isfinite(z) & (z > 0)
        cam = np.stack([X, Y, z, np.ones_like(z)], axis=-1)
        out["camera"] = np.where(ok[..., None], cam, F(0.0)).astype(F)
    for name, bit, src in (("coord", _abi.POINTS_COORD, coord), ("normals", _abi.POINTS_NORMALS, normals), ("rgb", _abi.POINTS_RGB, rgb)):
        if bits & bit:
            out[name] = np.where(found[..., None], src[b, y, x], src.dtype.type(0))
    return out
