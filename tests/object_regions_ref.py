"""NumPy restatement of the object region rules (include/slhip.h "Object regions", csrc/slhip_region_rules.h): the centres by
the keypoints' farthest point sampling, the nearest centre with its tie rule, the per-vertex regions with counts and extents and
the per-pixel label, every float32 operation rounded on its own and parenthesised as the header writes it.  The tests compare
the library with these bit for bit."""
import numpy as np

import object_keypoints_ref as K

F = np.float32
NONE = 255


def centres(pos, assets, templates, n_regions):
    """(centres float32 [A, R, 4], vertex int32 [A, R]): the FPS of the keypoints with n_fps = R"""
    return K.fps(pos, assets, templates, n_regions)


def nearest(points, bank):
    """points [P, 3] float32, bank [R, >= 3] float32 -> region int64 [P]: a scan upwards from region 0 that takes a centre only
    on a strict <; a NaN is never smaller; nothing wins -> 0"""
    points = np.asarray(points, F)
    best, idx = np.full(len(points), np.inf, F), np.zeros(len(points), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(len(bank)):
            d = K.d2(points, np.asarray(bank[r], F)).astype(F)
            win = d < best
            best, idx = np.where(win, d, best), np.where(win, r, idx)
    return idx


def local_of(points, centre):
    """[P, 3] and [P, 3] -> float32 [P, 4] = (x - cx, y - cy, z - cz, (dx*dx + dy*dy) + dz*dz)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (np.asarray(points, F) - np.asarray(centre, F)).astype(F)
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
    return np.concatenate([d, d2[:, None]], axis=1).astype(F)


def vertices(pos, assets, templates, bank):
    """bank [A, R, 4] -> (vertex_region uint8 [V], count int32 [A, R], extent float32 [A, R, 4]).  Classes upwards, so the
    highest class labels a shared vertex; the maxima are taken on the bit patterns with the sign cleared."""
    pos, bank = np.asarray(pos, F).reshape(-1, 4), np.asarray(bank, F)
    A, R = bank.shape[:2]
    vr, count, extent = np.full(len(pos), NONE, np.uint8), np.zeros((A, R), np.int32), np.zeros((A, R, 4), np.uint32)
    for c in range(A):
        a = assets[c]
        base, n = K.class_vertices(a, templates, len(pos))
        if n == 0:
            continue
        pts = K.object_points(a["mesh_to_object"], pos[base:base + n])
        r = nearest(pts, bank[c])
        mag = local_of(pts, bank[c][r, :3]).view(np.uint32) & np.uint32(0x7fffffff)
        np.add.at(count[c], r, 1)
        np.maximum.at(extent[c], r, mag)
        vr[base:base + n] = r
    return vr, count, extent.view(F)


def label(instance, coord, classes, bank):
    """instance int16 [N, H, W], coord float32 [N, H, W, 4], classes int [N, O], bank float32 [A, R, 4] ->
    (region uint8 [N, H, W], local float32 [N, H, W, 4], histogram uint32 [N, O, R])"""
    instance, coord, classes, bank = np.asarray(instance), np.asarray(coord, F), np.asarray(classes), np.asarray(bank, F)
    N, H, W = instance.shape
    O, (A, R) = classes.shape[1], bank.shape[:2]
    region, local, hist = np.full((N, H, W), NONE, np.uint8), np.zeros((N, H, W, 4), F), np.zeros((N, O, R), np.uint32)
    inst = instance.astype(np.int64)
    own = (inst >= 1) & (inst <= O)
    obj = np.where(own, inst - 1, 0)
    cls = classes.astype(np.int64)[np.arange(N)[:, None, None], obj]
    with np.errstate(invalid="ignore"):
        finite = ((coord[..., :3] - coord[..., :3]) == 0).all(axis=-1)      # v - v == 0: neither NaN nor inf
    live = own & (cls >= 0) & (cls < A) & finite
    for c in np.unique(cls[live]):
        at = live & (cls == c)
        pts = coord[at][:, :3]
        r = nearest(pts, bank[c])
        region[at] = r
        local[at] = local_of(pts, bank[c][r, :3])
    n, y, x = np.nonzero(live)
    np.add.at(hist, (n, obj[n, y, x], region[n, y, x].astype(np.int64)), 1)
    return region, local, hist
