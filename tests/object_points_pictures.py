"""Hand-painted pictures of the object-points tests (host and GPU): dense visible and whole masks, and the statistics, mask
records and u64 word pool a render of them would give."""
import numpy as np

from stillleben_amd import _abi


def np_stats(dense_vis, dense_all):
    """slhip_object_stats [B, S] of dense masks [B, S, H, W]."""
    B, S = dense_vis.shape[:2]
    s = np.zeros((B, S), _abi.OBJECT_STATS_DTYPE)
    for b in range(B):
        for i in range(S):
            for m, px, box in ((dense_vis[b, i], "px_visib", "bbox_visib"), (dense_all[b, i], "px_all", "bbox_obj")):
                s[b, i][px] = int(m.sum())
                ys, xs = np.nonzero(m)
                s[b, i][box] = (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1) if len(xs) else (-1,) * 4
    return s


def np_tiles(dense_vis, dense_all, lead=3):
    """slhip_object_mask [B, S] and the u64 word pool of dense masks: per slot the tiles of the whole silhouette's box, kind 0
    then kind 1, behind `lead` words of ones that belong to nobody (a wrong offset reads them)."""
    B, S, H, W = dense_all.shape
    rec = np.zeros((B, S), _abi.OBJECT_MASK_DTYPE)
    words = [0xFFFFFFFFFFFFFFFF] * lead
    bit = (np.arange(8)[:, None] * 8 + np.arange(8)[None, :]).astype(object)
    for b in range(B):
        for i in range(S):
            ys, xs = np.nonzero(dense_all[b, i])
            if not len(xs):
                rec[b, i]["tile_box"] = (0, 0, -1, -1)
                continue
            tx0, ty0, tx1, ty1 = xs.min() >> 3, ys.min() >> 3, xs.max() >> 3, ys.max() >> 3
            rec[b, i]["tile_box"] = (tx0, ty0, tx1, ty1)
            for kind, m in enumerate((dense_all[b, i], dense_vis[b, i])):
                rec[b, i]["word_offset"][kind] = len(words)
                for ty in range(ty0, ty1 + 1):
                    for tx in range(tx0, tx1 + 1):
                        t = m[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
                        words.append(sum(1 << int(v) for v in bit[:t.shape[0], :t.shape[1]][t]))
    return rec, np.array(words, dtype=np.uint64)


def slot_words(host, b, i):
    """tile box and kind-1 words of (scene b, slot i) of a painted picture"""
    r = host["mask_records"][b, i]
    tx0, ty0, tx1, ty1 = (int(v) for v in r["tile_box"])
    n = (tx1 - tx0 + 1) * (ty1 - ty0 + 1) if tx0 <= tx1 else 0
    o = int(r["word_offset"][1])
    return r["tile_box"], host["words"][o:o + n]


def finish(visib, whole, seed):
    rng = np.random.default_rng(seed)
    B, S, H, W = whole.shape
    host = dict(visib=visib, whole=whole, stats=np_stats(visib, whole), rgb=rng.integers(0, 256, (B, H, W, 4), dtype=np.uint8),
                coord=rng.standard_normal((B, H, W, 4)).astype(np.float32), normals=rng.standard_normal((B, H, W, 4)).astype(np.float32))
    host["coord"][..., 3] = np.abs(host["coord"][..., 3]) + np.float32(0.25)      # a camera z: positive
    host["mask_records"], host["words"] = np_tiles(visib, whole)
    return host


def picture_a(B=3, H=37, W=53, S=7):
    """53 x 37: partial right and bottom tiles.  Per scene: 1 a rectangle, 2 a disc in front of part of it (in scene 0 it
    hides whole tiles in the middle of 1's box: all-zero visible words between others), 3 a rectangle in the bottom right
    corner, 4 a rectangle in the top left corner, 5 a single pixel, 6 one whole 8 x 8 tile (its word is all ones: bit 63).
    Scene 1: the disc hides object 1 altogether.  Scene 2: no object 4."""
    yy, xx = np.mgrid[0:H, 0:W]
    whole = np.zeros((B, S, H, W), bool)
    for b in range(B):
        if b == 0:                                       # the disc covers whole tiles in the middle of this one's box
            whole[b, 1, 8:32, 10:26] = True
        elif b == 1:
            whole[b, 1, 16:21, 22:27] = True
        else:
            whole[b, 1, 8 + b:21 + b, 10:26 + b] = True
        whole[b, 2] = (xx - (24 + b)) ** 2 + (yy - 18) ** 2 <= 49 if b else (xx - 20) ** 2 + (yy - 20) ** 2 <= 49
        whole[b, 3, 28 - b:, 40 - 2 * b:] = True
        if b != 2:
            whole[b, 4, :4 + b, :7] = True
        whole[b, 5, 2 + b, 50] = True
        whole[b, 6, 8:16, 40:48] = True
    inst = np.zeros((B, H, W), np.uint16)
    for i in range(1, S):
        inst[whole[:, i]] = i
    visib = np.stack([inst == i for i in range(S)], axis=1)
    visib[:, 0] = False
    return finish(visib, whole, 20261018)


def picture_b(H=136, W=160):
    """160 x 136, one object over the whole viewport: 20 x 17 = 340 tiles, more than the 256 threads of the gather's workgroup
    and no multiple of them, so its segments hold two words and the last ones are short or empty.  Visible bits only in every
    third tile (a quarter of their pixels): runs of empty words, whole empty segments, ties in the search."""
    rng = np.random.default_rng(340)
    whole = np.ones((1, 2, H, W), bool)
    whole[0, 0] = False
    yy, xx = np.mgrid[0:H, 0:W]
    tile = (yy >> 3) * ((W + 7) // 8) + (xx >> 3)
    visib = np.zeros_like(whole)
    visib[0, 1] = (tile % 3 == 0) & (rng.random((H, W)) < 0.25)
    return finish(visib, whole, 340)
