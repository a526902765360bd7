"""Per-object masks (slhip_render_object_masks, slhip_object_masks_expand, sl.ObjectMasks) without a device: the C-ABI
entries resolve, the pool sizing, the record layout, the argument checks, the RLE definition on hand-written vectors, and the
scene_gt_coco form of hand-made masks."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from stillleben_amd import _abi
from stillleben_amd.object_masks import ObjectMasks, rle_decode, rle_encode
from stillleben_amd.object_stats import ObjectStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_resolve():
    L = _abi.lib()
    for name in ("slhip_render_object_masks", "slhip_render_object_masks_bytes", "slhip_object_masks_expand"):
        assert hasattr(L, name), name
    assert L.slhip_abi_version() == 5


def test_record_dtype_matches_header():
    hdr = open(os.path.join(ROOT, "include", "slhip.h")).read()
    m = re.search(r"typedef struct \{\s*int32_t\s+tile_box\[4\];.*?uint64_t\s+word_offset\[2\];.*?uint64_t\s+rle_offset\[2\];.*?"
                  r"uint32_t\s+rle_count\[2\];[^}]*\} slhip_object_mask;", hdr, re.S)
    assert m, "slhip_object_mask changed in include/slhip.h"
    assert "56 bytes" in hdr[max(0, m.start() - 400):m.start()]
    assert _abi.OBJECT_MASK_DTYPE.itemsize == 56
    assert _abi.OBJECT_MASK_DTYPE.names == ("tile_box", "word_offset", "rle_offset", "rle_count")
    assert [_abi.OBJECT_MASK_DTYPE.fields[n][1] for n in _abi.OBJECT_MASK_DTYPE.names] == [0, 16, 32, 48]
    assert "#define SLHIP_OBJECT_MASKS_CAPACITY %d " % _abi.OBJECT_MASKS_CAPACITY in hdr
    assert _abi.OBJECT_MASKS_CAPACITY == 2 and _abi.OBJECT_MASKS_CAPACITY != _abi.OBJECT_STATS_CAPACITY


@pytest.mark.parametrize("B,S,W,H,words,runs", [
    (1, 2, 8, 8, 2 * 1, 2 * (65 + 1)),                       # one object: W * H + 1 per kind; slot 0: one run per kind
    (3, 21, 640, 480, 2 * 3 * 20 * 80 * 60, 2 * (3 * 20 * (640 * 480 + 1) + 3)),
    (2, 4, 100, 50, 2 * 2 * 3 * 13 * 7, 2 * (2 * 3 * 5001 + 2)),   # W, H not multiples of 8: partial tiles count
    (5, 1, 640, 480, 0, 2 * 5),                              # slot 0 only: no words, the single run [W * H] of every mask
])
def test_worst_case_pools(B, S, W, H, words, runs):
    w, r = C.c_uint64(123), C.c_uint64(123)
    assert _abi.lib().slhip_render_object_masks_bytes(B, S, W, H, C.byref(w), C.byref(r)) == 0
    assert (w.value, r.value) == (words, runs)
    stats = C.c_uint64(0)
    _abi.lib().slhip_render_object_stats_bytes(B, S, W, H, C.byref(stats))
    assert w.value == 2 * stats.value


@pytest.mark.parametrize("missing", ["words", "runs"])
def test_bytes_rejects_null(missing):
    L = _abi.lib()
    v = C.c_uint64(0)
    assert L.slhip_render_object_masks_bytes(1, 2, 8, 8, None if missing == "words" else C.byref(v),
                                             None if missing == "runs" else C.byref(v)) != 0
    assert b"slhip_render_object_masks_bytes" in L.slhip_last_error() and b"null" in L.slhip_last_error()


@pytest.mark.parametrize("missing", ["masks", "runs", "words", "out"])
def test_null_pointer_is_an_error(missing):
    """The argument checks run before anything touches a device: fake (never dereferenced) addresses for the rest."""
    L = _abi.lib()
    pool = _abi.MeshPool()
    scratch = _abi.RenderScratch()
    fake = C.c_void_p(0x1000)
    nw, nr = C.c_uint64(0), C.c_uint64(0)
    a = {k: (None if k == missing else fake) for k in ("masks", "runs", "words", "out")}
    st = L.slhip_render_object_masks(C.byref(pool), fake, fake, fake, 1, 1, 1, 64, 64, C.byref(scratch), 2, a["words"], 16,
                                     a["out"], C.byref(nw), a["masks"], a["runs"], 16, C.byref(nr), None)
    assert st < 0
    assert b"slhip_render_object_masks:" in L.slhip_last_error()


def test_expand_argument_checks():
    L = _abi.lib()
    fake = C.c_void_p(0x1000)
    assert L.slhip_object_masks_expand(fake, fake, 1, 2, 64, 64, 2, fake, 1, fake, None) < 0
    assert b"slhip_object_masks_expand" in L.slhip_last_error() and b"kind" in L.slhip_last_error()
    for args in ((None, fake, 1, 2, 64, 64, 0, fake, 1, fake), (fake, fake, 1, 2, 64, 64, 1, fake, 1, None),
                 (fake, fake, 1, 2, 0, 64, 0, fake, 1, fake), (fake, fake, 1, 2, 64, 64, 0, fake, 0, fake)):
        assert L.slhip_object_masks_expand(*args, None) < 0
        assert b"slhip_object_masks_expand" in L.slhip_last_error()


# ---- the RLE definition -------------------------------------------------------------------------------------------------

def test_rle_hand_vectors():
    m = np.array([[0, 1, 1], [1, 1, 0]])                       # H = 2, W = 3: column-major 0,1,1,1,1,0
    assert rle_encode(m) == {"counts": [1, 4, 1], "size": [2, 3]}
    m = np.array([[1, 0], [0, 0], [0, 1]])                     # pixel (0, 0) set: 1,0,0,0,0,1
    assert rle_encode(m) == {"counts": [0, 1, 4, 1], "size": [3, 2]}
    assert rle_encode(np.zeros((5, 7), bool)) == {"counts": [35], "size": [5, 7]}
    assert rle_encode(np.ones((5, 7), np.uint8)) == {"counts": [0, 35], "size": [5, 7]}
    # a run goes on from the bottom of a column into the top of the next
    m = np.array([[0, 1], [1, 0]])                             # 0,1,1,0
    assert rle_encode(m)["counts"] == [1, 2, 1]
    assert rle_decode({"counts": [1, 4, 1], "size": [2, 3]}).tolist() == [[False, True, True], [True, True, False]]
    assert rle_decode({"counts": [0, 35], "size": [5, 7]}).all()
    assert not rle_decode({"counts": [35], "size": [5, 7]}).any()
    with pytest.raises(ValueError):
        rle_decode({"counts": [3, 3], "size": [5, 7]})
    with pytest.raises(ValueError):
        rle_encode(np.zeros((2, 2, 2)))


@pytest.mark.parametrize("seed,p", [(0, 0.5), (1, 0.05), (2, 0.95)])
def test_rle_round_trip(seed, p):
    m = np.random.default_rng(seed).random((37, 53)) < p
    r = rle_encode(m)
    assert r["size"] == [37, 53] and sum(r["counts"]) == 37 * 53
    assert all(c > 0 for c in r["counts"][1:])
    assert np.array_equal(rle_decode(r), m)
    assert rle_encode(rle_decode(r)) == r


# ---- scene_gt_coco ------------------------------------------------------------------------------------------------------

def hand_made_masks(dense_visib, dense_all):
    """An ObjectMasks of CPU tensors from dense [B, S, H, W] arrays: the records and the run pool laid out as the device call
    lays them out (record-major, kind minor); no bit tiles."""
    B, S, H, W = dense_all.shape
    rec = np.zeros((B, S), _abi.OBJECT_MASK_DTYPE)
    rec["tile_box"] = (0, 0, -1, -1)
    runs = []
    for b in range(B):
        for i in range(S):
            for k, d in enumerate((dense_all, dense_visib)):
                c = rle_encode(d[b, i])["counts"]
                rec[b, i]["rle_offset"][k], rec[b, i]["rle_count"][k] = len(runs), len(c)
                runs += c

    def box(m):
        ys, xs = np.nonzero(m)
        return [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1] if len(xs) else [-1] * 4

    t = lambda a: torch.tensor(np.array(a), dtype=torch.int32)   # noqa: E731
    stats = ObjectStats(t(dense_visib.sum(axis=(2, 3))), t(dense_all.sum(axis=(2, 3))),
                        t([[box(dense_visib[b, i]) for i in range(S)] for b in range(B)]),
                        t([[box(dense_all[b, i]) for i in range(S)] for b in range(B)]))
    records = torch.from_numpy(rec.view(np.int32).reshape(B, S, 14).copy())
    return ObjectMasks(stats, records, torch.zeros(1, dtype=torch.int64), torch.tensor(runs, dtype=torch.int32), (H, W))


def test_scene_gt_coco_annotations():
    from stillleben_amd import bop

    B, S, H, W = 2, 4, 6, 9
    whole = np.zeros((B, S, H, W), bool)
    whole[1, 1, 1:5, 2:6] = True          # object 1: a 4 x 4 square, its right half hidden
    whole[1, 2, 0:2, 0:3] = True          # object 2: covers pixel (0, 0), fully visible
    visib = whole.copy()                  # object 3: nothing at all
    visib[1, 1, :, 4:] = False
    masks = hand_made_masks(visib, whole)
    ann = bop.scene_gt_coco_annotations(masks, 1, [5, 9, 2], image_id=17, first_id=40)
    assert len(ann) == 3
    keys = {"id", "image_id", "category_id", "iscrowd", "area", "bbox", "segmentation", "segmentation_all", "width", "height"}
    for k, a in enumerate(ann):
        assert set(a) == keys
        assert a["id"] == 40 + k and a["image_id"] == 17 and a["iscrowd"] == 0 and (a["width"], a["height"]) == (W, H)
        assert a["segmentation"] == rle_encode(visib[1, k + 1]) and a["segmentation_all"] == rle_encode(whole[1, k + 1])
        assert a["segmentation"]["size"] == [H, W]
    assert [a["category_id"] for a in ann] == [5, 9, 2]
    assert ann[0]["area"] == 8 and ann[0]["bbox"] == [2, 1, 2, 4]
    assert ann[1]["area"] == 6 and ann[1]["bbox"] == [0, 0, 3, 2] and ann[1]["segmentation"]["counts"][0] == 0
    assert ann[2]["area"] == 0 and ann[2]["bbox"] == [-1] * 4 and ann[2]["segmentation"]["counts"] == [H * W]
    # ids default to 1..; a single scene's view gives the same; scene 0 is empty
    assert [a["id"] for a in bop.scene_gt_coco_annotations(masks[1], None, [5, 9, 2], 17)] == [1, 2, 3]
    assert all(a["segmentation_all"]["counts"] == [H * W] for a in bop.scene_gt_coco_annotations(masks, 0, [5, 9, 2], 0))
    with pytest.raises(ValueError):
        bop.scene_gt_coco_annotations(masks, 1, [5, 9], 17)
    # rle() and rles() agree; the views keep the pools
    assert masks.rle(1, 2, "all") == masks.rles(1, "all")[1] == masks[1].rle(2, kind="all")
    with pytest.raises(ValueError):
        masks.rle(1, 2, "nope")
    with pytest.raises(RuntimeError):
        masks.dense("all")                # bit tiles are expanded on the device only


def test_object_masks_is_exported():
    import stillleben as sl
    import stillleben_amd

    assert sl.ObjectMasks is stillleben_amd.ObjectMasks is ObjectMasks
    import stillleben.lib.libstillleben_python as m

    assert not hasattr(m, "ObjectMasks")      # the reference's module keeps the reference's names
