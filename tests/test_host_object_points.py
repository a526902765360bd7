"""Host tests of the object points: the record layout against include/slhip.h, every rule of
slhip_object_points_check_params, the properties of the rank rule, and the pixel lookup of csrc/slhip_mask_select.h through
slhip_object_points_host_pixels against the NumPy restatement (tests/object_points_ref.py, the reference the GPU tests compare
the kernels against) on hand-painted masks.  No GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import object_points_pictures as P
import object_points_ref as R
from conftest import ROOT
from stillleben_amd import _abi
from stillleben_amd import object_points as op
from test_host_environment import philox4x32_10

K4 = (61.5, 60.25, 27.125, 17.75)


@pytest.fixture(scope="module")
def pic_a():
    return P.picture_a()


@pytest.fixture(scope="module")
def pic_b():
    return P.picture_b()


def host_pixels(p, scene, slot, n_visib, tile_box, words):
    K = int(p["n_points"])
    out = np.full((K, 2), -7, np.int16)
    box = np.ascontiguousarray(tile_box, dtype=np.int32)
    w = np.ascontiguousarray(np.concatenate([np.asarray(words, dtype=np.uint64), np.zeros(1, np.uint64)]))
    rec = np.ascontiguousarray(p.reshape(1))
    st = _abi.lib().slhip_object_points_host_pixels(rec.ctypes.data, int(scene), int(slot), int(n_visib), box.ctypes.data, w.ctypes.data,
                                                    out.ctypes.data)
    _abi.check(st, "slhip_object_points_host_pixels")
    return out


# ---- layout -------------------------------------------------------------------------------------------------------------------
def test_abi_layout_matches_the_header():
    src = open(os.path.join(ROOT, "stillleben_amd", "csrc", "slhip_object_points.hip")).read()
    sizes = {n: int(v) for n, v in re.findall(r"static_assert\(sizeof\((slhip_\w+)\) == (\d+)", src)}
    assert sizes["slhip_object_point_params"] == _abi.OBJECT_POINT_PARAMS_DTYPE.itemsize == 48
    assert sizes["slhip_object_point_set"] == _abi.OBJECT_POINT_SET_DTYPE.itemsize == 16
    hdr = open(os.path.join(ROOT, "include", "slhip.h")).read()
    for struct, dtype in (("slhip_object_point_params", _abi.OBJECT_POINT_PARAMS_DTYPE), ("slhip_object_point_set", _abi.OBJECT_POINT_SET_DTYPE)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        names = [n for n in re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))]
        assert names == list(dtype.names), struct
    body = re.search(r"typedef struct \{([^}]*)\} slhip_object_points_out;", hdr).group(1)
    assert re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in _abi.ObjectPointsOut._fields_]
    assert re.search(r"#define SLHIP_OBJECT_POINTS_CAPACITY\s+4\b", hdr) and _abi.OBJECT_POINTS_CAPACITY == 4
    assert re.search(r"#define SLHIP_OBJECT_POINTS_MAX\s+16384\b", hdr) and _abi.OBJECT_POINTS_MAX == 16384
    assert re.search(r"#define SLHIP_ABI_VERSION 5\b", hdr) and _abi.ABI_VERSION == 5
    for name, bit in op.OUTPUTS.items():
        assert re.search(r"#define SLHIP_POINTS_%s\s+%du\b" % (name.upper(), bit), hdr), name
    assert sorted(op.OUTPUTS.values()) == [1, 2, 4, 8, 16]
    L = _abi.lib()
    for entry in ("check_params", "scratch_bytes", "select", "gather", "host_pixels", "timing_enable", "timings"):
        assert hasattr(L, "slhip_object_points_" + entry), entry


def test_stream_6_is_a_stream_of_its_own():
    assert _abi.SYNTH_STREAM_POINTS == R.STREAM_POINTS == 6 and _abi.SYNTH_STREAM_CROP == 5
    assert "Stream 6, point ranks" in open(os.path.join(ROOT, "include", "slhip.h")).read()
    key = (12345, 77)
    p = op.make_params(K4, n_points=10, seed=(77 << 32) | 12345, scene_id_base=40)
    x = R.draws(p, 1, 3)
    assert x[:4] == list(philox4x32_10((41, 6, (3 << 12) | 0, 0x51DE5EED), key))
    assert x[8:10] == list(philox4x32_10((41, 6, (3 << 12) | 2, 0x51DE5EED), key))[:2]
    assert R.draws(op.make_params(K4, n_points=10, seed=key, scene_id_base=40), 1, 3) == x      # the key as a (lo, hi) pair
    assert set(x).isdisjoint(philox4x32_10((41, 5, 3 << 12, 0x51DE5EED), key))
    # K <= 16384 keeps j >> 2 inside its 12 bits: the last point of slot s and the first of slot s + 1 do not share a counter
    assert ((_abi.OBJECT_POINTS_MAX - 1) >> 2) < (1 << 12)


# ---- check_params -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change,message", [
    (dict(n_points=0), "n_points 0 must be in [1, 16384]"),
    (dict(n_points=16385), "n_points 16385 must be in [1, 16384]"),
    (dict(min_px=0), "min_px 0 must be at least 1"),
    (dict(min_visib_fract=1.25), "min_visib_fract 1.25 must be in [0, 1]"),
    (dict(min_visib_fract=-0.25), "min_visib_fract -0.25 must be in [0, 1]"),
    (dict(min_visib_fract=float("nan")), "min_visib_fract nan must be in [0, 1]"),
    (dict(outputs=()), "outputs 0x0 must name at least one"),
])
def test_check_params_rules(change, message):
    with pytest.raises(_abi.SlhipError) as e:
        op.check_params(op.make_params(K4, **change), 320, 240)
    assert message in str(e.value)


@pytest.mark.parametrize("field,value,message", [
    ("outputs", 32, "outputs 0x20 must name at least one"),
    ("fx", 0.0, "fx and fy must be positive"),
    ("fy", -3.0, "fx and fy must be positive"),
    ("fx", np.inf, "all four finite"),
    ("cx", np.inf, "all four finite"),
    ("cy", np.nan, "all four finite"),
])
def test_check_params_rules_of_the_raw_record(field, value, message):
    p = op.make_params(K4)
    p[field] = value
    with pytest.raises(_abi.SlhipError) as e:
        op.check_params(p, 320, 240)
    assert message in str(e.value)


def test_check_params_accepts_the_limits_and_refuses_bad_pictures_and_slot_counts():
    for kw in (dict(n_points=1), dict(n_points=16384), dict(min_visib_fract=1.0), dict(min_visib_fract=0.0),
               dict(outputs=("pixel", "camera", "coord", "normals", "rgb")), dict(outputs="rgb")):
        op.check_params(op.make_params(K4, **kw), 320, 240)
    op.check_params(op.make_params(K4), 32768, 4)
    for W, H in ((0, 240), (320, -1), (32769, 4), (4, 32769)):
        with pytest.raises(_abi.SlhipError) as e:
            op.check_params(op.make_params(K4), W, H)
        assert "bad picture size" in str(e.value)
    L = _abi.lib()
    assert L.slhip_object_points_check_params(None, 320, 240) < 0
    with pytest.raises(ValueError):
        op.make_params(K4, outputs=("pixel", "depth"))
    # the slot range, where it is known: select and gather refuse more than 65536 slots before they touch anything
    good = op.make_params(K4).reshape(1)
    n = C.c_uint64(7)
    one = np.zeros(8, np.uint64)
    ptr = C.c_void_p(one.ctypes.data)
    assert L.slhip_object_points_select(good.ctypes.data, ptr, ptr, 1, 65537, ptr, 1, ptr, C.byref(n), None) < 0
    assert b"n_slots 65537 must be in [1, 65536]" in L.slhip_last_error()
    assert L.slhip_object_points_select(good.ctypes.data, ptr, ptr, 1, 0, ptr, 1, ptr, C.byref(n), None) < 0
    src, out = _abi.RenderOut(), _abi.ObjectPointsOut()
    assert L.slhip_object_points_gather(good.ctypes.data, ptr, 1, C.byref(src), ptr, 4, 1, 8, 8, ptr, ptr, 65537, C.byref(out), None) < 0
    assert b"n_slots 65537" in L.slhip_last_error()


def test_null_arguments_are_refused_without_a_device():
    L = _abi.lib()
    bad = op.make_params(K4, n_points=0).reshape(1)
    good = op.make_params(K4, outputs=("pixel", "camera", "coord")).reshape(1)
    n = C.c_uint64(7)
    assert L.slhip_object_points_select(bad.ctypes.data, None, None, 1, 2, None, 0, None, C.byref(n), None) < 0
    assert b"n_points 0" in L.slhip_last_error()
    assert L.slhip_object_points_select(good.ctypes.data, None, None, 1, 2, None, 0, None, C.byref(n), None) < 0
    assert b"null argument" in L.slhip_last_error()
    assert L.slhip_object_points_gather(bad.ctypes.data, None, 1, None, None, 0, 1, 8, 8, None, None, 2, None, None) < 0
    assert L.slhip_object_points_gather(good.ctypes.data, None, 0, None, None, 0, 1, 8, 8, None, None, 2, None, None) == 0   # n_sets == 0
    assert L.slhip_object_points_gather(good.ctypes.data, None, 1, None, None, 0, 1, 8, 8, None, None, 2, None, None) < 0
    assert b"null argument" in L.slhip_last_error()
    # every pointer a requested output needs, one missing at a time
    one = np.zeros(8, np.uint64)
    ptr = one.ctypes.data
    src, out = _abi.RenderOut(), _abi.ObjectPointsOut()

    def call(depth=ptr, stride=4):
        return L.slhip_object_points_gather(good.ctypes.data, C.c_void_p(ptr), 1, C.byref(src), C.c_void_p(depth), stride, 1, 8, 8,
                                            C.c_void_p(ptr), C.c_void_p(ptr), 2, C.byref(out), None)

    assert call() < 0 and b"a render target they read is NULL" in L.slhip_last_error()
    src.d_coord = ptr
    assert call(depth=None) < 0 and b"camera output needs d_depth" in L.slhip_last_error()
    assert call(stride=0) < 0 and b"camera output needs d_depth" in L.slhip_last_error()
    assert call() < 0 and b"a requested output pointer is NULL" in L.slhip_last_error()
    out.d_pixel, out.d_coord = ptr, ptr
    assert call() < 0 and b"a requested output pointer is NULL" in L.slhip_last_error()      # camera still missing
    ms = (C.c_float * 2)()
    assert L.slhip_object_points_timings(C.byref(ms)) < 0 and b"no timed calls" in L.slhip_last_error()
    nb = C.c_uint64(0)
    assert L.slhip_object_points_scratch_bytes(300, C.byref(nb)) == 0 and nb.value == 301 * 8
    box = np.zeros(4, np.int32)
    assert L.slhip_object_points_host_pixels(good.ctypes.data, 0, 1, 1, None, C.c_void_p(ptr), C.c_void_p(ptr)) < 0
    assert L.slhip_object_points_host_pixels(good.ctypes.data, 0, 65536, 1, box.ctypes.data, C.c_void_p(ptr), C.c_void_p(ptr)) < 0


# ---- the rank rule ------------------------------------------------------------------------------------------------------------
def test_rank_properties():
    """Non-decreasing in j and below n; n >= K: all distinct; n <= K: every pixel appears; n == K: point j is pixel j -- for
    random draws and for the extreme draws 0 and 2^32 - 1 throughout."""
    rng = np.random.default_rng(6)
    top = (1 << 32) - 1
    cases = [(1, 1), (1, 16384), (16384, 1), (7, 7), (64, 69), (69, 64), (307200, 1024), (307200, 16384), (1000, 1000),
             ((1 << 31) - 1, 16384), ((1 << 32) - 1, 16383)]
    cases += [(int(rng.integers(1, 5000)), int(rng.integers(1, 2049))) for _ in range(200)]
    for n, K in cases:
        for draw in ("zero", "top", "random"):
            x = {"zero": [0] * K, "top": [top] * K, "random": [int(v) for v in rng.integers(0, 1 << 32, K)]}[draw]
            r = [R.rank(j, n, K, x[j]) for j in range(K)]
            assert all(a <= b for a, b in zip(r, r[1:])), (n, K, draw)
            assert 0 <= r[0] and r[-1] < n, (n, K, draw)
            if n >= K:
                assert len(set(r)) == K, (n, K, draw)
            if n <= K:
                assert set(r) == set(range(n)), (n, K, draw)
            if n == K:
                assert r == list(range(n))


# ---- the lookup ---------------------------------------------------------------------------------------------------------------
def test_tile_order_of_the_reference_is_the_order_of_the_words(pic_a, pic_b):
    for host in (pic_a, pic_b):
        B, S = host["stats"].shape
        for b in range(B):
            for i in range(1, S):
                box, words = P.slot_words(host, b, i)
                a, w = R.tile_order(host["visib"][b, i]), R.words_order(box, words)
                assert np.array_equal(a, w) and len(a) == host["stats"][b, i]["px_visib"], (b, i)
    # a known answer: two pixels of one tile, one of the tile to its right, one of the tile below
    m = np.zeros((16, 16), bool)
    m[1, 2] = m[0, 5] = m[0, 9] = m[8, 0] = True
    assert R.tile_order(m).tolist() == [[5, 0], [2, 1], [9, 0], [0, 8]]


@pytest.mark.parametrize("K", [1, 7, 64, 69, 1000])
def test_host_pixels_on_picture_a(pic_a, K):
    host = pic_a
    p = op.make_params(K4, n_points=K, seed=(5 << 32) | 77, scene_id_base=1000)
    sets = R.select(p, host["stats"], host["mask_records"])
    pairs = [(int(r["scene"]), int(r["slot"])) for r in sets]
    assert pairs == sorted(pairs) and len(pairs) == 3 * 6 - 2 and (1, 1) not in pairs and (2, 4) not in pairs
    visible = {k: R.tile_order(host["visib"][k]) for k in pairs}
    want, found = R.pixels(p, sets, visible)
    assert found.all()
    for k, r in enumerate(sets):
        b, i = pairs[k]
        box, words = P.slot_words(host, b, i)
        got = host_pixels(p, b, i, r["n_visib"], box, words)
        assert np.array_equal(got, want[k]), (b, i)
        assert host["visib"][b, i][got[:, 1], got[:, 0]].all(), (b, i)           # every pixel is a visible pixel of the object
        n = int(r["n_visib"])
        distinct = len({(int(x), int(y)) for x, y in got})
        assert distinct == min(n, K), (b, i, n, distinct)                        # without replacement / the whole mask
    if K == 64:                                                                  # n == K: point j is pixel j of the full tile
        k = pairs.index((0, 6))
        assert want[k].tolist() == [[40 + (j & 7), 8 + (j >> 3)] for j in range(64)]


def test_host_pixels_on_picture_b(pic_b):
    host = pic_b
    n = int(host["stats"][0, 1]["px_visib"])
    box, words = P.slot_words(host, 0, 1)
    assert len(words) == 340 and tuple(box) == (0, 0, 19, 16) and n > 1005
    assert all(int(w) == 0 for t, w in enumerate(words) if t % 3) and sum(int(w) != 0 for w in words) > 100
    lst = R.tile_order(host["visib"][0, 1])
    for K in (1, 7, 1000, n, n + 5):
        p = op.make_params(K4, n_points=K, seed=9)
        sets = R.select(p, host["stats"], host["mask_records"])
        assert len(sets) == 1 and sets[0]["n_visib"] == n
        want, found = R.pixels(p, sets, {(0, 1): lst})
        got = host_pixels(p, 0, 1, n, box, words)
        assert found.all() and np.array_equal(got, want[0]), K
        if K == n:
            assert np.array_equal(got, lst)
    # statistics that claim more pixels than the words hold: (0, 0) for the ranks beyond them, as the reference says
    p = op.make_params(K4, n_points=50, seed=9)
    sets = R.select(p, host["stats"], host["mask_records"])
    sets["n_visib"] = 2 * n
    want, found = R.pixels(p, sets, {(0, 1): lst})
    got = host_pixels(p, 0, 1, 2 * n, box, words)
    assert np.array_equal(got, want[0]) and 0 < found.sum() < 50 and (got[~found[0]] == 0).all()


@pytest.mark.parametrize("word", [1, 1 << 63, (1 << 64) - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x8000000000000001,
                                  0x00FF00F00F0C0A01])
def test_nth_set_bit(word):
    """One tile at (3, 2), K = n = popcount: point j is the j-th set bit of the word."""
    bits = [k for k in range(64) if (word >> k) & 1]
    p = op.make_params(K4, n_points=len(bits), seed=1)
    got = host_pixels(p, 0, 1, len(bits), (3, 2, 3, 2), [word])
    assert got.tolist() == [[24 + (k & 7), 16 + (k >> 3)] for k in bits]
    # and behind a run of empty tiles in a wider box
    got = host_pixels(p, 0, 1, len(bits), (1, 2, 4, 3), [0, 0, 0, 0, 0, 0, word, 0])
    assert got.tolist() == [[24 + (k & 7), 24 + (k >> 3)] for k in bits]


# ---- the container and extract's refusals ---------------------------------------------------------------------------------------
def test_container_views_indexing_and_map():
    n, K, W = 4, 3, 53
    rec = np.zeros(n, _abi.OBJECT_POINT_SET_DTYPE)
    rec["scene"], rec["slot"], rec["n_visib"] = [0, 0, 1, 3], [1, 2, 1, 5], [10, 20, 30, 40]
    records = torch.from_numpy(rec.view(np.int32).reshape(n, 4).copy())
    pixel = torch.arange(n * K * 2, dtype=torch.int16).reshape(n, K, 2)
    camera = torch.ones((n, K, 4))
    camera[1, 2] = 0
    c = op.ObjectPoints(records, W, pixel=pixel, camera=camera)
    assert len(c) == n and c.scene.tolist() == [0, 0, 1, 3] and c.slot.tolist() == [1, 2, 1, 5] and c.n_visib.tolist() == [10, 20, 30, 40]
    assert c.scene.data_ptr() == records.data_ptr() and c.scene.dtype == torch.int32      # views of the record tensor
    assert c.valid.dtype == torch.bool and c.valid.sum() == n * K - 1 and not bool(c.valid[1, 2])
    assert c.index.dtype == torch.int64 and torch.equal(c.index, pixel[..., 1].long() * W + pixel[..., 0].long())
    assert c.coord is None and c.normals is None and c.rgb is None
    assert repr(c) == "ObjectPoints(4 x 3: pixel, camera)"
    one = c[3]
    assert int(one.slot) == 5 and tuple(one.pixel.shape) == (K, 2) and tuple(one.index.shape) == (K,) and int(c[-1].n_visib) == 40
    with pytest.raises(IndexError):
        c[4]
    with pytest.raises(TypeError):
        len(one)
    part = c[1:3]
    assert len(part) == 2 and part.slot.tolist() == [2, 1] and part.width == W
    sel = c.map(lambda t: t[c.scene == 0])
    assert len(sel) == 2 and sel.coord is None
    c.scene_global = c.scene + 16
    assert c[2:].scene_global.tolist() == [17, 19]
    empty = op.ObjectPoints(records, W)
    assert empty.valid is None and empty.index is None


def test_extract_argument_errors_need_no_device(pic_a):
    """What extract refuses before it asks anything of a device: missing masks, a target that was not rendered, tensors on the
    host."""
    from stillleben_amd.object_masks import ObjectMasks
    from stillleben_amd.object_stats import ObjectStats

    host = pic_a
    B, S = host["stats"].shape
    stats = ObjectStats.from_records(torch.from_numpy(host["stats"].view(np.int32).reshape(B, S, 10).copy()))
    masks = ObjectMasks(stats, torch.from_numpy(host["mask_records"].view(np.int32).reshape(B, S, 14).copy()),
                        torch.from_numpy(host["words"].view(np.int64).copy()), torch.zeros(1, dtype=torch.int32), (37, 53))
    full = types.SimpleNamespace(rgb=None, coord=torch.from_numpy(host["coord"]), normals=None, object_stats=stats, object_masks=masks)
    with pytest.raises(_abi.SlhipError) as e:
        op.extract(full, K4, n_points=8)
    assert "no CPU path" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        op.extract(types.SimpleNamespace(**{**vars(full), "object_masks": None}), K4, n_points=8)
    assert "object_masks=True" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        op.extract(full, K4, n_points=8, outputs=("normals",))
    assert "`normals` target was not rendered" in str(e.value)
    no_coord = types.SimpleNamespace(**{**vars(full), "coord": None})
    with pytest.raises(RuntimeError) as e:
        op.extract(no_coord, K4, n_points=8, outputs=("camera",))              # the default depth is the w of coord
    assert "`coord` target was not rendered" in str(e.value)
    with pytest.raises(_abi.SlhipError) as e:
        op.extract(no_coord, K4, n_points=8, outputs=("pixel", "camera"), depth=torch.zeros((B, 37, 53)))      # nothing reads coord now
    assert "no CPU path" in str(e.value)
    with pytest.raises(ValueError):
        op.extract(full, K4, n_points=8, depth=torch.zeros((B, 37, 52)))
    with pytest.raises(_abi.SlhipError) as e:
        op.extract(full, K4, n_points=20000)
    assert "n_points 20000" in str(e.value)


def test_scene_batch_has_points(sl):
    from stillleben_amd.scene_batch import SceneBatch

    assert "points" in vars(SceneBatch) and sl.ObjectPoints is op.ObjectPoints and sl.object_points is op
