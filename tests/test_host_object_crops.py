"""Host tests of the object crops: every rule of slhip_object_crops_check_params, the record layout against include/slhip.h,
the known answers of the NumPy restatement (tests/object_crops_ref.py, the reference the GPU tests compare the kernels against)
and the ObjectCrops container.  No GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

import object_crops_ref as R
from conftest import ROOT
from stillleben_amd import _abi
from stillleben_amd import object_crops as oc
from test_host_environment import philox4x32_10, u01

F = np.float32
K = (533.389, 533.7435, 156.49345, 120.65545)


def stats_array(B, S):
    s = np.zeros((B, S), _abi.OBJECT_STATS_DTYPE)
    s["bbox_visib"] = -1
    s["bbox_obj"] = -1
    return s


def put(s, b, i, box, px_visib=None, px_all=None, box_obj=None):
    s[b, i]["bbox_visib"] = box
    s[b, i]["bbox_obj"] = box if box_obj is None else box_obj
    s[b, i]["px_visib"] = box[2] * box[3] if px_visib is None else px_visib
    s[b, i]["px_all"] = s[b, i]["px_visib"] if px_all is None else px_all


@pytest.mark.parametrize("change,message", [
    (dict(size=0), "size 0 must be in [1, 1024]"),
    (dict(size=1025), "size 1025 must be in [1, 1024]"),
    (dict(pad=0.0), "pad 0 must be positive"),
    (dict(pad=-1.0), "pad -1 must be positive"),
    (dict(pad=float("nan")), "must be positive and finite"),
    (dict(pad=float("inf")), "must be positive and finite"),
    (dict(jitter_scale=1.0), "jitter_scale 1 must be in [0, 1)"),
    (dict(jitter_scale=-0.1), "jitter_scale -0.1 must be in [0, 1)"),
    (dict(jitter_shift=1.5), "jitter_shift 1.5 must be in [0, 1]"),
    (dict(jitter_shift=-0.5), "jitter_shift -0.5 must be in [0, 1]"),
    (dict(min_px=0), "min_px 0 must be at least 1"),
    (dict(min_visib_fract=1.25), "min_visib_fract 1.25 must be in [0, 1]"),
    (dict(min_visib_fract=-0.25), "min_visib_fract -0.25 must be in [0, 1]"),
    (dict(min_visib_fract=float("nan")), "min_visib_fract nan must be in [0, 1]"),
    (dict(outputs=()), "outputs 0x0 must name at least one"),
])
def test_check_params_rules(change, message):
    p = oc.make_params(K, **change)
    with pytest.raises(_abi.SlhipError) as e:
        oc.check_params(p, 320, 240)
    assert message in str(e.value)


@pytest.mark.parametrize("field,value,message", [
    ("box", 2, "box 2 (0: bbox_visib, 1: bbox_obj)"),
    ("outputs", 32, "outputs 0x20 must name at least one"),
    ("isolate", 2, "isolate 2 must be 0 or 1"),
    ("fx", 0.0, "fx and fy must be positive"),
    ("fy", -3.0, "fx and fy must be positive"),
    ("cx", np.inf, "all four finite"),
    ("cy", np.nan, "all four finite"),
])
def test_check_params_rules_of_the_raw_record(field, value, message):
    """The rules make_params cannot break: set in the record itself."""
    p = oc.make_params(K)
    p[field] = value
    with pytest.raises(_abi.SlhipError) as e:
        oc.check_params(p, 320, 240)
    assert message in str(e.value)


def test_check_params_accepts_the_limits_and_refuses_bad_pictures():
    for kw in (dict(size=1), dict(size=1024), dict(jitter_scale=0.999), dict(jitter_shift=1.0), dict(min_visib_fract=1.0),
               dict(outputs=("rgb", "coord", "normals", "instance", "mask")), dict(box="obj", isolate=False)):
        oc.check_params(oc.make_params(K, **kw), 320, 240)
    for W, H in ((0, 240), (320, -1)):
        with pytest.raises(_abi.SlhipError) as e:
            oc.check_params(oc.make_params(K), W, H)
        assert "bad picture size" in str(e.value)
    L = _abi.lib()
    assert L.slhip_object_crops_check_params(None, 320, 240) < 0
    with pytest.raises(ValueError):
        oc.make_params(K, box="amodal")
    with pytest.raises(ValueError):
        oc.make_params(K, outputs=("rgb", "depth"))


def test_null_arguments_are_refused_without_a_device():
    """select and gather check their parameters and pointers before anything touches a device."""
    import ctypes as C

    L = _abi.lib()
    bad = oc.make_params(K, size=0).reshape(1)
    n = C.c_uint64(7)
    assert L.slhip_object_crops_select(bad.ctypes.data, None, 1, 2, 8, 8, None, 0, None, C.byref(n), None) < 0
    assert b"size 0" in L.slhip_last_error()
    good = oc.make_params(K).reshape(1)
    assert L.slhip_object_crops_select(good.ctypes.data, None, 1, 2, 8, 8, None, 0, None, C.byref(n), None) < 0
    assert b"null argument" in L.slhip_last_error()
    assert L.slhip_object_crops_gather(bad.ctypes.data, None, 1, None, 1, 8, 8, None, None, 2, None, None) < 0
    assert L.slhip_object_crops_gather(good.ctypes.data, None, 0, None, 1, 8, 8, None, None, 2, None, None) == 0   # n_crops == 0
    assert L.slhip_object_crops_gather(good.ctypes.data, None, 1, None, 1, 8, 8, None, None, 2, None, None) < 0
    ms = (C.c_float * 2)()
    assert L.slhip_object_crops_timings(C.byref(ms)) < 0 and b"no timed calls" in L.slhip_last_error()
    nb = C.c_uint64(0)
    assert L.slhip_object_crops_scratch_bytes(300, C.byref(nb)) == 0 and nb.value == 301 * 8


def test_abi_layout_matches_the_header():
    src = open(os.path.join(ROOT, "stillleben_amd", "csrc", "slhip_object_crops.hip")).read()
    sizes = {n: int(v) for n, v in re.findall(r"static_assert\(sizeof\((slhip_\w+)\) == (\d+)", src)}
    assert sizes["slhip_object_crop_params"] == _abi.OBJECT_CROP_PARAMS_DTYPE.itemsize == 64
    assert sizes["slhip_object_crop"] == _abi.OBJECT_CROP_DTYPE.itemsize == 48
    hdr = open(os.path.join(ROOT, "include", "slhip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} slhip_object_crop_params;", hdr).group(1)
    names = [n for n in re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))]
    assert names == list(_abi.OBJECT_CROP_PARAMS_DTYPE.names)
    assert re.search(r"#define SLHIP_OBJECT_CROPS_CAPACITY\s+3\b", hdr) and _abi.OBJECT_CROPS_CAPACITY == 3
    assert re.search(r"#define SLHIP_ABI_VERSION 5\b", hdr) and _abi.ABI_VERSION == 5
    for name, bit in oc.OUTPUTS.items():
        assert re.search(r"#define SLHIP_CROP_%s\s+%du\b" % (name.upper(), bit), hdr), name


def test_stream_5_is_a_stream_of_its_own():
    assert _abi.SYNTH_STREAM_CROP == R.STREAM_CROP == 5
    assert "Stream 5, crop jitter" in open(os.path.join(ROOT, "include", "slhip.h")).read()
    key = (12345, 77)
    for sid, idx in ((0, 1), (41, 3), (0xFFFFFFFF, 64)):
        draws = [tuple(philox4x32_10((sid, s, idx, 0x51DE5EED), key)) for s in range(6)]
        assert len(set(draws)) == 6
        assert all(set(draws[5]).isdisjoint(d) for d in draws[:5])
    p = oc.make_params(K, seed=(77 << 32) | 12345, scene_id_base=40)
    x = philox4x32_10((41, 5, 3, 0x51DE5EED), key)
    u = R.uniforms(p, 1, 3)
    assert u == tuple(u01(w) for w in x[:3])
    assert R.uniforms(oc.make_params(K, seed=key, scene_id_base=40), 1, 3) == u       # the key as a (lo, hi) pair


@pytest.mark.parametrize("N,x,y", [(16, 7, 3), (128, 100, 50), (24, 0, 0)])
def test_identity_window_has_step_one(N, x, y):
    s = stats_array(1, 2)
    put(s, 0, 1, (x, y, N, N))
    for seed in (0, 99):                 # the draw is made, its terms are exactly 0
        p = oc.make_params(K, size=N, pad=1.0, seed=seed)
        r = R.select(p, s)
        assert len(r) == 1
        r = r[0]
        assert r["step"] == F(1.0) and r["side"] == F(N) and r["x0"] == F(x) and r["y0"] == F(y)
        fx, fy, cx, cy = (F(v) for v in K)
        assert list(r["K"]) == [fx, fy, cx - F(x), cy - F(y)]


def test_jitter_moves_the_window_within_its_bounds():
    s = stats_array(4, 3)
    for b in range(4):
        put(s, b, 1, (40, 30, 20, 10))
        put(s, b, 2, (5, 6, 8, 24))
    p0 = oc.make_params(K, size=32, pad=1.5)
    pj = oc.make_params(K, size=32, pad=1.5, jitter_scale=0.25, jitter_shift=0.25, seed=5)
    r0, rj = R.select(p0, s), R.select(pj, s)
    assert len(r0) == len(rj) == 8
    assert len({float(v) for v in rj["side"][::2]}) == 4                  # every scene its own draw
    for a, j in zip(r0, rj):
        w, h = (20, 10) if a["slot"] == 1 else (8, 24)
        assert a["side"] == F(max(w, h)) * F(1.5)
        assert 0.75 * a["side"] <= j["side"] <= 1.25 * a["side"] and j["side"] != a["side"]
        ca, cj = (a["x0"] + F(0.5) * a["side"], a["y0"] + F(0.5) * a["side"]), (j["x0"] + F(0.5) * j["side"], j["y0"] + F(0.5) * j["side"])
        assert abs(cj[0] - ca[0]) <= 0.25 * w + 1e-3 and abs(cj[1] - ca[1]) <= 0.25 * h + 1e-3
    assert np.array_equal(R.select(pj, s), rj)                            # counter-based: the same again
    other = R.select(oc.make_params(K, size=32, pad=1.5, jitter_scale=0.25, jitter_shift=0.25, seed=6), s)
    assert not np.array_equal(other["x0"], rj["x0"])


def test_reference_order_and_eligibility():
    s = stats_array(5, 4)
    put(s, 0, 3, (1, 1, 4, 4))
    put(s, 0, 1, (2, 2, 3, 3))
    put(s, 2, 2, (0, 0, 2, 2), px_visib=3, px_all=12)                     # a quarter visible
    put(s, 4, 1, (3, 3, 2, 2), px_visib=2, px_all=2)
    put(s, 4, 3, (0, 0, 0, 0), px_visib=0, px_all=9, box_obj=(0, 0, 3, 3))  # hidden: no visible box, a whole silhouette
    s[4, 3]["bbox_visib"] = -1
    put(s, 3, 0, (0, 0, 8, 8))                                            # slot 0 never
    r = R.select(oc.make_params(K, size=8), s)
    pairs = [(int(a), int(b)) for a, b in zip(r["scene"], r["slot"])]
    assert pairs == [(0, 1), (0, 3), (2, 2), (4, 1)] and pairs == sorted(pairs)
    assert [(int(a), int(b)) for a, b in zip(*(R.select(oc.make_params(K, size=8, min_px=3), s)[k] for k in ("scene", "slot")))] \
        == [(0, 1), (0, 3), (2, 2)]
    assert [(int(a), int(b)) for a, b in zip(*(R.select(oc.make_params(K, size=8, min_visib_fract=0.5), s)[k] for k in ("scene", "slot")))] \
        == [(0, 1), (0, 3), (4, 1)]
    assert [(int(a), int(b)) for a, b in zip(*(R.select(oc.make_params(K, size=8, min_visib_fract=0.25), s)[k] for k in ("scene", "slot")))] \
        == pairs                                                          # 3 >= 0.25 * 12 exactly
    # the whole silhouette's box, min_px = 1: the hidden object has no visible pixel, so it stays out here too
    assert len(R.select(oc.make_params(K, size=8, box="obj"), s)) == 4
    assert len(R.select(oc.make_params(K, size=8), stats_array(3, 5))) == 0


def test_reference_samplers_reproduce_the_source_at_step_one():
    rng = np.random.default_rng(11)
    B, H, W, N = 2, 20, 30, 8
    rgb = rng.integers(0, 256, (B, H, W, 4), dtype=np.uint8)
    coord = rng.standard_normal((B, H, W, 4)).astype(F)
    inst = np.zeros((B, H, W), np.uint16)
    inst[1, 5:13, 9:17] = 2
    inst[1, 5:9, 9:12] = 1
    s = stats_array(B, 3)
    put(s, 1, 2, (9, 5, N, N))
    p = oc.make_params(K, size=N, pad=1.0, outputs=("rgb", "coord", "instance", "mask"), isolate=False)
    recs = R.select(p, s)
    dense = np.zeros((B, 3, H, W), bool)
    dense[1, 2, 5:13, 9:17] = True
    out = R.gather(p, recs, rgb=rgb, coord=coord, instance=inst, dense_all=dense)
    assert np.array_equal(out["rgb"][0], rgb[1, 5:13, 9:17])
    assert np.array_equal(out["coord"][0].view(np.int32), coord[1, 5:13, 9:17].view(np.int32))
    assert np.array_equal(out["instance"][0], inst[1, 5:13, 9:17].view(np.int16))
    assert np.array_equal(out["mask"][0], np.where(inst[1, 5:13, 9:17] == 2, 3, 2))
    iso = R.gather(oc.make_params(K, size=N, pad=1.0, outputs=("coord",)), recs, coord=coord, instance=inst)["coord"][0]
    assert (iso[inst[1, 5:13, 9:17] != 2] == 0).all() and np.array_equal(iso[inst[1, 5:13, 9:17] == 2], coord[1, 5:13, 9:17][inst[1, 5:13, 9:17] == 2])
    # half a pixel to the right: the mean of two neighbours, rounded half up; beyond the border a tap counts as 0
    recs2 = recs.copy()
    recs2["x0"] = F(22.5)
    shifted = R.gather(oc.make_params(K, size=N, pad=1.0, outputs=("rgb",)), recs2, rgb=rgb)["rgb"][0]
    a, b = rgb[1, 5:13, 22:30].astype(np.int64), np.concatenate([rgb[1, 5:13, 23:30], np.zeros((8, 1, 4), np.uint8)], axis=1).astype(np.int64)
    assert np.array_equal(shifted, (a + b + 1) // 2)


def test_container_indexing_map_and_K3x3():
    n, N = 5, 4
    rec = np.zeros(n, _abi.OBJECT_CROP_DTYPE)
    rec["scene"], rec["slot"] = [0, 0, 1, 3, 3], [1, 2, 1, 2, 5]
    rec["x0"], rec["y0"], rec["side"], rec["step"] = np.arange(n), -np.arange(n), 8.0, 2.0
    rec["K"] = np.arange(4 * n).reshape(n, 4) + 0.5
    records = torch.from_numpy(rec.view(np.int32).reshape(n, 12).copy())
    mask = torch.arange(n * N * N, dtype=torch.uint8).reshape(n, N, N) & 3
    c = oc.ObjectCrops(records, N, rgb=torch.zeros((n, N, N, 4), dtype=torch.uint8), mask=mask)
    assert len(c) == n and c.scene.tolist() == [0, 0, 1, 3, 3] and c.slot.tolist() == [1, 2, 1, 2, 5]
    assert c.scene.dtype == torch.int32 and c.box.dtype == torch.float32 and tuple(c.box.shape) == (n, 4) and tuple(c.K.shape) == (n, 4)
    assert c.box[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and c.box[:, 3].tolist() == [2.0] * n
    assert c.K[2].tolist() == [8.5, 9.5, 10.5, 11.5]
    assert c.scene.data_ptr() == records.data_ptr()                       # views of the record tensor
    k = c.K3x3()
    assert tuple(k.shape) == (n, 3, 3) and k[2].tolist() == [[8.5, 0.0, 10.5], [0.0, 9.5, 11.5], [0.0, 0.0, 1.0]]
    assert c.mask_visib.dtype == torch.bool and torch.equal(c.mask_visib, (mask & 1) != 0) and torch.equal(c.mask_all, (mask & 2) != 0)
    assert c.coord is None and c.normals is None and c.instance is None
    one = c[3]
    assert int(one.scene) == 3 and int(one.slot) == 2 and tuple(one.rgb.shape) == (N, N, 4) and tuple(one.K3x3().shape) == (3, 3)
    assert int(c[-1].slot) == 5
    with pytest.raises(IndexError):
        c[5]
    with pytest.raises(TypeError):
        len(one)
    part = c[1:4]
    assert len(part) == 3 and part.slot.tolist() == [2, 1, 2] and tuple(part.mask.shape) == (3, N, N) and part.size == N
    sel = c.map(lambda t: t[c.scene == 3])
    assert len(sel) == 2 and sel.slot.tolist() == [2, 5] and sel.coord is None
    c.scene_global = c.scene + 16
    assert c[2:].scene_global.tolist() == [17, 19, 19]


def test_extract_argument_errors_need_no_device():
    """What extract refuses before it asks anything of a device: missing statistics, a target that was not rendered, tensors
    on the host."""
    B, H, W, S = 2, 8, 8, 3
    st = sl_stats(B, S)
    full = types.SimpleNamespace(rgb=torch.zeros((B, H, W, 4), dtype=torch.uint8), coord=torch.zeros((B, H, W, 4)), normals=None,
                                 instance=torch.zeros((B, H, W, 1), dtype=torch.int16), object_stats=st, object_masks=None)
    with pytest.raises(_abi.SlhipError) as e:
        oc.extract(full, K, size=8)
    assert "no CPU path" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        oc.extract(full, K, size=8, outputs=("normals",))
    assert "`normals` target was not rendered" in str(e.value)
    no_inst = types.SimpleNamespace(**{**vars(full), "instance": None})
    with pytest.raises(RuntimeError) as e:
        oc.extract(no_inst, K, size=8, outputs=("coord",))                # isolate reads the instance target
    assert "`instance` target was not rendered" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        oc.extract(types.SimpleNamespace(**{**vars(full), "object_stats": None}), K, size=8)
    assert "statistics" in str(e.value)
    with pytest.raises(_abi.SlhipError) as e:
        oc.extract(full, K, size=2000)
    assert "size 2000" in str(e.value)


def sl_stats(B, S):
    from stillleben_amd.object_stats import ObjectStats

    return ObjectStats.from_records(torch.from_numpy(stats_array(B, S).view(np.int32).reshape(B, S, 10).copy()))


def test_scene_batch_intrinsics_round_trip(sl):
    """SceneBatch.crops reads (fx, fy, cx, cy) back from the projection set_camera_intrinsics built."""
    from stillleben_amd.scene import Scene
    from stillleben_amd.scene_batch import SceneBatch

    proto = Scene((320, 240))
    proto.set_camera_intrinsics(*K)
    got = SceneBatch.intrinsics(types.SimpleNamespace(_proto=proto, resolution=(320, 240)))
    assert np.allclose(got, K, rtol=2e-6, atol=0)
    assert "crops" in vars(SceneBatch) and "SYNTH_STREAM_CROP" in vars(_abi)
