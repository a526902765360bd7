"""Object regions without a device: the parameter rules, slhip_object_regions_centres_host, _vertices_host and _label_host
against the NumPy restatement tests/object_regions_ref.py (bit for bit, floats as their integer views), and known answers that
do not go through the restatement: on a dyadic grid the squared distances are exact, so a float64 brute force decides."""
import numpy as np
import pytest
import torch

import object_regions_ref as R
from stillleben_amd import _abi
from stillleben_amd import object_keypoints as ok
from stillleben_amd import object_regions as og
from test_host_object_keypoints import cloud

F = np.float32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the pool ------------------------------------------------------------------------------------------------------------------
def fps_pool():
    """The pool of the keypoints' device test, rebuilt: four classes with 0, 1, 70 and 2 500 vertices in one pool, each at its
    own non-zero vtx_base with vertices of nobody between them, each under its own non-identity mesh_to_object."""
    rng = np.random.default_rng(4)
    small = (rng.integers(-64, 65, (70, 3)) / 32.0).astype(F)
    small[66], small[3] = [2.5, -2.5, 2.5], [2.5, -2.5, 2.5]
    small[69] = [-2.5, 2.5, -2.5]
    parts = [(13, np.zeros((0, 3), F)), (5, np.array([[0.5, -1.0, 2.0]], F)), (3, small), (11, cloud())]
    pos, assets, templates = [], np.zeros(4, _abi.ASSET_DTYPE), np.zeros(5, _abi.DRAW_DTYPE)
    at = 0
    for c, (pad, p) in enumerate(parts):
        pos.append(np.full((pad, 3), 1e9, F))
        at += pad
        m = np.eye(4, dtype=F)
        m[:3, :3] = [[[0, 0.5, 0], [0, 0, 2], [1, 0, 0]], [[1, 0, 0], [0, 0, -1], [0, 1, 0]], [[0.5, 0, 0], [0, 2, 0], [0, 0, 1]],
                     [[0, 0.5, 0], [0, 0, 2], [1, 0, 0]]][c]
        m[:3, 3] = [0.25, -0.5, 0.125]
        assets[c]["mesh_to_object"] = m.reshape(-1)
        assets[c]["bbox_min"][:3], assets[c]["bbox_max"][:3] = m[:3, 3] - F(1.5), m[:3, 3] + F(1.5)
        assets[c]["draw_begin"], assets[c]["draw_count"], assets[c]["n_verts"] = c + 1, 1, len(p)      # template 0 is nobody's
        templates[c + 1]["vtx_base"], templates[c + 1]["n_verts"] = at, len(p)
        pos.append(p)
        at += len(p)
    pos.append(np.full((9, 3), 1e9, F))
    pos = np.concatenate(pos)
    return np.concatenate([pos, np.ones((len(pos), 1), F)], axis=1).astype(F), assets, templates


POOL_COUNTS = (0, 1, 70, 2500)
_REF = {}


def pool_reference(n_regions):
    """(pool, assets, templates, centres, vertex, vertex_region, count, extent) of the restatement, computed once per R"""
    if n_regions not in _REF:
        pool, assets, templates = fps_pool()
        cen, vertex = R.centres(pool, assets, templates, n_regions)
        _REF[n_regions] = (pool, assets, templates, cen, vertex) + R.vertices(pool, assets, templates, cen)
    return _REF[n_regions]


# ---- the label case ------------------------------------------------------------------------------------------------------------
LN, LH, LW, LO, LA = 3, 5, 37, 3, 4
LABEL_CLASSES = np.array([[0, 1, 2], [3, -1, 1], [2, LA, 0]], np.int32)      # one object of class -1, one of class A


def label_case(n_regions, seed=5):
    """3 pictures of 5 x 37 (odd, ragged against any vector width) with 3 objects over a bank of 4 classes.  Every pixel draws
    its instance from {0, -1, 1, 2, 3, O + 1}, so the classes of a picture meet inside every wave; NaN and +-inf sit in x, y and
    z separately, under pixels that would otherwise get a region; w is NaN in places (it is not read).  With R >= 8, class 1
    holds a duplicated centre (5 = 2) with a pixel exactly on it, and class 2 an equidistant pair (3 and 7) with a pixel exactly
    midway and every other centre farther away."""
    rng = np.random.default_rng(seed + n_regions)
    bank = np.ones((LA, n_regions, 4), F)
    bank[..., :3] = rng.integers(-64, 65, (LA, n_regions, 3)) / 32.0
    inst = rng.choice(np.array([0, 0, -1, 1, 2, 3, 1, 2, 3, LO + 1], np.int16), (LN, LH, LW))
    coord = rng.uniform(-2.0, 2.0, (LN, LH, LW, 4)).astype(F)
    coord[:, ::2, ::3, 3] = np.nan
    for (n, y, x), (axis, value) in zip([(0, 1, 3), (0, 2, 5), (0, 3, 7), (2, 4, 36), (2, 0, 0), (2, 2, 18)],
                                        [(0, np.nan), (1, np.inf), (2, -np.inf), (0, np.inf), (1, np.nan), (2, np.nan)]):
        inst[n, y, x] = 1 if n == 0 else 3      # objects with a class inside the bank
        coord[n, y, x, axis] = value
    if n_regions >= 8:
        bank[1, 5] = bank[1, 2]
        x = bank[2, :, 0]
        bank[2, :, 0] = np.where(x < 0, -1.0, 1.0) * (1.0 + np.abs(x) / 2.0)      # |x| >= 1: farther than the pair below
        bank[2, 3, :3], bank[2, 7, :3] = [-0.5, 0, 0], [0.5, 0, 0]
        inst[0, 0, 0], coord[0, 0, 0, :3] = 2, bank[1, 2, :3]
        inst[0, 0, 1], coord[0, 0, 1, :3] = 3, [0.0, 0.25, 0.0]
    return inst, coord, LABEL_CLASSES, bank


_LABEL_REF = {}


def label_reference(n_regions):
    """the case and the restatement's (region, local, histogram), computed once per R"""
    if n_regions not in _LABEL_REF:
        case = label_case(n_regions)
        want = R.label(*case)
        region = want[0]
        inst, coord = case[0], case[1]
        assert (region[(inst < 1) | (inst > LO)] == 255).all()
        assert (region[1][inst[1] == 2] == 255).all() and (region[2][inst[2] == 2] == 255).all()      # classes -1 and A
        for n, y, x in [(0, 1, 3), (0, 2, 5), (0, 3, 7), (2, 4, 36), (2, 0, 0), (2, 2, 18)]:
            assert region[n, y, x] == 255 and not want[1][n, y, x].any()
        assert (region != 255).sum() > 150 and (region[region != 255] < n_regions).all()
        if n_regions >= 8:
            assert region[0, 0, 0] == 2 and region[0, 0, 1] == 3 and want[1][0, 0, 0].tolist() == [0, 0, 0, 0]
        assert np.array_equal(want[2].reshape(-1), np.bincount(
            ((np.arange(LN)[:, None, None] * LO + inst.astype(np.int64) - 1) * n_regions + region)[region != 255],
            minlength=LN * LO * n_regions))
        _LABEL_REF[n_regions] = case + want
    return _LABEL_REF[n_regions]


# ---- bank ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_regions", [1, 8, 255])
def test_bank_host_against_the_restatement(n_regions):
    pool, assets, templates, cen, vertex, vr, count, extent = pool_reference(n_regions)
    got_c, got_v = og.centres_host(pool, assets, templates, n_regions)
    assert same_bits(got_v, vertex) and same_bits(got_c, cen)
    got_vr, got_n, got_e = og.vertices_host(pool, assets, templates, got_c)
    assert same_bits(got_vr, vr) and same_bits(got_n, count) and same_bits(got_e, extent)
    assert got_n.sum(axis=1).tolist() == list(POOL_COUNTS)
    assert (got_vr != 255).sum() == sum(POOL_COUNTS) and (got_vr[:13] == 255).all() and (got_vr[-9:] == 255).all()
    assert not got_e[got_n == 0].any()


def shared_pool():
    """100 vertices under three classes whose ranges overlap: [0, 60), [40, 100) and [10, 50), each under its own scale"""
    rng = np.random.default_rng(9)
    pool = np.ones((100, 4), F)
    pool[:, :3] = rng.integers(-64, 65, (100, 3)) / 32.0
    assets, templates = np.zeros(3, _abi.ASSET_DTYPE), np.zeros(3, _abi.DRAW_DTYPE)
    for c, (lo, hi) in enumerate(((0, 60), (40, 100), (10, 50))):
        assets[c]["mesh_to_object"] = (np.eye(4, dtype=F) * F(1 + c)).reshape(-1)
        assets[c]["bbox_min"][:3], assets[c]["bbox_max"][:3] = -2.0 * (1 + c), 2.0 * (1 + c)
        assets[c]["draw_begin"], assets[c]["draw_count"], assets[c]["n_verts"] = c, 1, hi - lo
        templates[c]["vtx_base"], templates[c]["n_verts"] = lo, hi - lo
    return pool, assets, templates


def test_a_shared_vertex_carries_the_region_of_its_highest_class():
    pool, assets, templates = shared_pool()
    cen, _ = og.centres_host(pool, assets, templates, 5)
    vr, count, extent = og.vertices_host(pool, assets, templates, cen)
    want = R.vertices(pool, assets, templates, cen)
    assert same_bits(vr, want[0]) and same_bits(count, want[1]) and same_bits(extent, want[2])
    assert count.sum(axis=1).tolist() == [60, 60, 40]                        # count and extent take every vertex of a class
    import object_keypoints_ref as K

    for c, (lo, hi) in ((0, (0, 10)), (2, (10, 50)), (1, (50, 100))):        # the class that labels each stretch
        pts = K.object_points(assets[c]["mesh_to_object"], pool[lo:hi])
        assert np.array_equal(vr[lo:hi], R.nearest(pts, cen[c]).astype(np.uint8)), c


def test_the_first_32_centres_are_the_keypoint_fps():
    pool, assets, templates = fps_pool()
    cen, vertex = og.centres_host(pool, assets, templates, 32)
    kps, idx = ok.fps_host(pool, assets, templates, 32)
    assert same_bits(cen, kps) and same_bits(vertex, idx)
    more, more_v = og.centres_host(pool, assets, templates, 100)
    assert same_bits(more[:, :32], kps) and same_bits(more_v[:, :32], idx)


def test_extent_bounds_its_members():
    pool, assets, templates, cen, vertex, vr, count, extent = pool_reference(8)
    import object_keypoints_ref as K

    for c in (2, 3):
        base, n = K.class_vertices(assets[c], templates, len(pool))
        pts = K.object_points(assets[c]["mesh_to_object"], pool[base:base + n])
        for r in range(8):
            members = pts[vr[base:base + n] == r]
            assert len(members) == count[c, r] > 0
            d2 = R.local_of(members, cen[c, r, :3])[:, 3]
            assert extent[c, r, 3] == d2.max()      # >= every member's, equal to one's


@pytest.mark.parametrize("n_regions", [1, 63, 64, 65, 255])
def test_label_host_against_the_restatement(n_regions):
    inst, coord, classes, bank, region, local, hist = label_reference(n_regions)
    got = og.label_host(inst, coord, classes, bank, local=True, histogram=True)
    assert same_bits(got[0], region) and same_bits(got[1], local) and same_bits(got[2], hist)
    only = og.label_host(inst, coord, classes, bank)
    assert same_bits(only[0], region) and only[1] is None and only[2] is None
    # the asset of slhip_synth_object records, read in place
    objs = np.zeros((LN, LO), _abi.SYNTH_OBJECT_DTYPE)
    objs["asset"], objs["instance_index"], objs["metallic"] = classes.view(np.uint32), 0x7fffffff, np.nan
    strided = og.label_host(inst, coord, objs.view(np.int32).reshape(LN, LO, 4), bank, histogram=True, class_stride=4)
    assert same_bits(strided[0], region) and same_bits(strided[2], hist)


def test_label_host_under_the_centres_of_the_pool():
    """the label case's pictures under the FPS centres of the four-class pool (class 0 has no vertices: eight bbox centres)"""
    inst, coord, classes, _ = label_case(8)
    pool, assets, templates, cen = pool_reference(8)[:4]
    got = og.label_host(inst, coord, classes, cen, local=True, histogram=True)
    want = R.label(inst, coord, classes, cen)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and same_bits(got[2], want[2])
    of_class_0 = got[0][0][inst[0] == 1]                                     # eight identical centres: the lowest index
    assert set(np.unique(of_class_0).tolist()) == {0, 255} and (of_class_0 == 255).sum() == 3      # (255: the three planted non-finite pixels)


# ---- known answers that do not go through the restatement ----------------------------------------------------------------------
def test_label_equals_a_float64_brute_force_on_a_dyadic_grid():
    """Coordinates and centres are multiples of 1/32 with |v| <= 4: every difference, square and sum is exact in float32 and in
    float64, so the label must equal the float64 argmin with lowest-index ties on every pixel."""
    rng = np.random.default_rng(17)
    N, H, W, O, A, Rn = 2, 16, 23, 3, 4, 16
    bank = np.ones((A, Rn, 4), F)
    bank[..., :3] = rng.integers(-128, 129, (A, Rn, 3)) / 32.0
    bank[1, 9] = bank[1, 4]                                                  # two identical centres
    bank[2, :, 0] = np.where(bank[2, :, 0] < 0, -1.0, 1.0) * (2.0 + np.floor(np.abs(bank[2, :, 0]) * 16) / 32)
    bank[2, 3, :3], bank[2, 7, :3] = [-0.5, 1.0, 0.25], [0.5, 1.0, 0.25]     # an equidistant pair, every other centre farther
    classes = np.array([[0, 1, 2], [2, 3, 1]], np.int32)
    inst = rng.integers(1, O + 1, (N, H, W)).astype(np.int16)
    coord = np.zeros((N, H, W, 4), F)
    coord[..., :3] = rng.integers(-128, 129, (N, H, W, 3)) / 32.0
    coord[..., :3][rng.random((N, H, W)) < 0.3] = 0                          # many pixels on a coarse sub-grid: real ties
    coord[..., :3] = np.where(rng.random((N, H, W, 1)) < 0.3, np.round(coord[..., :3] * 2) / 2, coord[..., :3])
    for r in range(Rn):                                                      # a pixel on every centre of class 1 ...
        inst[0, 0, r], coord[0, 0, r, :3] = 2, bank[1, r, :3]
    inst[0, 1, 0], coord[0, 1, 0, :3] = 3, [0.0, 1.5, 0.25]                  # ... and one midway between 3 and 7 of class 2
    region, local, hist = og.label_host(inst, coord, classes, bank, local=True, histogram=True)
    cls = classes[np.arange(N)[:, None, None], inst.astype(np.int64) - 1]
    d = coord[..., None, :3].astype(np.float64) - bank[cls][..., :3].astype(np.float64)      # [N, H, W, R, 3]
    d2 = (d * d).sum(axis=-1)
    want = d2.argmin(axis=-1)                                                # the first of the minima
    assert np.array_equal(region, want.astype(np.uint8))
    assert (np.sort(d2, axis=-1)[..., 0] == np.sort(d2, axis=-1)[..., 1]).sum() >= 5       # ties do occur
    assert region[0, 0, :Rn].tolist() == [r if r != 9 else 4 for r in range(Rn)]             # on a centre: that centre, the lower twin
    assert region[0, 1, 0] == 3 and d2[0, 1, 0, 3] == d2[0, 1, 0, 7] == d2[0, 1, 0].min()
    assert np.array_equal(local[..., 3].astype(np.float64), d2.min(axis=-1))
    assert hist.sum() == N * H * W


# ---- parameters ----------------------------------------------------------------------------------------------------------------
def good():
    return og.make_params((53, 37), 2, 3, 64, 4, local=True, histogram=True)


def test_a_good_record_passes():
    rec = og.check_params(good())
    assert rec.dtype == _abi.OBJECT_REGION_PARAMS_DTYPE and rec.itemsize == 32
    for name, v in (("W", 1), ("H", 32768), ("n_regions", 1), ("n_regions", 255), ("n_objects", 1), ("n_objects", 64),
                    ("n_images", 0), ("n_assets", 1024), ("outputs", 0)):
        p = good()
        p[name] = v
        og.check_params(p)


@pytest.mark.parametrize("name,value,word", [
    ("W", 0, "picture size"), ("H", 0, "picture size"), ("W", 32769, "picture size"), ("H", -4, "picture size"),
    ("n_images", 0x7fffffff, "2^32"), ("n_objects", 0, "n_objects"), ("n_objects", 65, "n_objects"),
    ("n_regions", 0, "n_regions"), ("n_regions", 256, "n_regions"), ("n_assets", 0, "n_assets"), ("n_assets", 1025, "n_assets"),
    ("outputs", 4, "outputs"),
])
def test_check_params_refuses_each_broken_rule(name, value, word):
    p = good()
    p[name] = value
    with pytest.raises(_abi.SlhipError) as e:
        og.check_params(p)
    assert word in str(e.value)
    assert _abi.lib().slhip_object_regions_check_params(None) < 0


POISON = 0x5B


def test_refused_calls_touch_nothing():
    L = _abi.lib()
    inst, coord, classes, bank = label_case(8)
    region, local = np.full((LN, LH, LW), POISON, np.uint8), np.full((LN, LH, LW, 4 * 4), POISON, np.uint8)
    hist = np.full((LN, LO, 8 * 4), POISON, np.uint8)
    ptr = dict(inst=inst.ctypes.data, coord=coord.ctypes.data, classes=classes.ctypes.data, bank=bank.ctypes.data,
               region=region.ctypes.data, local=local.ctypes.data, hist=hist.ctypes.data)

    def call(p, stride=1, **null):
        a = dict(ptr, **{k: None for k in null})
        return L.slhip_object_regions_label_host(p.reshape(1).ctypes.data, a["inst"], a["coord"], a["classes"], stride, a["bank"],
                                                 a["region"], a["local"], a["hist"])

    p = og.make_params((LW, LH), LN, LO, 8, LA, local=True, histogram=True)
    for change in (dict(n_regions=0), dict(n_regions=256), dict(n_objects=65), dict(W=0), dict(H=40000), dict(outputs=8)):
        q = p.copy()
        for k, v in change.items():
            q[k] = v
        assert call(q) < 0 and L.slhip_last_error(), change
    for null in ("inst", "coord", "classes", "bank", "region", "local", "hist"):
        assert call(p, **{null: True}) < 0, null
    assert call(p, stride=0) < 0
    assert (region == POISON).all() and (local == POISON).all() and (hist == POISON).all()
    assert call(p) == 0 and not (region == POISON).all()      # the same call with nothing wrong runs
    # the bank entries
    pool, assets, templates = fps_pool()
    for n in (0, 256):
        with pytest.raises(_abi.SlhipError) as e:
            og.centres_host(pool, assets, templates, n)
        assert "n_regions" in str(e.value)
    cen = np.full((4, 8, 4), 7.0, F)
    vr, count, extent = np.full(len(pool), POISON, np.uint8), np.full((4, 8), POISON, np.uint8), np.full((4, 8, 16), POISON, np.uint8)
    args = [pool.ctypes.data, len(pool), assets.ctypes.data, 4, templates.ctypes.data, len(templates), cen.ctypes.data, 8, vr.ctypes.data,
            count.ctypes.data, extent.ctypes.data]
    for i, v in ((2, None), (6, None), (8, None), (9, None), (10, None), (3, 0), (3, 1025), (7, 0), (7, 256)):
        bad = list(args)
        bad[i] = v
        assert L.slhip_object_regions_vertices_host(*bad) < 0, i
    assert (vr == POISON).all() and (count == POISON).all() and (extent == POISON).all()


def test_host_tensors_are_refused():
    inst, coord = torch.zeros((1, 4, 4), dtype=torch.int16), torch.zeros((1, 4, 4, 4))
    with pytest.raises(_abi.SlhipError) as e:
        og.label(inst, coord, torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 3, 4)))
    assert "no CPU path" in str(e.value)
    reg = og.ObjectRegions(torch.full((2, 3, 4), 255, dtype=torch.uint8), histogram=torch.tensor([[[0, 3]]], dtype=torch.int32))
    assert reg.visible.tolist() == [[[False, True]]]


def test_header_declares_the_entries_and_the_version_stays():
    import os

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "slhip.h")).read()
    for name in ("check_params", "centres_bytes", "centres", "centres_host", "vertices", "vertices_host", "label", "label_host",
                 "timing_enable", "timings"):
        assert "int slhip_object_regions_%s(" % name in text, name
        assert hasattr(_abi.lib(), "slhip_object_regions_%s" % name), name
    assert "#define SLHIP_ABI_VERSION 5 " in text and _abi.ABI_VERSION == 5
    assert "#define SLHIP_REGIONS_MAX 255" in text and "#define SLHIP_REGION_NONE 255" in text
