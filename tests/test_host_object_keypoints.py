"""Object keypoints without a device: the parameter rules, slhip_object_keypoints_fps_host against the NumPy restatement
tests/object_keypoints_ref.py (bit for bit, floats as their int32 views), the bank layout and offsets() on CPU tensors."""
import numpy as np
import pytest
import torch

import object_keypoints_ref as R
from stillleben_amd import _abi
from stillleben_amd import object_keypoints as ok

F = np.float32
K4 = (61.5, 60.25, 27.125, 17.75)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- parameters ----------------------------------------------------------------------------------------------------------------
def good():
    return ok.make_params(K4, (53, 37), 5, 3, depth_tol=0.01, mode="offset")


def test_a_good_record_passes():
    rec = ok.check_params(good())
    assert rec.dtype == _abi.OBJECT_KEYPOINT_PARAMS_DTYPE and rec.itemsize == 48
    for name, v in (("W", 1), ("H", 32768), ("n_keypoints", 1), ("n_keypoints", 32), ("n_objects", 1), ("n_objects", 64),
                    ("mode", 1), ("depth_tol", 0.0), ("cx", -3.5)):
        p = good()
        p[name] = v
        ok.check_params(p)


@pytest.mark.parametrize("name,value,word", [
    ("fx", 0.0, "fx"), ("fx", -1.0, "fx"), ("fy", 0.0, "fx"), ("fx", np.inf, "finite"), ("fy", np.nan, "finite"),
    ("cx", np.nan, "finite"), ("cy", -np.inf, "finite"),
    ("W", 0, "picture size"), ("H", 0, "picture size"), ("W", 32769, "picture size"), ("H", -4, "picture size"),
    ("n_keypoints", 0, "n_keypoints"), ("n_keypoints", 33, "n_keypoints"),
    ("n_objects", 0, "n_objects"), ("n_objects", 65, "n_objects"),
    ("mode", 2, "mode"),
    ("depth_tol", -0.001, "depth_tol"), ("depth_tol", np.nan, "depth_tol"), ("depth_tol", np.inf, "depth_tol"),
])
def test_check_params_refuses_each_broken_rule(name, value, word):
    p = good()
    p[name] = value
    with pytest.raises(_abi.SlhipError) as e:
        ok.check_params(p)
    assert word in str(e.value)


def test_check_params_refuses_null_and_unknown_mode_names():
    assert _abi.lib().slhip_object_keypoints_check_params(None) < 0
    with pytest.raises(ValueError):
        ok.make_params(K4, (53, 37), 5, 3, mode="heatmap")


# ---- FPS -----------------------------------------------------------------------------------------------------------------------
def one_class(pos, n_verts=None, vtx_base=0, m2o=None, bbox=None, pad_before=0):
    """records of a table of one class over `pos` ([n, 3])"""
    pos = np.asarray(pos, F).reshape(-1, 3)
    pool = np.zeros((pad_before + len(pos), 4), F)
    pool[:pad_before] = 1e9      # vertices of nobody: never read
    pool[pad_before:, :3] = pos
    pool[:, 3] = 1
    a = np.zeros(1, _abi.ASSET_DTYPE)
    a["mesh_to_object"][0] = np.eye(4, dtype=F).reshape(-1) if m2o is None else np.asarray(m2o, F).reshape(-1)
    lo, hi = (pos.min(0), pos.max(0)) if bbox is None and len(pos) else (np.zeros(3, F), np.zeros(3, F)) if bbox is None else bbox
    a["bbox_min"][0, :3], a["bbox_max"][0, :3] = lo, hi
    a["draw_begin"], a["draw_count"], a["n_verts"] = 0, 1, len(pos) if n_verts is None else n_verts
    t = np.zeros(1, _abi.DRAW_DTYPE)
    t["vtx_base"], t["n_verts"] = pad_before + vtx_base, a["n_verts"][0]
    return pool, a, t


def test_cube_known_answer(sl):
    """tests/fixtures/cube.glb: 24 vertices at 8 positions, all equidistant from the bbox centre.  By hand: the first keypoint
    is vertex 0 (every vertex ties, the lowest index wins); after k corners are taken every vertex of a taken corner has dmin 0
    and every other corner at least an edge, so the first 8 keypoints are the 8 corners, each by its lowest vertex index."""
    from test_oracle_synth import make_table

    table, pool, _ = make_table(sl, n_cubes=1, bunny=False)
    pos = pool.arrays()[0]
    a = table.records[0]
    base, n = int(table.templates[int(a["draw_begin"])]["vtx_base"]), int(a["n_verts"])
    assert n == 24
    pts = R.object_points(a["mesh_to_object"], pos[base:base + n])
    corners = np.unique(pts, axis=0)
    assert len(corners) == 8
    o = (a["bbox_min"][:3] + a["bbox_max"][:3]) * F(0.5)
    assert len(np.unique(R.d2(pts, o.astype(F)))) == 1                      # all equidistant, to the bit
    kps, idx = ok.fps_host(pos, table.records, table.templates, 12)
    want_k, want_i = R.fps(pos, table.records, table.templates, 12, scan=True)
    assert same_bits(kps, want_k) and same_bits(idx, want_i)
    assert idx[0, 0] == 0
    first8 = idx[0, :8]
    assert len({tuple(pts[i]) for i in first8}) == 8                         # the 8 corners
    for i in first8:                                                         # each by its lowest vertex index
        assert i == np.flatnonzero((pts == pts[i]).all(axis=1))[0]
    assert (idx[0, 8:] == 0).all()                                           # nothing is left: the rule repeats the lowest index
    assert same_bits(kps[0, :, :3], pts[idx[0]]) and (kps[0, :, 3] == 1).all()


def cloud(n=2500, seed=11):
    """a cloud with planted trouble: exact duplicates (low and high indices), pairs equidistant from the centre and from each
    other's rivals (mirror images about the centre on a dyadic grid, so the float32 distances tie to the bit)"""
    rng = np.random.default_rng(seed)
    pos = (rng.integers(-512, 513, (n, 3)) / 1024.0).astype(F)             # dyadic: sums of squares are exact in float32
    far = np.array([0.75, -0.75, 0.75], F)
    for i, sgn in ((1700, 1), (40, 1), (2300, -1), (41, -1), (900, 1)):      # the farthest position four times and its mirror
        pos[i] = far * sgn
    pos[1234], pos[77] = pos[2000], pos[2000]                                # duplicates of an ordinary vertex
    pos[5], pos[2499] = [0.75, 0.75, -0.75], [-0.75, -0.75, 0.75]            # two more corners of the same sphere
    return pos


def test_cloud_with_duplicates_and_ties():
    pos = cloud()
    m2o = np.eye(4, dtype=F)
    m2o[:3, :3] = [[0, 0.5, 0], [0, 0, 2], [1, 0, 0]]
    m2o[:3, 3] = [0.25, -0.5, 0.125]
    pool, a, t = one_class(pos, m2o=m2o, pad_before=37, bbox=(np.array([-0.125, -2.0, -0.625], F), np.array([0.625, 1.0, 0.875], F)))
    kps, idx = ok.fps_host(pool, a, t, 32)
    want_k, want_i = R.fps(pool, a, t, 32)
    scan_k, scan_i = R.fps(pool, a, t, 32, scan=True)
    assert same_bits(want_k, scan_k) and same_bits(want_i, scan_i)           # the restatement's two forms agree
    assert same_bits(idx, want_i), (idx, want_i)
    assert same_bits(kps, want_k)
    assert idx[0, 0] == 5                                                    # a planted corner, by its lowest index ...
    pts = R.object_points(m2o.reshape(-1), pool[37:])
    d0 = R.d2(pts, np.array([0.25, -0.5, 0.125], F))
    assert idx[0, 0] == np.flatnonzero(d0 == d0.max())[0] and (d0 == d0.max()).sum() >= 7       # ... among at least 7 ties
    assert len(set(idx[0].tolist())) == 32                                   # 32 distinct vertices while positions remain


def test_fewer_vertices_than_keypoints_and_none():
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 2, 0]], F)
    pool, a, t = one_class(pos)
    kps, idx = ok.fps_host(pool, a, t, 6)
    # centre (0.5, 1, 0): all four are equally far (1.25), the lowest wins; then 3 (dmin 1.25), then 1 (dmin 1, before its
    # duplicate 2); then every dmin is 0 and the lowest index repeats
    assert idx.tolist() == [[0, 3, 1, 0, 0, 0]]
    assert same_bits(kps[0, :, :3], pos[idx[0]])
    want = R.fps(pool, a, t, 6, scan=True)
    assert same_bits(kps, want[0]) and same_bits(idx, want[1])
    # no vertices: every keypoint is the bbox centre, every index -1 -- by n_verts, by draw_count, by a template outside the table
    lo, hi = np.array([-1, 2, 0.5], F), np.array([3, 4, 0.75], F)
    for change in ("n_verts", "draw_count", "draw_begin", "past_the_pool"):
        pool, a, t = one_class(pos, bbox=(lo, hi))
        if change == "past_the_pool":
            t["vtx_base"] = 1
        else:
            a[change] = 7 if change == "draw_begin" else 0
        kps, idx = ok.fps_host(pool, a, t, 3)
        assert (idx == -1).all() and same_bits(kps[0], np.tile(np.array([1, 3, 0.625, 1], F), (3, 1))), change
        want = R.fps(pool, a, t, 3)
        assert same_bits(kps, want[0]) and same_bits(idx, want[1])


def test_a_nan_vertex_never_wins():
    pos = np.array([[np.nan, 0, 0], [0.5, 0, 0], [np.inf, 0, 0], [-1, 0, 0]], F)
    pool, a, t = one_class(pos, bbox=(np.zeros(3, F), np.zeros(3, F)))
    kps, idx = ok.fps_host(pool, a, t, 3)
    # vertex 0 is NaN, vertex 2 becomes NaN in the matrix product (0 * inf): neither ever wins.  Vertex 3 is the
    # farthest finite one, then vertex 1; then both have dmin 0 and the lowest index that is no NaN repeats
    assert idx[0].tolist() == [3, 1, 1]
    want = R.fps(pool, a, t, 3, scan=True)
    assert same_bits(idx, want[1])


def test_fps_host_refuses_bad_counts():
    pool, a, t = one_class(np.zeros((3, 3), F))
    for n in (0, 33):
        with pytest.raises(_abi.SlhipError) as e:
            ok.fps_host(pool, a, t, n)
        assert "n_fps" in str(e.value)


# ---- bank ----------------------------------------------------------------------------------------------------------------------
def test_bank_layout_and_names():
    rec = np.zeros(2, _abi.ASSET_DTYPE)
    rec["bbox_min"][:, :3] = [[-1, -2, -3], [0, 0, 0]]
    rec["bbox_max"][:, :3] = [[1, 4, 5], [2, 2, 2]]
    fps_points = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(2, 3, 4)
    b = ok.assemble_bank(rec, fps_points, center=True, corners=True)
    assert b.names == ("center", "fps0", "fps1", "fps2") + tuple("corner%d" % c for c in range(8))
    assert tuple(b.points.shape) == (2, 12, 4) and len(b) == 12 and b.index("corner0") == 4
    assert b.points[0, 0].tolist() == [0, 1, 1, 1] and b.points[1, 0].tolist() == [1, 1, 1, 1]
    assert torch.equal(b.points[:, 1:4], fps_points)
    assert b.points[0, 4].tolist() == [-1, -2, -3, 1] and b.points[0, 5].tolist() == [1, -2, -3, 1]      # corner c: bit 0 = x
    assert b.points[0, 6].tolist() == [-1, 4, -3, 1] and b.points[0, 8].tolist() == [-1, -2, 5, 1]
    assert b.points[0, 11].tolist() == [1, 4, 5, 1]
    only = ok.assemble_bank(rec, fps_points, center=False, corners=False)
    assert only.names == ("fps0", "fps1", "fps2") and torch.equal(only.points, fps_points)
    cen = ok.assemble_bank(rec, None, center=True)
    assert cen.names == ("center",) and tuple(cen.points.shape) == (2, 1, 4)
    with pytest.raises(ValueError):
        ok.assemble_bank(rec, None, center=False)
    with pytest.raises(ValueError):
        ok.assemble_bank(rec, torch.zeros((2, 30, 4)), center=True, corners=True)      # 39 > 32


# ---- offsets -------------------------------------------------------------------------------------------------------------------
def test_offsets_on_cpu_tensors():
    from stillleben_amd.object_points import ObjectPoints

    g = torch.Generator().manual_seed(3)
    camera = torch.randn((3, 4, 5, 4), generator=g)
    kps = ok.ObjectKeypoints(camera, torch.zeros((3, 4, 5, 2)), torch.zeros((3, 4, 5), dtype=torch.uint8), ok.make_params(K4, (8, 8), 5, 4))
    records = torch.tensor([[0, 1, 9, 0], [0, 4, 9, 0], [2, 2, 9, 0]], dtype=torch.int32)
    pc = torch.randn((3, 6, 4), generator=g)
    pc[..., 3] = 1
    pc[1, 2] = 0                                                             # an invalid point
    pts = ObjectPoints(records, 8, camera=pc)
    off = kps.offsets(pts)
    assert tuple(off.shape) == (3, 6, 5, 3)
    for n, (b, o) in enumerate([(0, 0), (0, 3), (2, 1)]):
        for j in range(6):
            want = camera[b, o, :, :3] - pc[n, j, :3]
            if n == 1 and j == 2:
                want = torch.zeros_like(want)
            assert torch.equal(off[n, j], want), (n, j)
    # a later render chunk: scene_global pairs with scene0
    pts.scene_global = pts.scene + 10
    kps.scene0 = 10
    assert torch.equal(kps.offsets(pts), off)
    with pytest.raises(RuntimeError):
        kps.offsets(ObjectPoints(records, 8))


def test_host_tensors_are_refused():
    o2c = torch.zeros((1, 2, 3, 4))
    with pytest.raises(_abi.SlhipError) as e:
        ok.project(o2c, torch.zeros((1, 2), dtype=torch.int32), torch.zeros((1, 3, 4)), K4, (8, 8))
    assert "no CPU path" in str(e.value)
    kps = ok.ObjectKeypoints(torch.zeros((1, 2, 3, 4)), torch.zeros((1, 2, 3, 2)), torch.zeros((1, 2, 3), dtype=torch.uint8),
                             ok.make_params(K4, (8, 8), 3, 2))
    with pytest.raises(_abi.SlhipError) as e:
        kps.field(torch.zeros((1, 8, 8), dtype=torch.int16))
    assert "no CPU path" in str(e.value)


def test_header_declares_the_entries_and_the_version_stays():
    import os

    from conftest import ROOT

    text = open(os.path.join(ROOT, "include", "slhip.h")).read()
    for name in ("check_params", "fps_bytes", "fps", "fps_host", "project", "field", "timing_enable", "timings"):
        assert "int slhip_object_keypoints_%s(" % name in text, name
        assert hasattr(_abi.lib(), "slhip_object_keypoints_%s" % name), name
    assert "#define SLHIP_ABI_VERSION 5 " in text and _abi.ABI_VERSION == 5
