"""Object points on the device (slhip_object_points_select, slhip_object_points_gather, sl.object_points, SceneBatch.points)
against the NumPy restatement tests/object_points_ref.py.  Every comparison with the reference is bit for bit -- floats as their
int32 views, every record, every point of every set."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import object_points_pictures as P
import object_points_ref as R
from stillleben_amd import _abi
from stillleben_amd import object_points as op
from stillleben_amd.object_masks import ObjectMasks
from stillleben_amd.object_stats import ObjectStats

pytestmark = pytest.mark.gpu

F = np.float32
K4 = (61.5, 60.25, 27.125, 17.75)
ALL = ("pixel", "camera", "coord", "normals", "rgb")
SHAPES = {"pixel": (2, torch.int16), "camera": (4, torch.float32), "coord": (4, torch.float32), "normals": (4, torch.float32),
          "rgb": (4, torch.uint8)}


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def device_buffers(host, dev, stats=None):
    B, S = host["stats"].shape
    H, W = host["visib"].shape[2:]
    st = host["stats"] if stats is None else stats
    stats_t = ObjectStats.from_records(torch.from_numpy(st.view(np.int32).reshape(B, S, 10).copy()).to(dev))
    om = ObjectMasks(stats_t, torch.from_numpy(host["mask_records"].view(np.int32).reshape(B, S, 14).copy()).to(dev),
                     torch.from_numpy(host["words"].view(np.int64).copy()).to(dev), torch.zeros(1, dtype=torch.int32, device=dev), (H, W))
    return types.SimpleNamespace(rgb=torch.from_numpy(host["rgb"]).to(dev), coord=torch.from_numpy(host["coord"]).to(dev),
                                 normals=torch.from_numpy(host["normals"]).to(dev), object_stats=stats_t, object_masks=om)


def visible_lists(host):
    B, S = host["stats"].shape
    return {(b, i): R.tile_order(host["visib"][b, i]) for b in range(B) for i in range(1, S) if host["visib"][b, i].any()}


@pytest.fixture(scope="module")
def pic_a(dev):
    host = P.picture_a()
    return host, device_buffers(host, dev), visible_lists(host)


@pytest.fixture(scope="module")
def pic_b(dev):
    host = P.picture_b()
    return host, device_buffers(host, dev), visible_lists(host)


def assert_same(points, sets, want):
    """records and every output of `points` against the reference's, bit for bit"""
    n = len(sets)
    got = points.records.cpu().numpy()
    assert got.shape == (n, 4) and len(points) == n
    assert np.array_equal(got, sets.view(np.int32).reshape(n, 4)), "records"
    for name in ALL:
        t = getattr(points, name)
        if name not in want:
            assert t is None, name
            continue
        g = t.cpu().numpy()
        assert g.shape == want[name].shape and g.dtype == want[name].dtype, name
        diff = (g.view(np.uint8) != want[name].view(np.uint8)).reshape(n, g.shape[1], -1).any(axis=-1)
        assert not diff.any(), "%s: %d of %d points differ, the first (set, point) %s" % (name, int(diff.sum()), diff.size,
                                                                                       tuple(np.argwhere(diff)[0]))


def reference(host, visible, **kw):
    p = op.make_params(K4, **kw)
    sets = R.select(p, host["stats"], host["mask_records"])
    return p, sets, R.gather(p, sets, visible, coord=host["coord"], normals=host["normals"], rgb=host["rgb"])


def raw_select(host, dev, capacity=None, stats=None, **kw):
    """slhip_object_points_select alone: (status, n_out, records on the host)"""
    st = host["stats"] if stats is None else stats
    B, S = st.shape
    p = op.make_params(K4, **kw).reshape(1)
    d_stats = torch.from_numpy(st.view(np.int32).reshape(B, S, 10).copy()).to(dev)
    d_masks = torch.from_numpy(host["mask_records"].view(np.int32).reshape(B, S, 14).copy()).to(dev)
    cap = B * (S - 1) if capacity is None else capacity
    out = torch.full((max(cap, 1) + 1, 4), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty((B + 1) * 8, dtype=torch.uint8, device=dev)
    n = C.c_uint64(0)
    with torch.cuda.device(dev):
        status = _abi.lib().slhip_object_points_select(p.ctypes.data, C.c_void_p(d_stats.data_ptr()), C.c_void_p(d_masks.data_ptr()), B, S,
                                                       C.c_void_p(out.data_ptr()), cap, C.c_void_p(scratch.data_ptr()), C.byref(n),
                                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return status, int(n.value), out.cpu().numpy()


POISON = 0x5B


def raw_gather(bufs, sets, dev, **kw):
    """slhip_object_points_gather alone on a record array of the caller's, all five output tensors allocated and filled with
    POISON bytes: (status, {name: numpy})"""
    p = op.make_params(K4, **kw).reshape(1)
    K, n = int(p["n_points"][0]), len(sets)
    d_sets = torch.from_numpy(sets.view(np.int32).reshape(n, 4).copy()).to(dev)
    outs = {k: torch.full((n, K, c * torch.empty(0, dtype=dt).element_size()), POISON, dtype=torch.uint8, device=dev).view(dt)
            for k, (c, dt) in SHAPES.items()}
    om = bufs.object_masks
    B, S = (int(v) for v in om.records.shape[:2])
    H, W = om.size
    src = _abi.RenderOut()
    src.d_rgb, src.d_coord, src.d_normals = bufs.rgb.data_ptr(), bufs.coord.data_ptr(), bufs.normals.data_ptr()
    out = _abi.ObjectPointsOut()
    out.d_pixel, out.d_camera, out.d_coord, out.d_normals, out.d_rgb = (outs[k].data_ptr() for k in ALL)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_object_points_gather(p.ctypes.data, C.c_void_p(d_sets.data_ptr()), n, C.byref(src),
                                                   C.c_void_p(bufs.coord.data_ptr() + 12), 4, B, W, H, C.c_void_p(om.records.data_ptr()),
                                                   C.c_void_p(om.words.data_ptr()), S, C.byref(out),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return st, {k: t.cpu().numpy() for k, t in outs.items()}


# ---- 1. the hand-painted pictures ---------------------------------------------------------------------------------------------
def test_the_pictures_are_the_hard_ones(pic_a, pic_b):
    host = pic_a[0]
    tb, st = host["mask_records"]["tile_box"], host["stats"]
    assert (tb[:, 3, 2] == (53 - 1) // 8).all() and (tb[:, 3, 3] == (37 - 1) // 8).all()      # boxes that end in the partial tiles
    assert tb[2, 4, 0] > tb[2, 4, 2]                                                          # an absent slot
    assert st[1, 1]["px_visib"] == 0 and st[1, 1]["px_all"] > 0                               # a hidden object
    assert (st[:, 5]["px_visib"] == 1).all() and (st[:, 6]["px_visib"] == 64).all()           # one pixel; one whole tile
    box, words = P.slot_words(host, 0, 6)
    assert [int(w) for w in words] == [(1 << 64) - 1]
    box, words = P.slot_words(host, 0, 1)                      # the disc hides whole tiles in the middle of slot 1's box
    filled = [int(w) != 0 for w in words]
    assert filled == [True] * 4 + [False] * 2 + [True] * 3
    r = host["mask_records"][0, 1]
    assert all(int(w) for w in host["words"][int(r["word_offset"][0]):int(r["word_offset"][0]) + 9])      # occluded, not absent
    assert (host["words"][:3] == np.uint64((1 << 64) - 1)).all()                               # nobody's words lead the pool
    box, words = P.slot_words(pic_b[0], 0, 1)
    assert len(words) == 340 and len(words) > 256 and len(words) % 256


@pytest.mark.parametrize("K", [1, 7, 64, 69, 1000])
def test_picture_a(pic_a, K):
    host, bufs, visible = pic_a
    kw = dict(n_points=K, outputs=ALL, seed=(5 << 32) | 77, scene_id_base=1000)
    p, sets, want = reference(host, visible, **kw)
    assert len(sets) == 3 * 6 - 2                               # less the hidden one and the absent one
    pts = op.extract(bufs, K4, **kw)
    assert_same(pts, sets, want)
    assert bool(pts.valid.all())
    idx = pts.index.cpu().numpy()
    for k, r in enumerate(sets):
        flat = host["visib"][int(r["scene"]), int(r["slot"])].reshape(-1)
        assert flat[idx[k]].all()                               # every point is a visible pixel of its object
        assert len(set(idx[k].tolist())) == min(K, int(r["n_visib"]))
    if K == 64:                                                 # n == K on the whole tile: point j is pixel j
        k = [(int(r["scene"]), int(r["slot"])) for r in sets].index((0, 6))
        assert pts.pixel[k].cpu().tolist() == [[40 + (j & 7), 8 + (j >> 3)] for j in range(64)]


def test_picture_b(pic_b):
    host, bufs, visible = pic_b
    n = int(host["stats"][0, 1]["px_visib"])
    for K in (1, 7, n, n + 5, 1000):
        kw = dict(n_points=K, outputs=ALL, seed=9)
        p, sets, want = reference(host, visible, **kw)
        pts = op.extract(bufs, K4, **kw)
        assert_same(pts, sets, want)
        assert len(sets) == 1 and len(torch.unique(pts.index)) == min(n, K)
        if K == n:
            assert np.array_equal(pts.pixel.cpu().numpy()[0], visible[(0, 1)])


def test_single_output_leaves_the_other_tensors_alone(pic_a, dev):
    host, bufs, visible = pic_a
    kw = dict(n_points=69, seed=4)
    p, sets, want = reference(host, visible, outputs=ALL, **kw)
    for name in ALL:
        st, got = raw_gather(bufs, sets, dev, outputs=(name,), **kw)
        assert st == 0
        assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), name
        for other in ALL:
            if other != name:
                assert (got[other].view(np.uint8) == POISON).all(), (name, other)


def test_depth_plane_with_holes(pic_a, dev):
    """depth= a stride-1 plane: zeros, NaN, +inf and negatives at sampled pixels give (0, 0, 0, 0) and valid False there; coord
    is still gathered."""
    host, bufs, visible = pic_a
    B, H, W = host["coord"].shape[:3]
    rng = np.random.default_rng(3)
    depth = (rng.random((B, H, W)) + 0.5).astype(F)
    kind = rng.integers(0, 8, (B, H, W))
    for k, v in ((1, 0.0), (2, np.nan), (3, np.inf), (4, -1.5), (5, -np.inf), (6, -0.0)):
        depth[kind == k] = v
    kw = dict(n_points=69, outputs=("pixel", "camera", "coord"), seed=11)
    p = op.make_params(K4, **kw)
    sets = R.select(p, host["stats"], host["mask_records"])
    want = R.gather(p, sets, visible, coord=host["coord"], depth=depth)
    pts = op.extract(bufs, K4, depth=torch.from_numpy(depth).to(dev), **kw)
    assert_same(pts, sets, want)
    xy = want["pixel"].astype(np.int64)
    z = depth[sets["scene"].astype(np.int64)[:, None], xy[..., 1], xy[..., 0]]
    valid = pts.valid.cpu().numpy()
    for bad in (z == 0, np.isnan(z), np.isposinf(z), z < 0):
        assert bad.any() and not valid[bad].any()
    good = np.isfinite(z) & (z > 0)
    assert np.array_equal(valid, good) and good.any()
    cam = pts.camera.cpu().numpy()
    assert (cam[~good].view(np.int32) == 0).all() and np.array_equal(cam[good][:, 2], z[good]) and (cam[good][:, 3] == 1).all()
    assert np.array_equal(pts.coord.cpu().numpy().view(np.int32), host["coord"][sets["scene"].astype(np.int64)[:, None], xy[..., 1], xy[..., 0]].view(np.int32))
    # the default plane is the w of coord, read in place
    ideal = op.extract(bufs, K4, **kw)
    assert torch.equal(ideal.camera[..., 2], ideal.coord[..., 3]) and bool(ideal.valid.all())


# ---- 2. selection -------------------------------------------------------------------------------------------------------------
def test_selection_order_and_thresholds(pic_a, dev):
    host = pic_a[0]
    stats = host["stats"].copy()
    stats[0, 2]["px_visib"], stats[0, 2]["px_all"] = 3, 12        # a quarter visible, exactly
    stats[2, 3]["px_visib"], stats[2, 3]["px_all"] = 5, 6
    everything = [(b, i) for b in range(3) for i in range(1, 7) if (b, i) not in ((1, 1), (2, 4))]
    for kw, gone in ((dict(), ()),
                     (dict(min_px=3), [(b, 5) for b in range(3)]),                       # 3 >= 3 passes, the single pixels go
                     (dict(min_px=4), [(b, 5) for b in range(3)] + [(0, 2)]),
                     (dict(min_visib_fract=0.25), ()),                                   # 3 >= 0.25 * 12 exactly
                     (dict(min_visib_fract=0.26), [(0, 2)])):
        sets = R.select(op.make_params(K4, **kw), stats, host["mask_records"])
        assert [(int(r["scene"]), int(r["slot"])) for r in sets] == [k for k in everything if k not in gone], kw
        st, n, got = raw_select(host, dev, stats=stats, **kw)
        assert st == 0 and n == len(sets) and np.array_equal(got[:n], sets.view(np.int32).reshape(-1, 4)), kw
        assert (got[n:] == -1).all()                               # nothing is written behind the last record
    # a slot with visible pixels in its statistics but no tiles gets no set
    records = host["mask_records"].copy()
    records[0, 3]["tile_box"] = (0, 0, -1, -1)
    other = {**host, "mask_records": records}
    st, n, got = raw_select(other, dev)
    assert st == 0 and n == len(everything) - 1 and (0, 3) not in {(int(a), int(b)) for a, b in got[:n, :2]}
    # a capacity one short of the need: the status, and n_out still the needed count
    st, n, got = raw_select(host, dev, capacity=15)
    assert st == _abi.OBJECT_POINTS_CAPACITY == 4 and n == 16
    assert b"holds 15 records, this batch needs 16" in _abi.lib().slhip_last_error()
    assert (got[15:] == -1).all()                                  # and nothing behind the capacity
    st, n, got = raw_select(host, dev, capacity=16)
    assert st == 0 and n == 16


def test_selection_beyond_one_wave_of_slots_and_many_scenes(dev):
    B, S = 300, 70
    stats = np.zeros((B, S), _abi.OBJECT_STATS_DTYPE)
    records = np.zeros((B, S), _abi.OBJECT_MASK_DTYPE)
    records["tile_box"] = (0, 0, -1, -1)
    where = {(0, 3), (0, 63), (0, 64), (0, 65), (0, 69), (1, 64), (1, 1), (299, 69), (150, 2)}
    for b in range(2, 290, 3):
        if not 40 <= b < 130:
            where.add((b, 1 + b % 69))
    for k in sorted(where) + [(0, 0), (5, 0)]:                     # slot 0 never
        stats[k]["px_visib"], stats[k]["px_all"] = 6 + k[0], 9 + k[0]
        records[k]["tile_box"] = (0, 0, 0, 0)
    host = {"stats": stats, "mask_records": records}
    sets = R.select(op.make_params(K4), stats, records)
    assert [(int(r["scene"]), int(r["slot"])) for r in sets] == sorted(where)
    st, n, got = raw_select(host, dev)
    assert st == 0 and n == len(where) and np.array_equal(got[:n], sets.view(np.int32).reshape(-1, 4))


def test_seeds_and_scene_ids(pic_a):
    host, bufs, visible = pic_a
    kw = dict(n_points=7, outputs=ALL)
    a, b = op.extract(bufs, K4, seed=4, **kw), op.extract(bufs, K4, seed=4, **kw)
    torch.cuda.synchronize()
    for name in ("records",) + ALL:
        assert torch.equal(getattr(a, name).view(torch.uint8), getattr(b, name).view(torch.uint8)), name      # the same seed: the same bytes
    other = op.extract(bufs, K4, seed=5, **kw)
    assert torch.equal(other.records, a.records) and not torch.equal(other.pixel, a.pixel)
    # another scene_id_base shifts the draws by scene: scene s under base 1 draws what scene s + 1 draws under base 0
    d0 = [R.draws(op.make_params(K4, n_points=7, seed=4, scene_id_base=0), s, 3) for s in range(3)]
    d1 = [R.draws(op.make_params(K4, n_points=7, seed=4, scene_id_base=1), s, 3) for s in range(3)]
    assert d1[0] == d0[1] and d1[1] == d0[2] and d1[0] != d0[0]
    shifted = op.extract(bufs, K4, seed=4, scene_id_base=1, **kw)
    p, sets, want = reference(host, visible, seed=4, scene_id_base=1, **kw)
    assert_same(shifted, sets, want)
    assert not torch.equal(shifted.pixel, a.pixel)
    assert a._keepalive[0] is bufs                                 # the inputs live as long as the outputs


# ---- 3. inconsistent and foreign records ----------------------------------------------------------------------------------------
def test_statistics_that_claim_more_pixels_than_the_words_hold(pic_a, pic_b, dev):
    for (host, _, visible), K in ((pic_a, 69), (pic_b, 1000)):
        stats = host["stats"].copy()
        stats["px_visib"] = stats["px_visib"] * 2 + (stats["px_visib"] > 0)      # 2 n + 1 for every visible slot
        bufs = device_buffers(host, dev, stats=stats)
        kw = dict(n_points=K, outputs=ALL, seed=21)
        p = op.make_params(K4, **kw)
        sets = R.select(p, stats, host["mask_records"])
        want = R.gather(p, sets, visible, coord=host["coord"], normals=host["normals"], rgb=host["rgb"])
        pts = op.extract(bufs, K4, **kw)                                         # returns: status 0
        assert_same(pts, sets, want)
        _, found = R.pixels(p, sets, visible)
        assert found.any() and not found.all()
        for name in ALL:
            assert (getattr(pts, name).cpu().numpy()[~found].view(np.uint8) == 0).all(), name      # zeros for the excess ranks


def test_records_out_of_range_give_zeros(pic_a, dev):
    host, bufs, visible = pic_a
    kw = dict(n_points=7, seed=2)
    p, sets, want = reference(host, visible, outputs=ALL, **kw)
    mine = sets[:4].copy()
    mine[1]["scene"] = 3                                            # one past the last scene
    mine[2]["slot"] = 7                                             # one past the last slot
    mine[3]["scene"], mine[3]["slot"] = 0xFFFFFFFF, 0xFFFFFFFF
    mine = np.concatenate([mine, np.array([(2, 4, 5, 0)], dtype=_abi.OBJECT_POINT_SET_DTYPE)])      # a slot without tiles
    st, got = raw_gather(bufs, mine, dev, outputs=ALL, **kw)
    assert st == 0
    for name in ALL:
        assert np.array_equal(got[name][0].view(np.uint8), want[name][0].view(np.uint8)), name
        assert (got[name][1:].view(np.uint8) == 0).all(), name


def test_argument_errors(pic_a, dev):
    host, bufs, visible = pic_a
    cpu = device_buffers(host, torch.device("cpu"))
    with pytest.raises(_abi.SlhipError) as e:
        op.extract(cpu, K4, n_points=16)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError) as e:
        op.extract(bufs, K4, n_points=16, depth=torch.zeros((3, 37, 53)))
    assert "no CPU path" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        op.extract(types.SimpleNamespace(**{**vars(bufs), "object_masks": None}), K4)
    assert "object_masks=True" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        op.extract(types.SimpleNamespace(**{**vars(bufs), "normals": None}), K4, outputs=("normals",))
    assert "`normals` target was not rendered" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        op.extract(bufs, K4, n_points=0)
    only = op.extract(types.SimpleNamespace(**{**vars(bufs), "coord": None, "normals": None, "rgb": None}), K4, n_points=5, outputs="pixel")
    assert tuple(only.pixel.shape) == (16, 5, 2) and only.camera is None and only.valid is None
    empty = device_buffers(host, dev, stats=np.zeros_like(host["stats"]))
    none = op.extract(empty, K4, n_points=5)
    assert len(none) == 0 and tuple(none.pixel.shape) == (0, 5, 2) and tuple(none.index.shape) == (0, 5)


# ---- 4. a real render -----------------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS = 4, 4, (320, 240), (533.4, 533.7, 156.5, 120.6)
POINT_KW = dict(n_points=500, outputs=ALL)


@pytest.fixture(scope="module")
def rendered(sl):
    from test_gpu_synth import small_table

    batch = sl.SceneBatch(small_table(sl), N_SCENES, N_OBJ, resolution=RES, seed=(77 << 32) | 5, render_chunk=N_SCENES,
                          manual_exposure=1.0, scene_id_base=1000)
    batch.set_camera_intrinsics(*INTRINSICS)
    batch.stage()
    batch.settle(frames=5)
    batch.place(object_to_camera=True)
    bufs = batch.render(0, object_masks=True)
    pts = batch.points(bufs, **POINT_KW)
    torch.cuda.synchronize()
    om = bufs.object_masks
    S = N_OBJ + 1
    host = dict(rgb=bufs.rgb.cpu().numpy(), coord=bufs.coord.cpu().numpy(), normals=bufs.normals.cpu().numpy(),
                instance=bufs.instance.cpu().numpy()[..., 0].view(np.uint16),
                stats=bufs.object_stats.records().cpu().numpy().view(_abi.OBJECT_STATS_DTYPE).reshape(N_SCENES, S),
                mask_records=om.records.cpu().numpy().view(_abi.OBJECT_MASK_DTYPE).reshape(N_SCENES, S),
                words=om.words.cpu().numpy().view(np.uint64), o2c=batch.object_to_camera.cpu().numpy().copy())
    return batch, bufs, pts, host


def test_real_render(rendered):
    batch, bufs, pts, host = rendered
    key = _abi.view_key(5, 77, 0)
    p = op.make_params(batch.intrinsics(), seed=key, scene_id_base=1000, **POINT_KW)
    sets = R.select(p, host["stats"], host["mask_records"])
    assert len(sets) >= N_SCENES * N_OBJ // 2                      # most of the objects show
    visible = {}
    for r in sets:                                                 # the real tiles, and the instance picture says the same
        b, i = int(r["scene"]), int(r["slot"])
        visible[(b, i)] = R.words_order(*P.slot_words(host, b, i))
        assert np.array_equal(visible[(b, i)], R.tile_order(host["instance"][b] == i)), (b, i)
    want = R.gather(p, sets, visible, coord=host["coord"], normals=host["normals"], rgb=host["rgb"])
    assert_same(pts, sets, want)
    xy = pts.pixel.cpu().numpy().astype(np.int64)
    b = sets["scene"].astype(np.int64)[:, None]
    assert (host["instance"][b, xy[..., 1], xy[..., 0]] == sets["slot"][:, None]).all()       # instance at each pixel is the slot
    assert np.array_equal(pts.coord.cpu().numpy().view(np.int32), host["coord"][b, xy[..., 1], xy[..., 0]].view(np.int32))
    assert bool(pts.valid.all()) and torch.equal(pts.scene_global, pts.scene)
    assert torch.equal(pts.index, torch.from_numpy(xy[..., 1] * RES[0] + xy[..., 0]).to(pts.index.device))
    assert torch.equal(pts.object_to_camera.cpu(), torch.from_numpy(host["o2c"][sets["scene"].astype(np.int64), sets["slot"].astype(np.int64) - 1]))
    with pytest.raises(TypeError):
        batch.points(bufs, seed=3)                                 # the batch sets intrinsics, seed and scene ids itself


def test_camera_points_against_object_to_camera(rendered):
    """|X - (o2c [coord.xyz, 1]).x| <= 0.05 z / fx, and likewise Y: a twentieth of a pixel's footprint at the point's depth.
    The bound is derived, not measured: a wrong pixel-centre convention shows as 0.5 z / fx, ten times the bound, and float32
    rounding of metre-sized values lies orders below it."""
    batch, bufs, pts, host = rendered
    cam = pts.camera.cpu().numpy().astype(np.float64)
    xyz = pts.coord.cpu().numpy()[..., :3].astype(np.float64)
    o2c = pts.object_to_camera.cpu().numpy().astype(np.float64)
    ref = np.einsum("nij,nkj->nki", o2c[:, :, :3], xyz) + o2c[:, None, :, 3]
    fx, fy = (float(v) for v in batch.intrinsics()[:2])
    z = cam[..., 2]
    ex, ey = np.abs(cam[..., 0] - ref[..., 0]) * fx / z, np.abs(cam[..., 1] - ref[..., 1]) * fy / z
    print("camera point against object_to_camera: max |dX| fx / z = %.6f px, max |dY| fy / z = %.6f px, max |dZ| = %.3g m over %d points"
          % (ex.max(), ey.max(), np.abs(z - ref[..., 2]).max(), z.size))
    assert (ex <= 0.05).all() and (ey <= 0.05).all()


def test_sensor_depth_decides_validity(rendered, sl):
    batch, bufs, pts, host = rendered
    params = [sl.depth_sensor.make_params(INTRINSICS[0], seed=i) for i in range(N_SCENES)]
    depth = sl.depth_sensor.process_buffers(bufs, params)
    assert depth.dtype == torch.float32 and tuple(depth.shape) == (N_SCENES, RES[1], RES[0])
    sensed = batch.points(bufs, depth=depth, **POINT_KW)
    assert torch.equal(sensed.pixel, pts.pixel) and torch.equal(sensed.coord, pts.coord)      # the draw does not depend on the plane
    z = depth[sensed.scene.long()[:, None], sensed.pixel[..., 1].long(), sensed.pixel[..., 0].long()]
    assert torch.equal(sensed.valid, z != 0) and bool(sensed.valid.any()) and not bool(sensed.valid.all())
    assert torch.equal(sensed.camera[..., 2], z) and bool((sensed.camera[~sensed.valid] == 0).all())
