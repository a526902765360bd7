"""Object crops on the device (slhip_object_crops_select, slhip_object_crops_gather, sl.object_crops, SceneBatch.crops) against
the NumPy restatement tests/object_crops_ref.py.  Every comparison with the reference is bit for bit -- floats as their int32
views, every record, every pixel of every crop."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import object_crops_ref as R
from stillleben_amd import _abi
from stillleben_amd import object_crops as oc
from stillleben_amd.object_masks import ObjectMasks
from stillleben_amd.object_stats import ObjectStats

pytestmark = pytest.mark.gpu

F = np.float32
K = (61.5, 60.25, 27.125, 17.75)
ALL = ("rgb", "coord", "normals", "instance", "mask")


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


# ---- a hand-painted picture -------------------------------------------------------------------------------------------------
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
                        w = 0
                        for y in range(8 * ty, min(8 * ty + 8, H)):
                            for x in range(8 * tx, min(8 * tx + 8, W)):
                                if m[y, x]:
                                    w |= 1 << ((y & 7) * 8 + (x & 7))
                        words.append(w)
    return rec, np.array(words, dtype=np.uint64)


def paint(B=3, H=37, W=53, S=5):
    """Per scene: 1 a rectangle, 2 a disc in front of part of it, 3 a rectangle in the bottom right corner (the partial tiles of
    53 x 37), 4 a rectangle in the top left corner.  Scene 1: the disc hides object 1 altogether.  Scene 2: no object 4."""
    yy, xx = np.mgrid[0:H, 0:W]
    whole = np.zeros((B, S, H, W), bool)
    for b in range(B):
        if b == 1:
            whole[b, 1, 16:21, 22:27] = True
        else:
            whole[b, 1, 8 + b:21 + b, 10:26 + b] = True
        whole[b, 2] = (xx - (24 + b)) ** 2 + (yy - 18) ** 2 <= 49
        whole[b, 3, 28 - b:, 40 - 2 * b:] = True
        if b != 2:
            whole[b, 4, :4 + b, :7] = True
    inst = np.zeros((B, H, W), np.uint16)
    for i in range(1, S):
        inst[whole[:, i]] = i
    visib = np.stack([inst == i for i in range(S)], axis=1)
    visib[:, 0] = False
    return inst, visib, whole


@pytest.fixture(scope="module")
def picture(dev):
    rng = np.random.default_rng(20261018)
    inst, visib, whole = paint()
    B, H, W = inst.shape
    host = dict(rgb=rng.integers(0, 256, (B, H, W, 4), dtype=np.uint8), coord=rng.standard_normal((B, H, W, 4)).astype(F),
                normals=rng.standard_normal((B, H, W, 4)).astype(F), instance=inst, visib=visib, whole=whole,
                stats=np_stats(visib, whole))
    host["mask_records"], host["words"] = np_tiles(visib, whole)
    return host, device_buffers(host, dev)


def device_buffers(host, dev, masks=True):
    B, H, W = host["instance"].shape
    S = host["stats"].shape[1]
    stats = ObjectStats.from_records(torch.from_numpy(host["stats"].view(np.int32).reshape(B, S, 10).copy()).to(dev))
    om = None
    if masks and "words" in host:
        om = ObjectMasks(stats, torch.from_numpy(host["mask_records"].view(np.int32).reshape(B, S, 14).copy()).to(dev),
                         torch.from_numpy(host["words"].view(np.int64).copy()).to(dev), torch.zeros(1, dtype=torch.int32, device=dev),
                         (H, W))

    def up(name):
        return torch.from_numpy(host[name]).to(dev) if name in host else None

    return types.SimpleNamespace(rgb=up("rgb"), coord=up("coord"), normals=up("normals"),
                                 instance=torch.from_numpy(host["instance"].view(np.int16).reshape(B, H, W, 1).copy()).to(dev),
                                 object_stats=stats, object_masks=om)


def assert_same(crops, recs, want):
    """records and every output of `crops` against the reference's, bit for bit"""
    n = len(recs)
    got = crops.records.cpu().numpy()
    assert got.shape == (n, 12) and len(crops) == n
    assert np.array_equal(got, recs.view(np.int32).reshape(n, 12)), "records"
    assert np.array_equal(crops.K.cpu().numpy().view(np.int32), recs["K"].view(np.int32)), "K"
    for name in ALL:
        t = getattr(crops, name)
        if name not in want:
            assert t is None, name
            continue
        g = t.cpu().numpy()
        assert g.shape == want[name].shape and g.dtype == want[name].dtype, name
        assert np.array_equal(g.view(np.uint8), want[name].view(np.uint8)), \
            "%s: %d of %d values differ" % (name, int((g != want[name]).sum()), g.size)


# ---- 1. the synthetic picture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("isolate", [True, False])
@pytest.mark.parametrize("jitter", [(0.0, 0.0), (0.25, 0.25)])
@pytest.mark.parametrize("box", ["visib", "obj"])
@pytest.mark.parametrize("pad", [1.0, 1.5])
@pytest.mark.parametrize("N", [16, 24])
def test_synthetic_picture(picture, N, pad, box, jitter, isolate):
    host, bufs = picture
    kw = dict(size=N, box=box, pad=pad, jitter_scale=jitter[0], jitter_shift=jitter[1], outputs=ALL, isolate=isolate,
              seed=(5 << 32) | 77, scene_id_base=1000)
    p = oc.make_params(K, **kw)
    recs = R.select(p, host["stats"])
    assert len(recs) == 10                                    # 3 x 4 objects less the hidden one and the absent one
    if pad == 1.5:
        assert R.reaches_outside(recs, 53, 37) == (True, True, True, True)
    want = R.gather(p, recs, rgb=host["rgb"], coord=host["coord"], normals=host["normals"], instance=host["instance"],
                    dense_all=host["whole"])
    crops = oc.extract(bufs, K, **kw)
    assert_same(crops, recs, want)
    assert int(crops.mask_visib.sum()) > 0 and bool((crops.mask_all & ~crops.mask_visib).any())      # something is occluded
    assert not bool((crops.mask_visib & ~crops.mask_all).any())
    if isolate:
        assert bool((crops.coord[~crops.mask_visib] == 0).all()) and bool((crops.normals[~crops.mask_visib] == 0).all())


def test_mask_tiles_of_the_picture_are_the_hard_ones(picture):
    host, _ = picture
    tb = host["mask_records"]["tile_box"]
    assert (tb[:, 1:4, 0] > 0).any() and (tb[:, 1:4, 1] > 0).any()                 # boxes that do not start at tile 0
    assert (tb[:, 3, 2] == (53 - 1) // 8).all() and (tb[:, 3, 3] == (37 - 1) // 8).all()      # and end in the partial tiles
    assert tb[2, 4, 0] > tb[2, 4, 2]                                                # an empty slot
    assert host["stats"][1, 1]["px_visib"] == 0 and host["stats"][1, 1]["px_all"] > 0


# ---- 2. identity ------------------------------------------------------------------------------------------------------------
def test_identity(picture, dev):
    host, _ = picture
    stats = np.zeros((3, 3), _abi.OBJECT_STATS_DTYPE)
    stats["bbox_visib"] = stats["bbox_obj"] = -1
    stats[1, 2]["bbox_visib"] = stats[1, 2]["bbox_obj"] = (31, 17, 16, 16)
    stats[1, 2]["px_visib"] = stats[1, 2]["px_all"] = 256
    bufs = device_buffers({**{k: host[k] for k in ("rgb", "coord", "normals", "instance")}, "stats": stats}, dev)
    crops = oc.extract(bufs, K, size=16, pad=1.0, outputs=("rgb", "coord", "instance"), isolate=False, seed=9)
    assert len(crops) == 1 and crops.box.cpu().tolist() == [[31.0, 17.0, 16.0, 1.0]]
    assert np.array_equal(crops.K.cpu().numpy()[0], np.array([F(K[0]), F(K[1]), F(K[2]) - F(31), F(K[3]) - F(17)], F))
    assert np.array_equal(crops.rgb.cpu().numpy()[0], host["rgb"][1, 17:33, 31:47])
    assert np.array_equal(crops.coord.cpu().numpy()[0].view(np.int32), host["coord"][1, 17:33, 31:47].view(np.int32))
    assert np.array_equal(crops.instance.cpu().numpy()[0].view(np.uint16), host["instance"][1, 17:33, 31:47])


# ---- 3. selection and compaction ------------------------------------------------------------------------------------------
def made_up_stats(B, S, where):
    """where: {(scene, slot): (px_visib, px_all)}; every named slot gets a 3 x 2 box inside an 8 x 8 picture"""
    s = np.zeros((B, S), _abi.OBJECT_STATS_DTYPE)
    s["bbox_visib"] = s["bbox_obj"] = -1
    for (b, i), (pv, pa) in where.items():
        s[b, i]["bbox_visib"] = s[b, i]["bbox_obj"] = (1 + (b + i) % 4, 2 + i % 3, 3, 2)
        s[b, i]["px_visib"], s[b, i]["px_all"] = pv, pa
    return s


def tiny_buffers(stats, dev):
    B = stats.shape[0]
    rng = np.random.default_rng(B)
    return device_buffers({"instance": rng.integers(0, 3, (B, 8, 8)).astype(np.uint16), "stats": stats}, dev)


def select_only(stats, dev, capacity=None, null_records=False, **kw):
    """slhip_object_crops_select alone: (status, n_out, records on the host); `null_records`: no record array at all"""
    B, S = stats.shape
    p = oc.make_params(K, **kw).reshape(1)
    d_stats = torch.from_numpy(stats.view(np.int32).reshape(B, S, 10).copy()).to(dev)
    cap = B * (S - 1) if capacity is None else capacity
    out = torch.full((max(cap, 1) + 1, 12), -1, dtype=torch.int32, device=dev)
    scratch = torch.empty((B + 1) * 8, dtype=torch.uint8, device=dev)
    n = C.c_uint64(0)
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_object_crops_select(p.ctypes.data, C.c_void_p(d_stats.data_ptr()), B, S, 8, 8,
                                                  C.c_void_p(None if null_records else out.data_ptr()), cap, C.c_void_p(scratch.data_ptr()), C.byref(n),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return st, int(n.value), out.cpu().numpy()


def test_selection_beyond_one_wave_of_slots(dev):
    where = {(0, 3): (6, 6), (0, 63): (6, 6), (0, 64): (6, 6), (0, 65): (6, 6), (0, 69): (6, 6), (1, 64): (6, 6), (1, 1): (6, 6),
             (0, 0): (6, 6)}                                   # slot 0 never
    stats = made_up_stats(2, 70, where)
    p = oc.make_params(K, size=8, jitter_scale=0.5, jitter_shift=0.5, seed=3, outputs=("instance",))
    recs = R.select(p, stats)
    assert [(int(a), int(b)) for a, b in zip(recs["scene"], recs["slot"])] == [(0, 3), (0, 63), (0, 64), (0, 65), (0, 69), (1, 1), (1, 64)]
    crops = oc.extract(tiny_buffers(stats, dev), K, size=8, jitter_scale=0.5, jitter_shift=0.5, seed=3, outputs=("instance",))
    assert np.array_equal(crops.records.cpu().numpy(), recs.view(np.int32).reshape(-1, 12))


def test_selection_over_300_scenes(dev):
    where = {}
    for b in range(300):
        k = 0 if 40 <= b < 130 or b >= 290 else (b * 7 + b // 5) % 3           # runs of empty scenes, the last scenes among them
        for i in [(), (2,), (1, 4)][k]:
            where[(b, i)] = (6, 6)
    stats = made_up_stats(300, 5, where)
    p = oc.make_params(K, size=4, jitter_shift=1.0, seed=8, scene_id_base=7, outputs=("instance",))
    recs = R.select(p, stats)
    counts = np.bincount(recs["scene"], minlength=300)
    assert set(counts.tolist()) == {0, 1, 2} and len(recs) == len(where) and counts[40:130].sum() == 0
    bufs = tiny_buffers(stats, dev)
    crops = oc.extract(bufs, K, size=4, jitter_shift=1.0, seed=8, scene_id_base=7, outputs=("instance",))
    assert np.array_equal(crops.records.cpu().numpy(), recs.view(np.int32).reshape(-1, 12))
    pairs = list(zip(crops.scene.tolist(), crops.slot.tolist()))
    assert pairs == sorted(where)
    want = R.gather(p, recs, instance=bufs.instance.cpu().numpy()[..., 0].view(np.uint16))
    assert np.array_equal(crops.instance.cpu().numpy(), want["instance"])


def test_selection_thresholds_empty_input_and_capacity(dev):
    where = {(0, 1): (6, 6), (0, 2): (2, 6), (1, 1): (3, 24), (1, 3): (5, 6), (2, 2): (6, 6)}
    stats = made_up_stats(3, 4, where)
    for kw, gone in ((dict(), ()), (dict(min_px=3), ((0, 2),)), (dict(min_visib_fract=0.25), ((1, 1),)),
                     (dict(min_px=6, min_visib_fract=0.9), ((0, 2), (1, 1), (1, 3)))):
        recs = R.select(oc.make_params(K, size=8, **kw), stats)
        assert [(int(a), int(b)) for a, b in zip(recs["scene"], recs["slot"])] == [k for k in sorted(where) if k not in gone]
        st, n, got = select_only(stats, dev, size=8, **kw)
        assert st == 0 and n == len(recs) and np.array_equal(got[:n], recs.view(np.int32).reshape(-1, 12))
        assert (got[n:] == -1).all()                           # nothing is written behind the last record
    # nothing eligible: no crops, empty tensors, no error
    empty = made_up_stats(3, 4, {})
    crops = oc.extract(tiny_buffers(empty, dev), K, size=8, outputs=("instance", "mask"))
    assert len(crops) == 0 and tuple(crops.instance.shape) == (0, 8, 8) and tuple(crops.mask.shape) == (0, 8, 8)
    assert tuple(crops.K3x3().shape) == (0, 3, 3) and crops.rgb is None
    single = oc.extract(tiny_buffers(made_up_stats(2, 1, {}), dev), K, size=8, outputs=("instance",))      # S = 1: only slot 0
    assert len(single) == 0
    # a capacity one short of the need
    st, n, got = select_only(stats, dev, capacity=4, size=8)
    assert st == _abi.OBJECT_CROPS_CAPACITY == 3 and n == 5
    assert b"holds 4 records, this batch needs 5" in _abi.lib().slhip_last_error()
    assert (got[4:] == -1).all()                               # and nothing behind the capacity
    st, n, got = select_only(stats, dev, capacity=5, size=8)
    assert st == 0 and n == 5


@pytest.mark.parametrize("S", [66, 130])
def test_selection_ragged_trips_capacity_and_no_array(dev, S):
    """The shared select pass under the crops' rule, through the raw entry: five scenes -- the second block has one live wave
    and three that leave at once -- of 66 and 130 slots, a ragged second and third trip of 64, about half the slots eligible
    (the others fail min_px or hold nothing); then a capacity one short of the need, and no record array at all."""
    B = 5
    pick = np.random.default_rng(S).random((B, S)) < 0.5
    pick[:, 1] = pick[:, S - 1] = True                         # the first slot and the last one of the ragged trip
    pick[:, 0] = False
    where = {(b, i): ((6, 6) if pick[b, i] else (2, 6)) for b in range(B) for i in range(1, S) if pick[b, i] or i % 3 == 0}
    stats = made_up_stats(B, S, where)
    kw = dict(size=8, min_px=3, jitter_scale=0.5, jitter_shift=0.5, seed=11, scene_id_base=40)
    want = R.select(oc.make_params(K, **kw), stats).view(np.int32).reshape(-1, 12)
    need = len(want)
    assert need == int(pick.sum()) and 0.35 * B * (S - 1) < need < 0.65 * B * (S - 1)
    assert [tuple(r) for r in want[:, :2]] == [(b, i) for b in range(B) for i in range(1, S) if pick[b, i]]
    st, n, got = select_only(stats, dev, **kw)
    assert st == 0 and n == need and np.array_equal(got[:n], want) and (got[n:] == -1).all()
    st, n, got = select_only(stats, dev, capacity=need - 1, **kw)
    assert st == _abi.OBJECT_CROPS_CAPACITY and n == need       # the need, not what fitted
    assert np.array_equal(got[:need - 1], want[:need - 1]) and (got[need - 1:] == -1).all()      # nothing at or behind the capacity
    st, n, _ = select_only(stats, dev, capacity=0, null_records=True, **kw)
    assert st == _abi.OBJECT_CROPS_CAPACITY and n == need


def test_step_timer_needs_every_step(picture, dev):
    """slhip_object_crops_timings (the step timer under the crops' convention): an error until both steps of the module were
    timed since the last timing_enable(1); a refused call and a call with timing off record nothing."""
    host, bufs = picture
    L = _abi.lib()
    ms = (C.c_float * 2)()

    def read():
        return L.slhip_object_crops_timings(C.byref(ms))

    def extract():
        return len(oc.extract(bufs, K, size=16, outputs=("instance",)))

    try:
        assert L.slhip_object_crops_timing_enable(1) == 0
        assert select_only(host["stats"], dev, size=8)[0] == 0
        assert read() == -1 and b"no timed calls" in L.slhip_last_error()      # a select alone
        assert extract() > 0                                                    # select and gather
        assert read() == 0 and all(np.isfinite(v) and v >= 0.0 for v in ms)
        assert select_only(host["stats"], dev, size=0)[0] == -1                 # refused by its checks: the flags stay
        assert read() == 0 and all(np.isfinite(v) and v >= 0.0 for v in ms)
        assert L.slhip_object_crops_timing_enable(1) == 0                       # clears the flags
        assert select_only(host["stats"], dev, size=0)[0] == -1
        assert read() == -1 and b"no timed calls" in L.slhip_last_error()
        assert L.slhip_object_crops_timing_enable(0) == 0
        assert extract() > 0                                                    # timing off: nothing is recorded
        assert read() == -1 and b"no timed calls" in L.slhip_last_error()
    finally:
        L.slhip_object_crops_timing_enable(0)


# ---- 4. and 5. a real render ----------------------------------------------------------------------------------------------
CROP_KW = dict(size=32, jitter_scale=0.25, jitter_shift=0.25, outputs=ALL)


@pytest.fixture(scope="module")
def rendered(sl):
    from stillleben_amd import synthetic

    table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))
    batch = sl.SceneBatch(table, 8, 6, resolution=(320, 240), seed=2027, render_chunk=8)
    batch.set_camera_intrinsics(533.389, 533.7435, 156.49345, 120.65545)
    batch.stage()
    batch.settle()
    batch.place(object_to_camera=True)
    bufs = batch.render(0, object_masks=True)
    crops = batch.crops(bufs, **CROP_KW)
    torch.cuda.synchronize()
    host = dict(rgb=bufs.rgb.cpu().numpy(), coord=bufs.coord.cpu().numpy(), normals=bufs.normals.cpu().numpy(),
                instance=bufs.instance.cpu().numpy()[..., 0].view(np.uint16),
                whole=bufs.object_masks.dense("all", slots=range(7)).cpu().numpy(),
                stats=bufs.object_stats.records().cpu().numpy().view(_abi.OBJECT_STATS_DTYPE).reshape(8, 7),
                o2c=batch.object_to_camera.cpu().numpy().copy())
    return batch, bufs, crops, host


def test_real_render(rendered):
    batch, bufs, crops, host = rendered
    key = _abi.view_key(2027, 0, 0)
    p = oc.make_params(batch.intrinsics(), seed=key, scene_id_base=0, **CROP_KW)
    recs = R.select(p, host["stats"])
    assert len(recs) >= 24                                     # most of the 48 objects show
    want = R.gather(p, recs, rgb=host["rgb"], coord=host["coord"], normals=host["normals"], instance=host["instance"],
                    dense_all=host["whole"])
    assert_same(crops, recs, want)
    assert int(crops.mask_visib.sum()) > 0 and not bool((crops.mask_visib & ~crops.mask_all).any())      # amodal is a superset
    assert torch.equal(crops.scene_global, crops.scene)
    with pytest.raises(TypeError):
        batch.crops(bufs, seed=3)                              # the batch sets intrinsics, seed and scene ids itself
    assert torch.equal(crops.object_to_camera.cpu(), torch.from_numpy(host["o2c"][recs["scene"].astype(np.int64), recs["slot"].astype(np.int64) - 1]))


def reprojection_residual(xyz, o2c, k4, centres):
    """|K (R X + t) - centre| per axis, float64; xyz [n, 3], o2c [n, 3, 4], k4 [n, 4], centres [n, 2]"""
    cam = np.einsum("nij,nj->ni", o2c[:, :, :3].astype(np.float64), xyz.astype(np.float64)) + o2c[:, :, 3]
    u = k4[:, 0] * cam[:, 0] / cam[:, 2] + k4[:, 2]
    v = k4[:, 1] * cam[:, 1] / cam[:, 2] + k4[:, 3]
    return np.abs(np.stack([u, v], axis=1) - centres)


def test_window_intrinsics_known_answer(rendered):
    """object_to_camera applied to coord.xyz and projected with K' lands on the output pixel's centre, up to the renderer's
    own reprojection error e (measured on the full picture with the batch's intrinsics, in source pixels) plus the half pixel
    of the nearest sample, both divided by the window's step: |residual| <= (e + 0.5) / step per axis.
    Measured on an MI355X: e = (0.001947, 0.001934) px over the 100 442 object pixels of the eight pictures; the largest crop
    residual is 0.444 px, 0.9967 of its bound (a sample next to a pixel edge).  The bound is derived, not tuned."""
    batch, bufs, crops, host = rendered
    inst = host["instance"]
    b, y, x = np.nonzero((inst >= 1) & (inst <= 6))
    slot = inst[b, y, x].astype(np.int64)
    k = np.broadcast_to(np.array(batch.intrinsics(), np.float64), (len(b), 4))
    full = reprojection_residual(host["coord"][b, y, x, :3], host["o2c"][b, slot - 1], k, np.stack([x + 0.5, y + 0.5], axis=1))
    e = full.max(axis=0)
    print("renderer reprojection error e = (%.6f, %.6f) px over %d object pixels" % (e[0], e[1], len(b)))
    assert e.max() < 0.5                                       # a centre's coordinates project into its own pixel
    vis = crops.mask_visib.cpu().numpy()
    c, v, u = np.nonzero(vis)
    assert len(c) > 1000
    res = reprojection_residual(crops.coord.cpu().numpy()[c, v, u, :3], crops.object_to_camera.cpu().numpy()[c],
                                crops.K.cpu().numpy().astype(np.float64)[c], np.stack([u + 0.5, v + 0.5], axis=1))
    step = crops.box.cpu().numpy().astype(np.float64)[c, 3]
    bound = (e[None, :] + 0.5) / step[:, None]
    print("crop residual: max %.6f px, largest share of its bound %.4f" % (res.max(), (res / bound).max()))
    assert (res <= bound).all()


def test_views_get_their_own_jitter(rendered):
    batch, bufs, crops, host = rendered
    first = crops.records.clone()
    try:
        boxes = []
        for _ in range(2):
            batch.place(view=1, object_to_camera=True)
            c1 = batch.crops(batch.render(0, object_masks=True), **CROP_KW)
            boxes.append((c1.records.clone(), c1.rgb.clone()))
        assert torch.equal(boxes[0][0], boxes[1][0]) and torch.equal(boxes[0][1], boxes[1][1])      # placed again: the same
        assert len(boxes[0][0]) > 0
        same_pairs = boxes[0][0].shape == first.shape and torch.equal(boxes[0][0][:, :2], first[:, :2])
        assert not (same_pairs and torch.equal(boxes[0][0][:, 2:6], first[:, 2:6]))                  # another view: other boxes
        # the jitter itself differs, not only the picture: the same statistics under the two views' keys
        p0, p1 = (oc.make_params(batch.intrinsics(), seed=_abi.view_key(2027, 0, v), **CROP_KW) for v in (0, 1))
        r0, r1 = R.select(p0, host["stats"]), R.select(p1, host["stats"])
        assert not np.array_equal(r0["side"], r1["side"]) and not np.array_equal(r0["x0"], r1["x0"])
    finally:
        batch.place(object_to_camera=True)                       # back to view 0 for whoever comes next


# ---- 6. hygiene ---------------------------------------------------------------------------------------------------------------
def test_repeatable_and_inputs_untouched(picture):
    host, bufs = picture
    inputs = {"rgb": bufs.rgb, "coord": bufs.coord, "normals": bufs.normals, "instance": bufs.instance,
              "mask records": bufs.object_masks.records, "words": bufs.object_masks.words,
              "px_visib": bufs.object_stats.px_count_visib, "px_all": bufs.object_stats.px_count_all,
              "bbox_visib": bufs.object_stats.bbox_visib, "bbox_obj": bufs.object_stats.bbox_obj}
    before = {k: t.clone() for k, t in inputs.items()}
    kw = dict(size=24, pad=1.5, jitter_scale=0.25, jitter_shift=0.25, outputs=ALL, seed=4)
    a, b = oc.extract(bufs, K, **kw), oc.extract(bufs, K, **kw)
    torch.cuda.synchronize()
    for name in ("records",) + ALL:
        assert torch.equal(getattr(a, name).view(torch.uint8), getattr(b, name).view(torch.uint8)), name
    for k, t in inputs.items():
        assert torch.equal(t, before[k]), k                     # (no NaN among them: equal values are equal bits here)
    assert a._keepalive[0] is bufs                              # the inputs live as long as the outputs


def test_without_masks_the_amodal_bit_stays_zero(picture, dev):
    host, _ = picture
    bufs = device_buffers(host, dev, masks=False)
    crops = oc.extract(bufs, K, size=16, pad=1.5, outputs=("mask",))
    p = oc.make_params(K, size=16, pad=1.5, outputs=("mask",))
    recs = R.select(p, host["stats"])
    assert_same(crops, recs, R.gather(p, recs, instance=host["instance"]))
    assert int(crops.mask_visib.sum()) > 0 and not bool(crops.mask_all.any())


def test_argument_errors(picture, dev):
    host, bufs = picture
    no_normals = types.SimpleNamespace(**{**vars(bufs), "normals": None})
    with pytest.raises(RuntimeError) as e:
        oc.extract(no_normals, K, size=16, outputs=("rgb", "normals"))
    assert "`normals` target was not rendered" in str(e.value)
    no_inst = types.SimpleNamespace(**{**vars(bufs), "instance": None})
    for outputs in (("mask",), ("instance",), ("coord",)):
        with pytest.raises(RuntimeError) as e:
            oc.extract(no_inst, K, size=16, outputs=outputs)
        assert "`instance` target was not rendered" in str(e.value)
    assert len(oc.extract(no_inst, K, size=16, outputs=("rgb", "coord"), isolate=False)) == 10      # nothing reads it here
    with pytest.raises(RuntimeError) as e:
        oc.extract(types.SimpleNamespace(**{**vars(bufs), "object_stats": None}), K, size=16)
    assert "statistics" in str(e.value)
    cpu = device_buffers(host, torch.device("cpu"))
    with pytest.raises(_abi.SlhipError) as e:
        oc.extract(cpu, K, size=16)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        oc.extract(bufs, K, size=16, jitter_scale=1.0)
