"""Object regions on the device (slhip_object_regions_centres, _vertices, _label, sl.object_regions, SceneBatch.regions) against
the host entries and the NumPy restatement tests/object_regions_ref.py.  Every comparison is bit for bit -- floats as their
integer views; every device output lies between poisoned guard bytes that must stay poison."""
import ctypes as C

import numpy as np
import pytest
import torch

import object_regions_ref as R
from stillleben_amd import _abi
from stillleben_amd import object_regions as og
from test_host_object_regions import LH, LN, LO, LW, POOL_COUNTS, label_reference, pool_reference, shared_pool

pytestmark = pytest.mark.gpu

F = np.float32
POISON = 0x5B
GUARD = 256      # bytes of poison before and after every output (a multiple of the 16-byte alignment the wide accesses want)


@pytest.fixture(scope="module")
def dev(sl):
    from stillleben_amd._context import engine

    return engine().device


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class Guarded:
    """`nbytes` of device memory between two guards, everything poisoned (or filled with `fill`'s bytes between the guards)"""

    def __init__(self, nbytes, dev, offset=0, fill=None):
        self.raw = torch.full((GUARD + offset + nbytes + GUARD,), POISON, dtype=torch.uint8, device=dev)
        self.lo, self.n = GUARD + offset, nbytes
        if fill is not None:
            self.raw[self.lo:self.lo + nbytes] = torch.from_numpy(np.frombuffer(np.ascontiguousarray(fill).tobytes(), np.uint8).copy()).to(dev)

    def ptr(self):
        return C.c_void_p(self.raw.data_ptr() + self.lo)

    def host(self, dtype, shape):
        torch.cuda.synchronize()
        h = self.raw.cpu().numpy()
        assert (h[:self.lo] == POISON).all() and (h[self.lo + self.n:] == POISON).all(), "a guard byte was written"
        return h[self.lo:self.lo + self.n].view(dtype).reshape(shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.raw == POISON).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def to_dev(a, dev):
    raw = np.frombuffer(np.ascontiguousarray(a).tobytes(), dtype=np.uint8)
    return torch.from_numpy(raw.copy()).to(dev)


# ---- 1. centres, vertices --------------------------------------------------------------------------------------------------------
def run_bank(dev, pool, assets, templates, Rn, max_verts):
    """centres, then vertices under them, every output guarded: (centres, vertex, vertex_region, count, extent) on the host"""
    A, V = len(assets), len(pool)
    d_pos, d_assets, d_templates = to_dev(pool, dev), to_dev(assets, dev), to_dev(templates, dev)
    L = _abi.lib()
    nbytes = C.c_uint64(0)
    assert L.slhip_object_regions_centres_bytes(A, max_verts, C.byref(nbytes)) == 0 and nbytes.value == A * max_verts * 4
    scratch, cen, vertex = Guarded(int(nbytes.value), dev), Guarded(A * Rn * 16, dev), Guarded(A * Rn * 4, dev)
    vr, count, extent = Guarded(V, dev, offset=3), Guarded(A * Rn * 4, dev), Guarded(A * Rn * 16, dev)
    table = (C.c_void_p(d_pos.data_ptr()), V, C.c_void_p(d_assets.data_ptr()), A, C.c_void_p(d_templates.data_ptr()), len(templates))
    with torch.cuda.device(dev):
        assert L.slhip_object_regions_centres(*table, Rn, max_verts, scratch.ptr(), cen.ptr(), vertex.ptr(), stream(dev)) == 0
        assert L.slhip_object_regions_vertices(*table, cen.ptr(), Rn, vr.ptr(), count.ptr(), extent.ptr(), stream(dev)) == 0
    scratch.host(F, (A, max_verts))                                         # (its guards)
    return (cen.host(F, (A, Rn, 4)), vertex.host(np.int32, (A, Rn)), vr.host(np.uint8, (V,)), count.host(np.int32, (A, Rn)),
            extent.host(F, (A, Rn, 4)))


@pytest.mark.parametrize("n_regions", [1, 8, 255])
def test_bank_of_the_pool(dev, n_regions):
    pool, assets, templates, want_c, want_v, want_vr, want_n, want_e = pool_reference(n_regions)
    A, V, Rn = len(assets), len(pool), n_regions
    got_c, got_v, got_vr, got_n, got_e = run_bank(dev, pool, assets, templates, Rn, 2500)
    # the restatement
    assert np.array_equal(got_v, want_v) and np.array_equal(bits(got_c), bits(want_c))
    assert np.array_equal(got_vr, want_vr) and np.array_equal(got_n, want_n) and np.array_equal(bits(got_e), bits(want_e))
    # the host twins
    host_c, host_v = og.centres_host(pool, assets, templates, Rn)
    assert np.array_equal(got_v, host_v) and np.array_equal(bits(got_c), bits(host_c))
    host_vr, host_n, host_e = og.vertices_host(pool, assets, templates, host_c)
    assert np.array_equal(got_vr, host_vr) and np.array_equal(got_n, host_n) and np.array_equal(bits(got_e), bits(host_e))
    # what they mean
    assert got_n.sum(axis=1).tolist() == list(POOL_COUNTS)
    import object_keypoints_ref as K

    owned = np.zeros(V, bool)
    for c in range(A):
        base, n = K.class_vertices(assets[c], templates, V)
        owned[base:base + n] = True
        if n == 0:
            continue
        pts = K.object_points(assets[c]["mesh_to_object"], pool[base:base + n])
        d2 = R.local_of(pts, got_c[c][got_vr[base:base + n], :3])[:, 3]
        for r in np.unique(got_vr[base:base + n]):
            mine = d2[got_vr[base:base + n] == r]
            assert got_e[c, r, 3] == mine.max()                            # >= every member's d2, equal to one's
    assert (got_vr[~owned] == 255).all() and (~owned).sum() == 13 + 5 + 3 + 11 + 9 and (got_vr[owned] < Rn).all()


def test_shared_vertices_on_the_device(dev):
    """classes whose ranges overlap: one writer per vertex byte, the highest class's; counts and extents per class"""
    pool, assets, templates = shared_pool()
    got = run_bank(dev, pool, assets, templates, 5, 60)
    cen, vertex = og.centres_host(pool, assets, templates, 5)
    want = (cen, vertex) + og.vertices_host(pool, assets, templates, cen)
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    assert got[3].sum(axis=1).tolist() == [60, 60, 40]


def test_bank_refusals_leave_the_device_untouched(dev):
    L = _abi.lib()
    out = Guarded(4096, dev)
    with torch.cuda.device(dev):
        for n_regions, n_assets in ((0, 4), (256, 4), (8, 0), (8, 1025)):
            assert L.slhip_object_regions_centres(out.ptr(), 4, out.ptr(), n_assets, out.ptr(), 1, n_regions, 4, out.ptr(), out.ptr(),
                                                  out.ptr(), stream(dev)) < 0
            assert L.slhip_object_regions_vertices(out.ptr(), 4, out.ptr(), n_assets, out.ptr(), 1, out.ptr(), n_regions, out.ptr(),
                                                   out.ptr(), out.ptr(), stream(dev)) < 0
        assert L.slhip_object_regions_centres(out.ptr(), 4, None, 1, out.ptr(), 1, 8, 4, out.ptr(), out.ptr(), out.ptr(), stream(dev)) < 0
        assert L.slhip_object_regions_centres(out.ptr(), 4, out.ptr(), 1, out.ptr(), 1, 8, 4, out.ptr(), None, out.ptr(), stream(dev)) < 0
        for null in (0, 2, 6, 8, 9, 10):
            args = [out.ptr(), 4, out.ptr(), 1, out.ptr(), 1, out.ptr(), 8, out.ptr(), out.ptr(), out.ptr(), stream(dev)]
            args[null] = None
            assert L.slhip_object_regions_vertices(*args) < 0, null
    assert out.untouched() and _abi.lib().slhip_last_error()


# ---- 2. label --------------------------------------------------------------------------------------------------------------------
def run_label(dev, inst, coord, classes, bank, outputs=0, stride=1, offset=0, null=None, centres=None, n_regions=None, **change):
    """classes: int32 [N, O] (stride 1) or slhip_synth_object records [N, O] (stride 4).  `offset`: bytes the region output is
    moved off its 16-byte boundary."""
    N, H, W = inst.shape
    O = classes.shape[1]
    A, Rn = bank.shape[:2]
    Rn = Rn if n_regions is None else n_regions
    d = dict(inst=to_dev(inst, dev), coord=to_dev(coord, dev), classes=to_dev(classes, dev), bank=to_dev(bank, dev))
    region, local, hist = Guarded(N * H * W, dev, offset), Guarded(N * H * W * 16, dev), Guarded(N * O * max(Rn, 1) * 4, dev)
    p = og.make_params((W, H), N, O, Rn, A).reshape(1)
    p["outputs"] = outputs
    for k, v in change.items():
        p[k] = v
    args = {k: C.c_void_p(t.data_ptr()) for k, t in d.items()}
    args.update(region=region.ptr(), local=local.ptr(), hist=hist.ptr())
    if centres is not None:
        args["bank"] = centres.ptr()
    if null:
        args[null] = None
    with torch.cuda.device(dev):
        st = _abi.lib().slhip_object_regions_label(p.ctypes.data, args["inst"], args["coord"], args["classes"], stride, args["bank"],
                                                   args["region"], args["local"], args["hist"], stream(dev))
    return st, region, local, hist


@pytest.mark.parametrize("n_regions", [1, 63, 64, 65, 255])
def test_label(dev, n_regions):
    inst, coord, classes, bank, want_r, want_l, want_h = label_reference(n_regions)
    shape = (LN, LH, LW)
    objs = np.zeros((LN, LO), _abi.SYNTH_OBJECT_DTYPE)
    objs["asset"], objs["instance_index"], objs["metallic"] = classes.view(np.uint32), 0x7fffffff, np.nan      # only .asset is read
    # every combination of the output bits once, the region moved 0, 1, 3 and 2 bytes off its boundary, both class layouts
    for outputs, offset, stride in ((0, 1, 1), (1, 3, 4), (2, 0, 4), (3, 2, 1)):
        st, region, local, hist = run_label(dev, inst, coord, objs if stride == 4 else classes, bank, outputs, stride, offset)
        assert st == 0
        got = region.host(np.uint8, shape)
        diff = got != want_r
        assert not diff.any(), "outputs %d: %d of %d regions differ, the first at %s" % (outputs, int(diff.sum()), diff.size, tuple(np.argwhere(diff)[0]))
        if outputs & 1:
            assert np.array_equal(bits(local.host(F, shape + (4,))), bits(want_l)), outputs
        else:
            assert local.untouched()
        if outputs & 2:
            got_h = hist.host(np.uint32, (LN, LO, n_regions))
            assert np.array_equal(got_h, want_h), outputs
            keys = ((np.arange(LN)[:, None, None] * LO + inst.astype(np.int64) - 1) * n_regions + got)[got != 255]
            assert np.array_equal(got_h.reshape(-1), np.bincount(keys, minlength=LN * LO * n_regions))
        else:
            assert hist.untouched()


def test_one_region_owns_the_picture(dev):
    """64 x 64 pixels of one (object, region): 16 waves add to one counter, and it says 4096 exactly"""
    rng = np.random.default_rng(2)
    bank = np.ones((1, 4, 4), F)
    bank[0, :, :3] = [[5, 0, 0], [0, 5, 0], [0, 0, 5], [0.25, -0.5, 0.125]]
    inst = np.full((1, 64, 64), 2, np.int16)
    coord = np.zeros((1, 64, 64, 4), F)
    coord[..., :3] = bank[0, 3, :3] + rng.uniform(-0.5, 0.5, (1, 64, 64, 3)).astype(F)
    st, region, local, hist = run_label(dev, inst, coord, np.zeros((1, 2), np.int32), bank, outputs=2)
    assert st == 0
    assert (region.host(np.uint8, (1, 64, 64)) == 3).all()
    got = hist.host(np.uint32, (1, 2, 4))
    assert got[0, 1, 3] == 4096 and got.sum() == 4096


def test_background_does_not_read_the_bank(dev):
    """no pixel has an object (0, negative, above O): the centres are a guarded buffer of NaN, and nothing depends on them"""
    rng = np.random.default_rng(3)
    inst = rng.choice(np.array([0, 0, 0, -1, 4, 300], np.int16), (2, 19, 33))
    coord = rng.uniform(-1, 1, (2, 19, 33, 4)).astype(F)
    bank = np.full((4, 64, 4), np.nan, F)
    centres = Guarded(bank.nbytes, dev, fill=bank)
    st, region, local, hist = run_label(dev, inst, coord, np.zeros((2, 3), np.int32), bank, outputs=3, offset=1, centres=centres)
    assert st == 0
    assert (region.host(np.uint8, (2, 19, 33)) == 255).all()
    assert not local.host(np.uint32, (2, 19, 33, 4)).any() and not hist.host(np.uint32, (2, 3, 64)).any()
    assert np.array_equal(bits(centres.host(F, bank.shape)), bits(bank))


def test_label_refusals_leave_the_device_untouched(dev):
    inst, coord, classes, bank = label_reference(8)[:4]
    for kw in (dict(null="inst"), dict(null="coord"), dict(null="classes"), dict(null="bank"), dict(null="region"), dict(null="local"),
               dict(null="hist"), dict(stride=0), dict(n_regions=0), dict(n_regions=256), dict(n_objects=65), dict(W=0), dict(H=32769),
               dict(outputs=4), dict(n_assets=0)):
        outputs = kw.pop("outputs", 3)
        st, region, local, hist = run_label(dev, inst, coord, classes, bank, outputs, **kw)
        assert st < 0, kw
        assert region.untouched() and local.untouched() and hist.untouched(), kw
    assert b"" != _abi.lib().slhip_last_error()
    empty = np.zeros((0, LH, LW), np.int16)                                  # no pictures: fine, and nothing is written
    st, region, local, hist = run_label(dev, empty, np.zeros((0, LH, LW, 4), F), np.zeros((0, LO), np.int32), bank, 3)
    assert st == 0 and region.untouched() and local.untouched() and hist.untouched()


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------
N_SCENES, N_OBJ, RES, INTRINSICS, N_REGIONS = 2, 3, (320, 240), (533.4, 533.7, 156.5, 120.6), 16


@pytest.fixture(scope="module")
def rendered(sl):
    """the batch of the keypoints' device test: three cubes, two scenes at 320 x 240"""
    import scenes as S

    meshes = []
    for i in range(3):
        m = sl.Mesh(S.CUBE)
        m.center_bbox()
        m.scale_to_bbox_diagonal(0.12 + 0.05 * i)
        m.class_index = i + 1
        meshes.append(m)
    table = sl.AssetTable(meshes)
    batch = sl.SceneBatch(table, N_SCENES, N_OBJ, resolution=RES, seed=(77 << 32) | 5, render_chunk=N_SCENES, manual_exposure=1.0,
                          scene_id_base=1000)
    batch.set_camera_intrinsics(*INTRINSICS)
    batch.stage()
    batch.settle(frames=5)
    batch.place(object_to_camera=True)
    bufs = batch.render(0, object_masks=True)
    bank = sl.object_regions.bank(table, N_REGIONS)
    reg = batch.regions(bufs, bank=bank, local=True, histogram=True)
    torch.cuda.synchronize()
    objs = np.frombuffer(batch.d_objects.cpu().numpy().tobytes()[:N_SCENES * N_OBJ * _abi.SYNTH_OBJECT_DTYPE.itemsize],
                         dtype=_abi.SYNTH_OBJECT_DTYPE)
    classes = objs["asset"].astype(np.int32).reshape(N_SCENES, N_OBJ)
    return batch, table, bufs, bank, reg, classes


def test_bank_of_the_table(rendered):
    batch, table, bufs, bank, reg, classes = rendered
    assert tuple(bank.centres.shape) == (3, N_REGIONS, 4) and len(bank) == N_REGIONS and tuple(bank.vertex.shape) == (3, N_REGIONS)
    pos = batch.eng.pool.arrays()[0]
    want_c, want_v = R.centres(pos, table.records, table.templates, N_REGIONS)
    assert np.array_equal(bank.vertex.cpu().numpy(), want_v) and np.array_equal(bits(bank.centres.cpu().numpy()), bits(want_c))
    want_vr, want_n, want_e = R.vertices(pos, table.records, table.templates, want_c)
    assert np.array_equal(bank.vertex_region.cpu().numpy(), want_vr)
    assert np.array_equal(bank.count.cpu().numpy(), want_n) and np.array_equal(bits(bank.extent.cpu().numpy()), bits(want_e))
    assert bank.count.sum(dim=1).cpu().tolist() == [int(n) for n in table.records["n_verts"]]
    kps, idx = sl_keypoints_fps(table, 8)
    assert torch.equal(bank.centres[:, :8], kps) and torch.equal(bank.vertex[:, :8], idx)


def sl_keypoints_fps(table, n):
    from stillleben_amd import object_keypoints

    return object_keypoints.fps(table, n)


def test_regions_of_the_render(rendered):
    batch, table, bufs, bank, reg, classes = rendered
    inst = bufs.instance.cpu().numpy()[..., 0]
    coord = bufs.coord.cpu().numpy()
    want_r, want_l, want_h = R.label(inst, coord, classes, bank.centres.cpu().numpy())
    got = reg.region.cpu().numpy()
    assert tuple(got.shape) == (N_SCENES, RES[1], RES[0]) and np.array_equal(got, want_r)
    assert np.array_equal(bits(reg.local.cpu().numpy()), bits(want_l))
    assert np.array_equal(reg.histogram.cpu().numpy().view(np.uint32), want_h)
    assert np.array_equal(reg.visible.cpu().numpy(), want_h > 0)
    own = (inst >= 1) & (inst <= N_OBJ)
    assert np.isfinite(coord[own][:, :3]).all()                              # the render's coord is finite on every object pixel
    assert np.array_equal(got != 255, own) and own.sum() > 20000
    assert (want_h > 0).sum(axis=2).max() >= 3                               # a cube shows several of its 16 regions
    with pytest.raises(TypeError):
        batch.regions(bufs, bank=bank, classes=None)
    with pytest.raises(TypeError):
        batch.regions(bufs)
    plain = og.label(bufs.instance, bufs.coord, torch.from_numpy(classes).to(reg.region.device), bank.centres)      # [N, O] classes, a bare bank
    assert torch.equal(plain.region, reg.region) and plain.local is None and plain.histogram is None and plain.visible is None


def test_regions_of_crops_and_points(rendered):
    batch, table, bufs, bank, reg, classes = rendered
    crops = batch.crops(bufs, size=32, outputs=("coord", "instance"))
    assert len(crops) >= 4
    nb = N_OBJ * _abi.SYNTH_OBJECT_DTYPE.itemsize
    of = og.ObjectRegions.of_crops(crops, batch.d_objects[:N_SCENES * nb], bank, local=True, histogram=True, n_objects=N_OBJ)
    per_crop = classes[crops.scene.cpu().numpy().astype(np.int64)]
    want_r, want_l, want_h = R.label(crops.instance.cpu().numpy(), crops.coord.cpu().numpy(), per_crop, bank.centres.cpu().numpy())
    assert np.array_equal(of.region.cpu().numpy(), want_r) and (want_r != 255).any()
    assert np.array_equal(bits(of.local.cpu().numpy()), bits(want_l))
    assert np.array_equal(of.histogram.cpu().numpy().view(np.uint32), want_h)
    pts = batch.points(bufs, n_points=64)
    got = reg.at(pts)
    assert tuple(got.shape) == (len(pts), 64) and got.dtype == torch.uint8
    assert torch.equal(got, reg.region.view(N_SCENES, -1)[pts.scene.long()[:, None], pts.index])
    assert bool((got != 255).all())                                          # sampled pixels are object pixels


def test_argument_errors(rendered):
    batch, table, bufs, bank, reg, classes = rendered
    inst, coord, cen = bufs.instance, bufs.coord, bank.centres
    cls = torch.from_numpy(classes).to(inst.device)
    with pytest.raises(_abi.SlhipError) as e:
        og.label(inst.cpu(), coord, cls, cen)
    assert "no CPU path" in str(e.value)
    with pytest.raises(_abi.SlhipError):
        og.label(inst, coord, cls.cpu(), cen)
    with pytest.raises(_abi.SlhipError):
        og.label(inst, coord, cls, cen.cpu())
    with pytest.raises(_abi.SlhipError):
        og.vertices(table, cen.cpu())
    for bad in (dict(instance=inst.to(torch.int32)), dict(coord=coord.double()), dict(coord=coord[:, :, :, :3]),
                dict(coord=coord[:, ::2]), dict(instance=inst[:, :, ::2]), dict(classes=cls.long()), dict(classes=cls[:1]),
                dict(classes=cls.t()), dict(bank=cen[:, :, :3]), dict(bank=cen.half()), dict(classes=batch.d_objects)):
        kw = dict(instance=inst, coord=coord, classes=cls, bank=cen)
        kw.update(bad)
        with pytest.raises(ValueError):
            og.label(**kw)
    with pytest.raises(_abi.SlhipError) as e:
        og.label(inst, coord, cls, torch.zeros((3, 256, 4), device=inst.device))
    assert "n_regions" in str(e.value)
    with pytest.raises(ValueError):
        og.vertices(table, cen[:2])
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            og.label(inst, coord, cls, cen.to("cuda:1"))
