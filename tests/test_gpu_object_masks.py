"""Per-object masks on the device (slhip_render_object_masks, slhip_object_masks_expand, sl.ObjectMasks).  For every scene, slot
and kind the comparison is exact, against an independent construction:
  (a) dense(): "visib" against instance == i of the same render, "all" against the object rendered alone (no other object, no
      background plane, `predicate`);
  (b) rle() / rles(): against a numpy encoding of that independent mask (np.diff over the column-major pixels, written here
      and not the package's rle_encode);
  (c) masks.stats: field for field what object_stats=True gives for the same scene."""
import ctypes as C

import numpy as np
import pytest
import torch

import scenes as S
from stillleben_amd import _abi, _loaders
from stillleben_amd._batch import HostPool, build_batch

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("px_count_visib", "px_count_all", "bbox_visib", "bbox_obj", "visib_fract")
OUTPUTS = ("rgb", "coord", "cls", "instance", "normals", "vertex_idx", "bary", "cam_coord")


@pytest.fixture(scope="module")
def eng(sl):
    from stillleben_amd._context import engine

    return engine()


def np_rle(mask):
    """COCO's uncompressed counts of a bool [H, W] mask: runs over the column-major pixels, zeros first."""
    flat = np.asarray(mask, dtype=np.int8).ravel(order="F")
    cuts = np.flatnonzero(np.diff(flat)) + 1
    counts = np.diff(np.concatenate([[0], cuts, [flat.size]])).tolist()
    return ([0] + counts) if flat[0] else counts


def alone(eng, scene, i):
    """instance == i of scene's object(s) with index i rendered alone: no other object, no plane."""
    keep = scene._background_plane_size.copy()
    scene._background_plane_size = np.zeros(2, np.float32)
    try:
        bufs = eng.render([scene], _abi.OUT_INSTANCE, ssao=False, shadows=False, predicate=lambda o: o.instance_index == i)
    finally:
        scene._background_plane_size = keep
    inst = bufs.instance.cpu().numpy()[0, ..., 0].view(np.uint16)
    return inst == i


def render_masks(eng, scenes_, **kw):
    bufs = eng.render(scenes_, _abi.OUT_ALL, ssao=kw.pop("ssao", True), shadows=True, object_masks=True, **kw)
    torch.cuda.synchronize()
    assert eng.last_masks_calls[-1][0] == 0
    return bufs


def check_stats(eng, scenes_, masks, **kw):
    """(c): the statistics of the masks call are those of the statistics call."""
    ref = eng.render(scenes_, _abi.OUT_ALL, ssao=kw.pop("ssao", True), shadows=True, object_stats=True, **kw).object_stats
    for f in STAT_FIELDS:
        assert torch.equal(getattr(masks.stats, f), getattr(ref, f)), f


def check_scene(eng, scene, bufs, b=0, slots=None, want=None):
    """(a) and (b) of scene b for both kinds.  `want`: {slot: alone mask} computed by the caller (else rendered here).
    Returns {slot: (visible mask, alone mask)}."""
    om = bufs.object_masks
    H, W = om.size
    S_ = om.n_slots
    slots = list(range(1, S_)) if slots is None else list(slots)
    inst = bufs.instance.cpu().numpy()[b, ..., 0].view(np.uint16)
    dv = om.dense("visib", scenes=[b], slots=slots)
    da = om.dense("all", scenes=[b], slots=slots)
    assert dv.dtype == torch.bool and dv.is_cuda and tuple(dv.shape) == (1, len(slots), H, W) and da.shape == dv.shape
    dv, da = dv.cpu().numpy()[0], da.cpu().numpy()[0]
    rv, ra = om.rles(b, "visib"), om.rles(b, "all")
    assert len(rv) == len(ra) == S_ - 1
    rec = om.host_records()[b]
    got = {}
    for k, i in enumerate(slots):
        mv = inst == i
        ma = want[i] if want is not None and i in want else alone(eng, scene, i)
        assert np.array_equal(dv[k], mv), "slot %d: dense visible mask" % i
        assert np.array_equal(da[k], ma), "slot %d: dense whole silhouette (%d vs %d pixels)" % (i, da[k].sum(), ma.sum())
        for kind, m, lst in (("visib", mv, rv), ("all", ma, ra)):
            r = om.rle(b, i, kind)
            assert r["size"] == [H, W] and sum(r["counts"]) == H * W
            assert r["counts"] == np_rle(m), "slot %d: %s run lengths" % (i, kind)
            assert lst[i - 1] == r
            assert int(rec[i]["rle_count"][0 if kind == "all" else 1]) == len(r["counts"])
        got[i] = (mv, ma)
    return got


@pytest.mark.parametrize("seed", [3, 21])
def test_clutter(sl, eng, seed):
    scene = S.clutter_scene(sl, seed, n_objects=6)
    bufs = render_masks(eng, [scene])
    assert bufs.object_masks.n_slots == 7 and bufs.object_stats is bufs.object_masks.stats
    got = check_scene(eng, scene, bufs)
    check_stats(eng, [scene], bufs.object_masks)
    assert sum(int(v.sum()) for v, _ in got.values()) > 0
    assert any((a & ~v).any() for v, a in got.values())        # something is occluded: the two kinds differ
    # slot 0 is empty in every form
    assert bufs.object_masks.rle(0, 0, "all")["counts"] == [320 * 240]
    assert not bufs.object_masks.dense("visib", slots=[0]).any()


def _cube(sl, diag):
    m = sl.Mesh(S.CUBE, physics=False)
    m.center_bbox()
    m.scale_to_bbox_diagonal(diag)
    return m


def _place(sl, scene, mesh, xyz, rot=None):
    o = sl.Object(mesh)
    p = np.eye(4, dtype=np.float32)
    if rot is not None:
        p[:3, :3] = rot
    p[:3, 3] = xyz
    o.set_pose(torch.from_numpy(p))
    scene.add_object(o)
    return o


def corner_scene(sl, size):
    """camera at (1, 0, 0) looking at the origin, no plane: 1 a cube in the middle, 2 a large cube over the bottom right corner
    of the picture, 3 a small cube in front of part of it"""
    scene = sl.Scene(size, seed=1)
    big, small = _cube(sl, 0.5), _cube(sl, 0.25)
    rng = np.random.default_rng(5)
    _place(sl, scene, small, (0.0, 0.1, 0.1), S.random_rotation(rng))
    _place(sl, scene, big, (0.0, 0.45, -0.3), S.random_rotation(rng))
    _place(sl, scene, small, (0.3, 0.27, -0.18), S.random_rotation(rng))
    scene.set_camera_look_at(torch.tensor([1.0, 0.0, 0.0]), torch.tensor([0.0, 0.0, 0.0]))
    scene.choose_random_light_direction()
    return scene


@pytest.mark.parametrize("size", [(150, 100), (240, 180)])
def test_partial_tiles(sl, eng, size):
    """Neither dimension a multiple of 8 (150 x 100), the height not (240 x 180): the rows and columns of a partial tile beyond
    the image do not exist, and a run that reaches the bottom of a column goes on at the top of the next."""
    W, H = size
    scene = corner_scene(sl, size)
    bufs = render_masks(eng, [scene])
    got = check_scene(eng, scene, bufs)
    check_stats(eng, [scene], bufs.object_masks)
    v2, a2 = got[2]
    assert a2[-1, :].any() and a2[:, -1].any() and v2[-1, -1]          # object 2 reaches the bottom and the right border
    assert (a2 & ~v2).any()                                            # and object 3 hides part of it
    tb = bufs.object_masks.host_records()[0, 2]["tile_box"]
    assert tb[2] == (W - 1) // 8 and tb[3] == (H - 1) // 8             # its box ends in the partial tiles


@pytest.mark.parametrize("closer,shift,covers_origin", [(1.0, (0.0, 0.0, 0.0), False), (0.85, (0.0, 0.03, 0.0), True)])
def test_near_plane(sl, eng, closer, shift, covers_origin):
    """The scene of test_gpu_object_stats.py::test_near_plane_scene (triangles cross the near plane, an object covers whole
    columns: its runs go on from the bottom of one column into the top of the next), and the same scene from a little closer
    and to the side, where the object covers pixel (0, 0) as well: its counts start with 0."""
    scene = S.clutter_scene(sl, 11, n_objects=3, size=(320, 240))
    c = scene.objects[0].pose()[:3, 3]
    scene.set_camera_look_at(c + closer * torch.tensor([0.16, 0.05, 0.06]), c + torch.tensor(shift))
    bufs = render_masks(eng, [scene])
    om = bufs.object_masks
    got = check_scene(eng, scene, bufs)
    check_stats(eng, [scene], om)
    assert (bufs.instance.cpu().numpy() != 0).mean() > 0.5
    a = got[1][1]
    assert a.all(axis=0).any() and not a.all()                          # whole columns, not the whole picture
    r = om.rle(0, 1, "all")["counts"]
    assert max(r) > 240                                                 # a run longer than a column: it went on into the next
    assert bool(a[0, 0]) == covers_origin and (r[0] == 0) == covers_origin
    tb = om.host_records()[0, 1]["tile_box"]
    assert tb[1] == 0 and tb[3] == 29 and tb[2] - tb[0] >= 28           # the tile box spans the viewport's height


def edge_scene(sl, lateral):
    """camera at (2, 0, 0) looking at the origin: 1 a cube in the middle, 2 a small cube right behind it (hidden), 3 a cube at
    `lateral` metres to the side, 4 a cube behind the camera (test_gpu_object_stats.py)"""
    scene = sl.Scene((320, 240), seed=1)
    big, small = _cube(sl, 0.4), _cube(sl, 0.1)
    _place(sl, scene, big, (0.0, 0.0, 0.0))
    _place(sl, scene, small, (-0.6, 0.0, 0.0))
    _place(sl, scene, big, (0.0, lateral, 0.0))
    _place(sl, scene, big, (3.0, 0.0, 0.0))
    scene.set_camera_look_at(torch.tensor([2.0, 0.0, 0.0]), torch.tensor([0.0, 0.0, 0.0]))
    scene.background_plane_size = torch.tensor([3.0, 3.0])
    scene.choose_random_light_direction()
    return scene


def test_hidden_outside_and_behind_camera(sl, eng):
    W, H = 320, 240
    lateral = None
    for y in np.linspace(0.3, 1.5, 25):       # the offset at which object 3 straddles the image border
        m = alone(eng, edge_scene(sl, float(y)), 3)
        if m.any() and (m[:, 0].any() or m[:, -1].any()) and not (m[:, 0].all() or m[:, -1].all()):
            lateral = float(y)
            break
    assert lateral is not None
    scene = edge_scene(sl, lateral)
    bufs = render_masks(eng, [scene])
    om = bufs.object_masks
    got = check_scene(eng, scene, bufs, want={3: m})
    check_stats(eng, [scene], om)
    rec = om.host_records()[0]
    assert om.rle(0, 2, "visib")["counts"] == [W * H] and got[2][1].any() and len(om.rle(0, 2, "all")["counts"]) > 1   # hidden
    assert got[3][1][:, 0].any() or got[3][1][:, -1].any()                                                        # cut by the border
    assert om.rle(0, 4, "visib")["counts"] == [W * H] and om.rle(0, 4, "all")["counts"] == [W * H]                    # behind
    assert rec[4]["tile_box"][0] > rec[4]["tile_box"][2]
    assert list(rec[4]["rle_count"]) == [1, 1]


def holey_quad(seed):
    """A 0.4 m textured square whose base texture is transparent in a checker of holes (alpha-tested draw)."""
    rng = np.random.default_rng(seed)
    m = _loaders.ConsolidatedMesh()
    m.positions = np.array([[-0.2, -0.2, 0], [0.2, -0.2, 0], [0.2, 0.2, 0], [-0.2, 0.2, 0]], np.float32)
    m.normals = np.array([[0, 0, 1]] * 4, np.float32)
    m.uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    m.colors = np.ones((4, 4), np.float32)
    m.indices = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    y, x = np.mgrid[0:64, 0:64]
    t = np.zeros((64, 64, 4), np.uint8)
    t[..., :3] = (rng.random((64, 64, 3)) * 255).astype(np.uint8)
    t[..., 3] = np.where(((x // 8) + (y // 8)) % 2 == 0, 255, 0)
    m.textures = [t]
    m.tex_samplers = [_abi.SAMPLER_DEFAULT]
    m._tex_alpha = [True]
    m.materials = [_loaders.Material(base_color=(1, 1, 1, 1), metallic=0.0, roughness=0.9, base_texture=0)]
    m.submeshes = [_loaders.SubMesh(0, 6, 0)]
    return m


def test_alpha_tested_holes(sl, eng):
    mesh = sl.Mesh.from_data(holey_quad(2))
    scene = sl.Scene((240, 180), seed=1)
    rng = np.random.default_rng(4)
    for k in range(3):
        o = sl.Object(mesh)
        p = np.eye(4, dtype=np.float32)
        p[:3, :3] = S.random_rotation(rng)
        p[:3, 3] = [0.15 * (k - 1), 0.05 * k, 0.1 + 0.05 * k]
        o.set_pose(torch.from_numpy(p))
        scene.add_object(o)
    scene.set_camera_look_at(torch.tensor([0.1, -0.8, 0.6]), torch.tensor([0.0, 0.0, 0.1]))
    scene.background_plane_size = torch.tensor([2.0, 2.0])
    _, drec, _ = build_batch([scene], HostPool())
    assert (drec["flags"][1:] & _abi.DRAW_ALPHA_TEST).all()
    bufs = render_masks(eng, [scene])
    om = bufs.object_masks
    check_scene(eng, scene, bufs)
    check_stats(eng, [scene], om)
    bo = om.stats.bbox_obj[0].cpu().numpy()
    pa = om.stats.px_count_all[0].cpu().numpy()
    assert pa[1] > 0 and pa[1] < bo[1][2] * bo[1][3]                    # the amodal mask has holes
    assert len(om.rle(0, 1, "all")["counts"]) > 2 * bo[1][2] + 1        # many short runs: well above two per column of the box


def test_shared_slot_and_slot_300(sl, eng):
    """Two objects with one index share a slot (the union of their silhouettes); an index beyond the 256-slot LDS table of the
    visible pass takes the global path; the unused slots between them are the single run [W * H]."""
    scene = S.clutter_scene(sl, 17, n_objects=4)
    objs = scene.objects
    objs[1].instance_index = 1          # objects 0 and 1 share slot 1
    objs[3].instance_index = 300
    bufs = render_masks(eng, [scene])
    om = bufs.object_masks
    assert om.n_slots == 301
    got = check_scene(eng, scene, bufs, slots=(1, 3, 300))
    check_stats(eng, [scene], om)
    assert got[1][1].sum() > 0 and got[300][0].sum() > 0
    for i in (2, 150, 299):
        assert om.rle(0, i, "all")["counts"] == [320 * 240] and om.rle(0, i, "visib")["counts"] == [320 * 240]
    assert not om.dense("all", slots=[2, 299]).any()


def mask_tensors(om):
    rec = om.host_records()
    S_ = om.n_slots
    out = {"records": om.records.clone()}
    for kind in ("all", "visib"):
        out["dense_" + kind] = om.dense(kind)
        out["rle_" + kind] = [om.rles(b, kind) for b in range(rec.shape[0])]
    end = int(rec[-1, S_ - 1]["rle_offset"][1]) + int(rec[-1, S_ - 1]["rle_count"][1])
    out["runs"] = om.runs[:end].clone()
    return out


def same(a, b):
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_capacity_grows_and_repeats(sl, eng):
    scs = [S.clutter_scene(sl, 40 + k, n_objects=5, size=(160, 120)) for k in range(2)]
    ample = eng.render(scs, _abi.OUT_INSTANCE, ssao=False, shadows=False, object_masks=True).object_masks
    assert len(eng.last_masks_calls) == 1 and eng.last_masks_calls[0][0] == 0
    srec, drec, crec = build_batch(scs, eng.pool, with_shadows=False)
    small = eng.render_records(srec, drec, crec, 160, 120, _abi.OUT_INSTANCE, ssao=False, shadows=False, object_masks=True,
                               n_slots=6, masks_capacity=(4, 4)).object_masks
    calls = eng.last_masks_calls
    assert calls[0][0] == _abi.OBJECT_MASKS_CAPACITY and calls[0][1] == 4 and calls[0][2] > 4 and calls[0][3] == 4
    assert all(c[0] == _abi.OBJECT_MASKS_CAPACITY for c in calls[:-1]) and calls[-1][0] == 0 and len(calls) <= 3
    st, cw, nw, cr, nr = calls[-1]
    assert cw >= nw > 4 and cr >= nr > 4
    ww, wr = C.c_uint64(0), C.c_uint64(0)
    _abi.lib().slhip_render_object_masks_bytes(2, 6, 160, 120, C.byref(ww), C.byref(wr))
    assert nw <= ww.value and nr <= wr.value
    eng.render_records(srec, drec, crec, 160, 120, _abi.OUT_INSTANCE, ssao=False, shadows=False, object_stats=True, n_slots=6)
    assert nw == 2 * eng.last_stats_calls[-1][2]                       # both kinds: twice the words of the statistics call
    for f in STAT_FIELDS:
        assert torch.equal(getattr(small.stats, f), getattr(ample.stats, f)), f
    same(mask_tensors(small), mask_tensors(ample))
    rec = small.host_records()
    assert nr == int(rec["rle_count"].sum())


def test_outputs_unchanged_and_deterministic(sl, eng):
    scs = [S.clutter_scene(sl, 30 + k, n_objects=5, size=(160, 120)) for k in range(3)]
    off = eng.render(scs, _abi.OUT_ALL, ssao=True, shadows=True)
    a = {n: getattr(off, n).clone() for n in OUTPUTS}
    assert off.object_masks is None and off.object_stats is None
    on = render_masks(eng, scs)
    for n, t in a.items():
        assert torch.equal(t.view(torch.uint8), getattr(on, n).view(torch.uint8)), n
    first = mask_tensors(on.object_masks)
    again = render_masks(eng, scs)
    assert len(eng.last_masks_calls) == 1                              # the pools have settled: records are comparable
    same(first, mask_tensors(again.object_masks))
    assert eng.render(scs, _abi.OUT_ALL, buffers=again).object_masks is None


def test_several_scenes_in_one_call(sl, eng):
    scs = [S.clutter_scene(sl, 60 + k, n_objects=4, size=(160, 120)) for k in range(3)]
    bufs = render_masks(eng, scs)
    om = bufs.object_masks
    for b, scene in enumerate(scs):
        check_scene(eng, scene, bufs, b=b)
    check_stats(eng, scs, om)
    # the runs of the masks lie one after the other in scan order (record-major, kind minor), the words kind-major
    rec = om.host_records()
    off, cnt = rec["rle_offset"].reshape(-1), rec["rle_count"].reshape(-1)
    assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(cnt)[:-1])
    assert eng.last_masks_calls[-1][4] == int(cnt.sum())
    half = eng.last_masks_calls[-1][2] // 2
    assert np.array_equal(rec["word_offset"][..., 1], rec["word_offset"][..., 0] + half)
    one = om[1]
    assert one.rle(2, "all") == om.rle(1, 2, "all") and torch.equal(one.dense("all"), om.dense("all", scenes=[1])[0])


@pytest.fixture(scope="module")
def small_batch(sl):
    from stillleben_amd import synthetic

    table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))
    batch = sl.SceneBatch(table, 8, 6, resolution=(320, 240), seed=2027, render_chunk=8)
    batch.set_camera_intrinsics(533.389, 533.7435, 156.49345, 120.65545)
    batch.stage()
    batch.settle()
    batch.place()
    return batch


def test_scene_batch(sl, eng, small_batch):
    bufs = small_batch.render(0, object_masks=True)
    torch.cuda.synchronize()
    om = bufs.object_masks
    assert om.n_slots == 7 and om.size == (240, 320) and bufs.object_stats is om.stats
    inst = bufs.instance[..., 0].to(torch.int32) & 0xFFFF
    visib, whole = om.dense("visib"), om.dense("all")
    assert tuple(visib.shape) == (8, 6, 240, 320)
    want = torch.stack([inst == i for i in range(1, 7)], dim=1)
    assert torch.equal(visib, want)
    assert int(visib.sum()) > 0
    assert not (visib & ~whole).any()                                   # visib is a subset of all, bit by bit
    assert torch.equal(whole.sum(dim=(2, 3)).to(torch.int32), om.stats.px_count_all[:, 1:])
    assert torch.equal(visib.sum(dim=(2, 3)).to(torch.int32), om.stats.px_count_visib[:, 1:])
    v = visib.cpu().numpy()
    for b in (0, 7):
        rl = om.rles(b, "visib")
        for i in range(6):
            assert rl[i]["counts"] == np_rle(v[b, i])
    keep = inst.clone()
    again = small_batch.render(0)
    torch.cuda.synchronize()
    assert again.object_masks is None and again.object_stats is None
    assert torch.equal(again.instance[..., 0].to(torch.int32) & 0xFFFF, keep)
    chunks = list(small_batch.render_chunks(object_masks=True))
    assert len(chunks) == 1 and torch.equal(chunks[0].object_masks.dense("all"), whole)


def test_argument_rules(sl, eng):
    scene = S.clutter_scene(sl, 9, n_objects=4, size=(160, 120))
    rp = sl.RenderPass()
    first = rp.render(scene)
    with pytest.raises(RuntimeError):
        first.object_masks()                                           # a render without masks
    rp.object_masks_enabled = True
    with pytest.raises(ValueError):
        rp.render(scene, result=sl.RenderPassResult(), depth_peel=first)
    with pytest.raises(ValueError):
        eng.render([scene], _abi.OUT_ALL, depth_peel=torch.zeros((1, 120, 160, 4), device=eng.device), object_masks=True)
    res = rp.render(scene)
    om = res.object_masks()                                            # the single scene's view
    assert om.n_slots == 5 and om.stats.px_count_all.shape == (5,) and om.stats.bbox_obj.shape == (5, 4)
    d = om.dense("visib")
    assert tuple(d.shape) == (4, 120, 160) and d.dtype == torch.bool
    inst = res.instance_index().cpu().numpy()[..., 0].view(np.uint16)
    assert np.array_equal(d.cpu().numpy(), np.stack([inst == i for i in range(1, 5)]))
    assert om.rle(2, "visib")["counts"] == np_rle(inst == 2) and len(om.rles("all")) == 4
    assert not om.dense("all", slots=[0]).any() and tuple(om.dense("all", slots=[0]).shape) == (1, 120, 160)
    with pytest.raises(ValueError):
        om.dense(kind="nope")
    with pytest.raises(IndexError):
        om.dense(slots=[5])
    assert res.object_stats().px_count_all.shape == (5,)               # the statistics come along
    rp.object_masks_enabled = False
    res = rp.render(scene)
    with pytest.raises(RuntimeError):
        res.object_masks()
