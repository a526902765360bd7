"""Per-object visibility statistics on the device (slhip_render_object_stats, sl.ObjectStats): every number is checked exactly
against an independent construction --
  * the visible part against the instance output of the same render,
  * the whole silhouette against the object rendered alone (no other object, no background plane, `predicate`), and once
    against the CPU oracle's render of the same alone records,
  * the render's eight outputs are the same bits with and without statistics."""
import ctypes as C

import numpy as np
import pytest
import torch

import scenes as S
from stillleben_amd import _abi, _loaders
from stillleben_amd._batch import HostPool, build_batch

pytestmark = pytest.mark.gpu

EMPTY = [-1, -1, -1, -1]


@pytest.fixture(scope="module")
def eng(sl):
    from stillleben_amd._context import engine

    return engine()


def count_and_box(inst, S_):
    """count [S], box [S, 4] (x, y, w, h; -1 when empty) of the pixels of each instance value in an [H, W] mask."""
    inst = np.asarray(inst).astype(np.int64) & 0xFFFF
    cnt = np.zeros(S_, np.int64)
    box = np.full((S_, 4), -1, np.int64)
    for i in range(1, S_):
        ys, xs = np.nonzero(inst == i)
        cnt[i] = len(xs)
        if len(xs):
            box[i] = (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
    return cnt, box


def np_stats(st, b):
    return (st.px_count_visib[b].cpu().numpy(), st.px_count_all[b].cpu().numpy(), st.bbox_visib[b].cpu().numpy(),
            st.bbox_obj[b].cpu().numpy())


def check_visible(bufs, S_):
    st = bufs.object_stats
    assert st is not None and st.px_count_visib.shape == (bufs.B, S_)
    inst = bufs.instance.cpu().numpy()[..., 0].view(np.uint16)
    for b in range(bufs.B):
        cnt, box = count_and_box(inst[b], S_)
        pv, _, bv, _ = np_stats(st, b)
        assert np.array_equal(pv, cnt), "scene %d: visible counts %s vs %s" % (b, pv, cnt)
        assert np.array_equal(bv, box), "scene %d: visible boxes" % b


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


def check_silhouette(eng, scene, st, b=0):
    _, pa, _, bo = np_stats(st, b)
    for i in range(1, st.n_slots):
        m = alone(eng, scene, i)
        cnt, box = count_and_box(m.astype(np.int64) * i, i + 1)
        assert pa[i] == cnt[i], "object %d: px_count_all %d, alone %d" % (i, pa[i], cnt[i])
        assert np.array_equal(bo[i], box[i]), "object %d: bbox_obj %s, alone %s" % (i, bo[i], box[i])


def check_invariants(st):
    pv, pa, bv, bo = (t.cpu().numpy().astype(np.int64) for t in (st.px_count_visib, st.px_count_all, st.bbox_visib, st.bbox_obj))
    vf = st.visib_fract.cpu().numpy()
    assert (pv <= pa).all()
    assert ((vf >= 0) & (vf <= 1)).all() and vf.dtype == np.float32
    assert (pv[:, 0] == 0).all() and (pa[:, 0] == 0).all() and (bo[:, 0] == -1).all()
    has = pv > 0
    assert (bv[has][:, 0] >= bo[has][:, 0]).all() and (bv[has][:, 1] >= bo[has][:, 1]).all()
    assert (bv[has][:, 0] + bv[has][:, 2] <= bo[has][:, 0] + bo[has][:, 2]).all()
    assert (bv[has][:, 1] + bv[has][:, 3] <= bo[has][:, 1] + bo[has][:, 3]).all()
    assert ((bv == -1).all(axis=-1) == (pv == 0)).all() and ((bo == -1).all(axis=-1) == (pa == 0)).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(pa > 0, pv.astype(np.float32) / np.maximum(pa, 1).astype(np.float32), 0).astype(np.float32)
    assert np.array_equal(vf, want)


def render_stats(eng, scenes_, **kw):
    bufs = eng.render(scenes_, _abi.OUT_ALL, ssao=kw.pop("ssao", True), shadows=True, object_stats=True, **kw)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("seed", [3, 8, 21])
def test_clutter_visible_and_silhouette(sl, eng, seed):
    scene = S.clutter_scene(sl, seed, n_objects=6)
    bufs = render_stats(eng, [scene])
    check_visible(bufs, 7)
    check_silhouette(eng, scene, bufs.object_stats)
    check_invariants(bufs.object_stats)
    assert int(bufs.object_stats.px_count_visib.sum()) > 0


def test_bunny_640x480(sl, eng):
    scene = S.clutter_scene(sl, 5, n_objects=6, size=(640, 480), with_bunny=True)
    bufs = render_stats(eng, [scene])
    check_visible(bufs, 7)
    check_silhouette(eng, scene, bufs.object_stats)
    check_invariants(bufs.object_stats)


def test_near_plane_scene(sl, eng):
    # built like test_gpu_render.py::test_near_plane_clipping: triangles cross the near plane
    scene = S.clutter_scene(sl, 11, n_objects=3, size=(320, 240))
    c = scene.objects[0].pose()[:3, 3]
    scene.set_camera_look_at(c + torch.tensor([0.16, 0.05, 0.06]), c)
    bufs = render_stats(eng, [scene])
    assert (bufs.instance.cpu().numpy() != 0).mean() > 0.5
    check_visible(bufs, 4)
    check_silhouette(eng, scene, bufs.object_stats)
    check_invariants(bufs.object_stats)


def _cube(sl, diag):
    m = sl.Mesh(S.CUBE, physics=False)
    m.center_bbox()
    m.scale_to_bbox_diagonal(diag)
    return m


def _place(sl, scene, mesh, xyz):
    o = sl.Object(mesh)
    p = np.eye(4, dtype=np.float32)
    p[:3, 3] = xyz
    o.set_pose(torch.from_numpy(p))
    scene.add_object(o)
    return o


def edge_scene(sl, eng, lateral):
    """camera at (2, 0, 0) looking at the origin: 1 a cube in the middle, 2 a small cube right behind it (hidden), 3 a cube at
    `lateral` metres to the side, 4 a cube behind the camera"""
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
    # the lateral offset at which object 3 straddles the image border (found with renders of the object alone)
    W = 320
    lateral = None
    for y in np.linspace(0.3, 1.5, 25):
        m = alone(eng, edge_scene(sl, eng, float(y)), 3)
        if m.any() and (m[:, 0].any() or m[:, -1].any()) and not (m[:, 0].all() or m[:, -1].all()):
            lateral = float(y)
            break
    assert lateral is not None
    scene = edge_scene(sl, eng, lateral)
    bufs = render_stats(eng, [scene])
    st = bufs.object_stats
    check_visible(bufs, 5)
    check_silhouette(eng, scene, st)
    check_invariants(st)
    pv, pa, bv, bo = np_stats(st, 0)
    assert pa[1] > 0 and pv[1] > 0
    assert pv[2] == 0 and pa[2] > 0 and list(bv[2]) == EMPTY and float(st.visib_fract[0, 2]) == 0.0      # fully hidden
    assert pa[3] > 0 and (bo[3][0] == 0 or bo[3][0] + bo[3][2] == W)                                     # cut by the border
    assert pv[4] == 0 and pa[4] == 0 and list(bv[4]) == EMPTY and list(bo[4]) == EMPTY                   # behind the camera
    assert st.to_bop(0)[1]["visib_fract"] == 0.0


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


def test_alpha_tested_draw(sl, eng):
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
    assert (drec["flags"][1:] & _abi.DRAW_ALPHA_TEST).all()      # the discard path of the visibility pass
    bufs = render_stats(eng, [scene])
    check_visible(bufs, 4)
    check_silhouette(eng, scene, bufs.object_stats)
    check_invariants(bufs.object_stats)
    st = bufs.object_stats
    # the holes show: fewer pixels than the filled box of the silhouette
    _, pa, _, bo = np_stats(st, 0)
    assert pa[1] > 0 and pa[1] < bo[1][2] * bo[1][3]


def test_alpha_tested_draw_across_the_near_plane(sl, eng, oracle):
    # The one case in which the clipped sub-triangles, their barycentrics and the discard test meet, in the visibility pass, the
    # shading pass and the silhouette pass.  Object 1 faces the camera 0.1 m away, turned 0.03 rad about two axes: its plane cuts
    # the near plane (z = 0.1) along a slanted line through the picture, almost parallel to it, so some pixel centre next to
    # the cut has a camera z within 1e-6 of 0.1.  Object 2 stands 0.45 m from the camera and shows through the holes.
    mesh = sl.Mesh.from_data(holey_quad(2))
    scene = sl.Scene((64, 48), seed=1)
    upright = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)   # the quad's normal along -y, towards the camera
    c, s = np.cos(0.03), np.sin(0.03)
    turn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    for rot, xyz in ((turn @ upright, (0.0, 0.0, 0.5)), (upright, (0.02, 0.35, 0.52))):
        o = sl.Object(mesh)
        p = np.eye(4, dtype=np.float32)
        p[:3, :3] = rot.astype(np.float32)
        p[:3, 3] = xyz
        o.set_pose(torch.from_numpy(p))
        scene.add_object(o)
    scene.set_camera_look_at(torch.tensor([0.0, -0.1, 0.5]), torch.tensor([0.0, 1.0, 0.5]))
    scene.background_plane_size = torch.tensor([2.0, 2.0])
    pool = HostPool()
    srec, drec, _ = build_batch([scene], pool)
    assert (drec["flags"][1:] & _abi.DRAW_ALPHA_TEST).all()
    bufs = render_stats(eng, [scene])
    st = bufs.object_stats
    check_visible(bufs, 3)
    check_silhouette(eng, scene, st)
    check_invariants(st)
    ref = oracle.render(pool.arrays(), srec, drec, 64, 48, _abi.OUT_INSTANCE | _abi.OUT_COORD)
    inst = bufs.instance.cpu().numpy().view(np.uint16)
    coord = bufs.coord.cpu().numpy()
    assert np.array_equal(inst, ref.instance) and np.array_equal(coord.view(np.uint32), ref.coord.view(np.uint32))
    near = coord[0, :, :, 3][inst[0, ..., 0] == 1]
    assert abs(float(near.min()) - 0.1) < 1e-6          # cut exactly at the near plane, inside the picture
    pv, pa, _, bo = np_stats(st, 0)
    assert 0 < pa[1] < bo[1][2] * bo[1][3]              # the holes show
    assert 0 < pv[2] < pa[2]                            # ... and object 2 through them, partly


def test_silhouette_matches_the_oracle(sl, eng, oracle):
    scene = S.clutter_scene(sl, 13, n_objects=6)
    W, H = scene.viewport
    bufs = render_stats(eng, [scene])
    _, pa, _, bo = np_stats(bufs.object_stats, 0)
    keep = scene._background_plane_size.copy()
    scene._background_plane_size = np.zeros(2, np.float32)
    try:
        for i in range(1, 7):
            pool = HostPool()
            srec, drec, _ = build_batch([scene], pool, predicate=lambda o: o.instance_index == i, with_shadows=False)
            ref = oracle.render(pool.arrays(), srec, drec, W, H, _abi.OUT_INSTANCE)
            cnt, box = count_and_box(ref.instance[0][..., 0] if ref.instance.ndim == 4 else ref.instance[0], 7)
            assert pa[i] == cnt[i] and np.array_equal(bo[i], box[i]), "object %d" % i
    finally:
        scene._background_plane_size = keep


def test_outputs_unchanged_by_stats(sl, eng):
    scs = [S.clutter_scene(sl, 30 + k, n_objects=5, size=(160, 120)) for k in range(3)]
    off = eng.render(scs, _abi.OUT_ALL, ssao=True, shadows=True)
    a = {n: getattr(off, n).clone() for n in ("rgb", "coord", "cls", "instance", "normals", "vertex_idx", "bary", "cam_coord")}
    assert off.object_stats is None
    on = eng.render(scs, _abi.OUT_ALL, ssao=True, shadows=True, object_stats=True)
    torch.cuda.synchronize()
    for n, t in a.items():
        assert torch.equal(t.view(torch.uint8), getattr(on, n).view(torch.uint8)), n
    check_visible(on, 6)
    check_invariants(on.object_stats)


def test_pool_overflow_grows_and_repeats(sl, eng):
    scs = [S.clutter_scene(sl, 40 + k, n_objects=5, size=(160, 120)) for k in range(2)]
    ample = eng.render(scs, _abi.OUT_INSTANCE, ssao=False, shadows=False, object_stats=True).object_stats
    srec, drec, crec = build_batch(scs, eng.pool, with_shadows=False)
    small = eng.render_records(srec, drec, crec, 160, 120, _abi.OUT_INSTANCE, ssao=False, shadows=False, object_stats=True,
                               n_slots=6, stats_capacity=4)
    calls = eng.last_stats_calls
    assert calls[0][0] == _abi.OBJECT_STATS_CAPACITY and calls[0][1] == 4 and calls[0][2] > 4
    assert calls[1][0] == 0 and calls[1][1] >= calls[0][2]
    worst = C.c_uint64(0)
    _abi.lib().slhip_render_object_stats_bytes(2, 6, 160, 120, C.byref(worst))
    assert calls[0][2] <= worst.value
    for f in ("px_count_visib", "px_count_all", "bbox_visib", "bbox_obj", "visib_fract"):
        assert torch.equal(getattr(small.object_stats, f), getattr(ample, f)), f


def test_deterministic(sl, eng):
    scs = [S.clutter_scene(sl, 50 + k, n_objects=8, size=(320, 240), with_bunny=True) for k in range(2)]
    a = render_stats(eng, scs).object_stats
    b = render_stats(eng, scs).object_stats
    for f in ("px_count_visib", "px_count_all", "bbox_visib", "bbox_obj", "visib_fract"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    check_invariants(a)


def test_shared_and_large_instance_index(sl, eng):
    """Two objects with one index share a slot (the union of their silhouettes); an index beyond the LDS fast path of the
    visible pass (256 slots) takes the slow path and gives the same numbers."""
    scene = S.clutter_scene(sl, 17, n_objects=4)
    objs = scene.objects
    objs[1].instance_index = 1          # objects 0 and 1 share slot 1
    objs[3].instance_index = 300
    bufs = render_stats(eng, [scene])
    assert bufs.object_stats.n_slots == 301
    check_visible(bufs, 301)
    pv, pa, bv, bo = np_stats(bufs.object_stats, 0)
    for i in (1, 3, 300):
        m = alone(eng, scene, i)
        cnt, box = count_and_box(m.astype(np.int64) * i, i + 1)
        assert pa[i] == cnt[i] and np.array_equal(bo[i], box[i]), i
    assert pa[2] == 0 and pv[2] == 0 and pa[299] == 0


def test_argument_rules(sl, eng):
    scene = S.clutter_scene(sl, 9, n_objects=4, size=(160, 120))
    # depth peel + stats
    rp = sl.RenderPass()
    first = rp.render(scene)
    rp.object_stats_enabled = True
    with pytest.raises(ValueError):
        rp.render(scene, result=sl.RenderPassResult(), depth_peel=first)
    with pytest.raises(ValueError):
        eng.render([scene], _abi.OUT_ALL, depth_peel=torch.zeros((1, 120, 160, 4), device=eng.device), object_stats=True)
    # a predicate's filtered objects are all zero / -1
    bufs = eng.render([scene], _abi.OUT_ALL, predicate=lambda o: o.instance_index != 2, object_stats=True)
    pv, pa, bv, bo = np_stats(bufs.object_stats, 0)
    assert pv[2] == 0 and pa[2] == 0 and list(bv[2]) == EMPTY and list(bo[2]) == EMPTY
    assert float(bufs.object_stats.visib_fract[0, 2]) == 0.0
    check_visible(bufs, 5)
    # RenderPassResult.object_stats(): the single scene's view; raises after a render without stats
    res = rp.render(scene)
    st = res.object_stats()
    assert st.px_count_all.shape == (5,) and st.bbox_obj.shape == (5, 4)
    from stillleben_amd._context import require_context

    assert (st.px_count_visib.device.type == "cuda") == require_context().cuda_outputs   # like the other accessors
    assert len(st.to_bop()) == 4
    rp.object_stats_enabled = False
    res = rp.render(scene)
    with pytest.raises(RuntimeError):
        res.object_stats()


@pytest.fixture(scope="module")
def c2_batch(sl):
    from stillleben_amd import synthetic

    table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=256))
    batch = sl.SceneBatch(table, 256, 20, seed=2027, render_chunk=256)
    batch.set_camera_intrinsics(1066.778, 1067.487, 312.9869, 241.3109)
    batch.stage()
    batch.settle()
    batch.check_settled()
    batch.place()
    return batch


def test_scene_batch_chunk(sl, eng, c2_batch):
    bufs = c2_batch.render(0, object_stats=True)
    torch.cuda.synchronize()
    assert bufs.object_stats.px_count_all.shape == (256, 21)
    check_visible(bufs, 21)
    check_invariants(bufs.object_stats)
    # stats off: the same buffers' statistics are cleared, the outputs the same bits
    inst = bufs.instance.clone()
    again = c2_batch.render(0)
    torch.cuda.synchronize()
    assert again.object_stats is None and torch.equal(again.instance, inst)
    chunks = list(c2_batch.render_chunks(object_stats=True))
    assert len(chunks) == 1 and torch.equal(chunks[0].object_stats.px_count_visib, bufs.object_stats.px_count_visib)
