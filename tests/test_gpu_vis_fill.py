"""k_vis_fill, the pass that initialises the visibility keys and draws the fill draws of a scene (the background plane) with one
store per pixel, against the in-library reference SLHIP_VIS_FILL=0: a memset, the plane through k_raster, the tile queue and
k_large, and k_raster<true> skimming the chunk list.  One batch of seven scenes at 24 x 16, 64 x 48, 40 x 12 and 36 x 20 pixels (the
last two: a partial strip of columns, a single run of rows, rows that are no multiple of four) is rendered both ways in one
process, and every output, the float image behind the tone map, the visibility keys themselves and the per-object statistics
have the same bits:

  (a) the plane under an object with triangles on both sides of kSmallArea (two lights);
  (b) a camera 5 cm over the plane looking down along its diagonal: the plane crosses the near plane inside the picture, and
      each of its triangles becomes two sub-triangles with pixels of their own (checked in the reference's queue);
  (c) no plane: the pass is a pure clear;
  (d) a two-triangle quad floating over the plane and overlapping it on screen: two fill draws, the minimum decides;
  (e) three such quads: more than four eligible triangles, the scene has no fill triangle;
  (f) an object that reaches below the plane;
  (g) a quad with an alpha-tested base texture over the plane (the flag word of the queue header sends k_raster<true> to work),
      and, as a render of its own, scene (a) depth-peeled against its first layer (no fill triangle, every chunk is
      k_raster<true>'s; the statistics pass does not take a peeled render).

With every triangle queued (SLHIP_RASTER_SMALL=0) the reference's queue holds the planes' entries and that of SLHIP_VIS_FILL=3
holds none of a fill draw.  (a) and then (c) are rendered into the same buffers: no key of the first call survives.  The Python API
reaches every case the pass distinguishes; a batch with n_chunks == 0 is reached through scene (c) without its object."""
import contextlib
import os

import numpy as np
import pytest
import torch

from stillleben_amd import _abi, _loaders

pytestmark = pytest.mark.gpu

KEYS = ("SLHIP_VIS_FILL", "SLHIP_RASTER_SMALL", "SLHIP_SHADOW_SMALL")
DEFAULT, REFERENCE = {}, {"SLHIP_VIS_FILL": "0"}
SIZES = [(24, 16), (64, 48), (40, 12), (36, 20)]


@pytest.fixture(scope="module")
def eng(sl):
    from stillleben_amd._context import engine

    return engine()


@contextlib.contextmanager
def environment(mode):
    saved = {k: os.environ.get(k) for k in KEYS}
    try:
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(mode)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def write_obj(path, tris):
    with open(path, "w") as fh:
        for t in tris:
            for p in t:
                fh.write("v %.9g %.9g %.9g\n" % tuple(p))
        for i in range(len(tris)):
            fh.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    return str(path)


def both(t):
    return [t, (t[0], t[2], t[1])]


def quad_mesh(sl, alpha):
    """A 0.4 m square of two triangles; alpha: a base texture with a checker of holes (an alpha-tested draw)."""
    m = _loaders.ConsolidatedMesh()
    m.positions = np.array([[-0.2, -0.2, 0], [0.2, -0.2, 0], [0.2, 0.2, 0], [-0.2, 0.2, 0]], np.float32)
    m.normals = np.array([[0, 0, 1]] * 4, np.float32)
    m.uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    m.colors = np.ones((4, 4), np.float32)
    m.indices = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    y, x = np.mgrid[0:16, 0:16]
    t = np.zeros((16, 16, 4), np.uint8)
    t[..., :3] = (np.random.default_rng(3).random((16, 16, 3)) * 255).astype(np.uint8)
    t[..., 3] = np.where(((x // 4) + (y // 4)) % 2 == 0, 255, 0) if alpha else 255
    m.textures = [t]
    m.tex_samplers = [_abi.SAMPLER_DEFAULT]
    m._tex_alpha = [bool(alpha)]
    m.materials = [_loaders.Material(base_color=(1, 1, 1, 1), metallic=0.0, roughness=0.9, base_texture=0)]
    m.submeshes = [_loaders.SubMesh(0, 6, 0)]
    return sl.Mesh.from_data(m)


def pose(x, y, z, tilt=0.0):
    p = np.eye(4, dtype=np.float32)
    c, s = np.cos(tilt), np.sin(tilt)
    p[:3, :3] = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float32)
    p[:3, 3] = [x, y, z]
    return torch.from_numpy(p)


def make_scene(sl, size, objects, plane=True, eye=(0.0, 0.0, 1.0), at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), lights=1):
    sc = sl.Scene(size)
    for mesh, p in objects:
        o = sl.Object(mesh)
        o.metallic, o.roughness = 0.0, 1.0
        if p is not None:
            o.set_pose(p)
        sc.add_object(o)
    if plane:
        sc.background_plane_size = torch.tensor([3.0, 3.0])
    sc.set_camera_look_at(torch.tensor(eye), torch.tensor(at), up=up)
    dirs = [[-0.3, 0.2, -1.0], [0.5, 0.1, -1.0], [0.0, 0.0, 0.0]]
    cols = [[3.0, 3.0, 3.0], [2.0, 1.0, 0.5], [0.0, 0.0, 0.0]]
    sc.light_directions = torch.tensor([dirs[i] if i < lights else [0.0] * 3 for i in range(3)])
    sc.light_colors = torch.tensor([cols[i] if i < lights else [0.0] * 3 for i in range(3)])
    sc.ambient_light = torch.tensor([0.1, 0.1, 0.1])
    sc.manual_exposure = 1.0
    return sc


def scenes_of(sl, tmp_path, size):
    def mesh(name, tris):
        return sl.Mesh(write_obj(tmp_path / (name + ".obj"), tris), physics=False)

    # one triangle with legs of half a metre (a box of more than kSmallArea pixels at 64 x 48) and six of a few pixels
    obj = both(((-0.3, -0.25, 0.3), (0.2, -0.25, 0.3), (-0.3, 0.25, 0.3)))
    for k in range(6):
        x, y = 0.05 + 0.07 * (k % 3), -0.1 + 0.12 * (k // 3)
        obj += both(((x, y, 0.35), (x + 0.06, y, 0.35), (x, y + 0.08, 0.32)))
    few = both(((-0.1, -0.1, 0.2), (0.15, -0.1, 0.25), (0.0, 0.12, 0.3)))
    # a few centimetres on the ground, 12 cm in front of the low camera of (b)
    low = both(((-0.83, -0.80, 0.003), (-0.78, -0.85, 0.005), (-0.78, -0.80, 0.02)))
    # a wedge through the plane: from 20 cm above it to 15 cm below
    wedge = both(((-0.3, -0.2, 0.2), (0.3, -0.2, 0.2), (0.0, 0.25, -0.15))) + both(((-0.3, 0.2, -0.1), (0.3, 0.2, 0.1), (0.0, -0.2, 0.25)))
    quad, holey = quad_mesh(sl, False), quad_mesh(sl, True)
    return [
        make_scene(sl, size, [(mesh("a", obj), None)], lights=2),                                                    # (a)
        make_scene(sl, size, [(mesh("b", low), None)], eye=(-0.87, -0.9, 0.05), at=(-0.61, -0.6, -0.2), up=(0.0, 0.0, 1.0)),   # (b)
        make_scene(sl, size, [(mesh("c", few), None)], plane=False),                                                   # (c)
        make_scene(sl, size, [(quad, pose(0.05, 0.0, 0.3, 0.3))]),                                                      # (d)
        make_scene(sl, size, [(quad, pose(-0.2, 0.0, 0.2, 0.2)), (quad, pose(0.1, 0.1, 0.3, -0.3)), (quad, pose(0.0, -0.1, 0.4))]),  # (e)
        make_scene(sl, size, [(mesh("f", wedge), None)]),                                                               # (f)
        make_scene(sl, size, [(holey, pose(0.0, 0.05, 0.3, 0.2)), (mesh("g", few), None)]),                            # (g)
    ]


def render(eng, scenes, mode, stats=True, buffers=None, depth_peel=None):
    W, H = scenes[0].viewport
    with environment(mode):
        bufs = eng.render(scenes, _abi.OUT_ALL, ssao=True, shadows=True, keep_hdr=True, object_stats=stats, buffers=buffers,
                          depth_peel=depth_peel)
        torch.cuda.synchronize()
    out = {}
    for name in ("rgb", "instance", "cls", "vertex_idx", "coord", "bary", "cam_coord", "normals"):
        out[name] = getattr(bufs, name).cpu().numpy().copy()
    n = len(scenes) * H * W
    out["hdr"] = bufs._keepalive[0]["hdr"].view(torch.float32)[:2 * n * 4].cpu().numpy().copy()
    out["vis"] = bufs._keepalive[0]["vis"][:8 * n].cpu().numpy().copy()
    if stats:
        st = bufs.object_stats
        for name in ("px_count_visib", "px_count_all", "bbox_visib", "bbox_obj"):
            out["stats_" + name] = getattr(st, name).cpu().numpy().copy()
    return bufs, out


def assert_same_bits(ref, out, what):
    assert set(out) == set(ref)
    for name, a in ref.items():
        b = out[name]
        same = a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        assert same, "%s differs %s at %d values" % (name, what, int((a != b).sum()))


def queued_draws(bufs):
    """(draw, sub-triangle) of the queue entries the visibility pass left (no statistics pass behind it: it reuses the queue)."""
    q = bufs._keepalive[0]["queue"]
    n = int(q[:4].view(torch.int32).cpu().numpy().view(np.uint32)[0])
    e = q[16:16 + 32 * n].view(torch.int32).cpu().numpy().view(np.uint32).reshape(n, 8)
    return e[:, 0], e[:, 1] >> 31


@pytest.mark.parametrize("size", SIZES)
def test_fill_pass_equals_the_reference_sequence(sl, eng, tmp_path, size):
    from stillleben_amd._batch import HostPool, build_batch

    W, H = size
    scenes = scenes_of(sl, tmp_path, size)
    srec, drec, _ = build_batch(scenes, HostPool())
    first = [int(b) for b in srec["draw_begin"]]
    plane = {first[i] for i in (0, 1, 3, 4, 5, 6)}                   # draw 0 of every scene but (c)
    assert all(int(drec["n_tris"][d]) == 2 for d in plane)
    assert drec["flags"][first[6] + 1] & _abi.DRAW_ALPHA_TEST        # (g): the holey quad

    _, ref = render(eng, scenes, REFERENCE)
    inst = ref["instance"].reshape(len(scenes), H, W)
    assert all((inst[i] != 0).any() for i in range(len(scenes))), "an object of every scene is in the picture"
    keys = ref["vis"].view(np.uint64).reshape(len(scenes), H * W)
    assert (keys[0] != np.uint64(0xFFFFFFFFFFFFFFFF)).all()          # (a): the plane fills the picture ...
    assert (keys[2] == np.uint64(0xFFFFFFFFFFFFFFFF)).any()          # ... (c) has background
    _, out = render(eng, scenes, DEFAULT)
    assert_same_bits(ref, out, "between SLHIP_VIS_FILL=0 and the default")
    for knob in ("1", "2"):                                           # the two halves of the knob on their own
        _, out = render(eng, scenes, {"SLHIP_VIS_FILL": knob})
        assert_same_bits(ref, out, "under SLHIP_VIS_FILL=" + knob)

    # who draws the planes: with every triangle queued the reference's queue holds them -- (b)'s clipped triangle as two
    # sub-triangles -- and the default's holds the plane of (e) only, whose scene has no fill triangle
    all_queued = {"SLHIP_RASTER_SMALL": "0", "SLHIP_SHADOW_SMALL": "0"}
    bufs, _ = render(eng, scenes, dict(REFERENCE, **all_queued), stats=False)
    draws, sub = queued_draws(bufs)
    assert plane <= set(draws.tolist())
    assert ((draws == first[1]) & (sub == 1)).sum() == 2 and ((draws == first[1]) & (sub == 0)).sum() == 2
    bufs, out = render(eng, scenes, dict(all_queued, SLHIP_VIS_FILL="3"), stats=False)   # (SLHIP_RASTER_SMALL alone would send the fill draws to the queue as well)
    draws, _ = queued_draws(bufs)
    assert set(draws.tolist()) & plane == {first[4]}
    assert first[3] + 1 not in set(draws.tolist())                    # (d): the quad is a fill draw too
    assert first[4] + 1 in set(draws.tolist())                        # (e): its quads are not
    assert_same_bits({k: v for k, v in ref.items() if not k.startswith("stats_")}, out, "with every triangle queued")


@pytest.mark.parametrize("size", [(24, 16), (40, 12)])
def test_nothing_of_an_earlier_call_survives(sl, eng, tmp_path, size):
    scenes = scenes_of(sl, tmp_path, size)
    a, c = [scenes[0]], [scenes[2]]
    for objects in (True, False):
        if not objects:
            c = [make_scene(sl, size, [], plane=False)]               # no draw, no chunk: the pass still clears
        _, ref = render(eng, c, REFERENCE, stats=objects)
        for mode in (DEFAULT, REFERENCE):
            bufs, _ = render(eng, a, mode, stats=objects)
            _, out = render(eng, c, DEFAULT, stats=objects, buffers=bufs)             # same output buffers, same scratch: the keys of (a) are there
            assert_same_bits(ref, out, "after a render of the plane into the same buffers")
        assert (out["vis"].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).any()


@pytest.mark.parametrize("size", [(64, 48), (36, 20)])
def test_depth_peeled_render_has_no_fill_triangle(sl, eng, tmp_path, size):
    scenes = scenes_of(sl, tmp_path, size)
    a = [scenes[0]]
    first, _ = render(eng, a, REFERENCE, stats=False)
    peel = first.coord.clone()
    _, ref = render(eng, a, REFERENCE, stats=False, depth_peel=peel)
    _, out = render(eng, a, DEFAULT, stats=False, depth_peel=peel)
    assert_same_bits(ref, out, "depth-peeled")
    assert not np.array_equal(ref["instance"], first.instance.cpu().numpy())   # the second layer is another picture
