"""The large-triangle queue of the raster passes (stillleben_amd/csrc/slhip_tile_queue.h) on the device: one entry per queued
triangle, the 8 x 8 tiles of its box enumerated by k_large, k_shadow_large and k_os_large.  Two small scenes in one batch -- a
plane of two triangles under an object with triangles on both sides of kSmallArea and two active lights; a large triangle that
crosses the near plane, so that both of its sub-triangles are queued -- are rendered at 24 x 16 and 64 x 48 pixels

  - with the default thresholds, with SLHIP_RASTER_SMALL = SLHIP_SHADOW_SMALL = 0 (every triangle queued) and with both at 2^30
    (nothing queued), and
  - with everything queued into a queue of the test's own of 0, 1, 2, 3 units and of two units less than the visibility pass
    needs (the triangles that do not fit are walked in place by their producers),

and every output, the float image behind the tone map and the per-object statistics have the same bits every time.  The queue
of the test's own has guard bytes behind it, which stay as they were."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

from stillleben_amd import _abi

pytestmark = pytest.mark.gpu

MODES = ({}, {"SLHIP_RASTER_SMALL": "0", "SLHIP_SHADOW_SMALL": "0"},
         {"SLHIP_RASTER_SMALL": str(1 << 30), "SLHIP_SHADOW_SMALL": str(1 << 30)})
QUEUE_ALL = MODES[1]
GUARD = 256                 # bytes behind the test's own queue


def write_obj(path, tris):
    with open(path, "w") as fh:
        for t in tris:
            for p in t:
                fh.write("v %.9g %.9g %.9g\n" % tuple(p))
        for i in range(len(tris)):
            fh.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    return str(path)


def both(t):
    """A triangle and its mirror image: one of them faces the camera, one the light."""
    return [t, (t[0], t[2], t[1])]


def make_scene(sl, tmp_path, name, size, tris, lights):
    sc = sl.Scene(size)
    o = sl.Object(sl.Mesh(write_obj(tmp_path / (name + ".obj"), tris), physics=False))
    o.metallic, o.roughness = 0.0, 1.0
    sc.add_object(o)
    sc.background_plane_size = torch.tensor([3.0, 3.0])
    sc.set_camera_look_at(torch.tensor([0.0, 0.0, 1.0]), torch.tensor([0.0, 0.0, 0.0]), up=(0.0, 1.0, 0.0))
    dirs = [[-0.3, 0.2, -1.0], [0.5, 0.1, -1.0], [0.0, 0.0, 0.0]]
    cols = [[3.0, 3.0, 3.0], [2.0, 1.0, 0.5], [0.0, 0.0, 0.0]]
    sc.light_directions = torch.tensor([dirs[i] if i < lights else [0.0] * 3 for i in range(3)])
    sc.light_colors = torch.tensor([cols[i] if i < lights else [0.0] * 3 for i in range(3)])
    sc.ambient_light = torch.tensor([0.1, 0.1, 0.1])
    sc.manual_exposure = 1.0
    return sc


def scenes_of(sl, tmp_path, size):
    # scene 0: the plane (two triangles that fill the picture) under an object 30 cm above it -- one triangle with legs of half
    # a metre (41 pixels at 64 x 48: a box of more than kSmallArea pixels) and six of a few pixels; two lights
    obj = both(((-0.3, -0.25, 0.3), (0.2, -0.25, 0.3), (-0.3, 0.25, 0.3)))
    for k in range(6):
        x, y = 0.05 + 0.07 * (k % 3), -0.1 + 0.12 * (k // 3)
        obj += both(((x, y, 0.35), (x + 0.06, y, 0.35), (x, y + 0.08, 0.32)))
    # scene 1: one large triangle with a vertex behind the camera (which sits at z = 1, looking down): clipped at the near plane
    # it is a quadrilateral, two sub-triangles; one light
    cross = both(((-0.4, -0.3, 0.2), (0.4, -0.3, 0.2), (0.0, 0.2, 1.5)))
    return [make_scene(sl, tmp_path, "object", size, obj, lights=2), make_scene(sl, tmp_path, "crossing", size, cross, lights=1)]


@pytest.fixture(scope="module")
def eng(sl):
    from stillleben_amd._context import engine

    return engine()


@contextlib.contextmanager
def environment(mode):
    keys = {k for m in MODES for k in m}
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(mode)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def own_queue(eng, units):
    """Renders inside use a queue of `units` 16-byte units that belongs to the test, sized by slhip_render_scratch_bytes, with GUARD
    bytes of 0xAB behind it."""
    sizes = (C.c_uint64 * 7)()
    eng.L.slhip_render_scratch_bytes(1, 8, 8, 0, units, C.byref(sizes))
    nbytes = int(sizes[4])
    assert nbytes == 16 + 16 * units
    q = torch.full((nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=eng.device)
    inner = eng.scratch

    def scratch(*args, **kw):
        a, keep = inner(*args, **kw)
        a.d_queue = C.c_void_p(q.data_ptr())
        a.queue_capacity = units
        return a, keep

    eng.scratch = scratch
    try:
        yield q, nbytes
    finally:
        del eng.scratch


def render(eng, scenes, mode, stats=True):
    W, H = scenes[0].viewport
    with environment(mode):
        bufs = eng.render(scenes, _abi.OUT_ALL, ssao=True, shadows=True, keep_hdr=True, object_stats=stats)
        torch.cuda.synchronize()
    out = {}
    for name in ("rgb", "instance", "cls", "vertex_idx", "coord", "bary", "cam_coord", "normals"):
        out[name] = getattr(bufs, name).cpu().numpy().copy()
    n = 2 * len(scenes) * H * W * 4
    out["hdr"] = bufs._keepalive[0]["hdr"].view(torch.float32)[:n].cpu().numpy().copy()
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


def queue_entries(q):
    """(entries, tiles, carried) of the header and the entries [n, 8] of a queue tensor, as the last pass left them."""
    head = q[:16].view(torch.int32).cpu().numpy().view(np.uint32)
    n = int(head[0])
    return head, q[16:16 + 32 * n].view(torch.int32).cpu().numpy().view(np.uint32).reshape(n, 8)


@pytest.mark.parametrize("size", [(24, 16), (64, 48)])
def test_one_picture_however_the_large_triangles_are_walked(sl, eng, tmp_path, size):
    W, H = size
    scenes = scenes_of(sl, tmp_path, size)
    _, ref = render(eng, scenes, MODES[0])
    inst = ref["instance"].reshape(2, H, W)
    assert (inst[0] != 0).any() and (inst[1] != 0).any() and (inst == 0).any()       # both objects and the plane are in the picture
    assert int(ref["stats_px_count_all"].sum()) > 0
    hdr = ref["hdr"][: H * W * 4].reshape(H, W, 4)[..., 0][inst[0] == 0]
    assert (hdr < 0.8 * np.median(hdr)).any()                                         # ... and so is the object's shadow
    for mode in MODES[1:]:
        _, out = render(eng, scenes, mode)
        assert_same_bits(ref, out, "under %s" % mode)

    # what the visibility pass queues when everything is queued (no statistics pass behind it: it reuses the queue)
    bufs, _ = render(eng, scenes, QUEUE_ALL, stats=False)
    head, entries = queue_entries(bufs._keepalive[0]["queue"])
    assert head[2] == 0 and len(entries) >= 2 * 2 + 3                                 # two planes, the objects' triangles
    assert set(entries[:, 2].tolist()) == {0, 1}                                      # both scenes of the batch
    ntiles = (entries[:, 5] & 0xFFFF) * (entries[:, 5] >> 16)
    assert (ntiles > 0).all() and int(ntiles.sum()) == int(head[1])
    assert np.array_equal(entries[:, 3], np.concatenate([[0], np.cumsum(ntiles)[:-1]]))   # ordered by tile_base, no gaps
    assert ntiles.max() == ((W + 7) // 8) * ((H + 7) // 8)                              # the plane's box is the picture
    sub1 = entries[(entries[:, 1] >> 31) == 1]
    assert len(sub1) >= 1                                                             # the second sub-triangle of the clipped one ...
    firsts = {(int(e[0]), int(e[1]), int(e[2])) for e in entries[(entries[:, 1] >> 31) == 0]}
    assert all((int(e[0]), int(e[1]) & 0x7FFFFFFF, int(e[2])) in firsts for e in sub1)   # ... beside its first
    need = 2 * len(entries)

    for units in (0, 1, 2, 3, need - 2):
        with own_queue(eng, units) as (q, nbytes):
            _, out = render(eng, scenes, QUEUE_ALL)
            assert bool((q[nbytes:] == 0xAB).all()), "bytes behind a queue of %d units were written" % units
        assert_same_bits(ref, out, "with a queue of %d units" % units)
