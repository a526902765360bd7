"""What a render leaves behind in its scratch set.  slhip_render keeps its shadow maps CLEAN BETWEEN CALLS: k_shadow_raster marks
the 64 x 64-texel tiles its casters touch, k_shadow_restore puts exactly those back to 1.0 after k_shade, and only the first call
on a scratch set clears the maps wholesale (RENDER_SHADOW_RESET, `shadow_ready` of Engine.scratch).  A texel written outside a
marked tile would stay until a later render on that scratch marks its tile and reads it as a caster.  Two kinds of test:

  * after a render (synchronised) every word of the maps in use is 1.0 and every tile bit 0 (`scratch_is_clean`, counted on the
    device) -- under the three raster modes of tests/test_gpu_raster_paths.py, with one and three maps per scene, batches of two
    (maps are laid out [scene][nl], tile bits [scene][SLHIP_NUM_LIGHTS][words]), casters across the map's edges, renders that must
    not touch the maps at all, depth peeling, a predicate, and the chunks of a settled SceneBatch without and with an environment
    bank;
  * a render Y after a render X on the same scratch set gives the bytes of Y on a cold one: every output of OUT_ALL and the float
    image (the queue header, d_ao, d_lum and the per-stream clip buffer survive between calls as well).

Both have their control: the helper reports a texel and a tile bit written through the torch view of the scratch, and a stale
tile under Y's casters changes Y's float image.  Everything runs on the default stream."""
import contextlib
import os

import numpy as np
import pytest
import torch

import scenes as SC
from stillleben_amd import _abi
from test_gpu_raster_paths import MODES, S, calibrate, caster_boxes, main_soups, scene_of, strip_scene
from test_gpu_render import eng  # noqa: F401   (the module-scoped engine fixture)

pytestmark = pytest.mark.gpu

ONE = 0x3F800000            # 1.0f: a clean texel
TILE = 64                   # kShadowTile
TILES_X = S // TILE
WORDS = (TILES_X * TILES_X + 31) // 32      # shadow_tile_words(S)
OUTPUTS = ("rgb", "instance", "cls", "vertex_idx", "coord", "bary", "cam_coord", "normals")


# ---- the helper -----------------------------------------------------------------------------------------------------------------
def maps_of(keep, B):
    """(maps [B, nl, S, S], tile bits [B, SLHIP_NUM_LIGHTS, words]) as int32 views of a scratch set's buffers, the words in use."""
    nl = keep["shadow"].numel() // (B * S * S * 4)
    assert 1 <= nl <= _abi.NUM_LIGHTS
    maps = keep["shadow"].view(torch.int32)[: B * nl * S * S].view(B, nl, S, S)
    bits = keep["tiles"].view(torch.int32)[: B * _abi.NUM_LIGHTS * WORDS].view(B, _abi.NUM_LIGHTS, WORDS)
    return maps, bits


def keep_is_clean(keep, B):
    """None if the B scenes' maps of the scratch set `keep` are all 1.0 and all its tile bits 0, else a sentence that names the
    first offender.  Counts on the device: a map is 16.8 MB per scene and light."""
    if keep["shadow"] is None:
        return None if keep["tiles"] is None else "tile bits without maps"
    maps, bits = maps_of(keep, B)
    nl = maps.shape[1]
    said = []
    dirty = maps != ONE
    n = int(dirty.sum())
    if n:
        i = int(dirty.view(-1).nonzero()[0])
        scene, light, y, x = i // (nl * S * S), i // (S * S) % nl, i // S % S, i % S
        said.append("%d texel(s) not 1.0; the first: scene %d, light %d, tile (%d, %d) = bit %d, texel (%d, %d) = 0x%08x"
                    % (n, scene, light, x // TILE, y // TILE, (y // TILE) * TILES_X + x // TILE, x, y,
                       int(maps.view(-1)[i]) & 0xFFFFFFFF))
    marked = bits != 0
    n = int(marked.sum())
    if n:
        i = int(marked.view(-1).nonzero()[0])
        scene, light, w = i // (_abi.NUM_LIGHTS * WORDS), i // WORDS % _abi.NUM_LIGHTS, i % WORDS
        word = int(bits.view(-1)[i]) & 0xFFFFFFFF
        tile = 32 * w + (word & -word).bit_length() - 1
        said.append("%d word(s) of tile bits not 0; the first: scene %d, light %d, word %d = 0x%08x: tile (%d, %d), first texel (%d, %d)"
                    % (n, scene, light, w, word, tile % TILES_X, tile // TILES_X, tile % TILES_X * TILE, tile // TILES_X * TILE))
    return "; ".join(said) if said else None


def scratch_is_clean(bufs):
    """Asserts that the scratch set behind `bufs` (the render must have been synchronised) is what the next call expects."""
    why = keep_is_clean(bufs._keepalive[0], bufs.B)
    assert why is None, why


# ---- scenes and renders ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def calibrated_here(sl, tmp_path_factory):
    calibrate(sl, tmp_path_factory.mktemp("scratch_frame"))


@contextlib.contextmanager
def under(mode):
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


def collect(bufs, keep_hdr):
    """The outputs of `bufs` and the float image of its scratch set as numpy arrays (render_modes of test_gpu_raster_paths.py)."""
    out = {}
    for name in OUTPUTS:
        t = getattr(bufs, name, None)
        if t is not None:
            out[name] = t.cpu().numpy().copy()
    n = (2 if keep_hdr else 1) * bufs.B * bufs.H * bufs.W * 4
    out["hdr"] = bufs._keepalive[0]["hdr"].view(torch.float32)[:n].cpu().numpy().copy()
    return out


def render(eng, scenes, mode=MODES[0], **kw):
    with under(mode):
        bufs = eng.render(scenes, _abi.OUT_ALL, ssao=True, shadows=True, keep_hdr=True, **kw)
        torch.cuda.synchronize()
    return bufs


def cold(eng):
    """The next render allocates its scratch anew and resets it."""
    torch.cuda.synchronize()
    eng._scratch.clear()
    eng.__dict__.setdefault("_clips", {}).clear()


def assert_same_bytes(ref, out, what):
    assert set(out) == set(ref) and {"rgb", "instance", "coord", "normals", "hdr"} <= set(ref)
    for name, a in ref.items():
        b = out[name]
        same = a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert same, "%s differs %s at %d values" % (name, what, int((a != b).sum()))


class Scenes:
    pass


@pytest.fixture(scope="module")
def world(sl, tmp_path_factory):
    d = tmp_path_factory.mktemp("scratch_scenes")
    w = Scenes()
    w.main = {(1, (128, 96)): scene_of(sl, d, main_soups(), (128, 96), lights=1),
              (3, (130, 98)): scene_of(sl, d, main_soups(), (130, 98), lights=3),
              (1, (130, 98)): scene_of(sl, d, main_soups(), (130, 98), lights=1)}
    # (automatic exposure: d_lum, which survives between calls as well, decides its picture)
    w.clutter = {size: SC.clutter_scene(sl, 5, n_objects=6, size=size) for size in ((128, 96), (130, 98))}
    w.strips = [strip_scene(sl, d, h) for h in (0.9, 1.3)]
    w.dark = scene_of(sl, d, main_soups(), (128, 96), lights=0)
    return w


# ---- the control of the helper --------------------------------------------------------------------------------------------------
def test_the_helper_reports_a_texel_and_a_tile_bit(sl, eng, world):
    """No kernel involved: one texel, then one tile bit, written through the torch view of a clean scratch set."""
    bufs = render(eng, [world.clutter[(128, 96)], world.main[(1, (128, 96))]])
    keep = bufs._keepalive[0]
    try:
        scratch_is_clean(bufs)
        maps, bits = maps_of(keep, 2)
        assert maps.shape == (2, 1, S, S) and bits.shape == (2, 3, WORDS)
        maps[1, 0, 777, 1300] = 0x3F000000                      # 0.5 in scene 1: tile (20, 12)
        torch.cuda.synchronize()
        why = keep_is_clean(keep, 2)
        assert why is not None and "1 texel(s)" in why and "scene 1, light 0, tile (20, 12)" in why and "texel (1300, 777) = 0x3f000000" in why
        assert "tile bits" not in why
        with pytest.raises(AssertionError):
            scratch_is_clean(bufs)
        maps[1, 0, 777, 1300] = ONE
        assert keep_is_clean(keep, 2) is None
        bits[1, 0, 5] = 1 << 9                                  # tile 169 = (9, 5) of scene 1
        torch.cuda.synchronize()
        why = keep_is_clean(keep, 2)
        assert why is not None and "1 word(s)" in why and "scene 1, light 0, word 5" in why and "tile (9, 5), first texel (576, 320)" in why
        assert "texel(s) not 1.0" not in why
        bits[1, 0, 5] = 0
        assert keep_is_clean(keep, 2) is None
    finally:
        keep["shadow_ready"] = False                             # the next call on this scratch set resets it


# ---- 1, 2: the raster modes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lights,size", [(1, (128, 96)), (3, (130, 98))])
@pytest.mark.parametrize("batch", [1, 2])
def test_main_scene_leaves_clean_maps(sl, eng, world, lights, size, batch):
    """The main scene of test_gpu_raster_paths.py (boxes on every threshold of the shadow kernels) alone, and as scene 1 of a batch
    behind a different scene -- with one map per scene that is where the strides of maps and tile bits differ."""
    scenes = [world.main[(lights, size)]] if batch == 1 else [world.clutter[size], world.main[(lights, size)]]
    for mode in MODES:
        bufs = render(eng, scenes, mode)
        assert maps_of(bufs._keepalive[0], batch)[0].shape[1] == lights
        scratch_is_clean(bufs)
    bufs = render(eng, scenes)                                   # ... and of a call that did not reset
    scratch_is_clean(bufs)


def test_strips_across_the_map_edges_leave_clean_maps(sl, eng, world):
    for mode in MODES:
        bufs = render(eng, world.strips, mode)
        scratch_is_clean(bufs)


# ---- 3: renders that must not touch the maps ------------------------------------------------------------------------------------
def test_a_render_without_rgb_has_no_maps(sl, eng, world):
    bufs = eng.render([world.main[(1, (128, 96))]], _abi.OUT_ALL & ~_abi.OUT_RGB, ssao=True, shadows=True)
    torch.cuda.synchronize()
    keep = bufs._keepalive[0]
    assert keep["shadow"] is None and keep["tiles"] is None and not keep["shadow_ready"]
    scratch_is_clean(bufs)


@pytest.mark.parametrize("what", ["empty", "dark"])
def test_maps_untouched(sl, eng, world, what):
    """A batch of empty scenes (no chunk: the restore is skipped) and a scene whose only light is off: the first call resets the
    maps, the second writes nothing -- not even 1.0: maps filled with 0.5 behind the engine's back are 0.5 afterwards."""
    scenes = [sl.Scene((128, 96)), sl.Scene((128, 96))] if what == "empty" else [world.dark]
    cold(eng)
    bufs = render(eng, scenes)
    keep = bufs._keepalive[0]
    try:
        assert keep["shadow_ready"]
        scratch_is_clean(bufs)
        maps, bits = maps_of(keep, len(scenes))
        maps.fill_(0x3F000000)
        bufs = render(eng, scenes)
        assert bufs._keepalive[0] is keep
        assert int((maps != 0x3F000000).sum()) == 0 and int((bits != 0).sum()) == 0
    finally:
        keep["shadow_ready"] = False


# ---- 4: depth peeling, predicate ------------------------------------------------------------------------------------------------
def test_depth_peel_and_predicate_leave_clean_maps(sl, eng, world):
    scene = world.main[(1, (128, 96))]
    first = render(eng, [scene])
    scratch_is_clean(first)
    peeled = render(eng, [scene], depth_peel=first.coord.clone())
    scratch_is_clean(peeled)
    assert not torch.equal(peeled.instance, first.instance)
    n_objects = len(scene._objects)
    part = render(eng, [scene], predicate=lambda o: o.instance_index % 2 == 0)      # every other caster is gone
    scratch_is_clean(part)
    seen = set(np.unique(part.instance.cpu().numpy().view(np.uint16)).tolist())
    assert seen - {0} and all(i % 2 == 0 for i in seen) and n_objects >= 8
    again = render(eng, [scene])                                # ... and the full scene after them, on the same scratch
    scratch_is_clean(again)
    for name in OUTPUTS:                                         # (as bytes: the background's normals are not numbers)
        assert torch.equal(getattr(again, name).view(torch.uint8), getattr(first, name).view(torch.uint8)), name


# ---- 5: the chunks of a settled SceneBatch --------------------------------------------------------------------------------------
def settled(batch):
    batch.set_camera_intrinsics(533.389, 533.7435, 156.49345, 120.65545)
    batch.stage()
    batch.settle()
    batch.check_settled()
    batch.place()
    torch.cuda.synchronize()
    return batch


@pytest.fixture(scope="module")
def table(sl):
    from stillleben_amd import synthetic

    return sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))


@pytest.fixture(scope="module")
def plain_batch(sl, table):
    """The fixture shape of test_gpu_object_masks.py::small_batch, doubled: two render chunks, one map per scene."""
    return settled(sl.SceneBatch(table, 16, 6, resolution=(320, 240), seed=2027, render_chunk=8))


@pytest.fixture(scope="module")
def bank_batch(sl, table):
    """The same on the environment bank of test_gpu_environment.py: three maps per scene; light sets of 1, 3 and 0 lights and the
    drawn light (-1) in turn, so that every chunk has scenes with 0, 1 and 3 lights."""
    from test_gpu_environment import make_light_maps, make_textures

    bgs, pts = make_textures(sl, 11)
    bank = sl.EnvironmentBank(make_light_maps(sl), bgs, pts)
    assert bank.max_lights == 3
    ids = np.array([[(0, 1, 2, -1)[s % 4], s % 3, -1] for s in range(16)], np.int32)
    return settled(sl.SceneBatch(table, 16, 6, resolution=(320, 240), seed=2027, render_chunk=8, environment=bank, env_ids=ids))


def chunk(batch, c):
    """Render chunk c of the batch, OUT_ALL; SceneBatch.render keeps no second float image: the shaded one (before SSAO) is there."""
    bufs = batch.render(c, _abi.OUT_ALL, ssao=True)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("which", ["plain", "bank"])
def test_scene_batch_chunks_leave_clean_maps(sl, eng, request, which):
    batch = request.getfixturevalue(which + "_batch")
    if which == "bank":
        srec = batch.host_render_records()[0]
        on = (np.abs(srec["light_color"][:, :, :3]).sum(axis=2) > 0) & (np.abs(srec["light_dir"][:, :, :3]).sum(axis=2) > 0)
        for c in range(2):
            assert {0, 1, 3} <= set(on[8 * c:8 * c + 8].sum(axis=1).tolist())
    for c in (0, 1, 0):
        bufs = chunk(batch, c)
        assert bufs.B == 8 and maps_of(bufs._keepalive[0], 8)[0].shape[1] == (1 if which == "plain" else 3)
        scratch_is_clean(bufs)
        assert int((bufs.instance != 0).sum()) > 0


# ---- sequence equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["strips", "tiled"])
def test_second_render_on_a_scratch_equals_a_cold_one(sl, eng, world, pair):
    """Strip scenes (casters across all four map edges), then the main scene and a clutter scene, on one scratch set (B = 2,
    130 x 98, one light) -- and the other way round: the second render's bytes are those of a cold scratch.  `tiled`: the main
    scene and the clutter scene in turn at 128 x 96, where k_shade places its blocks on tiles and the SSAO pass keeps tile
    records and skip bytes in d_ao."""
    if pair == "strips":
        X, Y = world.strips, [world.main[(1, (130, 98))], world.clutter[(130, 98)]]
    else:
        X, Y = [world.main[(1, (128, 96))]], [world.clutter[(128, 96)]]
    for first, second, what in ((X, Y, "after the other scenes"), (Y, X, "after the other scenes, the other way round")):
        cold(eng)
        ref_bufs = render(eng, second)
        ref = collect(ref_bufs, True)
        cold(eng)
        a = render(eng, first)
        assert a._keepalive[0]["shadow_ready"]
        b = render(eng, second)
        assert b._keepalive[0] is a._keepalive[0] and b._keepalive[0] is not ref_bufs._keepalive[0]
        assert_same_bytes(ref, collect(b, True), what)
        scratch_is_clean(b)


@pytest.mark.parametrize("which", ["plain", "bank"])
def test_scene_batch_chunk_after_chunk_equals_a_cold_one(sl, eng, request, which):
    batch = request.getfixturevalue(which + "_batch")
    for first, second in ((0, 1), (1, 0)):
        cold(eng)
        ref_bufs = chunk(batch, second)
        ref = collect(ref_bufs, False)
        cold(eng)
        a = chunk(batch, first)
        b = chunk(batch, second)
        assert b._keepalive[0] is a._keepalive[0] and b._keepalive[0] is not ref_bufs._keepalive[0]
        assert_same_bytes(ref, collect(b, False), "chunk %d after chunk %d" % (second, first))


def test_a_stale_tile_would_be_seen(sl, eng, world):
    """The condition of the sequence tests: a 64 x 64 tile of 0.0 (nearest depth) left under Y's casters, its bit not set, changes
    Y's float image.  The tile: the one most of the main scene's drawn boxes touch, among the 8 x 8 tiles about the map's
    centre (which the camera looks at)."""
    Y = [world.main[(1, (130, 98))], world.clutter[(130, 98)]]
    boxes, _ = caster_boxes(Y[0])
    hits = np.zeros((TILES_X, TILES_X), np.int64)
    for t in boxes:
        d = t["drawn"]
        for x0, x1, y0, y1 in zip(t["xmin"][d] // TILE, t["xmax"][d] // TILE, t["ymin"][d] // TILE, t["ymax"][d] // TILE):
            hits[y0:y1 + 1, x0:x1 + 1] += 1
    lo, hi = TILES_X // 2 - 4, TILES_X // 2 + 4
    ty, tx = np.unravel_index(np.argmax(hits[lo:hi, lo:hi]), (hi - lo, hi - lo))
    ty, tx = int(ty) + lo, int(tx) + lo
    assert hits[ty, tx] > 0
    cold(eng)
    ref = collect(render(eng, Y), True)
    cold(eng)
    bufs = render(eng, Y)
    keep = bufs._keepalive[0]
    try:
        assert_same_bytes(ref, collect(bufs, True), "between two cold renders")
        maps, _ = maps_of(keep, 2)
        maps[0, 0, ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE] = 0      # 0.0f
        assert keep["shadow_ready"]
        out = collect(render(eng, Y), True)
        assert not np.array_equal(out["hdr"].view(np.uint8), ref["hdr"].view(np.uint8)), "a stale tile (%d, %d) went unseen" % (tx, ty)
        assert np.array_equal(out["instance"], ref["instance"])  # (shadows only: the geometry is what it was)
    finally:
        keep["shadow_ready"] = False
