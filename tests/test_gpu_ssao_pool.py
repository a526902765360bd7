"""The SSAO tap kernel drains the level queues of a block's four waves as ONE list at the end of a band (slhip_render.hip
k_ssao_tiled).  That is placement: rgb and the kept float image are bit for bit those of the per-wave drain (SLHIP_SSAO_POOL=0) and
of every tile at the full list (SLHIP_SSAO_DEBUG=2), at every band depth.  SLHIP_SSAO_APPLY_TILED=0 belongs to a tiled placement of
the blur pass that was measured slower and is not in the library (profiles/r17): the variable is rendered with all the same, so
that whoever brings the placement back finds its check here.  The scenes are those of tests/test_ssao_levels.py (batch_320 /
batch_64), restated here."""
import os

import numpy as np
import pytest
import torch

from stillleben_amd import _abi

KNOBS = ("SLHIP_SSAO_DEBUG", "SLHIP_SSAO_BAND_ROWS", "SLHIP_SSAO_POOL", "SLHIP_SSAO_APPLY_TILED")
# the four ways of the picture: as it is, the per-wave drain, every tile at the full list, the blur by strips
WAYS = ({}, {"SLHIP_SSAO_POOL": 0}, {"SLHIP_SSAO_DEBUG": 2}, {"SLHIP_SSAO_APPLY_TILED": 0})


@pytest.fixture(scope="module")
def ycb_table(sl):
    from stillleben_amd import synthetic

    sl.init_cuda(0)
    return sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))


def settled_batch(sl, table, n_scenes, n_objects, resolution, intrinsics, seed):
    batch = sl.SceneBatch(table, n_scenes, n_objects, resolution=resolution, seed=seed, manual_exposure=1.0)
    batch.set_camera_intrinsics(*intrinsics)
    batch.stage()
    batch.settle(frames=20)
    batch.place()
    return batch


def render(batch, **env):
    """Render chunk 0 of the batch with the given variables set (all are read at every slhip_render).  Returns (rgb, float image
    behind it), the level read-out and the run read-out."""
    md, mk, mv = (int(batch.params[k]) for k in ("max_draws_per_scene", "max_chunks_per_scene", "max_clip_verts_per_scene"))
    W, H = batch.resolution
    B = batch.n_scenes
    batch.eng.pool_abi()
    assert not any(k in os.environ for k in KNOBS)
    os.environ.update({k: str(v) for k, v in env.items() if v is not None})
    try:
        buf = batch.eng.render_device(batch.d_srec.data_ptr(), batch.d_drec.data_ptr(), batch.d_crec.data_ptr(), B, B * md, B * mk,
                                      B * mv, W, H, _abi.OUT_ALL, ssao=True, shadows=batch.shadows, shadow_lights=1, keep_hdr=True)
        torch.cuda.synchronize()
    finally:
        for k in env:
            os.environ.pop(k, None)
    hdr = buf._keepalive[0]["hdr"].view(torch.float32)[: 2 * B * H * W * 4].reshape(2, B, H, W, 4)[1].cpu().numpy().copy()
    return (buf.rgb.cpu().numpy().copy(), hdr), batch.eng.ssao_levels(buf, W, H), batch.eng.ssao_run_slots(buf, W, H)


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


class Case:
    """A settled batch and its reference picture: every tile at the full list, per-wave drain, blur by strips -- rendered once."""

    def __init__(self, batch):
        self.batch = batch
        self.reference, _, _ = render(batch, SLHIP_SSAO_DEBUG=2, SLHIP_SSAO_POOL=0, SLHIP_SSAO_APPLY_TILED=0)
        for a in self.reference:
            a.setflags(write=False)


@pytest.fixture(scope="module")
def case_320(sl, ycb_table):
    return Case(settled_batch(sl, ycb_table, 2, 8, (320, 240), (533.4, 533.7, 156.5, 120.6), seed=9))


@pytest.fixture(scope="module")
def case_64(sl, ycb_table):
    return Case(settled_batch(sl, ycb_table, 2, 6, (64, 32), (106.7, 106.7, 31.3, 16.1), seed=11))


@pytest.fixture(scope="module")
def case_40(sl, ycb_table):
    return Case(settled_batch(sl, ycb_table, 2, 6, (40, 12), (66.7, 66.7, 19.6, 6.0), seed=11))


def check_ways_and_counters(case, band_rows):
    ref = case.reference
    assert (ref[1][..., :3] > 0).any()
    for way in WAYS:
        env = dict(way)
        if band_rows != 16:
            env["SLHIP_SSAO_BAND_ROWS"] = band_rows
        pic, _, _ = render(case.batch, **env)
        assert same_bits(pic, ref), (band_rows, way)
    # the counters: the pooled drain and the per-wave drain see the same pixels -- the same full runs, the same lane-slots needed --
    # and the pool never makes more end-of-band runs than the four waves alone (ceil of a sum against the sum of ceils)
    band = {} if band_rows == 16 else {"SLHIP_SSAO_BAND_ROWS": band_rows}
    pic_p, (tiles_p, runs_p, mixed_p), slots_p = render(case.batch, SLHIP_SSAO_DEBUG=3, **band)
    pic_w, (tiles_w, runs_w, mixed_w), slots_w = render(case.batch, SLHIP_SSAO_DEBUG=3, SLHIP_SSAO_POOL=0, **band)
    print("band rows", band_rows, "tiles", tiles_p, "pooled: runs", runs_p, "mixed", mixed_p, "slots", slots_p,
          "| per wave: runs", runs_w, "mixed", mixed_w, "slots", slots_w)
    assert same_bits(pic_p, ref) and same_bits(pic_w, ref)
    assert tiles_p == tiles_w
    assert slots_p[0] == slots_w[0] and slots_p[1] == slots_w[1]              # full runs and their lane-slots
    assert slots_p[3] == slots_w[3] > 0                                       # lane-slots needed at the end of the bands
    assert slots_p[2] >= slots_p[3] and slots_w[2] >= slots_w[3]              # issued >= needed
    assert 0 < runs_p <= runs_w
    return slots_p, slots_w


@pytest.mark.gpu
@pytest.mark.parametrize("band_rows", [16, 32, 48])
def test_pool_and_tiles_keep_the_bits_320(case_320, band_rows):
    """Two scenes of 8 objects at 320 x 240: 15, 8 (the last one cut) and 5 bands, 320 to 960 candidates per wave and band."""
    check_ways_and_counters(case_320, band_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("band_rows", [16, 32, 48])
def test_pool_and_tiles_keep_the_bits_smallest_viewport(case_64, band_rows):
    """64 x 32, the smallest tiled viewport: at 16 rows a wave's class has 4 x 16 = 64 candidates per band, ONE scan, and (unless all
    64 share a level) everything it queues is drained by the pool."""
    check_ways_and_counters(case_64, band_rows)


@pytest.mark.gpu
def test_knobs_are_inert_where_neither_pass_runs_tiled(case_40):
    """40 x 12 divides into neither 32 x 8 regions nor 16-row bands: the plain tap kernel, whatever the knobs say."""
    ref = case_40.reference
    assert (ref[1][..., :3] > 0).any()
    for way in WAYS + ({"SLHIP_SSAO_DEBUG": 3}, {"SLHIP_SSAO_BAND_ROWS": 32}):
        pic, (tiles, runs, mixed), slots = render(case_40.batch, **way)
        assert same_bits(pic, ref), way
        assert sum(tiles) == 0 and runs == 0 and mixed == 0 and slots == (0, 0, 0, 0)
