"""k_shade gives the same bits in its default form and in the in-library reference form of the pieces the default does in fewer
instructions (SLHIP_SHADE_REFERENCE=1, read at every call): the exposure sum of a block behind one barrier and the PCF tile rows
without a division.  Both forms render the same batch in one process; every output array, the float image, the z plane, the
SSAO tile records and the `lum` scratch (per-block partials, then the scene's exposure luminance after k_lum_reduce) must be
byte-identical.

The batch: (0) a 6 m plane far beyond the light's fitted box -- the PCF windows of its pixels clamp at 0 and at S - 1 and straddle
64-texel tile borders -- that also reaches behind the camera (its triangles cross the near plane), with a textured and an
untextured sphere side by side so that one wave holds both kinds of lanes; (1) no geometry at all, a background image; auto
exposure in both.  Shapes: 64 x 16 (tiled placement, every wave on an image edge), 96 x 24 (tiled, interior waves; no SSAO tile
records at 24 rows), 96 x 32 (the same with tile records), 40 x 12 (untiled; 480 pixels: the last block sums inactive lanes).

The host test restates the two summation orders in numpy float32."""
import os

import numpy as np
import pytest
import torch

from stillleben_amd import _abi, _engine
from stillleben_amd._batch import HostPool, build_batch

S = 2048                    # the engine's shadow map (_engine.SHADOW_RES)
SHAPES = [(64, 16), (96, 24), (96, 32), (40, 12)]
OUTPUTS = ("rgb", "instance", "cls", "vertex_idx", "coord", "bary", "cam_coord", "normals")
SENTINEL = 0xA5             # what the scratch holds where a render writes nothing


# ---- host: the two orders of the block sum -------------------------------------------------------------------------------

def tree_sum(x):
    """The 256-wide LDS tree: strides 128 .. 1, lane i < s adds lane i + s."""
    red = x.astype(np.float32).copy()
    s = 128
    while s > 0:
        red[:s] = red[:s] + red[s:2 * s]
        s >>= 1
    return red[0]


def wave_sum(x):
    """One barrier: wave 0 forms (x0 + x2) + (x1 + x3) per lane, then six shuffle-down steps over its 64 lanes (a lane whose
    partner lies beyond the wave gets its own value back; nothing reads what it then holds)."""
    x = x.astype(np.float32)
    t = (x[0:64] + x[128:192]) + (x[64:128] + x[192:256])
    lane = np.arange(64)
    s = 32
    while s > 0:
        src = np.where(lane + s < 64, lane + s, lane)
        t = t + t[src]
        s >>= 1
    return t[0]


def test_block_sum_orders_agree_bit_for_bit():
    rng = np.random.default_rng(11)
    tiny = np.float32(1e-45)
    for trial in range(400):
        x = rng.random(256, dtype=np.float32)
        kind = trial % 5
        if kind == 1:
            x = x * np.float32(10.0) ** rng.integers(-30, 30, 256).astype(np.float32)      # mixed magnitude
        elif kind == 2:
            x = (rng.integers(0, 1 << 22, 256).astype(np.float32) * tiny).astype(np.float32)   # denormals
            assert (x[x > 0] < np.finfo(np.float32).tiny).all()
        elif kind == 3:
            x[rng.random(256) < 0.85] = 0.0                                                 # mostly zeros (the plane, the sky)
            x[rng.random(256) < 0.05] *= np.float32(1e-40)
        elif kind == 4:
            x = x * np.float32(10.0) ** rng.integers(-44, 38, 256).astype(np.float32)
            x[480 % 256:] = 0.0                                                             # the inactive lanes of a last block
        x = x.astype(np.float32)
        a, b = np.float32(tree_sum(x)), np.float32(wave_sum(x))
        assert a.view(np.uint32) == b.view(np.uint32), (trial, a, b)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

def geometry_scene(sl, size):
    from test_gpu_materials import textured_sphere

    textured = sl.Mesh.from_data(textured_sphere(1, n_lat=8, n_lon=12, with_tex=("base", "normal")))
    plain = sl.Mesh.from_data(textured_sphere(2, n_lat=8, n_lon=12, with_tex=()))
    sc = sl.Scene(size)
    for k, m in enumerate((textured, plain)):
        o = sl.Object(m)
        pose = np.eye(4, dtype=np.float32)
        pose[:3, 3] = [0.065 + 0.1 * (2 * k - 1), 0.0, 0.1]    # radius 0.1: the spheres touch, off the picture's centre column
        o.set_pose(torch.from_numpy(pose))
        sc.add_object(o)
    sc.background_plane_size = torch.tensor([6.0, 6.0])
    sc.set_camera_look_at(torch.tensor([0.0, -0.9, 0.5]), torch.tensor([0.0, 0.0, 0.05]))
    sc.light_directions = torch.tensor([[0.3, 0.4, -0.85]])
    return sc


def empty_scene(sl, size):
    rng = np.random.default_rng(3)
    sc = sl.Scene(size)
    sc.background_plane_size = torch.tensor([0.0, 0.0])
    sc.background_image = sl.Texture(torch.from_numpy((rng.random((9, 13, 4)) * 255).astype(np.uint8)))
    return sc


def grab(bufs, keep, B, W, H):
    out = {}
    for name in OUTPUTS:
        t = getattr(bufs, name, None)
        if t is not None:
            out[name] = t.cpu().numpy().copy()
    for name in ("hdr", "ao", "lum"):                            # the whole scratch: float image (both halves), AO + z plane + tile
        out[name] = keep[name].cpu().numpy().copy()              # records + skip bytes, partials + exposure luminance
    P = W * H
    z0 = 4 * B * P
    out["zplane"] = out["ao"][z0:z0 + 4 * B * (W + 2) * (H + 2)]
    if W % 32 == 0 and H % 16 == 0:                              # where the SSAO runs tile by tile (slhip_render)
        t0 = (z0 + 4 * B * (W + 2) * (H + 2) + 7) & ~7
        out["ssao_tiles"] = out["ao"][t0:t0 + 8 * B * (W // 8) * (H // 8)]
    out["lum_parts"] = out["lum"][:16 * B * ((P + 255) // 256)]
    return out


def render_both(eng, scenes):
    W, H = scenes[0].viewport
    B = len(scenes)
    saved = os.environ.get("SLHIP_SHADE_REFERENCE")
    outs = []
    try:
        os.environ.pop("SLHIP_SHADE_REFERENCE", None)
        bufs = eng.render(scenes, _abi.OUT_ALL, ssao=True, shadows=True, keep_hdr=True)     # (the scratch of this shape exists now)
        torch.cuda.synchronize()
        keep = bufs._keepalive[0]
        for ref in (False, True):
            for name in ("hdr", "ao", "lum"):
                keep[name].fill_(SENTINEL)
            if ref:
                os.environ["SLHIP_SHADE_REFERENCE"] = "1"
            bufs = eng.render(scenes, _abi.OUT_ALL, ssao=True, shadows=True, keep_hdr=True)
            torch.cuda.synchronize()
            assert bufs._keepalive[0] is keep
            outs.append(grab(bufs, keep, B, W, H))
    finally:
        os.environ.pop("SLHIP_SHADE_REFERENCE", None)
        if saved is not None:
            os.environ["SLHIP_SHADE_REFERENCE"] = saved
    return outs


def pcf_windows(srec, cam_coord):
    """First texel column / row of the 5 x 5 PCF window of every pixel with geometry (scene 0, light 0), in float64."""
    M = srec[0]["world_to_cam"].reshape(4, 4).astype(np.float64)
    L = srec[0]["shadow_mat"][0].reshape(4, 4).astype(np.float64)
    c = cam_coord.reshape(-1, 4).astype(np.float64)
    c = c[c[:, 3] == 1.0]
    world = c @ np.linalg.inv(M).T
    pc = world @ L.T
    p = pc[:, :2] / pc[:, 3:4] * 0.5 + 0.5
    return np.floor((p - 1.5 / S) * S - 0.5).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_default_and_reference_form_give_the_same_bits(sl, size):
    from stillleben_amd._context import engine

    W, H = size
    scenes = [geometry_scene(sl, size), empty_scene(sl, size)]
    new, ref = render_both(engine(), scenes)
    assert set(new) == set(ref) and {"rgb", "instance", "coord", "cam_coord", "normals", "hdr", "zplane", "lum_parts"} <= set(new)
    for name, a in new.items():
        b = ref[name]
        same = a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert same, "%s differs between the two forms at %d bytes" % (name, int((a.view(np.uint8) != b.view(np.uint8)).sum()))
    # ... and the renders wrote what is compared
    for name in ("zplane", "lum_parts") + (("ssao_tiles",) if "ssao_tiles" in new else ()):
        assert (new[name] != SENTINEL).any(), name
    assert ("ssao_tiles" in new) == (size in ((64, 16), (96, 32)))
    # the batch asks of the kernel what the docstring says
    pool = HostPool()
    srec, drec, _ = build_batch(scenes, pool, with_shadows=True)
    assert (srec["manual_exposure"] < 0).all()                                     # auto exposure: k_lum_reduce runs
    inst = new["instance"].reshape(2, H, W, -1)[..., 0]
    assert not inst[1].any() and (new["coord"].reshape(2, H, W, 4)[1] == 3000.0).all()      # scene 1: nothing but the image
    image = new["hdr"].view(np.float32)[4 * W * H:8 * W * H]                       # (its exposure average is 0 / 0: rgb says nothing)
    assert np.isfinite(image).all() and (image > 0).any()
    tex = drec["flags"] & (_abi.DRAW_HAS_BASE_TEX | _abi.DRAW_HAS_NORMAL_TEX)
    by_inst = {int(d["instance_index"]) & 0xFFFF: bool(t) for d, t in zip(drec, tex)}
    assert by_inst[1] and not by_inst[2]
    if W % 32 == 0 and H % 8 == 0:                                                 # a wave is an 8 x 8 tile
        waves = inst[0].reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    else:                                                                           # ... or 64 consecutive pixels
        flat = inst[0].reshape(-1)
        waves = np.pad(flat, (0, -len(flat) % 64)).reshape(-1, 64)
    assert any((w == 1).any() and (w == 2).any() and (w == 0).any() for w in waves)    # textured, untextured and plane lanes
    win = pcf_windows(srec, new["cam_coord"].reshape(2, H, W, 4)[0])
    for axis in (0, 1):
        lo = win[:, axis]
        assert (lo < 0).any() and (lo + 4 > S - 1).any(), "no PCF window clamps on axis %d" % axis
        inside = (lo >= 0) & (lo + 4 <= S - 1)
        assert ((lo[inside] >> 6) != ((lo[inside] + 4) >> 6)).any(), "no PCF window straddles a tile border on axis %d" % axis
    corners = np.array([[x, y, 0.0, 1.0] for x in (-3.0, 3.0) for y in (-3.0, 3.0)])
    depth = (corners @ srec[0]["world_to_cam"].reshape(4, 4).astype(np.float64).T)[:, 2]
    assert depth.min() < 0.0 < depth.max()                                         # the plane passes through the camera's plane
