"""The SSAO pass runs, tile by tile, only the taps that can reach an occluder (slhip_render.hip k_ssao_mask / k_ssao_tiled): sample k
lies radius * |s_k| from its pixel, so on a plane tile whose box at rho_j is clear only the samples with 1.001 |s_k| > rho_j can land
on anything but the plane.  CPU: the host's level lists, and the rule itself against the oracle (no left-out tap occludes).  GPU:
the picture with the levels is bit for bit the picture with every tile at the full list."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import scenes as S
from stillleben_amd import _abi

RHO = (0.81, 0.6, 0.45, 0.3, 0.2)        # level j: the box at RHO[j] is clear; level len(RHO): all 64 taps
FULL = len(RHO)


def kernel_lengths(oracle):
    noise, kern = oracle.ssao_tables()
    kern = np.asarray(kern, np.float32).reshape(64, 3).astype(np.float64)
    return np.asarray(noise, np.float32).reshape(16, 3).astype(np.float64), kern, np.sqrt((kern * kern).sum(axis=1))


def level_tables():
    L = _abi.lib()
    rho, counts, taps = (C.c_float * 5)(), (C.c_uint32 * 6)(), (C.c_uint8 * 384)()
    _abi.check(L.slhip_render_ssao_level_tables(C.byref(rho), C.byref(counts), C.byref(taps)), "slhip_render_ssao_level_tables")
    taps = np.frombuffer(taps, np.uint8).reshape(6, 64)
    return np.array(rho[:], np.float32), [taps[j, :counts[j]].astype(int).tolist() for j in range(6)]


def test_level_lists_of_the_host(oracle):
    """The lists the host derives from the kernel table (read-out slhip_render_ssao_level_tables) against lengths recomputed here."""
    _, _, ln = kernel_lengths(oracle)
    rho, lists = level_tables()
    assert np.array_equal(rho, np.array(RHO, np.float32))
    assert rho[0] >= 1.001 * ln.max() and np.all(np.diff(rho) < 0)
    assert lists[0] == [] and lists[FULL] == list(range(64))
    for j in range(FULL + 1):
        assert lists[j] == sorted(set(lists[j]))                                     # ascending k, no repeats
        if j < FULL:
            assert set(np.nonzero(1.001 * ln > float(rho[j]))[0].tolist()) <= set(lists[j])
        if j > 0:
            assert set(lists[j - 1]) <= set(lists[j])                                 # nested
    # (nothing superfluous either: the lists are as short as the rule allows, apart from samples within rounding of a threshold)
    for j in range(FULL):
        assert all(1.001 * ln[k] > float(rho[j]) * (1 - 1e-12) for k in lists[j])
    sizes = [len(x) for x in lists]
    assert sizes == sorted(sizes) and sizes[1] > 0 and sizes[FULL - 1] < 40


def tile_levels(cam_coord, normals, instance, P):
    """The rule of k_ssao_mask in numpy, tile by tile (8 x 8): 0 = skipped .. FULL = all taps."""
    H, W = instance.shape
    z = cam_coord[..., 2]
    geo = (normals[..., :3] != 0).any(axis=-1)
    fx, fy = P[0, 0] * W / 2, P[1, 1] * H / 2
    tmax = max((1 + abs(P[0, 2])) / P[0, 0], (1 + abs(P[1, 2])) / P[1, 1])
    reach = max(fx, fy) * 0.1 * math.sqrt(1 + tmax * tmax) * 1.001
    other = (geo & (instance != 0)).reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))
    anyg = geo.reshape(H // 8, 8, W // 8, 8).any(axis=(1, 3))
    zmin = np.where(geo, z, np.inf).reshape(H // 8, 8, W // 8, 8).min(axis=(1, 3))
    level = np.full((H // 8, W // 8), FULL, int)
    for ty in range(H // 8):
        for tx in range(W // 8):
            if not anyg[ty, tx]:
                level[ty, tx] = 0
                continue
            if other[ty, tx] or zmin[ty, tx] <= 0.2:
                continue
            for j in range(FULL - 1, -1, -1):                                         # the boxes grow with rho
                R = int(math.ceil(RHO[j] * reach / (zmin[ty, tx] - 0.1))) + 2
                x0, x1, y0, y1 = tx * 8 - R, tx * 8 + 7 + R, ty * 8 - R, ty * 8 + 7 + R
                if x0 < 0 or y0 < 0 or x1 >= W or y1 >= H or other[y0 // 8:y1 // 8 + 1, x0 // 8:x1 // 8 + 1].any():
                    break
                level[ty, tx] = j
    return level, geo


def check_rule(oracle, cam_coord, normals, instance, P):
    """Every tap the rule leaves out, of every pixel of the partial levels, restated in float64: none occludes.  Level-0 pixels
    have an occlusion of exactly 1 in the oracle's pass."""
    noise, kern, ln = kernel_lengths(oracle)
    H, W = instance.shape
    level, geo = tile_levels(cam_coord, normals, instance, P)
    ao = oracle.ssao_pass(P.astype(np.float32), cam_coord, normals)
    lv = np.kron(level, np.ones((8, 8), int))
    assert (ao[lv == 0] == 1.0).all()
    partial = [(level == j).mean() for j in range(1, FULL)]
    assert sum(partial) >= 0.05 and sum(p > 0 for p in partial) >= 2, partial         # the case is exercised
    radius, bias = 0.1, 0.0025
    P64 = P.astype(np.float64)
    zp = np.pad(cam_coord[..., 2], 1, mode="edge").astype(np.float64)                 # the clamped rect sampler
    worst, taps_left_out = np.inf, 0
    for j in range(1, FULL):
        ys, xs = np.nonzero((lv == j) & geo)
        if len(ys) == 0:
            continue
        n = normals[ys, xs, :3].astype(np.float64)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        rv = noise[(ys & 3) * 4 + (xs & 3)]
        rv = rv / np.linalg.norm(rv, axis=1, keepdims=True)
        tg = rv - n * (rv * n).sum(axis=1, keepdims=True)
        tg /= np.linalg.norm(tg, axis=1, keepdims=True)
        bt = np.cross(n, tg)
        F = cam_coord[ys, xs, :3].astype(np.float64)
        for k in np.nonzero(~(1.001 * ln > RHO[j]))[0]:
            Sp = F + radius * (tg * kern[k, 0] + bt * kern[k, 1] + n * kern[k, 2])
            cl = np.c_[Sp, np.ones(len(Sp))] @ P64.T
            u = (cl[:, 0] / cl[:, 3]) * 0.5 * W + 0.5 * W - 0.5
            v = (cl[:, 1] / cl[:, 3]) * 0.5 * H + 0.5 * H - 0.5
            fu, fv = np.floor(u), np.floor(v)
            ax, ay = u - fu, v - fv
            xc = np.clip(fu, -1, W - 1).astype(int) + 1
            yc = np.clip(fv, -1, H - 1).astype(int) + 1
            a, b, c, d = zp[yc, xc], zp[yc, xc + 1], zp[yc + 1, xc], zp[yc + 1, xc + 1]
            sd = (a + ax * (b - a)) * (1 - ay) + (c + ax * (d - c)) * ay
            worst = min(worst, float((sd - (Sp[:, 2] - bias)).min()))                 # occludes: sd <= spz - bias
            taps_left_out += len(ys)
    assert taps_left_out > 100000 and worst > 0.0, (taps_left_out, worst)
    return worst


def test_left_out_taps_never_occlude_clutter_scene(sl, oracle):
    from test_oracle_render import oracle_render

    scene = S.clutter_scene(sl, 5, n_objects=6, size=(640, 480))
    scene.set_camera_look_at(torch.tensor([2.2, -1.4, 1.9]), torch.tensor([0.0, 0.0, 0.1]))
    r = oracle_render(oracle, [scene], flags=_abi.OUT_ALL)
    check_rule(oracle, r.cam_coord[0], r.normals[0], r.instance[0, :, :, 0], scene.projection_matrix().numpy())


def test_left_out_taps_never_occlude_c2_scene(sl, oracle):
    """A scene of the benchmark's kind, built the way bench.cpu_baseline builds them (tabletop stage, 400-step settle, camera and
    light placement, 640 x 480)."""
    import bench
    from stillleben_amd import _settle_batch as SB
    from stillleben_amd import synthetic
    from stillleben_amd._batch import HostPool

    pool, hulls = HostPool(), SB.HullPool()
    table = sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64), mesh_pool=pool, hull_pool=hulls)
    hull_recs, hull_verts = hulls.arrays()
    W, H = bench.RESOLUTION
    proto = sl.Scene(bench.RESOLUTION)
    proto.set_camera_intrinsics(*bench.INTRINSICS)
    p = np.zeros((), dtype=_abi.SYNTH_PARAMS_DTYPE)
    p["n_scenes"], p["n_objects"], p["n_assets"] = 1, bench.N_OBJECTS, len(table)
    p["flags"] = _abi.SYNTH_SAMPLE_DISTINCT | _abi.SYNTH_RANDOM_PBR | _abi.SYNTH_SHADOWS
    p["seed_lo"], p["scene_id_base"], p["render_chunk"] = 900000, 0, 1
    p["max_draws_per_scene"] = table.bound(table.n_draws, bench.N_OBJECTS, True) + 1
    p["max_chunks_per_scene"] = table.bound(table.n_chunks, bench.N_OBJECTS, True) + 1
    p["max_clip_verts_per_scene"] = table.bound(table.n_clip, bench.N_OBJECTS, True) + 4
    p["plane_z"] = 0.04
    p["proj"] = proto._projection.reshape(-1)
    p["proj_inv"] = np.linalg.inv(proto._projection.astype(np.float64)).astype(np.float32).reshape(-1)
    p["plane_size"] = (3.0, 3.0)
    p["manual_exposure"] = -1.0
    p["light_color"][:3] = 300.0
    p["ambient"][:3] = 0.05
    bodies, ss, objs, scs = oracle.synth_stage(p, table.records)
    oracle.settle(ss, bodies, hull_recs, hull_verts, SB.default_params(tabletop=True))
    srec, drec, _ = oracle.synth_place(p, table.records, table.templates, bodies, objs, scs)
    nd = int(srec[0]["draw_end"] - srec[0]["draw_begin"])
    rs, rd = srec[0:1].copy(), drec[:nd].copy()
    rs["draw_begin"], rs["draw_end"] = 0, nd
    rd["scene"] = 0
    r = oracle.render(pool.arrays(), rs, rd, W, H, _abi.OUT_GT6 | _abi.OUT_CAM_COORD | _abi.OUT_NORMALS)
    check_rule(oracle, r.cam_coord[0], r.normals[0], r.instance[0, :, :, 0], np.asarray(proto._projection, np.float64).reshape(4, 4))


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ycb_table(sl):
    from stillleben_amd import synthetic

    sl.init_cuda(0)
    return sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=64))


def render_with_and_without_levels(batch, band_rows=None):
    """The batch's render chunk 0 three times in this process (both variables are read at every slhip_render): as it is, with
    SLHIP_SSAO_DEBUG=3 (the same levels, and the tap kernel counts its end-of-band runs) and with SLHIP_SSAO_DEBUG=2 (every tile at
    the full list: the reference).  `band_rows`: SLHIP_SSAO_BAND_ROWS for the first two.  Returns (rgb, hdr) of the three and
    the level read-out of the second."""
    md, mk, mv = (int(batch.params[k]) for k in ("max_draws_per_scene", "max_chunks_per_scene", "max_clip_verts_per_scene"))
    W, H = batch.resolution
    B = batch.n_scenes
    batch.eng.pool_abi()

    def once(**env):
        assert "SLHIP_SSAO_DEBUG" not in os.environ and "SLHIP_SSAO_BAND_ROWS" not in os.environ
        os.environ.update({k: str(v) for k, v in env.items() if v is not None})
        try:
            buf = batch.eng.render_device(batch.d_srec.data_ptr(), batch.d_drec.data_ptr(), batch.d_crec.data_ptr(), B, B * md,
                                          B * mk, B * mv, W, H, _abi.OUT_ALL, ssao=True, shadows=batch.shadows, shadow_lights=1,
                                          keep_hdr=True)
            torch.cuda.synchronize()
        finally:
            for k in env:
                os.environ.pop(k, None)
        hdr = buf._keepalive[0]["hdr"].view(torch.float32)[: 2 * B * H * W * 4].reshape(2, B, H, W, 4)[1].cpu().numpy().copy()
        return (buf.rgb.cpu().numpy().copy(), hdr), batch.eng.ssao_levels(buf, W, H)

    plain, levels_plain = once(SLHIP_SSAO_BAND_ROWS=band_rows)
    counted, levels = once(SLHIP_SSAO_BAND_ROWS=band_rows, SLHIP_SSAO_DEBUG=3)
    full, levels_full = once(SLHIP_SSAO_DEBUG=2)
    assert levels_plain == (levels[0], 0, 0)                                          # the same tiles; nothing counted unasked
    assert levels_full[0][:FULL] == [0] * FULL and levels_full[0][FULL] == B * (W // 8) * (H // 8)   # the reference ran every tap
    return plain, counted, full, levels


def settled_batch(sl, table, n_scenes, n_objects, resolution, intrinsics, seed):
    batch = sl.SceneBatch(table, n_scenes, n_objects, resolution=resolution, seed=seed, manual_exposure=1.0)
    batch.set_camera_intrinsics(*intrinsics)
    batch.stage()
    batch.settle(frames=20)
    batch.place()
    return batch


@pytest.fixture(scope="module")
def batch_320(sl, ycb_table):
    return settled_batch(sl, ycb_table, 2, 8, (320, 240), (533.4, 533.7, 156.5, 120.6), seed=9)


@pytest.fixture(scope="module")
def batch_64(sl, ycb_table):
    return settled_batch(sl, ycb_table, 2, 6, (64, 32), (106.7, 106.7, 31.3, 16.1), seed=11)


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("band_rows", [None, 32, 48])
def test_levels_leave_the_picture_bit_for_bit(batch_320, band_rows):
    """Two scenes of 8 objects at 320 x 240: rgb and the float image behind it are bit-identical with the levels and with every
    tile at the full list; every level occurs, and some wave ended its band with a run that mixes levels.  At the default band
    depth (16 rows) and at 32 and 48 rows (240 rows: 15, 8 -- the last one cut -- and 5 bands)."""
    plain, counted, full, (tiles, runs, mixed) = render_with_and_without_levels(batch_320, band_rows)
    print("band rows", band_rows, "tiles per level", tiles, "end-of-band runs", runs, "mixed", mixed)
    assert sum(tiles) == 2 * 40 * 30 and all(t > 0 for t in tiles), tiles
    assert runs > 0 and mixed > 0, (runs, mixed)
    assert same_bits(plain, full) and same_bits(counted, full)
    assert (full[1][..., :3] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("band_rows", [None, 32, 48])
def test_levels_smallest_viewport(batch_64, band_rows):
    """64 x 32, the smallest viewport the tiled pass accepts: the box of every tile at the border leaves the image (full list, or
    no geometry), so at most the 6 x 2 inner tiles of a scene can have a level between; two bands per scene at the default depth, one at 32 and at 48 rows
    (cut at the last row)."""
    plain, counted, full, (tiles, runs, mixed) = render_with_and_without_levels(batch_64, band_rows)
    print("band rows", band_rows, "tiles per level", tiles, "end-of-band runs", runs, "mixed", mixed)
    assert sum(tiles) == 2 * 8 * 4 and tiles[FULL] > 0 and sum(tiles[1:FULL]) <= 2 * 6 * 2, tiles
    assert runs > 0
    assert same_bits(plain, full) and same_bits(counted, full)
