"""GPU tests of the environment bank of the batch path (sl.EnvironmentBank + SceneBatch(environment=...) ->
slhip_synth_place_env): what the environment does not own is bit-equal to the plain, oracle-pinned path; what it owns equals the
choice of the Philox mirror of tests/test_host_environment.py and the records of the per-scene path for the handed-over scene;
shadow matrices of all lights carry the bits the plain path gives light 0; pictures against oracle/render_ref.c with the
project's bars for that comparison; the hand-over to sl.Scene / sl.RenderPass."""
import types

import numpy as np
import pytest
import torch

from stillleben_amd import _abi
from test_gpu_ibl import sky
from test_gpu_render import assert_geometry_equal, assert_rgb_close
from test_gpu_synth import _one_scene_records, assert_records_equal, small_table
from test_host_environment import GPU_COUNTS, GPU_N_SCENES, GPU_PROBS, GPU_SCENE_ID_BASE, GPU_SEED, env_choices, picture_scenes

pytestmark = pytest.mark.gpu

MAP_SIZES = dict(env_size=64, env_levels=7, irr_size=8, pre_size=32, pre_levels=5, lut_size=32)    # test_gpu_ibl's render test
RES, INTRINSICS = (320, 240), (533.4, 533.7, 156.5, 120.6)
IDENTITY = np.eye(4, dtype=np.float32).reshape(-1)
# fields of the records the environment owns (everything else must not move)
SCENE_LIGHT_FIELDS = ("light_dir", "light_color", "ambient", "light_map", "shadow_mat")
PLANE_FIELDS = ("base_color", "tex_offset", "tex_w", "tex_h", "tex_sampler", "flags")


@pytest.fixture(scope="module")
def ycb_table(sl):
    from stillleben_amd import synthetic

    return sl.AssetTable(synthetic.ycb_like_meshes(seed=0, tex_size=256))


def make_light_maps(sl):
    """3 small synthetic light maps; the second carries three lights, the third none."""
    maps = [sl.LightMap(sky(48, 96, seed=k), sizes=MAP_SIZES) for k in (2, 3, 4)]
    maps[0].light_directions = [np.array([0.3, -0.2, -0.93], np.float32)]
    maps[0].light_colors = [np.array([3.0, 2.8, 2.5], np.float32)]
    maps[1].light_directions = [np.array(d, np.float32) for d in ((-0.4, 0.1, -0.9), (0.5, 0.5, -0.7), (0.0, -0.6, -0.8))]
    maps[1].light_colors = [np.array(c, np.float32) for c in ((2.5, 2.5, 2.2), (1.0, 1.2, 1.5), (0.8, 0.6, 0.5))]
    return maps


def make_textures(sl, seed):
    """3 background images (random alpha, as test_gpu_ibl's) and 3 plane textures without green, alpha 255."""
    rng = np.random.default_rng(seed)
    bgs = []
    for k, (h, w) in enumerate(((30, 40), (48, 64), (25, 35))):
        img = (rng.random((h, w, 4)) * 255).astype(np.uint8)
        img[: h // 2, :, k] = 255
        img[..., :3] |= 1                    # never black: a background pixel is told from a cleared one by its colour
        bgs.append(sl.Texture(torch.from_numpy(img)))
    pts = []
    for k, (h, w) in enumerate(((64, 64), (32, 48), (16, 16))):
        img = np.zeros((h, w, 4), np.uint8)
        yy, xx = np.mgrid[:h, :w]
        check = ((yy // 4 + xx // 4) & 1).astype(np.uint8)
        img[..., 0] = 120 + 100 * check + (rng.random((h, w)) * 30).astype(np.uint8)
        img[..., 2] = (60, 200, 120)[k] + (rng.random((h, w)) * 30).astype(np.uint8)
        img[..., 3] = 255
        pts.append(sl.Texture2D(torch.from_numpy(img)))
    return bgs, pts


def host_maps_for(eng, maps):
    """oracle.render's light_maps list (indexed by slot) with the maps downloaded from the device; slots of other tests' maps
    are filled with the first of ours (no record of this file names them)."""
    def down(lm):
        return ({"env": lm.env.cpu().numpy(), "irradiance": lm.irradiance.cpu().numpy(), "prefilter": lm.prefilter.cpu().numpy(),
                 "brdf_lut": lm.brdf_lut.cpu().numpy()}, lm.sizes)

    ours = {lm._slot: down(lm) for lm in maps}
    return [ours.get(k, ours[maps[0]._slot]) for k in range(len(eng._light_maps))]


class World:
    pass


@pytest.fixture(scope="module")
def world(sl, ycb_table):
    """Batch A plain, batch B on a bank: same seed, table and settle.  64 scenes x 20 YCB-like objects, two render chunks."""
    w = World()
    w.maps = make_light_maps(sl)
    w.bgs, w.pts = make_textures(sl, 11)
    w.bank = sl.EnvironmentBank(w.maps, w.bgs, w.pts)
    kw = dict(resolution=RES, seed=GPU_SEED, scene_id_base=GPU_SCENE_ID_BASE, render_chunk=32, manual_exposure=1.0)
    w.A = sl.SceneBatch(ycb_table, GPU_N_SCENES, 20, **kw)
    w.B = sl.SceneBatch(ycb_table, GPU_N_SCENES, 20, environment=w.bank, p_light_map=GPU_PROBS[0], p_background=GPU_PROBS[1],
                        p_plane_texture=GPU_PROBS[2], **kw)
    for b in (w.A, w.B):
        b.set_camera_intrinsics(*INTRINSICS)
        b.stage()
        b.settle(frames=20)
        b.check_settled()
        b.place()
    torch.cuda.synchronize()
    w.ids = env_choices(GPU_SEED, GPU_SCENE_ID_BASE, GPU_N_SCENES, GPU_COUNTS, GPU_PROBS)
    w.recA, w.recB = w.A.host_render_records(), w.B.host_render_records()
    w.md = int(w.A.params["max_draws_per_scene"])
    return w


def test_nothing_else_moved(world):
    """Every field the environment does not own is bit-equal between the plain batch and the batch on a bank; a scene that got
    nothing is equal in ALL fields.  (The plain batch is the path tests/test_gpu_synth.py pins against oracle/synth_ref.c.)"""
    w = world
    assert np.array_equal(w.A.host_bodies()["pose"], w.B.host_bodies()["pose"])
    assert_records_equal("synth_scene", w.B.host_scenes(), w.A.host_scenes())
    (sa, da, ca), (sb, db, cb) = w.recA, w.recB
    assert_records_equal("slhip_chunk", cb, ca)
    plane = np.arange(GPU_N_SCENES) * w.md                       # the plane is every scene's first draw
    assert (da["flags"][plane] == _abi.DRAW_NO_VERTEX_ID).all() and (da["n_tris"][plane] == 2).all()
    for f in sa.dtype.names:
        if f in SCENE_LIGHT_FIELDS:
            rows = w.ids[:, 0] < 0
        elif f == "bg_tex":
            rows = w.ids[:, 1] < 0
        else:
            rows = np.ones(GPU_N_SCENES, bool)
        assert rows.sum() >= 8
        assert np.array_equal(np.ascontiguousarray(sb[f][rows]).view(np.uint8), np.ascontiguousarray(sa[f][rows]).view(np.uint8)), f
    for f in da.dtype.names:
        rows = np.ones(len(da), bool)
        if f in PLANE_FIELDS:
            rows[plane[w.ids[:, 2] >= 0]] = False
        assert np.array_equal(np.ascontiguousarray(db[f][rows]).view(np.uint8), np.ascontiguousarray(da[f][rows]).view(np.uint8)), f
    # without a bank host_env() says so
    assert (w.A.host_env() == -1).all()


def test_owned_fields_follow_the_mirror_and_the_per_scene_path(world):
    """light_map, lights, ambient, bg_tex and the plane draw's material equal (i) the bank's records for the mirror's choice
    and (ii) what the per-scene path (_batch.build_batch on the engine's pool) writes for SceneBatch.scene(i)."""
    from stillleben_amd._batch import build_batch

    w = world
    assert np.array_equal(w.B.host_env(), w.ids)
    sb, db, _ = w.recB
    ls, bg, pt = w.bank.light_sets, w.bank.backgrounds, w.bank.plane_textures
    sa = w.recA[0]
    cache = {"bodies": w.B.host_bodies(), "objects": w.B.host_objects(), "scenes": w.B.host_scenes(), "srec": sb, "env": w.ids}
    handed = set(picture_scenes(w.ids)) | {0, 63}
    for s in range(GPU_N_SCENES):
        li, bi, ti = (int(v) for v in w.ids[s])
        r, d = sb[s], db[s * w.md]
        if li >= 0:
            n = int(ls[li]["n_lights"])
            assert int(r["light_map"]) == int(ls[li]["light_map"]) == w.maps[li]._slot + 1
            assert np.array_equal(r["light_dir"], ls[li]["light_dir"]) and np.array_equal(r["light_color"], ls[li]["light_color"])
            assert (r["light_dir"][n:] == 0).all() and (r["ambient"] == 0).all()
        else:
            assert int(r["light_map"]) == 0 and np.array_equal(r["ambient"][:3], np.float32([0.05, 0.05, 0.05]))
            assert np.array_equal(r["light_dir"], sa[s]["light_dir"]) and (r["light_color"][0, :3] == 300.0).all()
        assert list(r["bg_tex"]) == ([int(bg[bi][k]) for k in ("offset", "w", "h")] if bi >= 0 else [0, 0, 0])
        if ti >= 0:
            assert list(d["base_color"]) == [1, 1, 1, 1] and int(d["flags"]) == _abi.DRAW_NO_VERTEX_ID | _abi.DRAW_HAS_BASE_TEX
            assert [int(d[k]) for k in ("tex_offset", "tex_w", "tex_h")] == [int(pt[ti][k]) for k in ("offset", "w", "h")]
            assert int(d["tex_sampler"][0]) == _abi.SAMPLER_DEFAULT and (d["tex_sampler"][1:] == 0).all()
        else:
            assert np.array_equal(d["base_color"], np.float32([0, 0.8, 0, 1])) and int(d["flags"]) == _abi.DRAW_NO_VERTEX_ID
            assert int(d["tex_w"]) == 0 and (d["tex_sampler"] == 0).all()
        if s not in handed:
            continue
        scene = w.B.scene(s, _cache=cache)
        assert scene.light_map is w.bank.light_map(li) and scene.background_image is w.bank.background(bi)
        assert scene.background_plane_texture is w.bank.plane_texture(ti)
        before = w.B.eng.pool.n_tex_bytes
        hs, hd, _ = build_batch([scene], w.B.eng.pool, with_shadows=False)
        assert w.B.eng.pool.n_tex_bytes == before              # the bank's textures already sit in the pool
        for f in ("light_map", "light_dir", "light_color", "ambient", "bg_tex"):
            assert np.array_equal(np.ascontiguousarray(hs[0][f]).view(np.uint8), np.ascontiguousarray(r[f]).view(np.uint8)), (s, f)
        for f in PLANE_FIELDS:
            assert np.array_equal(np.ascontiguousarray(hd[0][f]).view(np.uint8), np.ascontiguousarray(d[f]).view(np.uint8)), (s, f)


def test_shadow_matrices_carry_the_plain_paths_bits(sl):
    """The light the plain batch wrote for scene s, given back to scene s through a light set: in slot 0 it gets the very
    shadow matrix of the plain batch (which oracle/synth_ref.c pins), in slot 1 and slot 2 -- another light in front -- the
    same bits; an inactive slot (no light, or a light without colour) is the identity."""
    table = small_table(sl)
    n, n_obj = 8, 4
    kw = dict(seed=(77 << 32) | 5, render_chunk=4, manual_exposure=1.0, scene_id_base=1000)

    def run(**extra):
        b = sl.SceneBatch(table, n, n_obj, **kw, **extra)
        b.set_camera_intrinsics(1066.778, 1067.487, 312.9869, 241.3109)
        b.stage()
        b.settle(frames=5)
        b.check_settled()
        b.place()
        torch.cuda.synchronize()
        return b

    A = run()
    sa = A.host_render_records()[0]
    assert not any(np.array_equal(sa[s]["shadow_mat"][0], IDENTITY) for s in range(n))
    assert all(np.array_equal(sa[s]["shadow_mat"][l], IDENTITY) for s in range(n) for l in (1, 2))
    lm = sl.LightMap(sky(24, 48, seed=1), sizes=dict(env_size=16, env_levels=5, irr_size=4, pre_size=8, pre_levels=3, lut_size=8))
    bank = sl.EnvironmentBank()
    front, dark = (np.float32([0.2, 0.3, -0.9]), np.float32([5, 5, 5])), (np.float32([0.5, -0.1, -0.8]), np.float32([0, 0, 0]))
    for s in range(n):
        own = (sa[s]["light_dir"][0, :3].copy(), sa[s]["light_color"][0, :3].copy())
        for lights in ([own], [front, own], [front, dark, own]):
            bank.add_light_map(lm, directions=[d for d, _ in lights], colors=[c for _, c in lights])
    fronts = None
    for slot in range(3):
        ids = np.full((n, 3), -1, np.int32)
        ids[:, 0] = 3 * np.arange(n) + slot
        B = run(environment=bank, env_ids=ids)
        assert np.array_equal(B.host_env(), ids)
        sb = B.host_render_records()[0]
        for s in range(n):
            m = sb[s]["shadow_mat"]
            assert np.array_equal(m[slot].view(np.uint32), sa[s]["shadow_mat"][0].view(np.uint32)), (slot, s)
            assert np.array_equal(sb[s]["light_dir"][slot], sa[s]["light_dir"][0]) and int(sb[s]["light_map"]) == lm._slot + 1
            if slot == 0:
                assert np.array_equal(m[1], IDENTITY) and np.array_equal(m[2], IDENTITY)
            else:
                assert not np.array_equal(m[0], IDENTITY) and np.isfinite(m[0]).all()          # the light in front is fitted too
                assert np.array_equal(m[3 - slot], IDENTITY)          # slot 1: nothing in slot 2; slot 2: the dark light in slot 1
        if slot:
            f = sb["shadow_mat"][:, 0].copy()
            assert fronts is None or np.array_equal(f, fronts)      # the same front light gives the same matrix in both runs
            fronts = f
        # everything but lights / shadow matrices is the plain batch's
        for f in sb.dtype.names:
            if f not in SCENE_LIGHT_FIELDS:
                assert np.array_equal(np.ascontiguousarray(sb[f]).view(np.uint8), np.ascontiguousarray(sa[f]).view(np.uint8)), f


def test_more_lights_than_slots_and_ids_beyond_the_bank(sl):
    """What only the device can see: a light set record that claims more than NUM_LIGHTS lights is clamped, an id beyond its
    bank makes that scene EMPTY (no draws), its neighbours untouched."""
    table = small_table(sl)
    lm = sl.LightMap(sky(24, 48, seed=1), sizes=dict(env_size=16, env_levels=5, irr_size=4, pre_size=8, pre_levels=3, lut_size=8))
    bank = sl.EnvironmentBank()
    bank.add_light_map(lm, directions=[(0, 0, -1), (0.1, 0, -1), (0, 0.1, -1)], colors=[(1, 1, 1)] * 3)
    bank._light_sets[0]["n_lights"] = 7                            # a record no host layer would write
    ids = np.full((4, 3), -1, np.int32)
    ids[1, 0] = ids[2, 0] = 0
    B = sl.SceneBatch(table, 4, 3, seed=3, environment=bank, env_ids=ids)
    B.stage()
    B.settle(frames=5)
    B.place()
    torch.cuda.synchronize()
    sb = B.host_render_records()[0]
    assert np.array_equal(sb[1]["light_dir"][:, :3], np.float32([(0, 0, -1), (0.1, 0, -1), (0, 0.1, -1)]))
    assert (sb["draw_end"] > sb["draw_begin"]).all()
    bad = torch.from_numpy(ids.copy())
    bad[2, 0] = 1                                                  # the bank has one light set
    B.d_env_ids.copy_(bad)
    B.place()
    torch.cuda.synchronize()
    sc, dc, cc = B.host_render_records()
    md, mk = int(B.params["max_draws_per_scene"]), int(B.params["max_chunks_per_scene"])
    assert sc[2]["draw_end"] == sc[2]["draw_begin"] and sc[2]["n_prims"] == 0 and (dc["n_tris"][2 * md:3 * md] == 0).all()
    assert (cc["count"][2 * mk:3 * mk] == 0).all() and list(B.host_env()[2]) == [-1, -1, -1] and int(sc[2]["light_map"]) == 0
    for s in (0, 1, 3):
        assert_records_equal("slhip_scene %d" % s, sc[s:s + 1], sb[s:s + 1])
    with pytest.raises(ValueError):
        sl.SceneBatch(table, 4, 3, environment=bank, env_ids=bad.numpy())      # the host layer refuses it up front
    with pytest.raises(ValueError):
        sl.SceneBatch(table, 4, 3, environment=bank, p_light_map=1.5)
    with pytest.raises(ValueError):
        sl.SceneBatch(table, 4, 3, env_ids=ids)


@pytest.fixture(scope="module")
def pictures(world):
    w = world
    bufs = [w.B.render(c, mask=_abi.OUT_ALL) for c in range(w.B.n_render_chunks())]
    torch.cuda.synchronize()
    return bufs


def one(bufs, rc, s):
    """Scene s of the chunked render as a batch of one."""
    b, k = bufs[s // rc], s % rc
    return types.SimpleNamespace(**{f: getattr(b, f)[k:k + 1] for f in ("rgb", "coord", "cls", "instance", "normals", "vertex_idx",
                                                                        "bary", "cam_coord")})


def test_pictures_match_the_oracle(world, pictures, oracle):
    """6 scenes that cover every kind of environment and the three-light map, cut out of the batch records and rendered by
    oracle/render_ref.c with the light maps downloaded from the device: geometry bit for bit, rgb to the project's 8-bit bar."""
    from stillleben_amd._engine import SHADOW_RES

    w = world
    W, H = RES
    sb, db, _ = w.recB
    maps = host_maps_for(w.B.eng, w.maps)
    pool_arrays = w.B.eng.pool.arrays()
    flags = _abi.OUT_ALL | _abi.RENDER_SSAO | _abi.RENDER_SHADOWS
    chosen = picture_scenes(w.ids)
    assert len(chosen) == 6
    for s in chosen:
        rs, rd = _one_scene_records(w.B, sb, db, s)
        ref = oracle.render(pool_arrays, rs, rd, W, H, flags, shadow_res=SHADOW_RES, light_maps=maps)
        got = one(pictures, w.B.render_chunk, s)
        assert int((got.instance != 0).sum()) > 2000, s
        assert_geometry_equal(got, ref)
        assert_rgb_close(got, ref)


def test_hand_over_renders_the_same_picture(world, pictures, sl):
    """sl.RenderPass().render(batch.scene(i)) against the batch's picture for a three-light-map scene with everything bound and
    a one-light-map scene, with the bars of test_gpu_synth.test_batch_scene_hand_over_renders_the_same_picture: masks equal
    on > 99.9 % of the pixels, coordinates < 3e-4 on those, rgb off by more than 2 on < 5e-3 of them."""
    w = world
    chosen = picture_scenes(w.ids)
    full = [s for s in range(GPU_N_SCENES) if (w.ids[s] >= 0).all() and w.ids[s, 0] == 1]
    picks = [full[0] if full else chosen[4], chosen[1]]
    rp = sl.RenderPass()
    for i in picks:
        scene = w.B.scene(i)
        assert scene.light_map is not None and len(scene.objects) == 20
        res = rp.render(scene)
        got = one(pictures, w.B.render_chunk, i)
        a, b = res.instance_index().cpu(), got.instance[0].cpu()
        same = (a == b)
        m = same[..., 0]
        dc = float((res.coordDepth().cpu()[m] - got.coord[0].cpu()[m]).abs().max())
        d = (res.rgb().cpu().int() - got.rgb[0].cpu().int()).abs()[m]
        frac = float((d > 2).float().mean())
        print("hand-over scene %d (env %s): masks equal %.6f, coord max %.3g, rgb > 2 on %.3g" % (i, list(w.ids[i]), float(same.float().mean()), dc, frac))
        assert float(same.float().mean()) > 0.999 and int((b != 0).sum()) > 2000
        assert torch.equal(res.class_index().cpu()[same], got.cls[0].cpu()[same])
        assert dc < 3e-4
        assert frac < 5e-3


def test_it_shows(world, pictures, sl):
    """Background images and the sky fill the pixels without geometry (alpha 0, colour); a textured plane is not green; the
    per-object statistics of an environment batch are the plain batch's (the environment changes no geometry)."""
    w = world
    table = small_table(sl)
    ids = np.array([[-1, 0, -1], [0, -1, -1], [-1, -1, -1], [1, 2, 0]], np.int32)
    E = sl.SceneBatch(table, 4, 4, resolution=(200, 150), seed=4, plane_size=(0.0, 0.0), environment=w.bank, env_ids=ids,
                      manual_exposure=1.0)
    E.stage()
    E.settle(frames=5)
    E.place()
    buf = E.render(0, mask=_abi.OUT_ALL)
    torch.cuda.synchronize()
    rgb = buf.rgb.cpu().numpy()
    empty = buf.coord.cpu().numpy()[..., 0] == 3000.0                 # pixels without geometry (clear value)
    for s in (0, 1, 3):                                               # background image / sky / background image over the sky
        px = rgb[s][empty[s]]
        assert len(px) > 1000 and (px[:, 3] == 0).all() and (px[:, :3].max(axis=1) > 0).mean() > 0.99, s
    assert len(rgb[2][empty[2]]) > 1000 and (rgb[2][empty[2]] == 0).all()      # nothing bound: the cleared background
    assert (E.host_render_records()[0]["draw_end"] - E.host_render_records()[0]["draw_begin"] == 4).all()   # no plane draw
    # the plane: green without a texture, the texture's red / blue with one
    inst = torch.cat([b.instance for b in pictures]).cpu().numpy()[..., 0]
    coord = torch.cat([b.coord for b in pictures]).cpu().numpy()[..., 0]
    col = torch.cat([b.rgb for b in pictures]).cpu().numpy()
    seen = {True: 0, False: 0}
    for s in range(GPU_N_SCENES):
        plane = (inst[s] == 0) & (coord[s] != 3000.0)
        if plane.sum() < 2000:
            continue
        r, g, b = (float(col[s][plane][:, k].mean()) for k in range(3))
        textured = bool(w.ids[s, 2] >= 0)
        assert (max(r, b) > g) if textured else (g > max(r, b)), (s, textured, r, g, b)
        seen[textured] += 1
    assert seen[True] >= 8 and seen[False] >= 8
    # object statistics
    sa = w.A.render(0, object_stats=True).object_stats
    sb = w.B.render(0, object_stats=True).object_stats
    torch.cuda.synchronize()
    assert int((sb.px_count_visib > 0).sum()) > 20 * 16
    for f in ("px_count_visib", "px_count_all", "bbox_visib", "bbox_obj"):
        assert torch.equal(getattr(sa, f), getattr(sb, f)), f
