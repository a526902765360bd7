"""GPU tests of the views of the batch path (SceneBatch.place(view=..., camera_poses=..., object_to_camera=...) ->
slhip_synth_place_view): view 0 is the existing entries byte for byte; a drawn view equals oracle/synth_ref.c run under the
view's Philox key in everything a camera owns, and the plain records in everything it does not; its shadow matrices carry the
bits the existing environment entry gives the same light under the same camera; the caller's cameras reproduce a drawn view;
the camera fit holds in every view; object_to_camera; pictures against oracle/render_ref.c and the per-scene hand-over."""
import ctypes as C

import numpy as np
import pytest
import torch

from stillleben_amd import _abi
from test_gpu_environment import IDENTITY, host_maps_for, make_light_maps, make_textures, one
from test_gpu_render import assert_geometry_equal, assert_rgb_close
from test_gpu_synth import _one_scene_records, assert_records_equal, small_table

pytestmark = pytest.mark.gpu

SEED, SCENE_ID_BASE, N_SCENES, RENDER_CHUNK = (77 << 32) | 5, 1000, 37, 16
RES, INTRINSICS = (320, 240), (533.4, 533.7, 156.5, 120.6)


def make_batch(sl, table, n_obj=4, seed=SEED, n_scenes=N_SCENES, settle=True, **extra):
    b = sl.SceneBatch(table, n_scenes, n_obj, resolution=RES, seed=seed, render_chunk=RENDER_CHUNK, manual_exposure=1.0,
                      scene_id_base=SCENE_ID_BASE, **extra)
    b.set_camera_intrinsics(*INTRINSICS)
    if settle:
        b.stage()
        b.settle(frames=5)
        b.check_settled()
    return b


def records(batch):
    """Everything a place step writes, on the host: (slhip_scene, slhip_draw, slhip_chunk, slhip_synth_scene, env_out)."""
    torch.cuda.synchronize()
    return batch.host_render_records() + (batch.host_scenes(), batch.host_env())


def assert_all_equal(got, ref):
    for name, g, r in zip(("slhip_scene", "slhip_draw", "slhip_chunk", "slhip_synth_scene"), got, ref):
        assert_records_equal(name, g, r)
    assert np.array_equal(got[4], ref[4])


def view_seed(batch, v):
    k0, k1 = _abi.view_key(batch.params["seed_lo"], batch.params["seed_hi"], v)
    return (k1 << 32) | k0


class World:
    pass


@pytest.fixture(scope="module")
def world(sl):
    """Batch A plain, batch B on a bank (the bank of tests/test_gpu_environment.py), batch A9 with 9 objects named by
    asset_ids: 37 scenes of the small table, settled for 5 frames, placed; their plain records are the reference of this file."""
    w = World()
    w.table = small_table(sl)
    w.maps = make_light_maps(sl)
    w.bgs, w.pts = make_textures(sl, 11)
    w.bank = sl.EnvironmentBank(w.maps, w.bgs, w.pts)
    w.A = make_batch(sl, w.table)
    w.B = make_batch(sl, w.table, environment=w.bank, p_light_map=0.5, p_background=0.5, p_plane_texture=0.5)
    ids = np.random.default_rng(2).integers(0, len(w.table), (N_SCENES, 9))
    w.A9 = make_batch(sl, w.table, n_obj=9, asset_ids=ids)
    w.plain = {}
    for name in ("A", "B", "A9"):
        b = getattr(w, name)
        b.place()
        w.plain[name] = records(b)
    assert np.array_equal(w.A.host_bodies()["pose"], w.B.host_bodies()["pose"])
    env = w.plain["B"][4]
    assert (env[:, 0] >= 0).sum() >= 8 and (env[:, 0] < 0).sum() >= 8        # scenes with and without a light set
    return w


def direct_place_view(batch, view):
    """slhip_synth_place_view through ctypes, as place() calls it."""
    d_assets, d_templates = batch.table.device()
    v = _abi.SynthView()
    v.view = view
    e = batch._env() if batch.environment is not None else None
    a = batch._a
    stream = torch.cuda.current_stream(batch.eng.device).cuda_stream
    with torch.cuda.device(batch.eng.device):
        st = batch.eng.L.slhip_synth_place_view(batch._p(), C.byref(e) if e is not None else None, C.byref(v), a(d_assets),
                                                a(d_templates), a(batch.d_bodies), a(batch.d_objects), a(batch.d_scenes),
                                                a(batch.d_srec), a(batch.d_drec), a(batch.d_crec), a(batch.d_env_out),
                                                C.c_void_p(stream))
    _abi.check(st, "slhip_synth_place_view")


@pytest.mark.parametrize("name", ["A", "B"])
def test_view_0_is_todays_path(world, name):
    """place(view=0) and a direct slhip_synth_place_view call with view 0 write, over cleared buffers, the bytes of place()."""
    batch, ref = getattr(world, name), world.plain[name]

    def clear():
        for t in (batch.d_srec, batch.d_drec, batch.d_crec):
            t.fill_(0xCD)
        if batch.d_env_out is not None:
            batch.d_env_out.fill_(-7)

    clear()
    batch.place(view=0)
    assert_all_equal(records(batch), ref)
    clear()
    direct_place_view(batch, 0)
    assert_all_equal(records(batch), ref)
    assert batch.view == 0


def check_view_against_oracle(oracle, batch, table, v, plain=None):
    """Records of place(view=v) against oracle.synth_place under the view's key: every field a camera owns or leaves alone,
    bit for bit; light_dir and shadow_mat are the oracle's for ANOTHER light (it draws the light in the view's camera frame)."""
    batch.place(view=v)
    g_s, g_d, g_c, g_sc, _ = records(batch)
    p = np.array(batch.params)
    p["seed_lo"], p["seed_hi"] = _abi.view_key(p["seed_lo"], p["seed_hi"], v)
    rsc = g_sc.copy()
    rsc["camera_pose"] = 0
    srec, drec, crec = oracle.synth_place(p, table.records, table.templates, batch.host_bodies(), batch.host_objects(), rsc)
    assert_records_equal("slhip_draw", g_d, drec)
    assert_records_equal("slhip_chunk", g_c, crec)
    assert_records_equal("slhip_synth_scene", g_sc, rsc)
    for f in g_s.dtype.names:
        if f not in ("light_dir", "shadow_mat"):
            assert np.array_equal(np.ascontiguousarray(g_s[f]).view(np.uint8), np.ascontiguousarray(srec[f]).view(np.uint8)), (v, f)
    if plain is not None:
        for f in ("light_dir", "light_color", "ambient"):
            assert np.array_equal(np.ascontiguousarray(g_s[f]).view(np.uint8), np.ascontiguousarray(plain[0][f]).view(np.uint8)), (v, f)
    assert batch.view == v
    return g_sc["camera_pose"].copy()


@pytest.mark.parametrize("name", ["A", "A9"])
def test_drawn_view_against_the_oracle(world, oracle, name):
    batch, plain = getattr(world, name), world.plain[name]
    cams = [plain[3]["camera_pose"]] + [check_view_against_oracle(oracle, batch, world.table, v, plain) for v in (1, 2, 7)]
    for i in range(len(cams)):
        for j in range(i):
            assert (np.abs(cams[i] - cams[j]).max(axis=1) > 1e-3).all(), (i, j)      # another camera in every scene


def test_drawn_view_with_64_objects(world, oracle, sl):
    """n_objects = 64: lane 63 owns an object and the plane.  Staged (not settled) piles of cubes, view 1."""
    ids = np.random.default_rng(5).integers(0, 3, (3, 64))
    batch = make_batch(sl, world.table, n_obj=64, n_scenes=3, settle=False, asset_ids=ids)
    batch.stage()
    check_view_against_oracle(oracle, batch, world.table, 1)
    s, d, _ = batch.host_render_records()
    assert (s["draw_end"] - s["draw_begin"] == 65).all() and (d["n_tris"] > 0).all()


@pytest.mark.parametrize("v", [1, 7])
def test_shadow_matrices_of_a_view_carry_the_parent_paths_bits(world, sl, v):
    """A second batch keyed with the view's key draws the view's camera as ITS camera; given the first batch's piles and, through
    a light set per scene, the first batch's world lights, the existing place() fits the shadow matrix this view must carry."""
    from test_gpu_ibl import sky

    A, sa = world.A, world.plain["A"][0]
    assert not any(np.array_equal(sa[s]["shadow_mat"][0], IDENTITY) for s in range(N_SCENES))
    assert all(np.array_equal(sa[s]["shadow_mat"][l], IDENTITY) for s in range(N_SCENES) for l in (1, 2))
    lm = sl.LightMap(sky(24, 48, seed=1), sizes=dict(env_size=16, env_levels=5, irr_size=4, pre_size=8, pre_levels=3, lut_size=8))
    bank = sl.EnvironmentBank()
    for s in range(N_SCENES):
        bank.add_light_map(lm, directions=[sa[s]["light_dir"][0, :3].copy()], colors=[sa[s]["light_color"][0, :3].copy()])
    ids = np.full((N_SCENES, 3), -1, np.int32)
    ids[:, 0] = np.arange(N_SCENES)
    A2 = make_batch(sl, world.table, seed=view_seed(A, v), settle=False, environment=bank, env_ids=ids)
    for t in ("d_bodies", "d_objects", "d_scenes"):
        getattr(A2, t).copy_(getattr(A, t))
    A2.place()
    A.place(view=v)
    torch.cuda.synchronize()
    got, ref = A.host_render_records()[0], A2.host_render_records()[0]
    for s in range(N_SCENES):
        assert np.array_equal(got[s]["shadow_mat"][0].view(np.uint32), ref[s]["shadow_mat"][0].view(np.uint32)), s
        assert not np.array_equal(got[s]["shadow_mat"][0], IDENTITY) and np.isfinite(got[s]["shadow_mat"][0]).all()
        assert np.array_equal(got[s]["shadow_mat"][1], IDENTITY) and np.array_equal(got[s]["shadow_mat"][2], IDENTITY)
        assert not np.array_equal(got[s]["shadow_mat"][0], sa[s]["shadow_mat"][0])          # re-fitted to the view's frustum
    assert np.array_equal(got["world_to_cam"].view(np.uint32), ref["world_to_cam"].view(np.uint32))
    assert np.array_equal(got["light_dir"].view(np.uint32), ref["light_dir"].view(np.uint32))


@pytest.mark.parametrize("name,v", [("A", 0), ("A", 3), ("B", 3)])
def test_callers_cameras_reproduce_a_view(world, name, v):
    batch = getattr(world, name)
    batch.place(view=v)
    ref = records(batch)
    poses = torch.from_numpy(batch.host_cameras()).to(batch.eng.device)
    assert tuple(poses.shape) == (N_SCENES, 4, 4)
    for t in (batch.d_srec, batch.d_drec, batch.d_crec):
        t.fill_(0xCD)
    batch.place(view=v, camera_poses=poses)
    assert_all_equal(records(batch), ref)
    if v == 0:
        assert_all_equal(ref, world.plain[name])


def test_a_camera_that_is_not_finite_empties_its_scene_only(world):
    batch = world.A
    batch.place(view=3)
    ref = records(batch)
    poses = batch.host_cameras()
    poses[5, 1, 2] = np.nan
    poses[20, 2, 3] = np.inf
    batch.place(camera_poses=torch.from_numpy(poses).to(batch.eng.device))
    sc, dc, cc, _, _ = records(batch)
    md, mk = int(batch.params["max_draws_per_scene"]), int(batch.params["max_chunks_per_scene"])
    for s in range(N_SCENES):
        if s in (5, 20):
            assert sc[s]["draw_begin"] == sc[s]["draw_end"] and sc[s]["n_prims"] == 0
            assert (dc["n_tris"][s * md:(s + 1) * md] == 0).all() and (cc["count"][s * mk:(s + 1) * mk] == 0).all()
        else:
            assert_records_equal("slhip_scene %d" % s, sc[s:s + 1], ref[0][s:s + 1])
            assert_records_equal("slhip_draw %d" % s, dc[s * md:(s + 1) * md], ref[1][s * md:(s + 1) * md])
            assert_records_equal("slhip_chunk %d" % s, cc[s * mk:(s + 1) * mk], ref[2][s * mk:(s + 1) * mk])


@pytest.mark.parametrize("name", ["A", "A9"])
def test_the_fit_holds_in_every_view(world, name):
    """Views 0 to 4, every object: the 8 corners of the mesh's bounding box through the records' proj * world_to_cam *
    object_to_world * mesh_to_object, in float64, fall inside the viewport with 0.5 px of slack (a condition: the fit touches
    the frustum planes exactly, float32 rounding at these focal lengths is ~1e-4 px)."""
    batch, table = getattr(world, name), world.table
    W, H = RES
    md = int(batch.params["max_draws_per_scene"])
    objs = batch.host_objects()
    touched = 0
    for v in range(5):
        batch.place(view=v)
        torch.cuda.synchronize()
        sc, dc, _ = batch.host_render_records()
        for s in range(N_SCENES):
            P = sc[s]["proj"].reshape(4, 4).astype(np.float64) @ sc[s]["world_to_cam"].reshape(4, 4).astype(np.float64)
            draws = dc[s * md: s * md + int(sc[s]["draw_end"] - sc[s]["draw_begin"])]
            draws = draws[draws["instance_index"] > 0]                  # (instance 0 is the plane)
            assert set(draws["instance_index"].tolist()) == set(range(1, batch.n_objects + 1))
            px = []
            for d in draws:
                a = table.records[int(objs[s * batch.n_objects + int(d["instance_index"]) - 1]["asset"])]
                m2o = d["mesh_to_object"].reshape(4, 4).astype(np.float64)
                lo, hi = a["bbox_min"][:3].astype(np.float64), a["bbox_max"][:3].astype(np.float64)
                corners = np.array([[(hi if k & 1 else lo)[0], (hi if k & 2 else lo)[1], (hi if k & 4 else lo)[2], 1.0] for k in range(8)])
                mesh = np.linalg.solve(m2o, corners.T)                 # the bbox is kept in the object frame
                q = P @ d["object_to_world"].reshape(4, 4).astype(np.float64) @ m2o @ mesh
                assert (q[3] > 0).all(), (v, s)
                px.append(np.stack([(q[0] / q[3] * 0.5 + 0.5) * W, (q[1] / q[3] * 0.5 + 0.5) * H]))
            px = np.concatenate(px, axis=1)
            assert px[0].min() >= -0.5 and px[0].max() <= W + 0.5 and px[1].min() >= -0.5 and px[1].max() <= H + 0.5, (v, s, px.min(1), px.max(1))
            # ... and the fit is tight: the pile touches the frame on one axis at least
            touched += int(min(px[0].min(), W - px[0].max()) < 0.5 or min(px[1].min(), H - px[1].max()) < 0.5)
    assert touched == 5 * N_SCENES


def test_object_to_camera(world):
    """world_to_cam * pose, rows 0-2: against the float64 product of the records to 1e-5 absolute (four-term dot products of
    values below 3: rounding ~2e-6); the same with a bank; view 0 goes through the view entry for it and writes view 0's bytes."""
    A, B = world.A, world.B
    for v in (0, 2):
        A.place(view=v, object_to_camera=True)
        B.place(view=v, object_to_camera=True)
        torch.cuda.synchronize()
        assert tuple(A.object_to_camera.shape) == (N_SCENES, 4, 3, 4) and A.object_to_camera.dtype == torch.float32
        assert torch.equal(A.object_to_camera, B.object_to_camera)
        w2c = A.host_render_records()[0]["world_to_cam"].reshape(N_SCENES, 1, 4, 4).astype(np.float64)
        pose = A.host_bodies()["pose"].reshape(N_SCENES, 4, 4, 4).astype(np.float64)
        ref = (w2c @ pose)[:, :, :3, :]
        got = A.object_to_camera.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - ref).max())
        print("object_to_camera view %d: max abs error %.3g" % (v, err))
        assert err <= 1e-5 and np.abs(ref).max() < 3.0
        assert (ref[..., 2, 3] > 0.1).all()                                    # every object in front of the camera
        if v == 0:
            assert_all_equal(records(A), world.plain["A"])
            assert_all_equal(records(B), world.plain["B"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_pictures_of_view_2(world, oracle, sl, name):
    """View 2 of two scenes (one of them in the ragged last chunk): the GPU render against oracle.render on the same records
    with the bars of tests/test_gpu_render.py; batch.scene(s) through sl.RenderPass gives the same picture, with the bars of
    test_gpu_synth.test_batch_scene_hand_over_renders_the_same_picture."""
    from stillleben_amd._engine import SHADOW_RES

    batch = getattr(world, name)
    W, H = RES
    env = world.plain[name][4]
    lit = [s for s in range(RENDER_CHUNK) if env[s, 0] >= 0]
    picks = [lit[0] if lit else 3, N_SCENES - 1]
    batch.place(view=2)
    bufs = {c: batch.render(c, mask=_abi.OUT_ALL) for c in sorted({s // RENDER_CHUNK for s in picks})}
    torch.cuda.synchronize()
    sb, db, _ = batch.host_render_records()
    cams = batch.host_cameras()
    assert not np.array_equal(cams, world.plain[name][3]["camera_pose"].reshape(-1, 4, 4))
    maps = host_maps_for(batch.eng, world.maps)
    flags = _abi.OUT_ALL | _abi.RENDER_SSAO | _abi.RENDER_SHADOWS
    rp = sl.RenderPass()
    for s in picks:
        rs, rd = _one_scene_records(batch, sb, db, s)
        ref = oracle.render(batch.eng.pool.arrays(), rs, rd, W, H, flags, shadow_res=SHADOW_RES, light_maps=maps)
        got = one(bufs, RENDER_CHUNK, s)
        n_obj_px = int((got.instance != 0).sum())
        print("view 2, batch %s scene %d (env %s): %d object pixels" % (name, s, list(env[s]), n_obj_px))
        assert n_obj_px > 2000, s
        assert_geometry_equal(got, ref)
        assert_rgb_close(got, ref)
        # the hand-over carries the camera of the view placed last
        scene = batch.scene(s)
        assert np.array_equal(np.asarray(scene._camera_pose), cams[s])
        res = rp.render(scene)
        a, g = res.instance_index().cpu(), got.instance[0].cpu()
        same = (a == g)
        m = same[..., 0]
        dc = float((res.coordDepth().cpu()[m] - got.coord[0].cpu()[m]).abs().max())
        frac = float(((res.rgb().cpu().int() - got.rgb[0].cpu().int()).abs()[m] > 2).float().mean())
        print("hand-over: masks equal %.6f, coord max %.3g, rgb > 2 on %.3g" % (float(same.float().mean()), dc, frac))
        assert float(same.float().mean()) > 0.999
        assert torch.equal(res.class_index().cpu()[same], got.cls[0].cpu()[same])
        assert dc < 3e-4
        assert frac < 5e-3


def test_views_generator(world):
    batch = world.A
    seen, cams = [], []
    for v, c, buf in batch.views(3, mask=_abi.OUT_INSTANCE, ssao=False):
        assert batch.view == v and buf.instance.shape[0] == min(RENDER_CHUNK, N_SCENES - c * RENDER_CHUNK)
        seen.append((v, c))
        if c == 0:
            cams.append(batch.host_cameras())
    assert batch.n_render_chunks() == 3
    assert seen == [(v, c) for v in range(3) for c in range(3)]
    assert batch.view == 2
    assert np.array_equal(cams[0], world.plain["A"][3]["camera_pose"].reshape(-1, 4, 4))
    assert not np.array_equal(cams[1], cams[0]) and not np.array_equal(cams[2], cams[1])
