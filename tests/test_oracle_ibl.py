"""CPU: the ORACLE's image-based lighting (oracle/ibl_ref.c, cubemap_ref.h, the IBL term and the sky of render_ref.c) against
the float64 known answers of tests/ibl_analytic.py -- an environment whose radiance is linear in the direction, evaluated
from the documented rules without reading a cube texel.  This file is also where every tolerance of the IBL known answers
is MEASURED: each test prints its figures before it asserts them against ibl_analytic.BOUNDS (twice the measurement);
tests/test_gpu_ibl.py holds the kernels to the same bounds plus its device-vs-libm tolerances."""
import math

import numpy as np
import pytest
import torch

import ibl_analytic as A
import scenes as S
from stillleben_amd import _abi
from stillleben_amd._batch import HostPool, build_batch

N_PAIRS = len(A.PAIRS)
SHADE_CASES = ((0.0, 1.0), (0.0, 0.5), (1.0, 0.25))          # (metallic, roughness)
SHADE_BASE = (0.8, 0.8, 0.8)                                 # scenes.delaunay_sheet's material
SKY_SIZE = (320, 240)


class HostLightMap:
    """What the host builder reads of an sl.LightMap (its slot and the lights its .ibl file names): lets a scene name
    light map 0 of the oracle's pool without a device."""
    _slot = 0
    light_directions = []
    light_colors = []


def equirect_f32(pair):
    return A.equirect(pair, *A.EQUIRECT_SHAPE).astype(np.float32)


@pytest.fixture(scope="module")
def maps(oracle):
    """The oracle's light maps of both radiances at the full and at the coarse sizes: built once, never written to."""
    out = {}
    for p in range(N_PAIRS):
        out[p, "full"] = oracle.light_map_build(equirect_f32(p), A.SIZES)
        out[p, "coarse"] = oracle.light_map_build(equirect_f32(p), A.SIZES_COARSE)
    return out


# ---- the maps -------------------------------------------------------------------------------------------------------------
def env_texel_classes(n, H, W):
    """Masks [6, n, n] over the level-0 texels: `pole` = reads the image within two rows of its top or bottom (the rows
    clamp there), `seam` = reads it within one column of its left or right edge (azimuth +-pi; the image is clamped, not
    wrapped, as the reference's sampler is), `inner` = the rest, where the bilinear read sees four distinct pixels."""
    row, col = A.image_row_col(A.texel_dirs(n), H, W)
    pole = (row < 2.0) | (row > H - 2.0)
    seam = ~pole & ((col < 1.0) | (col > W - 1.0))
    return pole, seam, ~pole & ~seam


def map_errors(bufs, pair, sizes=A.SIZES, shape=A.EQUIRECT_SHAPE):
    """max |buffer - float64 reference| per map; prefilter per level.  Also checks the alpha channels and the layout."""
    n = sizes["env_size"]
    env = A.cube_levels(bufs["env"], n, sizes["env_levels"])[0]
    d = np.abs(env[..., :3] - A.env0(pair, n)).max(axis=-1)
    pole, seam, inner = env_texel_classes(n, *shape)
    fig = {"env_all": d.max(), "env_seam": d[seam].max(), "env_inner": d[inner].max()}
    assert (env[..., 3] == 1.0).all()
    irr = A.cube_levels(bufs["irradiance"], sizes["irr_size"], 1)[0]
    fig["irradiance"] = np.abs(irr[..., :3] - A.irradiance(pair, sizes["irr_size"])).max()
    assert (irr[..., 3] == 1.0).all()
    for l, pre in enumerate(A.cube_levels(bufs["prefilter"], sizes["pre_size"], sizes["pre_levels"])):
        want = A.prefilter(pair, sizes["pre_size"] >> l, A.level_roughness(l, sizes["pre_levels"]))
        fig["prefilter_%d" % l] = np.abs(pre[..., :3] - want).max()
        fig["prefilter_%d_errors" % l] = np.abs(pre[..., :3] - want)
        assert (pre[..., 3] == 1.0).all()
    lut = np.asarray(bufs["brdf_lut"]).reshape(sizes["lut_size"], sizes["lut_size"], 2)
    fig["brdf_lut"] = np.abs(lut - A.brdf_lut(sizes["lut_size"])).max()
    return fig


def report(title, fig):
    print("\n%s: %s" % (title, ", ".join("%s %.3g" % (k, v) for k, v in fig.items() if np.ndim(v) == 0)))


def assert_within(fig, bounds=None, extra=None):
    """Every scalar figure at or below its bound (plus `extra(key)` where a caller adds a margin)."""
    bounds = A.BOUNDS if bounds is None else bounds
    over = []
    for k, v in fig.items():
        if np.ndim(v) == 0:
            lim = bounds[k] + (extra(k) if extra else 0.0)
            if not v <= lim:
                over.append("%s: %.3g exceeds %.3g (x%.0f)" % (k, v, lim, v / lim))
    assert not over, "; ".join(over)


def test_reference_radiances_loop_counts_and_face_table():
    phi, theta = A.irradiance_steps()
    assert len(phi) == 315 and len(theta) == 79
    for p, (a, B) in enumerate(A.PAIRS):
        assert (a > np.linalg.norm(B, axis=1)).all() and (B != 0).all()            # L > 0 everywhere
        assert len(set(np.round(np.linalg.norm(B, axis=1), 6))) == 3
        assert len(set(np.abs(B).ravel())) == 9                                  # no two axes, no sign interchangeable
        dirs = A.texel_dirs(4)
        face, s, t = A.face_coords(dirs)
        c = (2.0 * (np.arange(4) + 0.5)) / 4 - 1.0
        assert (face == np.arange(6)[:, None, None]).all()
        assert np.allclose(s, c[None, None, :]) and np.allclose(t, c[None, :, None])
        # the unnormalised tangent frame is a pinned property: it departs from the closed form a + (2/3) B . N
        closed = a + (2.0 / 3.0) * A.texel_dirs(8) @ B.T
        gap = np.abs(A.irradiance(p, 8) - closed).max()
        print("\npair %d: irradiance rule vs closed form a + (2/3) B.N: %.4f" % (p, gap))
        assert 0.05 < gap < 0.2
    # the image has its row 0 at the top: +z is brighter where B_z > 0
    eq = A.equirect(0, 8, 16)
    assert np.sign(eq[0, :, 0].mean() - eq[-1, :, 0].mean()) == np.sign(A.PAIRS[0][1][0, 2])
    # the BRDF table's scale + bias stays in (0, 1]; a smooth surface seen head-on returns almost all of F0
    lut = A.brdf_lut(16)
    assert ((lut.sum(axis=2) > 0) & (lut.sum(axis=2) <= 1.0 + 1e-3)).all() and lut[0, -1, 0] > 0.9


@pytest.mark.parametrize("pair", range(N_PAIRS))
def test_maps_match_float64_reference(maps, pair):
    fig = map_errors(maps[pair, "full"], pair)
    report("pair %d maps" % pair, fig)
    assert_within(fig)
    # the inner texels' bound is no measurement: bilinear error of the image plus float32 rounding of the pixel coordinate
    # (u * W carries 2^-24 * W pixels) and of the stored value
    H, W = A.EQUIRECT_SHAPE
    grad = np.linalg.norm(A.PAIRS[pair][1], axis=1).max()
    derived = A.bilinear_image_bound(pair, H, W) + 2.0 ** -23 * (W * grad / (A.INV_ATAN[0] * W) + 4.0)
    print("derived bound of the inner texels: %.3g" % derived)
    assert fig["env_inner"] <= derived <= A.BOUNDS["env_inner"]
    # the oracle alone leaves no prefilter texel out of its bound (the GPU comparison may leave out a share of 1e-3)
    for l in range(A.SIZES["pre_levels"]):
        assert (fig["prefilter_%d_errors" % l] <= A.BOUNDS["prefilter_%d" % l]).all()


def check_mip_chain(env, size, levels):
    """Every level of the chain is the exact 2x2 box filter of the level below, in float32, down to one texel per face."""
    lv = A.cube_levels(env, size, levels)
    for l in range(1, levels):
        cur = lv[l - 1]
        nxt = ((cur[:, 0::2, 0::2] + cur[:, 0::2, 1::2]) + (cur[:, 1::2, 0::2] + cur[:, 1::2, 1::2])) * np.float32(0.25)
        assert np.array_equal(lv[l], nxt), "mip level %d" % l
    return lv


def test_mip_chain_is_the_exact_box_filter(maps):
    assert check_mip_chain(maps[0, "full"]["env"], 512, 10)[-1].shape[1] == 1
    assert check_mip_chain(maps[1, "coarse"]["env"], 32, 6)[-1].shape[1] == 1


# ---- edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1)])
def test_tiny_images_build_finite_maps(oracle, shape):
    rng = np.random.default_rng(shape[0] * 2 + shape[1])
    eq = (0.2 + rng.random(shape + (3,))).astype(np.float32)
    bufs = oracle.light_map_build(eq, A.SIZES_COARSE)
    for k, v in bufs.items():
        assert np.isfinite(v).all(), k
    env = A.cube_levels(bufs["env"], 32, 6)[0][..., :3]
    assert env.min() >= eq.min() and env.max() <= eq.max()          # bilinear: a convex combination of the pixels


def check_constant_maps(bufs, value, sizes):
    """A constant image gives the constant: the environment exactly (a bilinear blend of equal values), every prefilter
    level to float32 summation error (1024 terms), the irradiance to 1e-4 about its mean, which is the Riemann sum
    pi / count * sum(cos sin) = 0.9941 of the constant (the reference's normalisation: not pi times it)."""
    value = np.asarray(value, np.float32)
    for lv in A.cube_levels(bufs["env"], sizes["env_size"], sizes["env_levels"]):
        assert np.array_equal(lv[..., :3], np.broadcast_to(value, lv[..., :3].shape))
    for lv in A.cube_levels(bufs["prefilter"], sizes["pre_size"], sizes["pre_levels"]):
        assert np.abs(lv[..., :3] / value - 1.0).max() < 1e-4
    irr = A.cube_levels(bufs["irradiance"], sizes["irr_size"], 1)[0][..., :3] / value
    phi, theta = A.irradiance_steps()
    riemann = A.PI * (np.cos(theta) * np.sin(theta)).sum() / len(theta)
    assert np.abs(irr - irr.mean()).max() < 1e-4 and abs(irr.mean() - riemann) < 1e-4, (irr.mean(), riemann)


CONSTANT_IMAGES = [((1, 1), (1.0, 1.0, 1.0)), ((3, 5), (0.25, 2.0, 7.5)), ((16, 32), (1.0, 0.5, 3.0))]


@pytest.mark.parametrize("shape,value", CONSTANT_IMAGES)
def test_constant_image_gives_the_constant(oracle, shape, value):
    eq = np.broadcast_to(np.asarray(value, np.float32), shape + (3,)).copy()
    check_constant_maps(oracle.light_map_build(eq, A.SIZES_COARSE), value, A.SIZES_COARSE)


# ---- sky ------------------------------------------------------------------------------------------------------------------
def sky_scenes(sl, light_map):
    """(scene with a sheet filling the frame, the same view without it).  The camera sits at the origin, looks at the cube
    corner (1, 1, -1) with an 80 degree horizontal field of view (the corner and its three edges are in the picture, the
    poles are not) and is rolled by 23 degrees about its axis, so that no image axis lines up with a face axis."""
    sheet = S.delaunay_sheet(sl, 16, seed=5, half=4.0)
    out = []
    for with_object in (True, False):
        scene = sl.Scene(SKY_SIZE)
        scene.set_camera_hfov(math.radians(80.0))
        scene.set_camera_look_at(torch.tensor([0.0, 0.0, 0.0]), torch.tensor([1.0, 1.0, -1.0]))
        r = math.radians(23.0)
        roll = np.eye(4, dtype=np.float64)
        roll[:2, :2] = [[math.cos(r), -math.sin(r)], [math.sin(r), math.cos(r)]]
        cam = scene.camera_pose().numpy().astype(np.float64) @ roll
        scene.set_camera_pose(torch.from_numpy(cam.astype(np.float32)))
        scene.background_plane_size = torch.tensor([0.0, 0.0])
        scene.manual_exposure = 1.0
        scene._light_map = light_map
        if with_object:
            obj = sl.Object(sheet)
            P = np.eye(4)
            P[:3, :3] = np.diag([1.0, -1.0, -1.0])
            P[:3, 3] = [0.0, 0.0, 0.5]
            obj.set_pose(torch.from_numpy((scene.camera_pose().numpy().astype(np.float64) @ P).astype(np.float32)))
            scene.add_object(obj)
        out.append(scene)
    return out


def sky_directions(scene, cam_coord, instance):
    """World direction of every pixel from the renderer's own geometric outputs (pinned bit for bit elsewhere): the camera
    coordinates of the sheet that fills the frame, turned into the world by the camera pose."""
    assert (instance[..., 0] == 1).all()                         # the sheet covers every pixel
    R = scene.camera_pose().numpy().astype(np.float64)[:3, :3]
    d = cam_coord[..., :3].astype(np.float64) @ R.T
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def sky_errors(hdr, dirs, pair, env_size):
    """max |HDR rgb - L(direction)| over the pixels within one texel of a face edge and over the rest."""
    assert (hdr[..., 3] == 0.0).all()
    face, s, t = A.face_coords(dirs)
    assert len(np.unique(face)) == 3                             # three faces, hence three edges and the corner
    err = np.abs(hdr[..., :3] - A.radiance(pair, dirs)).max(axis=-1)
    near = np.maximum(np.abs(s), np.abs(t)) > 1.0 - 2.0 / env_size
    # about the middle of an edge the two faces' texel rows line up, so the seam rule (the texel the direction beyond the
    # edge points into) is nearly exact there, while a clamped or wrongly chosen neighbour still costs half a texel step
    mid = near & (np.minimum(np.abs(s), np.abs(t)) < 0.1)
    assert mid.sum() >= 30 and (~near).sum() > near.sum()
    return {"sky_%d_edge" % env_size: err[near].max(), "sky_%d_edge_mid" % env_size: err[mid].max(),
            "sky_%d_rest" % env_size: err[~near].max()}


def oracle_render(oracle, scene_list, bufs, sizes):
    pool = HostPool()
    srec, drec, _ = build_batch(scene_list, pool, with_shadows=False)
    W, H = scene_list[0].viewport
    return oracle.render(pool.arrays(), srec, drec, W, H, _abi.OUT_ALL, want_hdr=True, light_maps=[(bufs, sizes)])


@pytest.mark.parametrize("which", ["full", "coarse"])
@pytest.mark.parametrize("pair", range(N_PAIRS))
def test_sky_is_the_radiance_along_the_pixel_ray(sl, oracle, maps, pair, which):
    sizes = A.SIZES if which == "full" else A.SIZES_COARSE
    covered, empty = sky_scenes(sl, HostLightMap())
    r = oracle_render(oracle, [covered, empty], maps[pair, which], sizes)
    dirs = sky_directions(covered, r.cam_coord[0], r.instance[0])
    assert (r.instance[1] == 0).all()
    fig = sky_errors(r.hdr[1], dirs, pair, sizes["env_size"])
    report("pair %d sky" % pair, fig)
    assert_within(fig)


# ---- shading --------------------------------------------------------------------------------------------------------------
def shading_scenes(sl, light_map):
    """One sheet per (metallic, roughness) case seen from a generic viewpoint, facing the camera but tilted by 25 degrees
    (and rolled by 17), so that neither its normal nor the reflected ray lies along an axis or in a coordinate plane.  Lit
    by the light map only: no lights, no ambient term, manual exposure 1."""
    sheet = S.delaunay_sheet(sl, 16, seed=6, half=1.0)
    out = []
    for metallic, roughness in SHADE_CASES:
        scene = sl.Scene((160, 120))
        scene.set_camera_look_at(torch.tensor([1.5, -0.8, 1.1]), torch.tensor([0.1, 0.2, 0.0]))
        r, t = math.radians(17.0), math.radians(25.0)
        Rz = np.array([[math.cos(r), -math.sin(r), 0], [math.sin(r), math.cos(r), 0], [0, 0, 1]])
        Ry = np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]])
        P = np.eye(4)
        P[:3, :3] = Ry @ Rz @ np.diag([1.0, -1.0, -1.0])
        P[:3, 3] = [0.0, 0.0, 2.0]
        obj = sl.Object(sheet)
        obj.set_pose(torch.from_numpy((scene.camera_pose().numpy().astype(np.float64) @ P).astype(np.float32)))
        obj.metallic, obj.roughness = metallic, roughness
        scene.add_object(obj)
        scene.light_colors = torch.zeros(3, 3)
        scene.ambient_light = torch.tensor([0.0, 0.0, 0.0])
        scene.background_plane_size = torch.tensor([0.0, 0.0])
        scene.manual_exposure = 1.0
        scene._light_map = light_map
        out.append(scene)
    return out


def shading_expected(scene, cam_coord_centre, pair, sizes=A.SIZES):
    """Float64 expectation of the centre pixel: N from the object's pose, V from the pixel's camera coordinates."""
    cam = scene.camera_pose().numpy().astype(np.float64)
    obj = scene.objects[0]
    N = obj.pose().numpy().astype(np.float64)[:3, :3] @ np.array([0.0, 0.0, 1.0])
    world = cam[:3, :3] @ cam_coord_centre[:3].astype(np.float64) + cam[:3, 3]
    V = cam[:3, 3] - world
    assert min(np.abs(N / np.linalg.norm(N))) > 0.1              # the normal lies along no axis
    return A.shade(pair, SHADE_BASE, float(obj.metallic), float(obj.roughness), N, V, sizes["lut_size"], sizes["pre_levels"])


def shading_errors(scene_list, hdr, cam_coord, instance, pair):
    fig = {}
    W, H = scene_list[0].viewport
    for k, scene in enumerate(scene_list):
        assert instance[k, H // 2, W // 2, 0] == 1
        px = hdr[k, H // 2, W // 2]
        want = shading_expected(scene, cam_coord[k, H // 2, W // 2], pair)
        assert px[3] == 1.0
        fig["shade_m%g_r%g" % SHADE_CASES[k]] = np.abs(px[:3] - want).max()
        fig["shade_m%g_r%g_signal" % SHADE_CASES[k]] = want.min()
    return fig


@pytest.mark.parametrize("pair", range(N_PAIRS))
def test_ibl_shading_known_answer(sl, oracle, maps, pair):
    scs = shading_scenes(sl, HostLightMap())
    r = oracle_render(oracle, scs, maps[pair, "full"], A.SIZES)
    fig = shading_errors(scs, r.hdr, r.cam_coord, r.instance, pair)
    report("pair %d shading" % pair, fig)
    assert_within({k: v for k, v in fig.items() if not k.endswith("_signal")})
