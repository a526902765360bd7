"""Float64 definition of the material part of the fragment stage -- texture2D (wrap modes, texel filters, level of detail),
sRGB decode, tangent-space normal maps, the metallic-roughness / emissive channels, the projected sticker and the direct-light
lobe -- for ONE textured quad seen by a pinhole camera.  Written from include/slhip.h (SLHIP_SAMPLER_*, the slhip_draw fields),
DESIGN.md and OpenGL 4.6 section 8.14; it imports nothing of stillleben_amd/csrc or oracle/ and shares no code with either.
tests/test_oracle_materials.py holds the CPU oracle to it, tests/test_gpu_materials_known.py the kernels.

Conventions (and where they come from)
  camera    x right, y DOWN, z forward: pixel (col, row) has its centre at (col + 0.5, row + 0.5) = (fx X / Z + cx, fy Y / Z + cy)
            (Scene.set_camera_intrinsics: clip w = +z, window = (ndc + 1) / 2 * viewport, no flip).
  quad      object frame: x, y in [-0.2, 0.2], z = 0, vertex normal +z, counter-clockwise seen from +z.  uv = shift + scale *
            (xy + 0.2) / 0.4.  Seen from the -z side the face is a back face and the shading normal is negated.
  2D rows   texture arrays are [rows, cols, 4] with row 0 = the top of the image (_loaders.ConsolidatedMesh.textures), and
            v = 0 is that top row: texel (col, row) covers u in [col, col + 1) / w, v in [row, row + 1) / h.  This is glTF's
            origin (the glTF loader takes TEXCOORD_0 as it is; the OBJ loader turns its bottom-up v into 1 - v "our textures
            are stored top-down").  No flip anywhere for 2D textures.
  sticker   a rectangle texture (slhip.h: "clamp to edge, row 0 = top of the image") addressed with OpenGL's bottom-up texel
            rows: the sticker frame's +y is the image's UP, so texel row j of GL is array row h - 1 - j.
  footprint this project's definition: forward differences of the exact uv to the pixel centres (x + 1, y) and (x, y + 1), the rays
            extended past the quad's edge; rho = max(|(du w, dv h) / dx|, |(du w, dv h) / dy|), lambda = log2 rho; the pixel is
            magnified when rho <= 1.

Bound: a pixel passes when |got - ref| <= RTOL |ref| + S + ATOL, with S the definition's own sensitivity: the largest change of the
float64 value when uv moves by (|duv/dx| + |duv/dy|) / 256 (oblique placements: the rasteriser snaps each corner to 1/256 px) plus
2^-20 max(1, |u|, |v|) (float32 interpolation), and lambda by 4e-6 (the kernels' log2 polynomial).  The move of uv is a move of
the point on the face: the object coordinates (the sticker's input) and the world point (the view vector's) move with it, which
matters where a mapped normal stands at right angles to the view.  S is evaluated at the eight corners of that box.  A pixel where a DISCRETE choice (nearest texel, level under mip 1, magnify / minify side with two different
filters, inside / outside of the sticker) changes within the box is a near-tie: left out of the value comparison and counted."""
import math

import numpy as np

W, H = 96, 64
HALF = 0.2
RTOL, ATOL = 1e-3, 1e-6
UV_SNAP, UV_F32, LAMBDA_MOVE = 1.0 / 256.0, 2.0 ** -20, 4e-6
TIE_CAP, MIN_COMPARED = 0.03, 500
REPEAT, CLAMP, MIRROR = 0, 1, 2
PI = math.pi


def sampler(ws=REPEAT, wt=REPEAT, mag=False, min_=False, mip=0):
    """The SLHIP_SAMPLER_* byte."""
    return ws | (wt << 2) | (0x10 if mag else 0) | (0x20 if min_ else 0) | (mip << 6)


# ---- textures -------------------------------------------------------------------------------------------------------------------
def distinct_texture(w, h, seed=0, alpha_min=140):
    """[h, w, 4] uint8, every texel a different value in every channel as far as the channel's range has values to give (alpha
    stays above the 0.5 cut-off of the alpha test, which is not this module's subject), each channel in an order of its own."""
    n = w * h
    rng = np.random.default_rng(1000 * w + h + seed)
    t = np.zeros((n, 4), np.uint8)
    for c in range(4):
        lo = alpha_min if c == 3 else 8
        vals = lo + (np.arange(n) * (255 - lo)) // max(1, n - 1) if n > 1 else np.array([(90, 150, 210, 230)[c]])
        t[:, c] = rng.permutation(vals)
    return t.reshape(h, w, 4)


def mip_chain(img):
    """Level l + 1 is the 2 x 2 box of level l, (sum + 2) >> 2, of max(1, n >> 1) texels per axis (an axis of one texel is read
    twice); the last level is floor(log2(max(w, h)))."""
    levels = [np.asarray(img, np.uint8)]
    h, w = levels[0].shape[:2]
    for _ in range(int(math.floor(math.log2(max(w, h))))):
        src = levels[-1].astype(np.int64)
        sh, sw = src.shape[:2]
        nh, nw = max(1, sh >> 1), max(1, sw >> 1)
        dst = np.zeros((nh, nw, 4), np.int64)
        for y in range(nh):
            for x in range(nw):
                ys, xs = (min(2 * y, sh - 1), min(2 * y + 1, sh - 1)), (min(2 * x, sw - 1), min(2 * x + 1, sw - 1))
                dst[y, x] = (src[ys[0], xs[0]] + src[ys[0], xs[1]] + src[ys[1], xs[0]] + src[ys[1], xs[1]] + 2) >> 2
        levels.append(dst.astype(np.uint8))
    assert levels[-1].shape[:2] == (1, 1)
    return levels


def wrap(i, n, mode):
    """Texel index for any integer (OpenGL 4.6 table 8.20)."""
    i = np.asarray(i, np.int64)
    if mode == CLAMP:
        return np.clip(i, 0, n - 1)
    if mode == MIRROR:
        m = np.mod(i, 2 * n)                       # numpy's mod: the non-negative remainder
        return np.where(m < n, m, 2 * n - 1 - m)
    return np.mod(i, n)


def sample_level(level, ws, wt, linear, u, v):
    """(rgba in [0, 1], nearest texel id or -1) of one level at (u, v)."""
    h, w = level.shape[:2]
    tex = level.astype(np.float64) / 255.0
    if not linear:
        ix, iy = wrap(np.floor(u * w), w, ws), wrap(np.floor(v * h), h, wt)
        return tex[iy, ix], iy * w + ix
    x, y = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    a, b = (x - x0)[..., None], (y - y0)[..., None]
    xa, xb, ya, yb = wrap(x0, w, ws), wrap(x0 + 1, w, ws), wrap(y0, h, wt), wrap(y0 + 1, h, wt)
    top = tex[ya, xa] * (1 - a) + tex[ya, xb] * a
    bot = tex[yb, xa] * (1 - a) + tex[yb, xb] * a
    return top * (1 - b) + bot * b, np.full(np.shape(u), -1, np.int64)


def footprint_lambda(fp, w, h):
    dudx, dvdx, dudy, dvdy = fp
    rho = np.maximum(np.hypot(dudx * w, dvdx * h), np.hypot(dudy * w, dvdy * h))
    return np.log2(rho)


def texture2d(levels, smp, u, v, lam, lam_key):
    """texture2D() of a chain at (u, v) with level of detail `lam`.  Returns (rgba, key): key [..., 4] holds the discrete choices
    -- magnify / minify side (when the two filters differ), the level under mip 1, the nearest texel of the level(s) in use --
    taken at the levels that `lam_key` (the undisplaced lambda) selects, so that a continuous change of level never reads as one."""
    ws, wt = smp & 3, (smp >> 2) & 3
    mag_lin, min_lin, mip = bool(smp & 0x10), bool(smp & 0x20), (smp >> 6) & 3
    top = len(levels) - 1
    cache = {}

    def at(l, linear):
        if (l, linear) not in cache:
            cache[l, linear] = sample_level(levels[l], ws, wt, linear, u, v)
        return cache[l, linear]

    def pick(lv, linear, what):
        out = np.zeros(np.shape(u) + ((4,) if what == 0 else ()), np.float64 if what == 0 else np.int64)
        for l in range(top + 1):
            m = lv == l
            if m.any():
                out[m] = at(l, linear)[what][m]
        return out

    def levels_of(lm):
        """(magnified, first level, second level, blend) per pixel"""
        magn = lm <= 0.0
        if mip == 0:
            return magn, np.zeros(np.shape(lm), np.int64), None, None
        if mip == 1:
            return magn, np.where(magn, 0, np.clip(np.ceil(lm + 0.5) - 1, 0, top)).astype(np.int64), None, None
        lc = np.clip(lm, 0.0, top)
        l0 = np.floor(lc).astype(np.int64)
        return magn, np.where(magn, 0, l0), np.where(magn, 0, np.minimum(l0 + 1, top)), np.where(magn, 0.0, lc - l0)

    magn, la, lb, f = levels_of(lam)
    out = np.where(magn[..., None], pick(la, mag_lin, 0), pick(la, min_lin, 0))
    if lb is not None:
        out = out + f[..., None] * (np.where(magn[..., None], pick(lb, mag_lin, 0), pick(lb, min_lin, 0)) - out)
    kmag, ka, kb, _ = levels_of(lam_key)
    key = np.zeros(np.shape(u) + (4,), np.int64)
    key[..., 0] = magn if mag_lin != min_lin else 0
    key[..., 1] = la if mip == 1 else 0
    key[..., 2] = np.where(kmag, pick(ka, mag_lin, 1), pick(ka, min_lin, 1))
    if kb is not None:
        key[..., 3] = np.where(kmag, pick(kb, mag_lin, 1), pick(kb, min_lin, 1))
    return out, key


def texture_rect(img, x, y):
    """Rectangle texture: texel coordinates, linear filter, clamp to edge; GL row j (bottom-up) is array row h - 1 - j."""
    h, w = img.shape[:2]
    tex = img.astype(np.float64) / 255.0
    xs, ys = x - 0.5, y - 0.5
    x0, y0 = np.floor(xs), np.floor(ys)
    a, b = (xs - x0)[..., None], (ys - y0)[..., None]
    xa, xb = np.clip(x0, 0, w - 1).astype(np.int64), np.clip(x0 + 1, 0, w - 1).astype(np.int64)
    ya, yb = h - 1 - np.clip(y0, 0, h - 1).astype(np.int64), h - 1 - np.clip(y0 + 1, 0, h - 1).astype(np.int64)
    lo = tex[ya, xa] * (1 - a) + tex[ya, xb] * a
    hi = tex[yb, xa] * (1 - a) + tex[yb, xb] * a
    return lo * (1 - b) + hi * b


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def rot_x(t):
    c, s = math.cos(t), math.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


FACING = np.diag([1.0, -1.0, -1.0])        # turns the quad's +z normal towards the camera; object +y is then UP in the picture

PLACEMENTS = {
    # name: (fx, fy, rotation, translation, snapped corners).  `exact`: corners at (48 +- 32, 32 +- 32) px, whole pixels
    "exact": (128.0, 128.0, FACING, (0.0, 0.0, 0.8), True),
    "oblique": (110.0, 110.0, rot_x(1.1) @ FACING, (0.0, 0.03, 0.46), False),
    "back": (110.0, 110.0, rot_x(1.1), (0.0, 0.03, 0.46), False),
    "grazing": (128.0, 512.0, rot_x(1.45) @ FACING, (0.0, 0.0, 0.8), False),
}


class Case:
    """One scene: the quad, its material and textures, the lights."""

    def __init__(self, name, placement="exact", uv_scale=1.0, uv_shift=0.0, base_color=(1.0, 1.0, 1.0, 1.0), metallic=0.0,
                 roughness=1.0, emissive=(0.0, 0.0, 0.0), tangent=(1.0, 0.0, 0.0, 1.0), tex=None, lights=(), ambient=(0.0, 0.0, 0.0),
                 sticker=None, light_map=False):
        self.name, self.placement, self.uv_scale, self.uv_shift = name, placement, float(uv_scale), float(uv_shift)
        self.base_color, self.metallic, self.roughness, self.emissive = base_color, metallic, roughness, emissive
        self.tangent, self.tex, self.ambient = tangent, dict(tex or {}), ambient      # tex: kind -> (uint8 [h, w, 4], sampler)
        self.lights = [(np.asarray(d, np.float64), np.asarray(c, np.float64)) for d, c in lights]   # (direction of travel, colour)
        self.sticker = sticker                                                        # dict(image=, range=, rotation=) or None
        self.light_map = light_map                                                    # the test module binds a constant map

    def normal(self):
        """World normal of the face as the camera sees it."""
        n = PLACEMENTS[self.placement][2] @ np.array([0.0, 0.0, 1.0])
        return -n if n[2] > 0 else n


TEX_KINDS = ("base", "normal", "mr", "occlusion", "emissive")


def build_scene(sl, case, light_map=None):
    """The sl.Scene of a case: one quad mesh built like quad_mesh of tests/test_gpu_materials.py, manual exposure, no plane."""
    import torch

    from stillleben_amd import _loaders

    m = _loaders.ConsolidatedMesh()
    m.positions = np.array([[-HALF, -HALF, 0], [HALF, -HALF, 0], [HALF, HALF, 0], [-HALF, HALF, 0]], np.float32)
    m.normals = np.array([[0, 0, 1]] * 4, np.float32)
    m.uvs = (np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64) * case.uv_scale + case.uv_shift).astype(np.float32)
    m.colors = np.ones((4, 4), np.float32)
    m.tangents = np.tile(np.asarray(case.tangent, np.float32), (4, 1))
    m.indices = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    index = {}
    for kind in TEX_KINDS:
        if kind in case.tex:
            index[kind] = len(m.textures)
            m.textures.append(np.ascontiguousarray(case.tex[kind][0]))
            m.tex_samplers.append(int(case.tex[kind][1]))
    m._tex_alpha = [False] * len(m.textures)
    m.materials = [_loaders.Material(base_color=case.base_color, metallic=case.metallic, roughness=case.roughness,
                                     emissive=case.emissive, base_texture=index.get("base"), normal_texture=index.get("normal"),
                                     mr_texture=index.get("mr"), occlusion_texture=index.get("occlusion"),
                                     emissive_texture=index.get("emissive"))]
    m.submeshes = [_loaders.SubMesh(0, 6, 0)]
    fx, fy, R, t, _ = PLACEMENTS[case.placement]
    scene = sl.Scene((W, H))
    scene.set_camera_intrinsics(fx, fy, W / 2.0, H / 2.0)
    obj = sl.Object(sl.Mesh.from_data(m))
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, t
    obj.set_pose(torch.from_numpy(pose.astype(np.float32)))
    if case.sticker is not None:
        obj.sticker_texture = sl.Texture2D(torch.from_numpy(np.ascontiguousarray(case.sticker["image"])))
        obj.sticker_range = list(case.sticker["range"])
        obj.sticker_rotation = list(case.sticker["rotation"])
    scene.add_object(obj)
    dirs, cols = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
    for i, (d, c) in enumerate(case.lights):
        dirs[i], cols[i] = d, c
    scene.light_directions = torch.from_numpy(dirs)
    scene.light_colors = torch.from_numpy(cols)
    scene.ambient_light = torch.tensor(list(case.ambient), dtype=torch.float32)
    scene.background_plane_size = torch.tensor([0.0, 0.0])
    scene.manual_exposure = 1.0
    if light_map is not None:
        scene._light_map = light_map
    return scene


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def geometry(case, scene):
    """Where the ray through every pixel centre (and through the centres one to the right and one below) meets the quad's plane:
    object coordinates, uv, world point, forward differences -- float64, from the scene's projection and poses."""
    P = scene.projection_matrix().numpy().astype(np.float64)
    cam = scene.camera_pose().numpy().astype(np.float64)
    o2w = scene.objects[0].pose().numpy().astype(np.float64)
    M = P @ np.linalg.inv(cam) @ o2w
    xs, ys = np.meshgrid(np.arange(W + 1) + 0.5, np.arange(H + 1) + 0.5)
    xn, yn = xs / (W / 2.0) - 1.0, ys / (H / 2.0) - 1.0
    # clip = M (a, b, 0, 1); clip.x = xn clip.w and clip.y = yn clip.w: two linear equations in (a, b)
    r0 = M[0][None, None, :] - xn[..., None] * M[3][None, None, :]
    r1 = M[1][None, None, :] - yn[..., None] * M[3][None, None, :]
    det = r0[..., 0] * r1[..., 1] - r0[..., 1] * r1[..., 0]
    a = (-r0[..., 3] * r1[..., 1] + r0[..., 1] * r1[..., 3]) / det
    b = (-r0[..., 0] * r1[..., 3] + r0[..., 3] * r1[..., 0]) / det
    u = case.uv_shift + case.uv_scale * (a + HALF) / (2 * HALF)
    v = case.uv_shift + case.uv_scale * (b + HALF) / (2 * HALF)
    g = {"obj": np.stack([a, b, np.zeros_like(a)], -1)[:H, :W], "u": u[:H, :W], "v": v[:H, :W]}
    g["fp"] = (u[:H, 1:] - u[:H, :W], v[:H, 1:] - v[:H, :W], u[1:, :W] - u[:H, :W], v[1:, :W] - v[:H, :W])
    # what the corner snap of an oblique placement moves the object coordinates by: the rule of the uv move (module docstring)
    snapped = PLACEMENTS[case.placement][4]
    g["obj_move"] = 0.0 if snapped else np.stack([np.abs(a[:H, 1:] - a[:H, :W]) + np.abs(a[1:, :W] - a[:H, :W]),
                                                  np.abs(b[:H, 1:] - b[:H, :W]) + np.abs(b[1:, :W] - b[:H, :W]),
                                                  np.zeros((H, W))], -1) * UV_SNAP
    g["world"] = g["obj"] @ o2w[:3, :3].T + o2w[:3, 3]
    g["inside"] = (np.abs(g["obj"][..., 0]) <= HALF + 1e-4) & (np.abs(g["obj"][..., 1]) <= HALF + 1e-4)   # (+ the corner snap)
    g["cam_position"], g["world_to_cam"], g["o2w"] = cam[:3, 3], np.linalg.inv(cam)[:3, :3], o2w
    return g


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _pixel(case, scene, g, du, dv, dl):
    """The definition at uv + (du, dv) and lambda + dl: (hdr [H, W, 4], normals [H, W, 4], key [H, W, K])."""
    u, v = g["u"] + du, g["v"] + dv
    keys = []

    def tex(kind):
        img, smp = case.tex[kind]
        lam = footprint_lambda(g["fp"], img.shape[1], img.shape[0])
        rgba, key = texture2d(case.chains[kind], smp, u, v, lam + dl, lam)
        keys.append(key)
        return rgba

    base = np.broadcast_to(np.asarray(case.base_color, np.float64), (H, W, 4)).copy()
    if "base" in case.tex:
        t = tex("base")
        base[..., :3] *= t[..., :3] ** 2.2                      # decoded AFTER filtering
        base[..., 3] *= t[..., 3]
    obj = scene.objects[0]
    # the object coordinates that belong to the (displaced) uv: every interpolated attribute moves with it, the decal's
    # coordinates and the world point (hence V) included
    oxy = np.stack([(u - case.uv_shift) / case.uv_scale, (v - case.uv_shift) / case.uv_scale], -1) * (2 * HALF) - HALF
    if case.sticker is not None:
        SP = obj.sticker_view_projection().astype(np.float64)
        o4 = np.concatenate([oxy, np.zeros((H, W, 1)), np.ones((H, W, 1))], -1)
        p = o4 @ SP.T
        rng = np.asarray(obj.sticker_range, np.float64)
        size = np.maximum(1e-6, rng[2:] - rng[:2])
        s = (p[..., :2] / p[..., 3:4] - rng[:2]) / size
        inside = (s[..., 0] >= 0) & (s[..., 1] >= 0) & (s[..., 0] < 1) & (s[..., 1] < 1)
        img = case.sticker["image"]
        st = texture_rect(img, s[..., 0] * img.shape[1], s[..., 1] * img.shape[0])
        st[..., :3] = st[..., :3] ** 2.2
        al = st[..., 3:4]
        base = np.where(inside[..., None], base * (1 - al) + st * al, base)
        keys.append(inside[..., None].astype(np.int64))
    o2w = g["o2w"]
    n2w = np.linalg.inv(o2w[:3, :3]).T                          # normal_to_world: the inverse transpose
    Ng = _unit(n2w @ np.array([0.0, 0.0, 1.0]))
    N = np.broadcast_to(Ng, (H, W, 3)).copy()
    if "normal" in case.tex:
        n = 2.0 * tex("normal")[..., :3] - 1.0
        T = _unit(n2w @ np.asarray(case.tangent[:3], np.float64))
        B = _unit(np.cross(Ng, T)) * case.tangent[3]
        N = _unit(n[..., 0:1] * T + n[..., 1:2] * B + n[..., 2:3] * Ng)
    rough = np.full((H, W), float(case.roughness))
    metal = np.full((H, W), float(case.metallic))
    emis = np.broadcast_to(np.asarray(case.emissive, np.float64), (H, W, 3)).copy()
    if "mr" in case.tex:
        t = tex("mr")
        rough, metal = rough * t[..., 1], metal * t[..., 2]
    if "emissive" in case.tex:
        emis *= tex("emissive")[..., :3] ** 2.2
    V = _unit(g["cam_position"] - (oxy @ g["o2w"][:3, :2].T + g["o2w"][:3, 3]))
    front = (V @ Ng) > 0.0
    N = np.where(front[..., None], N, -N)
    NoV_raw = np.sum(N * V, -1)
    NoV = np.clip(NoV_raw, 1e-5, 1.0)
    r = np.maximum(rough, 0.045)
    a2 = (r * r) ** 2
    k = (r + 1.0) ** 2 / 8.0
    m = metal[..., None]
    rgb = base[..., :3]
    F0 = 0.04 * (1 - m) + rgb * m
    kS = F0 + (np.maximum(1 - r[..., None], F0) - F0) * ((1 - NoV) ** 5)[..., None]
    kD = (1 - kS) * (1 - m)
    col = np.zeros((H, W, 3))
    g_ = lambda x: x / (x * (1 - k) + k)
    for d, c in case.lights:
        if not (np.any(d != 0) and np.any(c != 0)):
            continue
        L = -_unit(d)
        NoL = np.maximum(N @ L, 0.0)
        NoH = np.maximum(np.sum(N * _unit(V + L), -1), 0.0)
        D = a2 / (PI * (NoH * NoH * (a2 - 1) + 1) ** 2)
        G = g_(NoL) * g_(np.maximum(NoV_raw, 0.0))
        spec = (D * G)[..., None] * kS / np.maximum(4 * NoV * NoL, 0.001)[..., None]
        col += (kD * rgb / PI + spec) * c * NoL[..., None]
    col += np.asarray(case.ambient, np.float64) * rgb + emis
    hdr = np.concatenate([col, base[..., 3:4]], -1)
    nc = _unit(N @ g["world_to_cam"].T)
    normals = np.concatenate([nc, NoV_raw[..., None]], -1)
    key = np.concatenate(keys, -1) if keys else np.zeros((H, W, 1), np.int64)
    return hdr, normals, key


def evaluate(case, scene):
    """Reference of a case: dict with hdr, normals [H, W, 4], their sensitivities S_hdr, S_normals (same shapes), tie [H, W]
    (a discrete choice changes within the displacement), inside [H, W] (the ray meets the quad) and the geometry."""
    case.chains = {kind: mip_chain(img) for kind, (img, _) in case.tex.items()}
    g = geometry(case, scene)
    dudx, dvdx, dudy, dvdy = g["fp"]
    f32 = UV_F32 * np.maximum(1.0, np.maximum(np.abs(g["u"]), np.abs(g["v"])))
    snapped = PLACEMENTS[case.placement][4]
    mu = f32 + (0.0 if snapped else (np.abs(dudx) + np.abs(dudy)) * UV_SNAP)
    mv = f32 + (0.0 if snapped else (np.abs(dvdx) + np.abs(dvdy)) * UV_SNAP)
    hdr, normals, key = _pixel(case, scene, g, 0.0, 0.0, 0.0)
    S_h, S_n, tie = np.zeros_like(hdr), np.zeros_like(normals), np.zeros((H, W), bool)
    for su in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            for sl_ in (-1.0, 1.0):
                h2, n2, k2 = _pixel(case, scene, g, su * mu, sv * mv, sl_ * LAMBDA_MOVE)
                S_h, S_n = np.maximum(S_h, np.abs(h2 - hdr)), np.maximum(S_n, np.abs(n2 - normals))
                tie |= (k2 != key).any(-1)
    return {"hdr": hdr, "normals": normals, "S_hdr": S_h, "S_normals": S_n, "tie": tie, "inside": g["inside"], "geometry": g,
            "lambda": {kind: footprint_lambda(g["fp"], img.shape[1], img.shape[0]) for kind, (img, _) in case.tex.items()}}


def compare(case, ref, hdr, normals, instance, coord):
    """Holds one rendered picture to the reference.  Returns the figures (share of the bound used by the worst pixel, share of
    covered pixels left out as near-ties, pixels compared); asserts the sanity check, the caps and the bound."""
    covered = instance == 1
    assert (covered <= ref["inside"]).all() and covered.sum() >= 0.97 * ref["inside"].sum(), "coverage"
    obj_err = (np.abs(coord[..., :3].astype(np.float64) - ref["geometry"]["obj"]) - ref["geometry"]["obj_move"])[covered].max()
    assert obj_err <= 1e-5, "object coordinates differ from the renderer's by %.3g m beyond the corner snap" % obj_err
    use = covered & ~ref["tie"]
    share = 0.0
    for got, want, S in ((hdr, ref["hdr"], ref["S_hdr"]), (normals, ref["normals"], ref["S_normals"])):
        err = np.abs(got.astype(np.float64) - want)[use]
        share = max(share, float((err / (RTOL * np.abs(want[use]) + S[use] + ATOL)).max()))
    fig = {"share": share, "ties": float((covered & ref["tie"]).sum()) / covered.sum(), "compared": int(use.sum())}
    print("%-40s share of bound %.3f, near-ties %.2f %%, pixels %d" % (case.name, fig["share"], 100 * fig["ties"], fig["compared"]))
    return fig


def check(fig):
    assert fig["ties"] <= TIE_CAP, "near-ties %.2f %% above the cap" % (100 * fig["ties"])
    assert fig["compared"] >= MIN_COMPARED, "%d pixels compared" % fig["compared"]
    assert fig["share"] <= 1.0, "%.2f of the bound" % fig["share"]


def check_chain_layout(img, levels):
    """The chain equals what HostPool.add_texture lays out: level count, level sizes, bytes."""
    from stillleben_amd._batch import HostPool

    pool = HostPool()
    off, w, h = pool.add_texture(np.ascontiguousarray(img))
    assert (off, w, h) == (0, img.shape[1], img.shape[0])
    want = np.concatenate([lv.reshape(-1) for lv in levels])
    sizes = [(max(1, w >> l), max(1, h >> l)) for l in range(len(levels))]
    assert [(lv.shape[1], lv.shape[0]) for lv in levels] == sizes
    assert pool.n_tex_bytes == want.size == 4 * sum(a * b for a, b in sizes), "level count or sizes"
    assert np.array_equal(np.concatenate(pool.tex), want), "bytes"


# ---- the cases ------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 4), (3, 3), (5, 6), (7, 2), (8, 8), (16, 16)]        # (w, h)
WRAP_PAIRS = [(REPEAT, CLAMP), (CLAMP, MIRROR), (MIRROR, REPEAT)]          # S and T differ: a swapped axis shows
AMBIENT = (0.7, 0.9, 1.1)


def _about(n, axis, deg):
    """n turned by deg degrees about `axis` (Rodrigues)."""
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = math.radians(deg)
    return n * math.cos(t) + np.cross(axis, n) * math.sin(t) + axis * (axis @ n) * (1 - math.cos(t))


def lights_for(placement):
    """Two directional lights of different colours: one at 50 degrees to the face's normal, swung towards the camera's side so
    that the mirror direction misses the face, one at 35 degrees sideways.  Directions of TRAVEL (the scene's convention)."""
    n = Case("", placement).normal()
    l1 = _about(_about(n, (1.0, 0.0, 0.0), -50.0), n, 20.0)
    l2 = _about(n, (0.0, 1.0, 0.0), 35.0)
    return [(-l1, (2.5, 2.0, 1.5)), (-l2, (0.4, 0.9, 1.6))]


def size_cases(w, h):
    """Case 1: a texture of w x h distinct texels, the three wraps on S and T, nearest and linear, base level; uv from -1.25 to
    1.75 (nearest) or 1.25 (linear): negative indices, more than one period, and for every size but 8 and 16 the remainder of a
    size that is no power of two."""
    img = distinct_texture(w, h)
    out = []
    for ws, wt in WRAP_PAIRS:
        for lin in (False, True):
            out.append(Case("size %dx%d wrap %d%d %s" % (w, h, ws, wt, "linear" if lin else "nearest"), "exact",
                            uv_scale=2.5 if lin else 3.0, uv_shift=-1.25, ambient=AMBIENT,
                            tex={"base": (img, sampler(ws, wt, lin, lin, 0))}))
    return out


FILTERS = [(False, False), (True, True), (False, True), (True, False)]      # (mag linear, min linear)


def filter_cases(placement):
    """Case 2: the four filter pairs x mip 0, 1, 2 on a 16 x 16 texture.  On the exact placement once magnified (rho = 0.625) and
    once minified (rho = 2.625); the oblique placement crosses lambda = 0 and 2 within the face."""
    img = distinct_texture(16, 16, seed=1)
    out = []
    for mag, min_ in FILTERS:
        for mip in (0, 1, 2):
            smp = sampler(REPEAT, MIRROR, mag, min_, mip)
            tag = "mag %s min %s mip %d" % ("L" if mag else "N", "L" if min_ else "N", mip)
            if placement == "exact":
                out.append(Case("exact magnified " + tag, "exact", 2.5, -1.25, ambient=AMBIENT, tex={"base": (img, smp)}))
                out.append(Case("exact minified " + tag, "exact", 10.5, -1.25, ambient=AMBIENT, tex={"base": (img, smp)}))
            else:
                out.append(Case("oblique " + tag, "oblique", 5.5, -1.25, ambient=AMBIENT, tex={"base": (img, smp)}))
    return out


def chain_cases():
    """Case 2, the ends of the chain: lambda beyond the last level (the clamp), and chains whose axes reach one texel at different
    levels (1 x 4, 7 x 2, 5 x 6), read at every level by trilinear and nearest-level sampling."""
    out = []
    for (w, h), scale in (((16, 16), 330.0), ((5, 6), 90.0)):
        for mip in (1, 2):
            out.append(Case("beyond the last level %dx%d mip %d" % (w, h, mip), "exact", scale, -1.25, ambient=AMBIENT,
                            tex={"base": (distinct_texture(w, h, seed=2), sampler(REPEAT, REPEAT, True, True, mip))}))
    for w, h in ((1, 4), (7, 2), (5, 6)):
        for mip, lin in ((2, True), (1, False)):
            for scale in (170.0 / max(w, h), 370.0 / max(w, h)):                # rho = 2.66 and 5.78
                out.append(Case("uneven chain %dx%d mip %d scale %g" % (w, h, mip, scale), "exact", scale, -1.25, ambient=AMBIENT,
                                tex={"base": (distinct_texture(w, h, seed=3), sampler(MIRROR, REPEAT, lin, lin, mip))}))
    out.append(Case("uneven chain 7x2 oblique", "oblique", 6.5, -1.25, ambient=AMBIENT,
                    tex={"base": (distinct_texture(7, 2, seed=3), sampler(REPEAT, MIRROR, True, True, 2))}))
    return out


ORIENTATION = np.array([[[255, 0, 0, 255], [0, 255, 0, 255]],              # row 0 (top of the image): red, green
                        [[0, 0, 255, 255], [255, 255, 0, 255]]], np.uint8)  # row 1: blue, yellow


def orientation_case():
    return Case("orientation", "exact", ambient=(1.0, 1.0, 1.0), tex={"base": (ORIENTATION, sampler(CLAMP, CLAMP, False, False, 0))})


SRGB_BASE = (0.9, 0.5, 0.25, 1.0)


def srgb_case():
    img = np.full((4, 4, 4), 128, np.uint8)
    img[..., 3] = 255
    return Case("srgb", "exact", base_color=SRGB_BASE, ambient=AMBIENT, tex={"base": (img, sampler(mag=True, min_=True, mip=2))})


NORMAL_TEXELS = [(128, 128, 255), (218, 128, 218), (128, 40, 200)]
TANGENT = (0.8, 0.6, 0.0)


def normal_cases():
    """Case 5: constant normal maps with both signs of tangent.w (the bitangent), on both placements, and a 2 x 1 map under the
    linear filter whose blend is no unit vector: filtering comes before normalisation."""
    out = []
    for placement in ("exact", "oblique"):
        for texel in NORMAL_TEXELS:
            for sign in (1.0, -1.0):
                img = np.zeros((2, 2, 4), np.uint8)
                img[...] = texel + (255,)
                out.append(Case("normal %s %s w %+g" % (placement, texel, sign), placement, tangent=TANGENT + (sign,), metallic=0.2,
                                roughness=0.6, base_color=(0.8, 0.6, 0.4, 1.0), lights=lights_for(placement), ambient=(0.05, 0.05, 0.05),
                                tex={"normal": (img, sampler(mag=True, min_=True, mip=2))}))
    img = np.array([[NORMAL_TEXELS[1] + (255,), NORMAL_TEXELS[2] + (255,)]], np.uint8)
    for sign in (1.0, -1.0):
        out.append(Case("normal 2x1 linear w %+g" % sign, "exact", tangent=TANGENT + (sign,), metallic=0.2, roughness=0.6,
                        base_color=(0.8, 0.6, 0.4, 1.0), lights=lights_for("exact"), ambient=(0.05, 0.05, 0.05),
                        tex={"normal": (img, sampler(CLAMP, CLAMP, True, True, 0))}))
    return out


def channel_cases():
    """Case 6: roughness from g and metallic from b of a 2 x 2 nearest texture whose r and alpha would show if read instead; the
    emissive factor times a texture."""
    mr = np.array([[[250, 60, 230, 20], [10, 120, 160, 240]], [[240, 190, 90, 30], [20, 250, 25, 250]]], np.uint8)
    em = distinct_texture(3, 2, seed=5)
    kw = dict(base_color=(0.7, 0.5, 0.3, 1.0), metallic=0.9, roughness=0.95, ambient=(0.05, 0.05, 0.05))
    return [Case("metallic-roughness %s" % p, p, lights=lights_for(p), tex={"mr": (mr, sampler(CLAMP, CLAMP, False, False, 0))}, **kw)
            for p in ("exact", "oblique")] + \
           [Case("emissive", "exact", 2.0, -0.5, emissive=(1.5, 0.5, 2.5), lights=lights_for("exact"),
                 tex={"emissive": (em, sampler(MIRROR, REPEAT, True, True, 2)), "mr": (mr, sampler(REPEAT, REPEAT, False, False, 0))}, **kw)]


OCCLUSION_VALUE = 102                                                       # o = 0.4
LIGHT_MAP_RADIANCE = (1.0, 0.5, 3.0)


def occlusion_cases():
    """Case 6, occlusion: (no map, map, map + constant occlusion texture).  Emissive only besides the map, so that the first
    picture is what the other two hold beside their light-map part."""
    occ = np.full((2, 2, 4), OCCLUSION_VALUE, np.uint8)
    kw = dict(placement="oblique", base_color=(0.7, 0.5, 0.3, 1.0), metallic=0.3, roughness=0.5, emissive=(0.2, 0.1, 0.05))
    return [Case("occlusion: no map", **kw), Case("occlusion: map", light_map=True, **kw),
            Case("occlusion: map and texture", light_map=True, tex={"occlusion": (occ, sampler(mag=True, min_=True, mip=2))}, **kw)]


def sticker_image():
    """9 x 6 (w x h): distinct rows and columns, a transparent band (rows 1 and 2) and half-transparent texels."""
    img = distinct_texture(9, 6, seed=7, alpha_min=0)
    img[1:3, :, 3] = 0
    img[0, :, 3] = 255
    return img


def sticker_cases():
    """Case 7: the projected coordinates of the face run over [-0.707, 0.707]^2; the range covers part of it, so that the border
    between inside and outside and the clamp at the image's edge are in view."""
    img = sticker_image()
    base = distinct_texture(8, 8, seed=8)
    kw = dict(placement="exact", ambient=AMBIENT, tex={"base": (base, sampler(mag=True, min_=True, mip=2))})
    s, c = math.sin(math.radians(15.0)), math.cos(math.radians(15.0))       # 30 degrees about z
    return [Case("sticker", sticker=dict(image=img, range=(-0.5, -0.3, 0.4, 0.6), rotation=(0.0, 0.0, 0.0, 1.0)), **kw),
            Case("sticker rotated", sticker=dict(image=img, range=(-0.45, -0.35, 0.3, 0.5), rotation=(0.0, 0.0, s, c)), **kw)]


def lobe_cases():
    """Case 8: the untextured quad under two lights and ambient; roughness 0 runs into the 0.045 floor."""
    out = []
    for r in (0.0, 0.3, 0.7, 1.0):
        for m in (0.0, 0.5, 1.0):
            out.append(Case("lobe r %g m %g" % (r, m), "oblique", base_color=(0.8, 0.5, 0.2, 1.0), metallic=m, roughness=r,
                            lights=lights_for("oblique"), ambient=(0.03, 0.04, 0.05)))
    out.append(Case("lobe back face", "back", base_color=(0.8, 0.5, 0.2, 1.0), metallic=0.5, roughness=0.4,
                    lights=lights_for("back"), ambient=(0.03, 0.04, 0.05)))
    n = Case("", "grazing").normal()
    graze = _about(n, (1.0, 0.0, 0.0), -(90.0 - math.degrees(math.asin(0.0015))))       # N.L = 0.0015
    out.append(Case("lobe grazing", "grazing", base_color=(0.8, 0.5, 0.2, 1.0), metallic=0.5, roughness=0.5,
                    lights=[(-graze, (300.0, 250.0, 200.0))]))
    return out
