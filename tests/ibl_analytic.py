"""Float64 known answers for image-based lighting: the light map's four buffers, the sky and the IBL shading term,
evaluated for an environment whose radiance is LINEAR in the direction, L_c(d) = a_c + B_c . d / |d|.

Plain numpy; nothing here comes from oracle/ or from the product.  Every function restates a rule documented at
slhip_light_map / slhip_light_map_build in include/slhip.h or in the kernel comments of slhip_ibl.hip and k_shade, and
evaluates it on L itself: no cube texel is ever read, so the answers do not share the kernels' (or the oracle's) face
table, texel addressing, seam rule, tangent frames or row order.  With B dense, its rows of different length and no two
entries equal in magnitude, no two axes and no sign of an axis are interchangeable: a swapped or mirrored face, a
transposed s / t, a wrong seam neighbour, a flipped sky ray or a flipped image row order changes L by 0.1 .. 1.

The irradiance rule keeps the reference's tangent frame UNNORMALISED (right = up x N, up = N x right with up = +y, neither
divided by its length): that is deliberate, it is what the reference's shader computes, and kernel and oracle both follow
it.  With the frame normalised the sum would be the closed form a + (2/3) B . N (times the Riemann sum's pi / 79 sum(cos sin) = 0.9941); the
unnormalised frame departs from that closed form by up to 0.133 for the radiances below.  A "fix" of the frame on either
side therefore fails these tests.

What a linear radiance cannot see: the mip level the prefilter picks per sample (every level of the environment's mip
chain holds the same linear function up to O(texel^2)); tests/test_gpu_ibl.py::test_precompute_matches_oracle covers it.

Measured on the CPU (tests/test_oracle_ibl.py prints them): max |oracle.light_map_build - float64 reference| over both
radiances at SIZES below with a 256 x 512 equirectangular image, and the bound each test asserts (twice the measurement,
rounded up; the GPU tests add the device-vs-libm tolerances of tests/test_gpu_ibl.py on top):

    map                                                 measured    bound
    env level 0, all texels (worst at the poles)        1.77e-03    3.60e-03
    env level 0, clamped azimuth seam column            1.40e-03    2.80e-03
    env level 0, inner texels (derived, see below)      2.11e-05    3.00e-05
    irradiance                                          4.05e-05    8.20e-05
    prefilter level 0 (roughness 0)                     4.11e-05    8.30e-05
    prefilter level 1 (roughness 0.25)                  5.66e-04    1.14e-03
    prefilter level 2 (roughness 0.5)                   6.59e-04    1.32e-03
    prefilter level 3 (roughness 0.75)                  1.07e-03    2.15e-03
    prefilter level 4 (roughness 1)                     1.72e-03    3.45e-03
    BRDF table                                          4.12e-06    8.30e-06
    sky, env 512, within a texel of a face edge         2.21e-04    4.50e-04
    sky, env 512, about the middle of a face edge       3.28e-05    6.60e-05
    sky, env 512, elsewhere                             1.97e-05    4.00e-05
    sky, env 32, within a texel of a face edge          4.21e-03    8.50e-03
    sky, env 32, about the middle of a face edge        6.15e-04    1.23e-03
    sky, env 32, elsewhere                              6.12e-04    1.23e-03
    shading, metallic 0 roughness 1                     2.94e-03    5.90e-03
    shading, metallic 0 roughness 0.5                   2.65e-03    5.30e-03
    shading, metallic 1 roughness 0.25                  3.56e-03    7.20e-03

The signal these residuals stand against is B . N, about 0.5: sky and shading values are 0.4 .. 1.9.  The environment's
texels fall into three classes.  Within two image rows of a pole both bilinear rows clamp to the first (last) row.  Within
one image column of azimuth +-pi the columns clamp, as the reference's ClampToEdge sampler does (the image is not wrapped):
a quarter of a pixel of the gradient.  Everywhere else the bound is no measurement but the bilinear error of the image,
h^2 / 8 |L''| (bilinear_image_bound), plus the float32 rounding of the pixel coordinate and of the stored value: 2.85e-5
for the larger radiance.  The prefilter's residual grows with the roughness because wider lobes read coarser mip levels,
whose box-filtered texels hold L only to O(texel^2).  The sky's is the bilinear read of a cube whose texels hold L but lie
on a projected grid; pixels within a texel of a face edge add the seam rule's choice of the nearest texel in the
neighbouring face, which costs up to half a texel ALONG the edge -- nothing about the middle of an edge (less than 0.1 of
the face's half width from it), where the two faces' rows line up: there a clamped or wrong neighbour stands out by a
factor of ten.  The shading's is the 8^2 irradiance and the 16^2 .. 1^2 prefilter faces read bilinearly at N and
reflect(-V, N).
"""
import functools
import math

import numpy as np

PI = 3.14159265359                      # the shaders' constant
INV_ATAN = (0.1591, 0.3183)             # the equirectangular shader's truncated 1 / (2 pi), 1 / pi
N_SAMPLES = 1024                        # Hammersley points of the prefilter and of the BRDF table
DELTA = 0.02                            # step of the irradiance sum

# a_c > |B_c| keeps L positive; rows of different length (0.616 0.495 0.729 / 0.577 0.628 0.482), all entries nonzero
PAIRS = (
    (np.array([1.0, 0.8, 1.2]), np.array([[0.5, -0.2, 0.3], [-0.15, 0.4, 0.25], [0.22, 0.35, -0.6]])),
    (np.array([0.9, 1.1, 0.7]), np.array([[-0.3, 0.45, 0.2], [0.35, 0.15, -0.5], [0.1, -0.25, 0.4]])),
)

SIZES = dict(env_size=512, env_levels=10, irr_size=8, pre_size=16, pre_levels=5, lut_size=16)
SIZES_COARSE = dict(env_size=32, env_levels=6, irr_size=4, pre_size=16, pre_levels=3, lut_size=16)
EQUIRECT_SHAPE = (256, 512)

# key -> bound; the table in the module docstring says where each comes from
BOUNDS = {
    "env_all": 3.60e-03,
    "env_seam": 2.80e-03,
    "env_inner": 3.00e-05,
    "irradiance": 8.20e-05,
    "prefilter_0": 8.30e-05,
    "prefilter_1": 1.14e-03,
    "prefilter_2": 1.32e-03,
    "prefilter_3": 2.15e-03,
    "prefilter_4": 3.45e-03,
    "brdf_lut": 8.30e-06,
    "sky_512_edge": 4.50e-04,
    "sky_512_edge_mid": 6.60e-05,
    "sky_512_rest": 4.00e-05,
    "sky_32_edge": 8.50e-03,
    "sky_32_edge_mid": 1.23e-03,
    "sky_32_rest": 1.23e-03,
    "shade_m0_r1": 5.90e-03,
    "shade_m0_r0.5": 5.30e-03,
    "shade_m1_r0.25": 7.20e-03,
}


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def radiance(pair, d):
    """L(d) = a + B . d / |d| for directions d [..., 3] -> [..., 3]."""
    a, B = PAIRS[pair] if isinstance(pair, int) else pair
    return a + _unit(d) @ B.T


def equirect(pair, H, W):
    """The image of L at the pixel centres, float64 [H, W, 3], row 0 at the top: the inverse of the documented mapping
    u = atan2(y, x) * 0.1591 + 0.5 along the row, w = asin(z) * 0.3183 + 0.5 with w = 1 at the top of the image."""
    u = (np.arange(W) + 0.5) / W
    w = 1.0 - (np.arange(H) + 0.5) / H
    az, lat = (u - 0.5) / INV_ATAN[0], (w - 0.5) / INV_ATAN[1]
    d = np.stack(np.broadcast_arrays(np.cos(lat)[:, None] * np.cos(az)[None, :], np.cos(lat)[:, None] * np.sin(az)[None, :],
                                     np.sin(lat)[:, None]), axis=-1)
    return radiance(pair, d)


def image_row_col(d, H, W):
    """Continuous pixel coordinates (row, column; pixel centres at integers + 0.5) at which direction d reads the image."""
    d = _unit(d)
    u = np.arctan2(d[..., 1], d[..., 0]) * INV_ATAN[0] + 0.5
    w = np.arcsin(np.clip(d[..., 2], -1.0, 1.0)) * INV_ATAN[1] + 0.5
    return (1.0 - w) * H, u * W


def face_dirs(face, s, t):
    """OpenGL 4.5 table 8.19 read backwards: the (unnormalised) direction at face coordinates s, t in [-1, 1]."""
    one = np.ones_like(s)
    return np.stack({0: (one, -t, -s), 1: (-one, -t, s), 2: (s, one, t), 3: (s, -one, -t), 4: (s, -t, one), 5: (-s, -t, -one)}[face],
                    axis=-1)


def face_coords(d):
    """OpenGL 4.5 table 8.19: direction -> (face, s, t), face order +X -X +Y -Y +Z -Z, s and t in [-1, 1]."""
    d = np.asarray(d, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    is_x = (ax >= ay) & (ax >= az)
    is_y = ~is_x & (ay >= az)
    face = np.where(is_x, np.where(x >= 0, 0, 1), np.where(is_y, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))
    sc = np.choose(face, [-z, z, x, x, x, -x])
    tc = np.choose(face, [-y, -y, z, -z, -y, -y])
    ma = np.where(is_x, ax, np.where(is_y, ay, az))
    return face, sc / ma, tc / ma


def texel_dirs(n):
    """Unit directions of all texel centres, [6, n, n, 3] indexed [face, row along t, column along s]."""
    c = (2.0 * (np.arange(n) + 0.5)) / n - 1.0
    t, s = np.meshgrid(c, c, indexing="ij")
    return _unit(np.stack([face_dirs(f, s, t) for f in range(6)]))


def env0(pair, n):
    """Level 0 of the environment cube: L at the texel centres, [6, n, n, 3]."""
    return radiance(pair, texel_dirs(n))


def _f32_steps(limit):
    """The values a float32 loop `for (x = 0; x < limit; x += 0.02f)` visits (the kernel accumulates in float32)."""
    out, x, d = [], np.float32(0.0), np.float32(DELTA)
    while x < limit:
        out.append(float(x))
        x = np.float32(x + d)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def irradiance_steps():
    """(phi values, theta values): 315 and 79 of them."""
    pi32 = np.float32(PI)
    return _f32_steps(np.float32(2.0) * pi32), _f32_steps(np.float32(0.5) * pi32)


def irradiance_at(pair, N):
    """The irradiance rule at unit normals N [..., 3]: sum over phi in [0, 2 pi), theta in [0, pi / 2) in steps of 0.02 of
    L(sin th cos ph right + sin th sin ph up + cos th N) cos th sin th, times pi / count; right = (0, 1, 0) x N and
    up = N x right, NOT normalised (see the module docstring)."""
    a, B = PAIRS[pair]
    N = _unit(N)
    shape = N.shape[:-1]
    N = N.reshape(-1, 3)
    phi, theta = irradiance_steps()
    st, ct = np.sin(theta), np.cos(theta)
    tx, ty, tz = st[None, :] * np.cos(phi)[:, None], st[None, :] * np.sin(phi)[:, None], np.broadcast_to(ct, (len(phi), len(theta)))
    wgt = np.broadcast_to(ct * st, (len(phi), len(theta)))
    out = np.empty((len(N), 3))
    for k0 in range(0, len(N), 32):
        n = N[k0:k0 + 32]
        right = np.cross(np.array([0.0, 1.0, 0.0]), n)
        up = np.cross(n, right)
        sv = (tx[None, :, :, None] * right[:, None, None, :] + ty[None, :, :, None] * up[:, None, None, :]
              + tz[None, :, :, None] * n[:, None, None, :])
        mean = (_unit(sv) * wgt[None, :, :, None]).sum(axis=(1, 2))
        out[k0:k0 + 32] = (a * wgt.sum() + mean @ B.T) * (PI / wgt.size)
    return out.reshape(shape + (3,))


def irradiance(pair, n):
    return irradiance_at(pair, texel_dirs(n))


@functools.lru_cache(maxsize=None)
def hammersley():
    """(i / 1024, radical inverse of i in base 2), i < 1024."""
    i = np.arange(N_SAMPLES, dtype=np.uint64)
    rev = np.zeros(N_SAMPLES, np.uint64)
    for b in range(32):
        rev |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return i.astype(np.float64) / N_SAMPLES, rev.astype(np.float64) * 2.0 ** -32


def ggx_half_vectors(N, roughness):
    """The 1024 importance-sampled GGX half vectors about each unit normal N [K, 3] -> [K, 1024, 3]: alpha = roughness^2,
    phi = 2 pi xi_x, cos theta = sqrt((1 - xi_y) / (1 + (alpha^2 - 1) xi_y)); tangent = normalize(up x N) with up = +z, or +x
    where |N.z| >= 0.999, bitangent = N x tangent."""
    xi_x, xi_y = hammersley()
    a = roughness * roughness
    phi = 2.0 * PI * xi_x
    cos_t = np.sqrt((1.0 - xi_y) / (1.0 + (a * a - 1.0) * xi_y))
    sin_t = np.sqrt(np.maximum(1.0 - cos_t * cos_t, 0.0))
    hx, hy, hz = np.cos(phi) * sin_t, np.sin(phi) * sin_t, cos_t
    up = np.where((np.abs(N[:, 2]) < 0.999)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    tangent = _unit(np.cross(up, N))
    bitangent = np.cross(N, tangent)
    return _unit(hx[None, :, None] * tangent[:, None, :] + hy[None, :, None] * bitangent[:, None, :] + hz[None, :, None] * N[:, None, :])


def prefilter_at(pair, N, roughness):
    """The prefilter rule at unit directions N [..., 3] (V = N): sum_k L(L_k) N.L_k / sum_k N.L_k over the samples with
    N.L_k > 0, L_k = reflect(-V, H_k)."""
    N = _unit(N)
    shape = N.shape[:-1]
    N = N.reshape(-1, 3)
    Hh = ggx_half_vectors(N, roughness)
    Lk = _unit(2.0 * (Hh * N[:, None, :]).sum(-1, keepdims=True) * Hh - N[:, None, :])
    ndl = np.maximum((Lk * N[:, None, :]).sum(-1), 0.0)
    out = (radiance(pair, Lk) * ndl[..., None]).sum(1) / ndl.sum(1)[:, None]
    return out.reshape(shape + (3,))


def prefilter(pair, n, roughness):
    return prefilter_at(pair, texel_dirs(n), roughness)


def level_roughness(level, levels):
    return level / (levels - 1) if levels > 1 else 0.0


@functools.lru_cache(maxsize=None)
def brdf_lut(n):
    """The split-sum table [n, n, 2] (scale, bias of F0), row = roughness (j + 0.5) / n, column = N.V (i + 0.5) / n; N = +z,
    V = (sqrt(1 - NdotV^2), 0, NdotV), G = product of x / (x (1 - k) + k) with k = roughness^2 / 2 for N.L and N.V,
    G_vis = G V.H / (N.H N.V), Fc = (1 - V.H)^5, scale = mean((1 - Fc) G_vis), bias = mean(Fc G_vis)."""
    out = np.zeros((n, n, 2))
    Nz = np.array([[0.0, 0.0, 1.0]])
    for j in range(n):
        r = (j + 0.5) / n
        Hh = ggx_half_vectors(Nz, r)[0]
        k = r * r / 2.0
        for i in range(n):
            ndv = (i + 0.5) / n
            V = np.array([math.sqrt(1.0 - ndv * ndv), 0.0, ndv])
            Lk = _unit(2.0 * (Hh @ V)[:, None] * Hh - V)
            ndl, ndh, vdh = np.maximum(Lk[:, 2], 0.0), np.maximum(Hh[:, 2], 0.0), np.maximum(Hh @ V, 0.0)
            m = ndl > 0.0
            G = (ndl[m] / (ndl[m] * (1.0 - k) + k)) * (ndv / (ndv * (1.0 - k) + k))
            g_vis = G * vdh[m] / (ndh[m] * ndv)
            fc = (1.0 - vdh[m]) ** 5
            out[j, i] = ((1.0 - fc) * g_vis).sum() / N_SAMPLES, (fc * g_vis).sum() / N_SAMPLES
    return out


def _bilinear_clamped(table, x, y):
    """Bilinear read of table [n, n, C] at column x, row y in texel units (centres at integers + 0.5), clamped to the edge."""
    n = table.shape[0]
    x, y = x - 0.5, y - 0.5
    x0, y0 = math.floor(x), math.floor(y)
    a, b = x - x0, y - y0
    cl = lambda i: min(max(i, 0), n - 1)
    top = table[cl(y0), cl(x0)] * (1 - a) + table[cl(y0), cl(x0 + 1)] * a
    bot = table[cl(y0 + 1), cl(x0)] * (1 - a) + table[cl(y0 + 1), cl(x0 + 1)] * a
    return top * (1 - b) + bot * b


def shade(pair, base, metallic, roughness, N, V, lut_size, pre_levels):
    """The IBL term of k_shade (render_shader.frag:375-394) with no other light: split sum with the multiple-scattering term.
    The irradiance is read at N, the prefiltered radiance at reflect(-V, N) as the linear blend of the two levels around
    roughness * 4, the BRDF table bilinearly at (N.V, roughness) -- all three from the rules above, evaluated at exactly
    those directions."""
    base, N, V = np.asarray(base, np.float64), _unit(N), _unit(V)
    roughness = max(roughness, 0.045)
    nov = min(max(float(N @ V), 1e-5), 1.0)
    F0 = 0.04 * (1.0 - metallic) + base * metallic
    kS = F0 + (np.maximum(1.0 - roughness, F0) - F0) * (1.0 - nov) ** 5
    fa, fb = _bilinear_clamped(brdf_lut(lut_size), nov * lut_size, roughness * lut_size)
    R = 2.0 * float(N @ V) * N - V
    lod = min(max(roughness * 4.0, 0.0), pre_levels - 1.0)
    l0 = int(math.floor(lod))
    l1, f = min(l0 + 1, pre_levels - 1), lod - l0
    rad = (1.0 - f) * prefilter_at(pair, R, level_roughness(l0, pre_levels)) + f * prefilter_at(pair, R, level_roughness(l1, pre_levels))
    irr = irradiance_at(pair, N)
    Ems = 1.0 - (fa + fb)
    FssEss = kS * fa + fb
    F_avg = F0 + (1.0 - F0) / 21.0
    FmsEms = Ems * FssEss * F_avg / (1.0 - F_avg * Ems)
    k_D = base * (1.0 - 0.04) * (1.0 - metallic) * (1.0 - FssEss - FmsEms)
    return FssEss * rad + (FmsEms + k_D) * irr


def cube_levels(buf, size, levels):
    """Splits a cube buffer laid out as slhip_light_map documents into its levels, each [6, m, m, 4]."""
    out, off = [], 0
    for l in range(levels):
        m = size >> l
        out.append(np.asarray(buf[off:off + 24 * m * m]).reshape(6, m, m, 4))
        off += 24 * m * m
    assert off == len(buf)
    return out


def bilinear_image_bound(pair, H, W):
    """h^2 / 8 |L''| for the bilinear read of the equirectangular image: along the row the image is L at azimuth steps of
    1 / (0.1591 W), down the column at latitude steps of 1 / (0.3183 H); both second derivatives of a + B_c . d are at most
    |B_c|."""
    hx, hy = 1.0 / (INV_ATAN[0] * W), 1.0 / (INV_ATAN[1] * H)
    return (hx * hx + hy * hy) / 8.0 * np.linalg.norm(PAIRS[pair][1], axis=1).max()
