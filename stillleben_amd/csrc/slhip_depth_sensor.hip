// Depth sensor model (this project's addition, no counterpart in the reference): the rasteriser's exact camera z as a
// rectified structured-light / active-stereo sensor with its projector at +baseline along camera x would deliver it.
// DESIGN.md "Depth sensor model" is the contract; tests/depth_sensor_ref.py restates it in the same float32 operation order
// (IEEE add, mul, div, floor, compare under -ffp-contract=off), so everything but the normal draws is bit-exact against it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "slhip.h"
#include "slhip_common.h"
#include "slhip_rng.h"

namespace {

static_assert(sizeof(slhip_depth_sensor_params) == 60, "slhip_depth_sensor_params layout");

constexpr int LINE = SLHIP_DEPTH_SENSOR_MAX_LINE;      // longest projector line (W + Dmax) pass 1 holds in LDS
constexpr int MAX_R = SLHIP_DEPTH_SENSOR_MAX_RADIUS;
constexpr int TILE_W = 32, TILE_H = 8;                 // output pixels of a pass-2 block
constexpr int MAX_HALO = 2 + MAX_R;                    // lateral jitter (+-2) + window radius
constexpr uint8_t OUTSIDE = 0x80;                      // LDS mark of a halo position beyond the image

// The limits slhip_depth_sensor_check_params refuses on the host, evaluated per image on the device: a record that breaks
// one must not index LDS.  *dmax = ceil(fb / z_min) >= every disparity fb / z of an in-range z (the f32 divide is monotone).
__host__ __device__ inline bool record_ok(const slhip_depth_sensor_params& p, int W, int* dmax)
{
    *dmax = 0;
    if (!(p.fb > 0.0f) || !(p.z_min > 0.0f) || !(p.z_max >= p.z_min) || p.window_radius > (uint32_t)MAX_R) return false;
    const float dm = ceilf(p.fb / p.z_min);
    if (!(dm <= (float)(LINE - W))) return false;
    *dmax = (int)dm;
    return true;
}

// projector column of pixel x at disparity d, as an index into the line (0 .. W + dmax - 1; the clamp never acts on a
// record that passed record_ok: 0 < d <= dmax gives -dmax <= k <= x)
__device__ __forceinline__ int line_index(int x, float d, int dmax, int len)
{
    const int k = (int)floorf((float)x - d + 0.5f) + dmax;
    return k < 0 ? 0 : (k >= len ? len - 1 : k);
}

// pass 1: one workgroup per image row.  Every in-range pixel splats its disparity onto the row's projector line with an
// integer max in LDS (positive floats order like their bits, so the result does not depend on the order); after the barrier
// a pixel whose projector column holds a disparity more than shadow_margin above its own lies in the projector's shadow.
__global__ __launch_bounds__(256) void k_depth_project(const float* __restrict__ z, uint32_t z_stride,
                                                       const float* __restrict__ c, uint32_t c_stride, uint32_t img0, int H,
                                                       int W, const slhip_depth_sensor_params* __restrict__ params,
                                                       float* __restrict__ d_plane, uint8_t* __restrict__ f_plane)
{
    __shared__ uint32_t line[LINE];
    __shared__ float drow[LINE];
    __shared__ uint8_t frow[LINE];
    const uint32_t img = img0 + blockIdx.x / (uint32_t)H;
    const int y = (int)(blockIdx.x % (uint32_t)H);
    const slhip_depth_sensor_params& p = params[img];
    const size_t row = ((size_t)img * H + y) * W;
    int dmax;
    if (!record_ok(p, W, &dmax)) {      // (uniform over the block)
        for (int x = threadIdx.x; x < W; x += 256) {
            d_plane[row + x] = 0.0f;
            f_plane[row + x] = SLHIP_DEPTH_FLAG_RANGE;
        }
        return;
    }
    const int len = W + dmax;
    for (int i = threadIdx.x; i < len; i += 256) line[i] = 0u;
    __syncthreads();
    const float fb = p.fb, z_min = p.z_min, z_max = p.z_max, cos_min = p.cos_min;
    const bool grazing = c != nullptr && cos_min > 0.0f;
    for (int x = threadIdx.x; x < W; x += 256) {
        const float zv = z[(row + x) * z_stride];
        float d = 0.0f;
        uint8_t f = SLHIP_DEPTH_FLAG_RANGE;
        if (zv >= z_min && zv <= z_max) {      // false for NaN
            d = fb / zv;
            f = 0;
            if (grazing && fabsf(c[(row + x) * c_stride]) < cos_min) f = SLHIP_DEPTH_FLAG_GRAZING;
            atomicMax(&line[line_index(x, d, dmax, len)], __float_as_uint(d));   // a grazing surface still blocks the projector
        }
        drow[x] = d;
        frow[x] = f;
    }
    __syncthreads();
    const float margin = p.shadow_margin;
    for (int x = threadIdx.x; x < W; x += 256) {
        const float d = drow[x];
        uint8_t f = frow[x];
        if (!(f & SLHIP_DEPTH_FLAG_RANGE) && __uint_as_float(line[line_index(x, d, dmax, len)]) > d + margin)
            f |= SLHIP_DEPTH_FLAG_SHADOW;
        d_plane[row + x] = d;
        f_plane[row + x] = f;
    }
}

// pass 2: 32 x 8 output pixels per block; disparity and flags of the tile and its halo of 2 + r pixels sit in LDS, the
// disparity of a flagged or outside pixel as NaN, so that the window count needs one read and one compare per pixel.
__global__ __launch_bounds__(256) void k_depth_measure(const float* __restrict__ d_plane, const uint8_t* __restrict__ f_plane,
                                                       uint32_t img0, int H, int W,
                                                       const slhip_depth_sensor_params* __restrict__ params,
                                                       float* __restrict__ out_f32, uint16_t* __restrict__ out_u16,
                                                       uint8_t* __restrict__ out_flags)
{
    __shared__ float td[(TILE_H + 2 * MAX_HALO) * (TILE_W + 2 * MAX_HALO)];
    __shared__ uint8_t tf[(TILE_H + 2 * MAX_HALO) * (TILE_W + 2 * MAX_HALO)];
    const uint32_t img = img0 + blockIdx.z;
    const int bx = blockIdx.x * TILE_W, by = blockIdx.y * TILE_H;
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int x = bx + lx, y = by + ly;
    const slhip_depth_sensor_params& p = params[img];
    const size_t plane = (size_t)img * H * W;
    int dmax;
    const int r = record_ok(p, W, &dmax) ? (int)p.window_radius : 0;   // (a refused record: pass 1 flagged every pixel)
    const int halo = 2 + r, tw = TILE_W + 2 * halo, th = TILE_H + 2 * halo;
    for (int i = threadIdx.x; i < tw * th; i += 256) {
        const int ty = i / tw, tx = i - ty * tw;
        const int xx = bx + tx - halo, yy = by + ty - halo;
        uint8_t f = OUTSIDE;
        float d = NAN;
        if (xx >= 0 && xx < W && yy >= 0 && yy < H) {
            const size_t at = plane + (size_t)yy * W + xx;
            f = f_plane[at];
            if (f == 0) d = d_plane[at];
        }
        td[i] = d;
        tf[i] = f;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    // the four draws are made whatever is switched off: the noise of one stage does not move when another is switched
    slhip::Rng rng(p.seed_lo, p.seed_hi, (uint32_t)(y * W + x), img);
    const float ex = rng.normal();
    const float ey = rng.normal();
    const float u = rng.uniform();
    const float en = rng.normal();
    const int jx = (int)fminf(fmaxf(floorf(p.sigma_lateral * ex + 0.5f), -2.0f), 2.0f);
    const int jy = (int)fminf(fmaxf(floorf(p.sigma_lateral * ey + 0.5f), -2.0f), 2.0f);
    const int sx = min(max(x + jx, 0), W - 1), sy = min(max(y + jy, 0), H - 1);
    const int ls = (sy - by + halo) * tw + (sx - bx + halo);
    uint32_t f = tf[ls];
    float z_out = 0.0f;
    if (f == 0) {
        const float ds = td[ls], tol = p.window_tol;
        uint32_t support = 0;
        for (int dy = -r; dy <= r; ++dy)
            for (int dx = -r; dx <= r; ++dx) support += fabsf(td[ls + dy * tw + dx] - ds) <= tol ? 1u : 0u;   // NaN: no
        if (support < p.min_support) f |= SLHIP_DEPTH_FLAG_SUPPORT;
        if (u < p.dropout_p) f |= SLHIP_DEPTH_FLAG_DROPOUT;
        const float dn = ds + p.sigma_disparity * en;
        float dq = dn;
        if (p.subpixel) {
            const float q = (float)p.subpixel;
            dq = floorf(dn * q + 0.5f) / q;
        }
        if (!(dq > 0.0f)) f |= SLHIP_DEPTH_FLAG_RANGE;
        else z_out = p.fb / dq;
    }
    const size_t at = plane + (size_t)y * W + x;
    if (out_f32) out_f32[at] = f ? 0.0f : z_out;
    if (out_u16) out_u16[at] = f ? (uint16_t)0 : (uint16_t)fminf(65535.0f, floorf(z_out * 1000.0f / p.depth_scale + 0.5f));
    if (out_flags) out_flags[at] = (uint8_t)f;
}

// optional HIP-event timing of the two passes (tools/time_depth_sensor.py): the events of the last timed call
bool g_timing = false;
hipEvent_t g_ev[3] = {nullptr, nullptr, nullptr};
bool g_timed = false;

}  // namespace

extern "C" int slhip_depth_sensor_timing_enable(int on)
{
    if (on && !g_ev[0])
        for (hipEvent_t& e : g_ev) SLHIP_CHECK(hipEventCreate(&e));
    g_timing = on != 0;
    g_timed = false;
    return 0;
}

extern "C" int slhip_depth_sensor_timings(float ms_out[2])
{
    if (!ms_out || !g_timed) {
        slhip::set_error("slhip_depth_sensor_timings: no timed call (slhip_depth_sensor_timing_enable(1), then slhip_depth_sensor)");
        return -1;
    }
    SLHIP_CHECK(hipEventSynchronize(g_ev[2]));
    SLHIP_CHECK(hipEventElapsedTime(&ms_out[0], g_ev[0], g_ev[1]));
    SLHIP_CHECK(hipEventElapsedTime(&ms_out[1], g_ev[1], g_ev[2]));
    return 0;
}

extern "C" int slhip_depth_sensor_check_params(const slhip_depth_sensor_params* h_params, uint32_t n_images, int W)
{
    if (!h_params && n_images) {
        slhip::set_error("slhip_depth_sensor_check_params: null argument");
        return -1;
    }
    if (W <= 0) {
        slhip::set_error("slhip_depth_sensor_check_params: bad image width %d", W);
        return -1;
    }
    for (uint32_t i = 0; i < n_images; ++i) {
        const slhip_depth_sensor_params& p = h_params[i];
        if (!(p.fb > 0.0f) || !(p.z_min > 0.0f) || !(p.z_max >= p.z_min) || !(p.depth_scale > 0.0f)) {
            slhip::set_error("slhip_depth_sensor: image %u: fb, z_min and depth_scale must be positive and z_max >= z_min "
                             "(fb %g, z_min %g, z_max %g, depth_scale %g)", i, p.fb, p.z_min, p.z_max, p.depth_scale);
            return -1;
        }
        if (p.window_radius > (uint32_t)MAX_R) {
            slhip::set_error("slhip_depth_sensor: image %u: window_radius %u exceeds %d", i, p.window_radius, MAX_R);
            return -1;
        }
        int dmax;
        if (!record_ok(p, W, &dmax)) {
            slhip::set_error("slhip_depth_sensor: image %u: W + Dmax = %d + %.0f exceeds %d, the projector line in LDS "
                             "(Dmax = ceil(fb / z_min): raise z_min or lower fb)", i, W, (double)ceilf(p.fb / p.z_min), LINE);
            return -1;
        }
    }
    return 0;
}

extern "C" int slhip_depth_sensor_scratch_bytes(uint32_t n_images, int W, int H, uint64_t* bytes)
{
    if (!bytes || W <= 0 || H <= 0 || (uint64_t)W * (uint64_t)H > 0x7fffffffu) {
        slhip::set_error("slhip_depth_sensor_scratch_bytes: bad argument (%d x %d)", W, H);
        return -1;
    }
    *bytes = (uint64_t)n_images * (uint64_t)W * (uint64_t)H * 5u;      // f32 disparity plane + u8 flag plane
    return 0;
}

extern "C" int slhip_depth_sensor(const float* d_depth, uint32_t depth_stride, const float* d_ndotv, uint32_t ndotv_stride,
                                  uint32_t n_images, int H, int W, const slhip_depth_sensor_params* d_params, float* d_out_f32,
                                  uint16_t* d_out_u16, uint8_t* d_flags, void* d_scratch, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_depth || !d_params || !d_scratch) {
        slhip::set_error("slhip_depth_sensor: null argument");
        return -1;
    }
    if (depth_stride == 0 || (d_ndotv && ndotv_stride == 0)) {
        slhip::set_error("slhip_depth_sensor: a stride of 0 floats");
        return -1;
    }
    if (H <= 0 || W <= 0 || (uint64_t)H * (uint64_t)W > 0x7fffffffu) {
        slhip::set_error("slhip_depth_sensor: bad image size %d x %d", W, H);
        return -1;
    }
    if (n_images == 0) return 0;
    float* d_plane = (float*)d_scratch;
    uint8_t* f_plane = (uint8_t*)d_scratch + (size_t)n_images * H * W * sizeof(float);
    // images per launch: what the grid's x (rows) and z (images) extents hold
    const uint32_t per_launch = (uint32_t)std::min<uint64_t>(65535u, 0x7fffffffu / (uint64_t)H);
    for (uint32_t i0 = 0; i0 < n_images; i0 += per_launch) {
        const uint32_t n = std::min(per_launch, n_images - i0);
        const bool timed = g_timing && i0 == 0;      // (the first launch pair: every image, up to 65535 of them)
        if (timed) SLHIP_CHECK(hipEventRecord(g_ev[0], stream));
        k_depth_project<<<dim3(n * (uint32_t)H), 256, 0, stream>>>(d_depth, depth_stride, d_ndotv, ndotv_stride, i0, H, W, d_params,
                                                                   d_plane, f_plane);
        if (timed) SLHIP_CHECK(hipEventRecord(g_ev[1], stream));
        k_depth_measure<<<dim3((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H, n), 256, 0, stream>>>(
            d_plane, f_plane, i0, H, W, d_params, d_out_f32, d_out_u16, d_flags);
        if (timed) {
            SLHIP_CHECK(hipEventRecord(g_ev[2], stream));
            g_timed = true;
        }
    }
    SLHIP_LAUNCH_CHECK();
    return 0;
}
