// Pose VSD (this project's addition, no counterpart in the reference): BOP's Visible Surface Discrepancy of pose estimates
// against a batch's ground truth.  include/slhip.h "Pose VSD" and DESIGN.md "Pose VSD" are the contract; the coverage is exact
// integer arithmetic, the floats one rounded operation at a time (-ffp-contract=off), through slhip_vsd_rules.h on host and
// device alike, so tests/pose_vsd_ref.py restates it and every output is bit-exact against it.
//   k_pose_vsd    one workgroup per (scene, object, hypothesis): (1) the window -- the union of the pixel boxes of the class's
//                 triangles under both poses, reduced in LDS;  (2) per band of whole window rows, two uint32 planes in LDS
//                 (ground truth, estimate) filled by atomicMin on the bits of z: a lane per triangle with a small pixel box, a
//                 wave per triangle with a large one, picked by a ballot;  (3) the comparison of the band's pixels with the
//                 scene's depth, 4 + T integer counts per lane, reduced once at the end.  No depth plane reaches HBM.
//   k_pose_depth  (1) and (2) for one pose; the band is written to the dense plane, zeros elsewhere
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_step_timer.h"
#include "slhip_vsd_rules.h"

#ifndef SLHIP_VSD_BAND_PIXELS
#define SLHIP_VSD_BAND_PIXELS 4096      // measured against 8192 and 16384: DESIGN.md "Pose VSD"
#endif

namespace {

static_assert(sizeof(slhip_pose_vsd_params) == 128, "slhip_pose_vsd_params layout");
static_assert(sizeof(slhip_pose_surface) == 56, "slhip_pose_surface layout");

using Params = slhip_pose_vsd_params;
using Surface = slhip_pose_surface;
using Out = slhip_pose_vsd_out;
namespace vr = slhip_vsd;

constexpr uint32_t BLOCK = vr::BLOCK;
constexpr uint32_t NWAVES = BLOCK / vr::WAVE;
constexpr uint32_t BAND_PIXELS = SLHIP_VSD_BAND_PIXELS;
constexpr int SMALL_BOX = 32;                               // a pixel box of more pixels than this is rastered by a whole wave
constexpr uint32_t TAUS = SLHIP_VSD_TAUS_MAX;
constexpr uint32_t N_COUNTS = 4u + TAUS;
static_assert(BAND_PIXELS >= SLHIP_VSD_WIDTH_MAX, "a band holds at least one row of the widest picture");

struct Window {
    int x0, x1, y0, y1;      // pixels, inclusive; x0 > x1: empty
};

// triangle `tri` of the table under the pose M, its box clamped to w
__device__ __forceinline__ int load_tri(const Surface& s, uint32_t tri, const float* M, const Params& p, const Window& w, vr::Tri& t)
{
    const uint32_t* ix = s.triangles + (size_t)tri * 3u;
    const uint32_t i0 = ix[0], i1 = ix[1], i2 = ix[2];
    if (i0 >= s.n_vertices || i1 >= s.n_vertices || i2 >= s.n_vertices) return vr::TRI_EMPTY;
    const float4* v = reinterpret_cast<const float4*>(s.vertices);
    const float4 a = v[i0], b = v[i1], c = v[i2];
    const vr::Vertex va = vr::project(M, a.x, a.y, a.z, p.fx, p.fy, p.cx, p.cy, p.z_near);
    const vr::Vertex vb = vr::project(M, b.x, b.y, b.z, p.fx, p.fy, p.cx, p.cy, p.z_near);
    const vr::Vertex vc = vr::project(M, c.x, c.y, c.z, p.fx, p.fy, p.cx, p.cy, p.z_near);
    return vr::setup(va, vb, vc, w.x0, w.x1, w.y0, w.y1, t);
}

// (1) the union of the pixel boxes of triangles [begin, begin + count) under the pose M into s_box (x0, y0 by min; x1, y1 by
// max), and whether one of them was clipped
__device__ __forceinline__ void window_pass(const Surface& s, uint32_t begin, uint32_t count, const float* M, const Params& p,
                                            int* s_box, uint32_t* s_clipped)
{
    const Window whole = {0, p.W - 1, 0, p.H - 1};
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    bool clipped = false;
    for (uint32_t i = threadIdx.x; i < count; i += BLOCK) {
        vr::Tri t;
        const int st = load_tri(s, begin + i, M, p, whole, t);
        clipped = clipped || st == vr::TRI_CLIPPED;
        if (st == vr::TRI_OK) {
            x0 = min(x0, t.x0); y0 = min(y0, t.y0);
            x1 = max(x1, t.x1); y1 = max(y1, t.y1);
        }
    }
    if (x1 >= 0) {
        atomicMin(&s_box[0], x0); atomicMin(&s_box[1], y0);
        atomicMax(&s_box[2], x1); atomicMax(&s_box[3], y1);
    }
    if (clipped) *s_clipped = 1u;
}

template <class I>
__device__ __forceinline__ void raster_lane(const vr::Tri& t, const Window& band, int ww, uint32_t* plane)
{
    for (int py = t.y0; py <= t.y1; ++py)
        for (int px = t.x0; px <= t.x1; ++px) {
            uint32_t bits;
            if (vr::pixel_depth<I>(t, px, py, &bits)) atomicMin(&plane[(py - band.y0) * ww + (px - band.x0)], bits);
        }
}

// the 64 lanes of a wave over the pixels of one triangle's box (t is the same in every lane)
template <class I>
__device__ __forceinline__ void raster_wave(const vr::Tri& t, const Window& band, int ww, uint32_t* plane, int lane)
{
    const int bw = t.x1 - t.x0 + 1, n = bw * (t.y1 - t.y0 + 1);
    const int step_y = (int)vr::WAVE / bw, step_x = (int)vr::WAVE - step_y * bw;      // 64 pixels on, without a division
    int oy = lane / bw, ox = lane - oy * bw;
    for (int i = lane; i < n; i += (int)vr::WAVE) {
        uint32_t bits;
        if (vr::pixel_depth<I>(t, t.x0 + ox, t.y0 + oy, &bits)) atomicMin(&plane[(t.y0 + oy - band.y0) * ww + (t.x0 + ox - band.x0)], bits);
        ox += step_x;
        oy += step_y;
        if (ox >= bw) {
            ox -= bw;
            ++oy;
        }
    }
}

__device__ __forceinline__ int bcast(int v, int src) { return __shfl(v, src); }
__device__ __forceinline__ float bcast(float v, int src) { return __shfl(v, src); }

// (2) triangles [begin, begin + count) under the pose M into the band's plane (ww pixels per row), by min on the bits of z
__device__ __forceinline__ void raster_band(const Surface& s, uint32_t begin, uint32_t count, const float* M, const Params& p,
                                            const Window& band, uint32_t* plane)
{
    const int ww = band.x1 - band.x0 + 1, lane = (int)(threadIdx.x % vr::WAVE);
    for (uint32_t base = 0u; base < count; base += BLOCK) {      // the same trips for every lane: the ballot below needs them all
        const uint32_t i = base + threadIdx.x;
        vr::Tri t = {};
        const bool live = i < count && load_tri(s, begin + i, M, p, band, t) == vr::TRI_OK;
        const bool large = live && (t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > SMALL_BOX;
        if (live && !large) {
            if (t.narrow) raster_lane<int>(t, band, ww, plane);
            else raster_lane<long long>(t, band, ww, plane);
        }
        unsigned long long todo = __ballot(large);
        while (todo) {      // wave-uniform
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            vr::Tri u;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                u.X[k] = bcast(t.X[k], src);
                u.Y[k] = bcast(t.Y[k], src);
                u.iz[k] = bcast(t.iz[k], src);
            }
            u.fa = bcast(t.fa, src);
            u.flipped = bcast(t.flipped, src);
            u.narrow = bcast(t.narrow, src);
            u.x0 = bcast(t.x0, src); u.x1 = bcast(t.x1, src);
            u.y0 = bcast(t.y0, src); u.y1 = bcast(t.y1, src);
            if (u.narrow) raster_wave<int>(u, band, ww, plane, lane);
            else raster_wave<long long>(u, band, ww, plane, lane);
        }
    }
}

struct ClassRange {
    uint32_t cls, begin, count;
    bool ok;
};

// (host and device: the host twins read their classes the same way)
__host__ __device__ __forceinline__ ClassRange class_range(const Surface& s, const int32_t* classes, uint32_t class_stride, size_t so)
{
    ClassRange c;
    c.cls = (uint32_t)classes[so * class_stride];
    c.begin = c.count = 0u;
    if (c.cls < s.n_assets) {
        c.begin = s.tri_begin[c.cls];
        c.count = s.tri_count[c.cls];
    }
    c.ok = vr::surface_ok(c.cls, s.n_assets, c.begin, c.count, s.n_triangles);
    return c;
}

// the rows [y0, y0 + rows) of a window that one band takes
__device__ __forceinline__ int band_rows(const Window& w) { return (int)(BAND_PIXELS / (uint32_t)(w.x1 - w.x0 + 1)); }

__device__ __forceinline__ void write_all(const Out& out, const Params& p, size_t at, float v, int n)
{
    const uint32_t T = p.n_taus, tid = threadIdx.x;
    if (tid < T) {
        if (p.outputs & SLHIP_VSD_OUT_VSD) out.vsd[at * T + tid] = v;
        if (p.outputs & SLHIP_VSD_OUT_COST) out.n_cost[at * T + tid] = n;
    }
    if (tid < 4u && (p.outputs & SLHIP_VSD_OUT_COUNTS)) out.counts[at * 4u + tid] = n;
    if (tid == 0u && (p.outputs & SLHIP_VSD_OUT_FLAGS)) out.flags[at] = 0u;
}

// Block x = (scene * O + object) * Hy + hypothesis.
__global__ __launch_bounds__(BLOCK) void k_pose_vsd(Params p, Surface s, const int32_t* __restrict__ classes, uint32_t class_stride,
                                                    const float* __restrict__ gt, const float* __restrict__ est,
                                                    const float* __restrict__ depth, uint32_t depth_stride, Out out)
{
    __shared__ uint32_t s_plane[2][BAND_PIXELS];
    __shared__ float s_M[2][12];
    __shared__ float s_thr[TAUS];
    __shared__ int s_box[4];
    __shared__ uint32_t s_clipped[2];
    __shared__ int s_cnt[NWAVES][N_COUNTS];

    const uint32_t tid = threadIdx.x, T = p.n_taus;
    const size_t at = blockIdx.x, so = at / p.n_hypotheses, scene = so / p.n_objects;
    const ClassRange c = class_range(s, classes, class_stride, so);
    if (!c.ok) {      // the same for every lane
        write_all(out, p, at, __builtin_inff(), -1);
        return;
    }
    if (tid < 12u) s_M[0][tid] = gt[so * 12u + tid];
    else if (tid < 24u) s_M[1][tid - 12u] = est[at * 12u + (tid - 12u)];
    if (tid < TAUS) s_thr[tid] = tid < T ? vr::threshold(p, tid, (p.flags & SLHIP_VSD_NORMALIZED) ? s.diameter[c.cls] : 0.0f) : 0.0f;
    if (tid < 2u) {
        s_box[tid] = 0x7fffffff;
        s_box[2u + tid] = -1;
        s_clipped[tid] = 0u;
    }
    __syncthreads();
    if (!vr::pose_finite(s_M[0]) || !vr::pose_finite(s_M[1])) {
        write_all(out, p, at, __builtin_nanf(""), -1);
        return;
    }
    window_pass(s, c.begin, c.count, s_M[0], p, s_box, &s_clipped[0]);
    window_pass(s, c.begin, c.count, s_M[1], p, s_box, &s_clipped[1]);
    __syncthreads();
    const Window w = {s_box[0], s_box[2], s_box[1], s_box[3]};

    int n_vg = 0, n_ve = 0, n_in = 0, n_un = 0, n_cost[TAUS];
#pragma unroll
    for (uint32_t t = 0u; t < TAUS; ++t) n_cost[t] = 0;
    if (w.x0 <= w.x1) {
        const int ww = w.x1 - w.x0 + 1, rows = band_rows(w);
        const int step_y = (int)BLOCK / ww, step_x = (int)BLOCK - step_y * ww;
        for (int by = w.y0; by <= w.y1; by += rows) {
            const Window band = {w.x0, w.x1, by, min(by + rows - 1, w.y1)};
            const int n = ww * (band.y1 - band.y0 + 1);      // <= BAND_PIXELS
            for (int i = (int)tid; i < n; i += (int)BLOCK) s_plane[0][i] = s_plane[1][i] = vr::ABSENT;
            __syncthreads();
            raster_band(s, c.begin, c.count, s_M[0], p, band, s_plane[0]);
            raster_band(s, c.begin, c.count, s_M[1], p, band, s_plane[1]);
            __syncthreads();
            // (3) the band's pixels, 256 at a time
            int oy = (int)tid / ww, ox = (int)tid - oy * ww;
            for (int i = (int)tid; i < n; i += (int)BLOCK) {
                const uint32_t zg = s_plane[0][i], ze = s_plane[1][i];
                if (zg != vr::ABSENT || ze != vr::ABSENT) {
                    const int px = band.x0 + ox, py = band.y0 + oy;
                    const float td = depth[((scene * (size_t)p.H + (size_t)py) * (size_t)p.W + (size_t)px) * depth_stride];
                    const vr::Compared r = vr::compare(zg, ze, td, vr::ray_length(px, py, p.fx, p.fy, p.cx, p.cy), p.delta);
                    const bool inter = r.vg && r.ve;
                    n_vg += r.vg;
                    n_ve += r.ve;
                    n_in += inter;
                    n_un += r.vg || r.ve;
#pragma unroll
                    for (uint32_t t = 0u; t < TAUS; ++t)
                        if (t < T) n_cost[t] += inter && r.diff >= s_thr[t];
                }
                ox += step_x;
                oy += step_y;
                if (ox >= ww) {
                    ox -= ww;
                    ++oy;
                }
            }
            __syncthreads();      // the planes are read before the next band clears them
        }
    }
    // the counts of the 256 lanes: integers, so the order is free
    int mine[N_COUNTS];
    mine[0] = n_vg; mine[1] = n_ve; mine[2] = n_in; mine[3] = n_un;
#pragma unroll
    for (uint32_t t = 0u; t < TAUS; ++t) mine[4u + t] = n_cost[t];
#pragma unroll
    for (uint32_t k = 0u; k < N_COUNTS; ++k) {
        int v = mine[k];
#pragma unroll
        for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
        if (tid % vr::WAVE == 0u) s_cnt[tid / vr::WAVE][k] = v;
    }
    __syncthreads();
    if (tid < N_COUNTS) {
        int v = 0;
        for (uint32_t k = 0u; k < NWAVES; ++k) v += s_cnt[k][tid];
        s_cnt[0][tid] = v;      // lane tid alone reads and writes column tid
    }
    __syncthreads();
    if (tid < T) {
        if (p.outputs & SLHIP_VSD_OUT_VSD) out.vsd[at * T + tid] = vr::vsd_value(s_cnt[0][4u + tid], s_cnt[0][2], s_cnt[0][3]);
        if (p.outputs & SLHIP_VSD_OUT_COST) out.n_cost[at * T + tid] = s_cnt[0][4u + tid];
    }
    if (tid < 4u && (p.outputs & SLHIP_VSD_OUT_COUNTS)) out.counts[at * 4u + tid] = s_cnt[0][tid];
    if (tid == 0u && (p.outputs & SLHIP_VSD_OUT_FLAGS)) out.flags[at] = (s_clipped[0] | s_clipped[1]) ? SLHIP_VSD_CLIPPED : 0u;
}

// Block x = (scene * O + object) * Hy + hypothesis: one pose into its dense plane, every float written once.
__global__ __launch_bounds__(BLOCK) void k_pose_depth(Params p, Surface s, const int32_t* __restrict__ classes, uint32_t class_stride,
                                                      const float* __restrict__ poses, float* __restrict__ planes,
                                                      uint32_t* __restrict__ flags)
{
    __shared__ uint32_t s_plane[BAND_PIXELS];
    __shared__ float s_M[12];
    __shared__ int s_box[4];
    __shared__ uint32_t s_clipped;

    const uint32_t tid = threadIdx.x;
    const size_t at = blockIdx.x, so = at / p.n_hypotheses;
    float* plane = planes + at * (size_t)p.H * (size_t)p.W;
    const ClassRange c = class_range(s, classes, class_stride, so);
    if (tid < 12u) s_M[tid] = poses[at * 12u + tid];
    if (tid < 2u) {
        s_box[tid] = 0x7fffffff;
        s_box[2u + tid] = -1;
    }
    if (tid == 0u) s_clipped = 0u;
    __syncthreads();
    if (c.ok && vr::pose_finite(s_M)) window_pass(s, c.begin, c.count, s_M, p, s_box, &s_clipped);      // the same for every lane
    __syncthreads();
    const Window w = {s_box[0], s_box[2], s_box[1], s_box[3]};
    if (tid == 0u && flags) flags[at] = s_clipped ? SLHIP_VSD_CLIPPED : 0u;
    // zeros outside the window (everywhere when it is empty)
    for (int py = 0; py < p.H; ++py) {
        const bool row_in = w.x0 <= w.x1 && py >= w.y0 && py <= w.y1;
        for (int px = (int)tid; px < p.W; px += (int)BLOCK)
            if (!row_in || px < w.x0 || px > w.x1) plane[(size_t)py * (size_t)p.W + (size_t)px] = 0.0f;
    }
    if (w.x0 > w.x1) return;
    const int ww = w.x1 - w.x0 + 1, rows = band_rows(w);
    const int step_y = (int)BLOCK / ww, step_x = (int)BLOCK - step_y * ww;
    for (int by = w.y0; by <= w.y1; by += rows) {
        const Window band = {w.x0, w.x1, by, min(by + rows - 1, w.y1)};
        const int n = ww * (band.y1 - band.y0 + 1);
        for (int i = (int)tid; i < n; i += (int)BLOCK) s_plane[i] = vr::ABSENT;
        __syncthreads();
        raster_band(s, c.begin, c.count, s_M, p, band, s_plane);
        __syncthreads();
        int oy = (int)tid / ww, ox = (int)tid - oy * ww;
        for (int i = (int)tid; i < n; i += (int)BLOCK) {
            const uint32_t z = s_plane[i];
            plane[(size_t)(band.y0 + oy) * (size_t)p.W + (size_t)(band.x0 + ox)] = z == vr::ABSENT ? 0.0f : vr::bits_float(z);
            ox += step_x;
            oy += step_y;
            if (ox >= ww) {
                ox -= ww;
                ++oy;
            }
        }
        __syncthreads();
    }
}

int check_surface(const char* who, const Params* p, const Surface* s, bool need_diameter)
{
    if (!s || !s->vertices || !s->triangles || !s->tri_begin || !s->tri_count) {
        slhip::set_error("%s: null argument (the surface and its vertices, triangles, tri_begin and tri_count are required)", who);
        return -1;
    }
    if (need_diameter && (p->flags & SLHIP_VSD_NORMALIZED) && !s->diameter) {
        slhip::set_error("%s: normalised thresholds need the surface's diameter", who);
        return -1;
    }
    if ((uintptr_t)s->vertices & 15u) {
        slhip::set_error("%s: the surface's vertices must be 16-byte aligned", who);
        return -1;
    }
    if (((uintptr_t)s->triangles & 3u) || ((uintptr_t)s->tri_begin & 3u) || ((uintptr_t)s->tri_count & 3u) || ((uintptr_t)s->diameter & 3u)) {
        slhip::set_error("%s: the surface's triangles, tri_begin, tri_count and diameter must be 4-byte aligned", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_assets", s->n_assets, 1u, SLHIP_SYNTH_MAX_ASSETS)) return st;
    if (const int st = slhip::check_range(who, "n_vertices", s->n_vertices, 1u, 0x7fffffffu)) return st;
    return slhip::check_range(who, "n_triangles", s->n_triangles, 1u, 0x7fffffffu);      // (the kernels step through them by 256)
}

// what the four entries share
int check_call(const char* who, const Params* params, const Surface* s, const int32_t* classes, uint32_t class_stride,
               const float* poses, uint32_t n_scenes, bool vsd)
{
    if (const int st = slhip_pose_vsd_check_params(params)) return st;
    if (const int st = check_surface(who, params, s, vsd)) return st;
    if (!classes || !poses) {
        slhip::set_error("%s: null argument (classes and poses are required)", who);
        return -1;
    }
    if (class_stride == 0u) {
        slhip::set_error("%s: class_stride must be at least 1 (1: a plain tensor, 4: slhip_synth_object records)", who);
        return -1;
    }
    if (((uintptr_t)classes & 3u) || ((uintptr_t)poses & 3u)) {
        slhip::set_error("%s: classes and poses must be 4-byte aligned", who);
        return -1;
    }
    if ((uint64_t)n_scenes * params->n_objects * params->n_hypotheses > 0x7fffffffu) {
        slhip::set_error("%s: %u scenes x %u objects x %u hypotheses do not fit one launch", who, n_scenes, params->n_objects,
                         params->n_hypotheses);
        return -1;
    }
    return 0;
}

int check_vsd_call(const char* who, const Params* params, const Surface* s, const int32_t* classes, uint32_t class_stride,
                   const float* gt, const float* est, const float* depth, uint32_t depth_stride, uint32_t n_scenes, const Out* out)
{
    if (const int st = check_call(who, params, s, classes, class_stride, gt, n_scenes, true)) return st;
    if (!est || !depth || !out) {
        slhip::set_error("%s: null argument (estimates, the scene's depth and the output record are required)", who);
        return -1;
    }
    if (depth_stride == 0u) {
        slhip::set_error("%s: depth_stride must be at least 1 (4: the w of coord, 1: a dense plane)", who);
        return -1;
    }
    if (((uintptr_t)est & 3u) || ((uintptr_t)depth & 3u)) {
        slhip::set_error("%s: estimates and the scene's depth must be 4-byte aligned", who);
        return -1;
    }
    const slhip::OutputList outputs = {
        {SLHIP_VSD_OUT_VSD, out->vsd}, {SLHIP_VSD_OUT_COUNTS, out->counts}, {SLHIP_VSD_OUT_COST, out->n_cost}, {SLHIP_VSD_OUT_FLAGS, out->flags}};
    if (const int st = slhip::check_outputs_present(who, params->outputs, outputs)) return st;
    if (((uintptr_t)out->vsd & 3u) || ((uintptr_t)out->counts & 3u) || ((uintptr_t)out->n_cost & 3u) || ((uintptr_t)out->flags & 3u)) {
        slhip::set_error("%s: the outputs must be 4-byte aligned", who);
        return -1;
    }
    return 0;
}

int check_depth_call(const char* who, const Params* params, const Surface* s, const int32_t* classes, uint32_t class_stride,
                     const float* poses, uint32_t n_scenes, const float* depth, const uint32_t* flags)
{
    if (const int st = check_call(who, params, s, classes, class_stride, poses, n_scenes, false)) return st;
    if (!depth || ((uintptr_t)depth & 3u) || ((uintptr_t)flags & 3u)) {
        slhip::set_error("%s: the depth planes need a 4-byte aligned pointer (and so do the flags, when given)", who);
        return -1;
    }
    return 0;
}

// one pose of a class into a W x H plane of bits (ABSENT where nothing is covered); true: a triangle was clipped
bool raster_host(const Params& p, const Surface& s, uint32_t begin, uint32_t count, const float* M, std::vector<uint32_t>& plane)
{
    plane.assign((size_t)p.W * (size_t)p.H, vr::ABSENT);
    bool clipped = false;
    for (uint32_t i = 0u; i < count; ++i) {
        const uint32_t* ix = s.triangles + (size_t)(begin + i) * 3u;
        if (ix[0] >= s.n_vertices || ix[1] >= s.n_vertices || ix[2] >= s.n_vertices) continue;
        vr::Vertex v[3];
        for (int k = 0; k < 3; ++k) {
            const float* q = s.vertices + (size_t)ix[k] * 4u;
            v[k] = vr::project(M, q[0], q[1], q[2], p.fx, p.fy, p.cx, p.cy, p.z_near);
        }
        vr::Tri t;
        const int st = vr::setup(v[0], v[1], v[2], 0, p.W - 1, 0, p.H - 1, t);
        clipped = clipped || st == vr::TRI_CLIPPED;
        if (st != vr::TRI_OK) continue;
        for (int py = t.y0; py <= t.y1; ++py)
            for (int px = t.x0; px <= t.x1; ++px) {
                uint32_t bits;
                uint32_t& at = plane[(size_t)py * (size_t)p.W + (size_t)px];
                if (vr::pixel_depth<long long>(t, px, py, &bits) && bits < at) at = bits;
            }
    }
    return clipped;
}

// optional HIP-event timing (tools/time_pose_vsd.py): events round the last slhip_pose_vsd and the last slhip_pose_depth
slhip::StepTimer<2> g_timer;

}  // namespace

extern "C" int slhip_pose_vsd_band_pixels(void) { return (int)BAND_PIXELS; }

extern "C" int slhip_pose_vsd_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_pose_vsd_timings(float ms_out[2]) { return g_timer.read_for("slhip_pose_vsd_timings", ms_out); }

extern "C" int slhip_pose_vsd_check_params(const slhip_pose_vsd_params* p)
{
    static const char* who = "slhip_pose_vsd";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_intrinsics(who, p->fx, p->fy, p->cx, p->cy)) return st;
    if (!slhip::picture_fits(p->W, p->H, 32768, ~0ull) || (uint32_t)p->W > SLHIP_VSD_WIDTH_MAX) {
        slhip::set_error("%s: bad picture size %d x %d (W 1..%u, H 1..32768)", who, p->W, p->H, SLHIP_VSD_WIDTH_MAX);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_objects", p->n_objects, 1u, SLHIP_SYNTH_MAX_OBJECTS)) return st;
    if (const int st = slhip::check_range(who, "n_hypotheses", p->n_hypotheses, 1u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_taus", p->n_taus, 1u, SLHIP_VSD_TAUS_MAX)) return st;
    if (!(p->delta >= 0.0f) || !slhip::is_finite(p->delta)) {
        slhip::set_error("%s: delta %g must be finite and not negative", who, (double)p->delta);
        return -1;
    }
    if (!(p->z_near > 0.0f) || !slhip::is_finite(p->z_near)) {
        slhip::set_error("%s: z_near %g must be finite and positive", who, (double)p->z_near);
        return -1;
    }
    if (p->flags & ~SLHIP_VSD_NORMALIZED) {
        slhip::set_error("%s: flags 0x%x: only SLHIP_VSD_NORMALIZED (1) is known", who, p->flags);
        return -1;
    }
    const uint32_t all = SLHIP_VSD_OUT_VSD | SLHIP_VSD_OUT_COUNTS | SLHIP_VSD_OUT_COST | SLHIP_VSD_OUT_FLAGS;
    if (p->outputs == 0u || (p->outputs & ~all)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of vsd 1, counts 2, n_cost 4, flags 8 and nothing else", who, p->outputs);
        return -1;
    }
    for (uint32_t t = 0u; t < p->n_taus; ++t)
        if (!(p->taus[t] >= 0.0f) || !slhip::is_finite(p->taus[t])) {
            slhip::set_error("%s: taus[%u] %g must be finite and not negative", who, t, (double)p->taus[t]);
            return -1;
        }
    return 0;
}

extern "C" int slhip_pose_vsd(const slhip_pose_vsd_params* params, const slhip_pose_surface* surface, const int32_t* d_classes,
                              uint32_t class_stride, const float* d_gt, const float* d_est, const float* d_test_depth,
                              uint32_t depth_stride, uint32_t n_scenes, const slhip_pose_vsd_out* out, void* stream_)
{
    static const char* who = "slhip_pose_vsd";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_vsd_call(who, params, surface, d_classes, class_stride, d_gt, d_est, d_test_depth, depth_stride, n_scenes, out))
        return st;
    if (n_scenes == 0u) return 0;
    const uint32_t blocks = n_scenes * params->n_objects * params->n_hypotheses;
    if (const int st = g_timer.begin(0, stream)) return st;
    k_pose_vsd<<<blocks, BLOCK, 0, stream>>>(*params, *surface, d_classes, class_stride, d_gt, d_est, d_test_depth, depth_stride, *out);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

extern "C" int slhip_pose_depth(const slhip_pose_vsd_params* params, const slhip_pose_surface* surface, const int32_t* d_classes,
                                uint32_t class_stride, const float* d_poses, uint32_t n_scenes, float* d_depth, uint32_t* d_flags,
                                void* stream_)
{
    static const char* who = "slhip_pose_depth";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_depth_call(who, params, surface, d_classes, class_stride, d_poses, n_scenes, d_depth, d_flags)) return st;
    if (n_scenes == 0u) return 0;
    const uint32_t blocks = n_scenes * params->n_objects * params->n_hypotheses;
    if (const int st = g_timer.begin(1, stream)) return st;
    k_pose_depth<<<blocks, BLOCK, 0, stream>>>(*params, *surface, d_classes, class_stride, d_poses, d_depth, d_flags);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(1, stream);
}

extern "C" int slhip_pose_vsd_host(const slhip_pose_vsd_params* params, const slhip_pose_surface* surface, const int32_t* h_classes,
                                   uint32_t class_stride, const float* h_gt, const float* h_est, const float* h_test_depth,
                                   uint32_t depth_stride, uint32_t n_scenes, const slhip_pose_vsd_out* out)
{
    static const char* who = "slhip_pose_vsd_host";
    if (const int st = check_vsd_call(who, params, surface, h_classes, class_stride, h_gt, h_est, h_test_depth, depth_stride, n_scenes, out))
        return st;
    const Params& p = *params;
    const Surface& s = *surface;
    const uint32_t Hy = p.n_hypotheses, T = p.n_taus, mask = p.outputs;
    auto write_all = [&](size_t at, float v, int n) {
        for (uint32_t t = 0u; t < T; ++t) {
            if (mask & SLHIP_VSD_OUT_VSD) out->vsd[at * T + t] = v;
            if (mask & SLHIP_VSD_OUT_COST) out->n_cost[at * T + t] = n;
        }
        if (mask & SLHIP_VSD_OUT_COUNTS)
            for (int k = 0; k < 4; ++k) out->counts[at * 4u + k] = n;
        if (mask & SLHIP_VSD_OUT_FLAGS) out->flags[at] = 0u;
    };
    std::vector<uint32_t> plane_g, plane_e;
    for (size_t so = 0; so < (size_t)n_scenes * p.n_objects; ++so) {
        const ClassRange c = class_range(s, h_classes, class_stride, so);
        const size_t scene = so / p.n_objects;
        const float* g = h_gt + so * 12u;
        bool g_drawn = false, g_clipped = false;
        for (uint32_t h = 0u; h < Hy; ++h) {
            const size_t at = so * Hy + h;
            const float* e = h_est + at * 12u;
            if (!c.ok) {
                write_all(at, __builtin_inff(), -1);
                continue;
            }
            if (!vr::pose_finite(g) || !vr::pose_finite(e)) {
                write_all(at, __builtin_nanf(""), -1);
                continue;
            }
            if (!g_drawn) {
                g_clipped = raster_host(p, s, c.begin, c.count, g, plane_g);
                g_drawn = true;
            }
            const bool e_clipped = raster_host(p, s, c.begin, c.count, e, plane_e);
            int32_t n[4] = {0, 0, 0, 0}, n_cost[TAUS] = {};
            float thr[TAUS] = {};
            for (uint32_t t = 0u; t < T; ++t) thr[t] = vr::threshold(p, t, (p.flags & SLHIP_VSD_NORMALIZED) ? s.diameter[c.cls] : 0.0f);
            for (int py = 0; py < p.H; ++py)
                for (int px = 0; px < p.W; ++px) {
                    const size_t i = (size_t)py * (size_t)p.W + (size_t)px;
                    if (plane_g[i] == vr::ABSENT && plane_e[i] == vr::ABSENT) continue;
                    const float td = h_test_depth[(scene * (size_t)p.H * (size_t)p.W + i) * depth_stride];
                    const vr::Compared r = vr::compare(plane_g[i], plane_e[i], td, vr::ray_length(px, py, p.fx, p.fy, p.cx, p.cy), p.delta);
                    const bool inter = r.vg && r.ve;
                    n[0] += r.vg;
                    n[1] += r.ve;
                    n[2] += inter;
                    n[3] += r.vg || r.ve;
                    for (uint32_t t = 0u; t < T; ++t) n_cost[t] += inter && r.diff >= thr[t];
                }
            for (uint32_t t = 0u; t < T; ++t) {
                if (mask & SLHIP_VSD_OUT_VSD) out->vsd[at * T + t] = vr::vsd_value(n_cost[t], n[2], n[3]);
                if (mask & SLHIP_VSD_OUT_COST) out->n_cost[at * T + t] = n_cost[t];
            }
            if (mask & SLHIP_VSD_OUT_COUNTS)
                for (int k = 0; k < 4; ++k) out->counts[at * 4u + k] = n[k];
            if (mask & SLHIP_VSD_OUT_FLAGS) out->flags[at] = (g_clipped || e_clipped) ? SLHIP_VSD_CLIPPED : 0u;
        }
    }
    return 0;
}

extern "C" int slhip_pose_depth_host(const slhip_pose_vsd_params* params, const slhip_pose_surface* surface, const int32_t* h_classes,
                                     uint32_t class_stride, const float* h_poses, uint32_t n_scenes, float* h_depth, uint32_t* h_flags)
{
    static const char* who = "slhip_pose_depth_host";
    if (const int st = check_depth_call(who, params, surface, h_classes, class_stride, h_poses, n_scenes, h_depth, h_flags)) return st;
    const Params& p = *params;
    const Surface& s = *surface;
    const size_t pixels = (size_t)p.W * (size_t)p.H;
    std::vector<uint32_t> plane;
    for (size_t at = 0; at < (size_t)n_scenes * p.n_objects * p.n_hypotheses; ++at) {
        const ClassRange c = class_range(s, h_classes, class_stride, at / p.n_hypotheses);
        const float* M = h_poses + at * 12u;
        float* dst = h_depth + at * pixels;
        bool clipped = false;
        if (c.ok && vr::pose_finite(M)) {
            clipped = raster_host(p, s, c.begin, c.count, M, plane);
            for (size_t i = 0; i < pixels; ++i) dst[i] = plane[i] == vr::ABSENT ? 0.0f : vr::bits_float(plane[i]);
        } else {
            std::fill(dst, dst + pixels, 0.0f);
        }
        if (h_flags) h_flags[at] = clipped ? SLHIP_VSD_CLIPPED : 0u;
    }
    return 0;
}
