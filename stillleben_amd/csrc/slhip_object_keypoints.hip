// Object keypoints (this project's addition, no counterpart in the reference): the targets of keypoint-voting pose networks
// (PVN3D, FFB6D, PVNet) from what a batch already keeps in HBM -- a bank of 3D keypoints per mesh class by farthest point
// sampling, their projection under object_to_camera, and per pixel the vectors towards the projected keypoints of the pixel's
// object.  include/slhip.h "Object keypoints" and DESIGN.md "Object keypoints" are the contract; all arithmetic is float32, one
// rounded operation at a time (-ffp-contract=off), through slhip_keypoint_rules.h on host and device alike, so
// tests/object_keypoints_ref.py restates it and every output is bit-exact against it.
//   fps                  k_fps of slhip_fps.hip (slhip::fps_device)
//   k_keypoints_project  one thread per (scene, object, keypoint)
//   k_keypoints_field    a pure write stream: a scene's uv and flags in LDS, (pixel, keypoint) pairs flattened across the lanes,
//                        two pairs = one 16-byte store per lane when a scene's pairs are even (8 bytes otherwise)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fps.h"
#include "slhip_keypoint_rules.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_object_keypoint_params) == 48, "slhip_object_keypoint_params layout");
static_assert(sizeof(slhip_synth_object) == 16, "slhip_synth_object layout");

using Params = slhip_object_keypoint_params;
namespace kp = slhip_kp;

constexpr uint32_t FIELD_BLOCK = 256u;
constexpr uint32_t FIELD_TRIPS = 4u;        // units a lane of k_keypoints_field has in flight
constexpr uint32_t MAX_KP = SLHIP_KEYPOINTS_MAX;
constexpr uint32_t MAX_SLOTS = SLHIP_SYNTH_MAX_OBJECTS * MAX_KP;      // (object, keypoint) of one scene

__global__ __launch_bounds__(256) void k_keypoints_project(Params p, const float4* __restrict__ bank, uint32_t n_assets,
                                                           const slhip_synth_object* __restrict__ objects,
                                                           const float* __restrict__ o2c, uint32_t n_scenes,
                                                           const float* __restrict__ depth, uint32_t depth_stride,
                                                           float4* __restrict__ camera, float2* __restrict__ uv,
                                                           uint8_t* __restrict__ flags)
{
    const uint32_t Kp = p.n_keypoints;
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)n_scenes * p.n_objects * Kp) return;
    const uint32_t k = (uint32_t)(t % Kp);
    const uint64_t so = t / Kp;      // scene * n_objects + object
    const uint32_t scene = (uint32_t)(so / p.n_objects);
    const uint32_t asset = objects[so].asset;
    float4 cam = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float2 at = make_float2(0.0f, 0.0f);
    uint32_t f = 0u;
    if (asset < n_assets) {
        const float4 q = bank[(size_t)asset * Kp + k];
        const kp::Projected r = kp::project(o2c + so * 12u, q.x, q.y, q.z, p.fx, p.fy, p.cx, p.cy, p.W, p.H);
        f = r.flags;
        if (f & SLHIP_KEYPOINT_IN_FRONT) {
            cam = make_float4(r.X, r.Y, r.Z, 1.0f);
            at = make_float2(r.u, r.v);
        }
        if (depth && (f & SLHIP_KEYPOINT_INSIDE)) {      // inside: 0 <= floor(u) < W and 0 <= floor(v) < H
            const size_t px = ((size_t)scene * (size_t)p.H + (size_t)(int)floorf(r.v)) * (size_t)p.W + (size_t)(int)floorf(r.u);
            if (kp::unoccluded(r.Z, depth[px * depth_stride], p.depth_tol)) f |= SLHIP_KEYPOINT_UNOCCLUDED;
        }
    }
    camera[t] = cam;
    uv[t] = at;
    flags[t] = (uint8_t)f;
}

// the two floats of (pixel, keypoint): sqrtf and / are the correctly rounded ones (hipcc's default for float32 in HIP code; the
// __fsqrt_rn of this toolchain's headers is the native, approximate instruction unless OCML_BASIC_ROUNDED_OPERATIONS is set)
__device__ __forceinline__ float2 field_vector(float2 at, uint32_t x, uint32_t y, uint32_t mode)
{
    const float dx = at.x - ((float)x + 0.5f), dy = at.y - ((float)y + 0.5f);
    if (mode == SLHIP_KEYPOINT_FIELD_OFFSET) return make_float2(dx, dy);
    const float l = sqrtf(dx * dx + dy * dy);
    if (l == 0.0f) return make_float2(0.0f, 0.0f);
    return make_float2(dx / l, dy / l);
}

// Blocks (x, y): scene first + y of the picture, scene y of the output; the blocks of a scene stride over its H * W * Kp pairs,
// VEC pairs per lane and unit, so a wave stores 64 * VEC * 8 contiguous bytes per unit.  A lane takes FIELD_TRIPS units per trip
// and reads the instances of all of them before it computes and stores any: a trip's loads wait for the stores of the trip
// before (one counter orders both), so with one unit per trip every store's round trip would stand between two loads -- measured,
// that form wrote 3.1 TB/s.  pairs < 2^31 (checked by the entry), and with VEC = 2 it is even, so no lane's pairs cross into
// the next scene.  Every pair is written exactly once, nothing else is.
struct FieldPair {
    uint32_t x, y, k;
    int i;
};

template <int VEC>
__global__ __launch_bounds__(FIELD_BLOCK) void k_keypoints_field(Params p, const int16_t* __restrict__ instance,
                                                                 const float2* __restrict__ uv, const uint8_t* __restrict__ flags,
                                                                 uint32_t first, float2* __restrict__ out)
{
    __shared__ float2 s_uv[MAX_SLOTS];
    __shared__ uint8_t s_flags[MAX_SLOTS];
    const uint32_t Kp = p.n_keypoints, W = (uint32_t)p.W, n_slots = p.n_objects * Kp;
    const uint32_t pixels = W * (uint32_t)p.H, pairs = pixels * Kp;
    const uint32_t scene = first + blockIdx.y;
    for (uint32_t i = threadIdx.x; i < n_slots; i += FIELD_BLOCK) {
        s_uv[i] = uv[(size_t)scene * n_slots + i];
        s_flags[i] = flags[(size_t)scene * n_slots + i];
    }
    __syncthreads();
    const int16_t* inst = instance + (size_t)scene * pixels;
    float2* dst = out + (size_t)blockIdx.y * pairs;
    const uint32_t units = pairs / VEC, stride = gridDim.x * (FIELD_BLOCK * FIELD_TRIPS);
    for (uint32_t e0 = blockIdx.x * (FIELD_BLOCK * FIELD_TRIPS) + threadIdx.x; e0 < units; e0 += stride) {
        FieldPair q[FIELD_TRIPS][VEC];
#pragma unroll
        for (uint32_t t = 0u; t < FIELD_TRIPS; ++t) {      // straight-line: a unit past the end reads the last unit's pixels
            const uint32_t g = min(e0 + t * FIELD_BLOCK, units - 1u) * VEC;
            uint32_t pixel = g / Kp, k = g - pixel * Kp;
            uint32_t y = pixel / W, x = pixel - y * W;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                q[t][j].x = x; q[t][j].y = y; q[t][j].k = k;
                q[t][j].i = inst[pixel];      // pixel < pixels: pair g + j < pairs
                const bool next = k + 1u == Kp, wrap = next && x + 1u == W;      // the next pair is the next pixel's first
                k = next ? 0u : k + 1u;
                pixel += next ? 1u : 0u;
                x = wrap ? 0u : x + (next ? 1u : 0u);
                y += wrap ? 1u : 0u;
            }
        }
#pragma unroll
        for (uint32_t t = 0u; t < FIELD_TRIPS; ++t) {
            const uint32_t e = e0 + t * FIELD_BLOCK;
            if (e >= units) break;
            float2 r[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                const int i = q[t][j].i;
                r[j] = make_float2(0.0f, 0.0f);
                if (i >= 1 && (uint32_t)i <= p.n_objects) {
                    const uint32_t slot = (uint32_t)(i - 1) * Kp + q[t][j].k;
                    if (s_flags[slot] & SLHIP_KEYPOINT_IN_FRONT) r[j] = field_vector(s_uv[slot], q[t][j].x, q[t][j].y, p.mode);
                }
            }
            if constexpr (VEC == 2)
                reinterpret_cast<float4*>(dst)[e] = make_float4(r[0].x, r[0].y, r[1].x, r[1].y);
            else
                dst[e] = r[0];
        }
    }
}

// optional HIP-event timing (tools/time_object_keypoints.py): events round the last call's kernel of each of the three steps
slhip::StepTimer<3> g_timer;

}  // namespace

extern "C" int slhip_object_keypoints_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_object_keypoints_timings(float ms_out[3]) { return g_timer.read_for("slhip_object_keypoints_timings", ms_out); }

extern "C" int slhip_object_keypoints_check_params(const slhip_object_keypoint_params* p)
{
    static const char* who = "slhip_object_keypoints";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_intrinsics(who, p->fx, p->fy, p->cx, p->cy)) return st;
    if (const int st = slhip::check_picture_sides(who, p->W, p->H)) return st;
    if (const int st = slhip::check_range(who, "n_keypoints", p->n_keypoints, 1u, MAX_KP)) return st;
    if (const int st = slhip::check_range(who, "n_objects", p->n_objects, 1u, SLHIP_SYNTH_MAX_OBJECTS)) return st;
    if (p->mode != SLHIP_KEYPOINT_FIELD_OFFSET && p->mode != SLHIP_KEYPOINT_FIELD_UNIT) {
        slhip::set_error("%s: mode %u must be offset 0 or unit 1", who, p->mode);
        return -1;
    }
    if (!(p->depth_tol >= 0.0f) || !slhip::is_finite(p->depth_tol)) {
        slhip::set_error("%s: depth_tol %g must be finite and >= 0 (metres)", who, (double)p->depth_tol);
        return -1;
    }
    return 0;
}

extern "C" int slhip_object_keypoints_fps_bytes(uint32_t n_assets, uint64_t max_verts, uint64_t* bytes)
{
    if (!bytes) {
        slhip::set_error("slhip_object_keypoints_fps_bytes: null argument");
        return -1;
    }
    *bytes = slhip::fps_scratch_bytes(n_assets, max_verts);
    return 0;
}

extern "C" int slhip_object_keypoints_fps(const float* d_pos, uint64_t n_vertices, const slhip_asset* d_assets, uint32_t n_assets,
                                          const slhip_draw* d_templates, uint32_t n_templates, uint32_t n_fps, uint64_t max_verts,
                                          void* d_scratch, float* d_keypoints, int32_t* d_vertex, void* stream_)
{
    static const char* who = "slhip_object_keypoints_fps";
    hipStream_t stream = (hipStream_t)stream_;
    // (the checks come first: a refused call records no event)
    if (const int st = slhip::check_fps(who, "n_fps", MAX_KP, n_assets, n_fps)) return st;
    if (const int st = g_timer.begin(0, stream)) return st;
    if (const int st = slhip::fps_device(who, "n_fps", MAX_KP, d_pos, n_vertices, d_assets, n_assets, d_templates, n_templates, n_fps,
                                         max_verts, d_scratch, d_keypoints, d_vertex, stream))
        return st;
    return g_timer.end(0, stream);
}

extern "C" int slhip_object_keypoints_fps_host(const float* h_pos, uint64_t n_vertices, const slhip_asset* h_assets,
                                               uint32_t n_assets, const slhip_draw* h_templates, uint32_t n_templates,
                                               uint32_t n_fps, float* h_keypoints, int32_t* h_vertex)
{
    return slhip::fps_host("slhip_object_keypoints_fps_host", "n_fps", MAX_KP, h_pos, n_vertices, h_assets, n_assets, h_templates,
                           n_templates, n_fps, h_keypoints, h_vertex);
}

extern "C" int slhip_object_keypoints_project(const slhip_object_keypoint_params* params, const float* d_bank, uint32_t n_assets,
                                              const slhip_synth_object* d_objects, const float* d_object_to_camera,
                                              uint32_t n_scenes, const float* d_depth, uint32_t depth_stride, float* d_camera,
                                              float* d_uv, uint8_t* d_flags, void* stream_)
{
    static const char* who = "slhip_object_keypoints_project";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = slhip_object_keypoints_check_params(params)) return st;
    if (n_scenes == 0u) return 0;
    if (!d_bank || !d_objects || !d_object_to_camera || !d_camera || !d_uv || !d_flags) {
        slhip::set_error("%s: null argument (bank, objects, object_to_camera and the three outputs are required)", who);
        return -1;
    }
    if (n_assets == 0u) {
        slhip::set_error("%s: n_assets must be at least 1", who);
        return -1;
    }
    if (d_depth && depth_stride == 0u) {
        slhip::set_error("%s: a depth plane needs a depth_stride of at least 1 (4: the w of d_coord, 1: a plane)", who);
        return -1;
    }
    if (d_depth && (uint64_t)params->W * (uint64_t)params->H > 0x7fffffffu) {
        slhip::set_error("%s: a depth plane of %d x %d has 2^31 pixels or more", who, params->W, params->H);
        return -1;
    }
    const uint64_t n = (uint64_t)n_scenes * params->n_objects * params->n_keypoints;
    if ((n + 255u) / 256u > 0x7fffffffu) {
        slhip::set_error("%s: %llu keypoints do not fit one launch", who, (unsigned long long)n);
        return -1;
    }
    if (const int st = g_timer.begin(1, stream)) return st;
    k_keypoints_project<<<(uint32_t)((n + 255u) / 256u), 256, 0, stream>>>(
        *params, reinterpret_cast<const float4*>(d_bank), n_assets, d_objects, d_object_to_camera, n_scenes, d_depth, depth_stride,
        reinterpret_cast<float4*>(d_camera), reinterpret_cast<float2*>(d_uv), d_flags);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(1, stream);
}

extern "C" int slhip_object_keypoints_field(const slhip_object_keypoint_params* params, const int16_t* d_instance,
                                            const float* d_uv, const uint8_t* d_flags, uint32_t n_scenes, uint32_t first,
                                            uint32_t count, float* d_out, void* stream_)
{
    static const char* who = "slhip_object_keypoints_field";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = slhip_object_keypoints_check_params(params)) return st;
    if ((uint64_t)first + count > n_scenes) {
        slhip::set_error("%s: scenes [%u, %u + %u) reach past the %u scenes of the picture", who, first, first, count, n_scenes);
        return -1;
    }
    if (count == 0u) return 0;
    if (!d_instance || !d_uv || !d_flags || !d_out) {
        slhip::set_error("%s: null argument (instance, uv, flags and the output are required)", who);
        return -1;
    }
    if (((uintptr_t)d_out & 7u) || ((uintptr_t)d_uv & 7u)) {
        slhip::set_error("%s: uv and the output must be 8-byte aligned", who);
        return -1;
    }
    const uint64_t pairs = (uint64_t)params->W * (uint64_t)params->H * params->n_keypoints;
    if (pairs > 0x7fffffffu) {
        slhip::set_error("%s: %d x %d x %u keypoints: a scene's field must stay below 2^31 (pixel, keypoint) pairs", who, params->W,
                         params->H, params->n_keypoints);
        return -1;
    }
    if (count > 65535u) {
        slhip::set_error("%s: at most 65535 scenes per call (%u asked for)", who, count);
        return -1;
    }
    const bool wide = (pairs & 1u) == 0u && ((uintptr_t)d_out & 15u) == 0u;
    const uint64_t units = wide ? pairs / 2u : pairs;
    // enough blocks to fill the device from a short range, few enough that the LDS fill is noise against a block's stores
    const uint64_t want = (units + FIELD_BLOCK * FIELD_TRIPS * 2u - 1u) / (FIELD_BLOCK * FIELD_TRIPS * 2u);
    const uint32_t per_scene = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(want, std::max<uint32_t>(32u, 4096u / count)));
    const dim3 grid(per_scene, count);
    const float2* uv = reinterpret_cast<const float2*>(d_uv);
    if (const int st = g_timer.begin(2, stream)) return st;
    if (wide)
        k_keypoints_field<2><<<grid, FIELD_BLOCK, 0, stream>>>(*params, d_instance, uv, d_flags, first, reinterpret_cast<float2*>(d_out));
    else
        k_keypoints_field<1><<<grid, FIELD_BLOCK, 0, stream>>>(*params, d_instance, uv, d_flags, first, reinterpret_cast<float2*>(d_out));
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(2, stream);
}
