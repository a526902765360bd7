// Render flow (this project's addition, no counterpart in the reference): where every pixel of one render lands in another
// render of the same scene -- optical flow, scene flow and an occlusion flag per pixel, counts per instance slot -- from what a
// batch already keeps in HBM: the depth in coord.w, the instance plane and the rigid motion of every slot between the two
// camera frames.  include/slhip.h "Render flow" and DESIGN.md "Render flow" are the contract; all arithmetic is float32, one
// rounded operation at a time (-ffp-contract=off), through slhip_flow_rules.h on host and device alike, so
// slhip_render_flow_host gives the kernel's outputs bit for bit and tests/render_flow_ref.py restates them.
//   k_render_flow   one lane per pixel, a workgroup of 256 lanes over 256 consecutive pixels of one scene: depth, instance and
//                   every output coalesce, the footprint reads of picture b are the only gathers.  The scene's motion table
//                   goes into LDS once per workgroup (the instance diverges across a wave); the counts of the workgroup are
//                   LDS atomics, flushed with one global atomic per non-zero entry
//   k_flow_motion   one lane per rigid frame
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_flow_rules.h"

namespace {

static_assert(sizeof(slhip_render_flow_params) == 48, "slhip_render_flow_params layout");

using Params = slhip_render_flow_params;
namespace fl = slhip_flow;

constexpr uint32_t BLOCK = 256u;
constexpr uint32_t MAX_SLOTS = SLHIP_FLOW_SLOTS_MAX;
constexpr uint32_t OUT_ALL = SLHIP_FLOW_OUT_FLOW | SLHIP_FLOW_OUT_SCENE | SLHIP_FLOW_OUT_FLAGS | SLHIP_FLOW_OUT_COUNTS;

struct F3 {
    float x, y, z;
};

// Blocks (x, y): 256 consecutive pixels of scene y.  LDS: 12 KB of motion table and 4 KB of counts whatever n_slots is.
// A wave whose live lanes all carry one instance -- nearly every wave of a render -- adds its four counts by ballot, one lane and
// four LDS atomics; a mixed wave adds lane by lane.  Integer sums: the same counts either way.
__global__ __launch_bounds__(BLOCK) void k_render_flow(Params p, const float* __restrict__ depth_a, uint32_t stride_a,
                                                       const uint16_t* __restrict__ inst_a, const float* __restrict__ motion,
                                                       const float* __restrict__ depth_b, uint32_t stride_b,
                                                       const uint16_t* __restrict__ inst_b, float2* __restrict__ flow,
                                                       F3* __restrict__ scene_flow, uint8_t* __restrict__ flags,
                                                       int32_t* __restrict__ counts)
{
    __shared__ float s_motion[MAX_SLOTS * 12u];
    __shared__ int32_t s_counts[MAX_SLOTS * 4u];
    const uint32_t n_slots = p.n_slots, W = (uint32_t)p.W, pixels = W * (uint32_t)p.H;      // pixels <= 2^30
    const uint32_t scene = blockIdx.y;
    const bool count = (p.outputs & SLHIP_FLOW_OUT_COUNTS) != 0u;
    for (uint32_t k = threadIdx.x; k < n_slots * 12u; k += BLOCK) s_motion[k] = motion[(size_t)scene * n_slots * 12u + k];
    if (count)
        for (uint32_t k = threadIdx.x; k < n_slots * 4u; k += BLOCK) s_counts[k] = 0;
    __syncthreads();

    const uint32_t pix = blockIdx.x * BLOCK + threadIdx.x;
    const bool live = pix < pixels;
    const size_t at = (size_t)scene * pixels + (live ? pix : 0u);      // a lane past the end reads the scene's pixel 0, stores nothing
    const float z = depth_a[at * stride_a];
    const uint32_t i = inst_a[at];
    const uint32_t y = pix / W, x = pix - y * W;
    const size_t base_b = (size_t)scene * pixels;
    const fl::Pixel r = fl::pixel(p, (int)x, (int)y, z, i, s_motion, depth_b ? depth_b + base_b * stride_b : nullptr, stride_b,
                                  inst_b ? inst_b + base_b : nullptr);
    if (live) {
        if (p.outputs & SLHIP_FLOW_OUT_FLOW) flow[at] = make_float2(r.u, r.v);
        if (p.outputs & SLHIP_FLOW_OUT_SCENE) {
            F3 s;
            s.x = r.x; s.y = r.y; s.z = r.z;
            scene_flow[at] = s;
        }
        if (p.outputs & SLHIP_FLOW_OUT_FLAGS) flags[at] = (uint8_t)r.flags;
    }
    if (count) {
        const bool mine = live && i < n_slots;
        const unsigned long long have = __ballot(mine);
        if (have) {      // wave-uniform
            const uint32_t lead = (uint32_t)__builtin_ctzll(have);
            const uint32_t i0 = (uint32_t)__shfl((int)i, (int)lead);
            if (__ballot(mine && i != i0) == 0ull) {
                const unsigned long long valid = __ballot(mine && (r.flags & SLHIP_FLOW_VALID));
                const unsigned long long inside = __ballot(mine && (r.flags & SLHIP_FLOW_INSIDE));
                const unsigned long long visible = __ballot(mine && (r.flags & SLHIP_FLOW_VISIBLE));
                if ((threadIdx.x & 63u) == lead) {
                    atomicAdd(&s_counts[i0 * 4u], __popcll(have));
                    if (valid) atomicAdd(&s_counts[i0 * 4u + 1u], __popcll(valid));
                    if (inside) atomicAdd(&s_counts[i0 * 4u + 2u], __popcll(inside));
                    if (visible) atomicAdd(&s_counts[i0 * 4u + 3u], __popcll(visible));
                }
            } else if (mine) {
                atomicAdd(&s_counts[i * 4u], 1);
                if (r.flags & SLHIP_FLOW_VALID) atomicAdd(&s_counts[i * 4u + 1u], 1);
                if (r.flags & SLHIP_FLOW_INSIDE) atomicAdd(&s_counts[i * 4u + 2u], 1);
                if (r.flags & SLHIP_FLOW_VISIBLE) atomicAdd(&s_counts[i * 4u + 3u], 1);
            }
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < n_slots * 4u; k += BLOCK) {
            const int32_t v = s_counts[k];
            if (v) atomicAdd(&counts[(size_t)scene * n_slots * 4u + k], v);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_flow_motion(const float* __restrict__ from, const float* __restrict__ to, uint32_t n,
                                                       float* __restrict__ out)
{
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n) return;
    float f[12], g[12], m[12];
    for (int k = 0; k < 12; ++k) {
        f[k] = from[(size_t)t * 12u + k];
        g[k] = to[(size_t)t * 12u + k];
    }
    fl::motion(f, g, m);
    for (int k = 0; k < 12; ++k) out[(size_t)t * 12u + k] = m[k];
}

// the checks that slhip_render_flow and slhip_render_flow_host share
int check_call(const char* who, const Params* params, const float* depth_a, uint32_t stride_a, const uint16_t* inst_a,
               const float* motion, const float* depth_b, uint32_t stride_b, const uint16_t* inst_b, uint32_t B, const float* flow,
               const float* scene_flow, const uint8_t* flags, const int32_t* counts)
{
    if (!depth_a || !inst_a || !motion) {
        slhip::set_error("%s: null argument (the depth and the instances of picture a and the motion table are required)", who);
        return -1;
    }
    if (stride_a == 0u || (depth_b && stride_b == 0u)) {
        slhip::set_error("%s: a depth plane needs a stride of at least 1 (4: the w of a coord target, 1: a plane)", who);
        return -1;
    }
    if (B > 65535u) {
        slhip::set_error("%s: at most 65535 scenes per call (%u asked for)", who, B);
        return -1;
    }
    const slhip::OutputList outputs = {{SLHIP_FLOW_OUT_FLOW, flow}, {SLHIP_FLOW_OUT_SCENE, scene_flow}, {SLHIP_FLOW_OUT_FLAGS, flags},
                                       {SLHIP_FLOW_OUT_COUNTS, counts}};
    if (const int st = slhip::check_outputs_present(who, params->outputs, outputs)) return st;
    if (((uintptr_t)depth_a & 3u) || ((uintptr_t)depth_b & 3u) || ((uintptr_t)motion & 3u) || (((uintptr_t)inst_a | (uintptr_t)inst_b) & 1u) ||
        ((params->outputs & SLHIP_FLOW_OUT_FLOW) && ((uintptr_t)flow & 7u)) ||
        ((params->outputs & SLHIP_FLOW_OUT_SCENE) && ((uintptr_t)scene_flow & 3u)) ||
        ((params->outputs & SLHIP_FLOW_OUT_COUNTS) && ((uintptr_t)counts & 3u))) {
        slhip::set_error("%s: the depths, the motion table, scene_flow and counts must be 4-byte aligned, flow 8-byte, instances 2-byte", who);
        return -1;
    }
    return 0;
}

}  // namespace

extern "C" int slhip_render_flow_check_params(const slhip_render_flow_params* p)
{
    static const char* who = "slhip_render_flow";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_intrinsics(who, p->fx, p->fy, p->cx, p->cy)) return st;
    if (const int st = slhip::check_picture_sides(who, p->W, p->H)) return st;
    if (const int st = slhip::check_range(who, "n_slots", p->n_slots, 1u, MAX_SLOTS)) return st;
    if (!(p->max_depth > 0.0f)) {
        slhip::set_error("%s: max_depth %g must be > 0 (+inf: no limit)", who, (double)p->max_depth);
        return -1;
    }
    if (!(p->depth_tol >= 0.0f) || !slhip::is_finite(p->depth_tol) || !(p->depth_rel >= 0.0f) || !slhip::is_finite(p->depth_rel)) {
        slhip::set_error("%s: depth_tol %g and depth_rel %g must be finite and >= 0", who, (double)p->depth_tol, (double)p->depth_rel);
        return -1;
    }
    if (p->outputs == 0u || (p->outputs & ~OUT_ALL)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of flow 1, scene flow 2, flags 4, counts 8 and nothing else", who,
                         p->outputs);
        return -1;
    }
    if (p->flags & ~SLHIP_FLOW_MATCH_INSTANCE) {
        slhip::set_error("%s: flags 0x%x has bits other than match-instance 1", who, p->flags);
        return -1;
    }
    return 0;
}

extern "C" int slhip_render_flow(const slhip_render_flow_params* params, const float* d_depth_a, uint32_t stride_a,
                                 const uint16_t* d_instance_a, const float* d_motion, const float* d_depth_b, uint32_t stride_b,
                                 const uint16_t* d_instance_b, uint32_t B, float* d_flow, float* d_scene_flow, uint8_t* d_flags,
                                 int32_t* d_counts, void* stream_)
{
    static const char* who = "slhip_render_flow";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = slhip_render_flow_check_params(params)) return st;
    if (B == 0u) return 0;
    if (const int st = check_call(who, params, d_depth_a, stride_a, d_instance_a, d_motion, d_depth_b, stride_b, d_instance_b, B, d_flow,
                                  d_scene_flow, d_flags, d_counts))
        return st;
    if (params->outputs & SLHIP_FLOW_OUT_COUNTS) SLHIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)B * params->n_slots * 16u, stream));
    const uint32_t pixels = (uint32_t)params->W * (uint32_t)params->H;
    const dim3 grid((pixels + BLOCK - 1u) / BLOCK, B);
    k_render_flow<<<grid, BLOCK, 0, stream>>>(*params, d_depth_a, stride_a, d_instance_a, d_motion, d_depth_b, stride_b, d_instance_b,
                                              reinterpret_cast<float2*>(d_flow), reinterpret_cast<F3*>(d_scene_flow), d_flags, d_counts);
    SLHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int slhip_render_flow_host(const slhip_render_flow_params* params, const float* h_depth_a, uint32_t stride_a,
                                      const uint16_t* h_instance_a, const float* h_motion, const float* h_depth_b, uint32_t stride_b,
                                      const uint16_t* h_instance_b, uint32_t B, float* h_flow, float* h_scene_flow, uint8_t* h_flags,
                                      int32_t* h_counts)
{
    static const char* who = "slhip_render_flow_host";
    if (const int st = slhip_render_flow_check_params(params)) return st;
    if (B == 0u) return 0;
    if (const int st = check_call(who, params, h_depth_a, stride_a, h_instance_a, h_motion, h_depth_b, stride_b, h_instance_b, B, h_flow,
                                  h_scene_flow, h_flags, h_counts))
        return st;
    const Params& p = *params;
    const uint32_t n_slots = p.n_slots;
    const size_t pixels = (size_t)p.W * (size_t)p.H;
    if (p.outputs & SLHIP_FLOW_OUT_COUNTS) std::memset(h_counts, 0, (size_t)B * n_slots * 16u);
    for (uint32_t scene = 0u; scene < B; ++scene) {
        const float* table = h_motion + (size_t)scene * n_slots * 12u;
        const size_t base = (size_t)scene * pixels;
        int32_t* cnt = (p.outputs & SLHIP_FLOW_OUT_COUNTS) ? h_counts + (size_t)scene * n_slots * 4u : nullptr;
        for (int y = 0; y < p.H; ++y)
            for (int x = 0; x < p.W; ++x) {
                const size_t at = base + (size_t)y * (size_t)p.W + (size_t)x;
                const uint32_t i = h_instance_a[at];
                const fl::Pixel r = fl::pixel(p, x, y, h_depth_a[at * stride_a], i, table,
                                              h_depth_b ? h_depth_b + base * stride_b : nullptr, stride_b,
                                              h_instance_b ? h_instance_b + base : nullptr);
                if (p.outputs & SLHIP_FLOW_OUT_FLOW) {
                    h_flow[at * 2u] = r.u;
                    h_flow[at * 2u + 1u] = r.v;
                }
                if (p.outputs & SLHIP_FLOW_OUT_SCENE) {
                    h_scene_flow[at * 3u] = r.x;
                    h_scene_flow[at * 3u + 1u] = r.y;
                    h_scene_flow[at * 3u + 2u] = r.z;
                }
                if (p.outputs & SLHIP_FLOW_OUT_FLAGS) h_flags[at] = (uint8_t)r.flags;
                if (cnt && i < n_slots) {
                    cnt[i * 4u] += 1;
                    cnt[i * 4u + 1u] += (r.flags & SLHIP_FLOW_VALID) ? 1 : 0;
                    cnt[i * 4u + 2u] += (r.flags & SLHIP_FLOW_INSIDE) ? 1 : 0;
                    cnt[i * 4u + 3u] += (r.flags & SLHIP_FLOW_VISIBLE) ? 1 : 0;
                }
            }
    }
    return 0;
}

extern "C" int slhip_render_flow_motion(const float* d_from, const float* d_to, uint32_t n, float* d_out, void* stream_)
{
    static const char* who = "slhip_render_flow_motion";
    if (n == 0u) return 0;
    if (!d_from || !d_to || !d_out || (((uintptr_t)d_from | (uintptr_t)d_to | (uintptr_t)d_out) & 3u)) {
        slhip::set_error("%s: from, to and the output are required, 4-byte aligned", who);
        return -1;
    }
    k_flow_motion<<<(n + BLOCK - 1u) / BLOCK, BLOCK, 0, (hipStream_t)stream_>>>(d_from, d_to, n, d_out);
    SLHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int slhip_render_flow_motion_host(const float* h_from, const float* h_to, uint32_t n, float* h_out)
{
    static const char* who = "slhip_render_flow_motion_host";
    if (n == 0u) return 0;
    if (!h_from || !h_to || !h_out) {
        slhip::set_error("%s: from, to and the output are required", who);
        return -1;
    }
    for (uint32_t t = 0u; t < n; ++t) fl::motion(h_from + (size_t)t * 12u, h_to + (size_t)t * 12u, h_out + (size_t)t * 12u);
    return 0;
}
