// Farthest point sampling per mesh class (slhip_fps.h): the keypoint banks of slhip_object_keypoints.hip and the region centres
// of slhip_object_regions.hip.  DESIGN.md "Object keypoints" states the rule; all arithmetic is float32, one rounded operation at
// a time (-ffp-contract=off), through slhip_keypoint_rules.h on host and device alike.
//   k_fps   one workgroup per class: n_fps rounds of {update dmin, max value then lowest index}; the reduction goes through the
//           wave by shuffles, then through LDS; it does not depend on the order
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fps.h"
#include "slhip_keypoint_rules.h"

namespace {

static_assert(sizeof(slhip_asset) == 224, "slhip_asset layout");
static_assert(sizeof(slhip_draw) == 432, "slhip_draw layout");

namespace kp = slhip_kp;

constexpr uint32_t FPS_BLOCK = 1024u;      // one workgroup per class
constexpr uint32_t FPS_WAVES = FPS_BLOCK / 64u;

using kp::class_vertices;

__device__ __forceinline__ kp::Best wave_best(kp::Best b)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        kp::Best o;
        o.val = __shfl_xor(b.val, d, 64);
        o.idx = __shfl_xor(b.idx, d, 64);
        b = kp::join(b, o);
    }
    return b;
}

// Block c is class c.  Thread t owns vertices t, t + FPS_BLOCK, ...: their dmin is read and written by it alone, in row c of the
// scratch (max_verts floats).  Every read of the pool is inside [base, base + n), which class_vertices bounds by n_vertices.
__global__ __launch_bounds__(FPS_BLOCK) void k_fps(const float4* __restrict__ pos, uint64_t n_vertices,
                                                   const slhip_asset* __restrict__ assets, const slhip_draw* __restrict__ templates,
                                                   uint32_t n_templates, uint32_t n_fps, uint64_t max_verts,
                                                   float* __restrict__ scratch, float4* __restrict__ keypoints,
                                                   int32_t* __restrict__ vertex)
{
    __shared__ float s_val[2][FPS_WAVES];
    __shared__ int s_idx[2][FPS_WAVES];
    const uint32_t c = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const slhip_asset& a = assets[c];
    uint64_t base;
    uint32_t n;
    class_vertices(a, templates, n_templates, n_vertices, max_verts, &base, &n);
    float m2o[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m2o[i] = a.mesh_to_object[i];
    const kp::P3 o = kp::bbox_centre(a.bbox_min, a.bbox_max);
    float4* kout = keypoints + (size_t)c * n_fps;
    int32_t* vout = vertex + (size_t)c * n_fps;
    if (n == 0u) {      // uniform over the block
        for (uint32_t k = tid; k < n_fps; k += FPS_BLOCK) {
            kout[k] = make_float4(o.x, o.y, o.z, 1.0f);
            vout[k] = -1;
        }
        return;
    }
    float* dmin = scratch + (size_t)c * max_verts;
    const float4* cp = pos + base;
    kp::P3 last = o;      // round 0 measures from the bbox centre
    for (uint32_t k = 0u; k < n_fps; ++k) {
        kp::Best mine = kp::best_start();
        for (uint32_t v = tid; v < n; v += FPS_BLOCK) {
            const float4 q = cp[v];
            const float d = kp::d2(kp::object_point(m2o, q.x, q.y, q.z), last);
            const float m = k == 0u ? d : kp::keep_min(dmin[v], d);
            dmin[v] = m;
            mine = kp::offer(mine, m, (int)v);
        }
        mine = wave_best(mine);
        if (lane == 0u) {
            s_val[k & 1u][wave] = mine.val;
            s_idx[k & 1u][wave] = mine.idx;
        }
        __syncthreads();      // (the other half of s_* is last read before the previous round's barrier is passed by all)
        kp::Best all = kp::best_start();
#pragma unroll
        for (uint32_t w = 0u; w < FPS_WAVES; ++w) {
            kp::Best b;
            b.val = s_val[k & 1u][w];
            b.idx = s_idx[k & 1u][w];
            all = kp::join(all, b);
        }
        const int i = kp::best_index(all);      // < n: only offered indices and 0 come out
        const float4 q = cp[i];
        last = kp::object_point(m2o, q.x, q.y, q.z);
        if (tid == 0u) {
            kout[k] = make_float4(last.x, last.y, last.z, 1.0f);
            vout[k] = i;
        }
    }
}

}  // namespace

int slhip::check_fps(const char* who, const char* what, uint32_t limit, uint32_t n_assets, uint32_t n_fps)
{
    if (const int st = check_range(who, "n_assets", n_assets, 1u, SLHIP_SYNTH_MAX_ASSETS)) return st;
    return check_range(who, what, n_fps, 1u, limit);
}

int slhip::fps_device(const char* who, const char* what, uint32_t limit, const float* d_pos, uint64_t n_vertices,
                      const slhip_asset* d_assets, uint32_t n_assets, const slhip_draw* d_templates, uint32_t n_templates,
                      uint32_t n_fps, uint64_t max_verts, void* d_scratch, float* d_keypoints, int32_t* d_vertex, hipStream_t stream)
{
    if (const int st = check_fps(who, what, limit, n_assets, n_fps)) return st;
    if (!d_assets || !d_keypoints || !d_vertex || (n_templates && !d_templates) || (n_vertices && !d_pos) ||
        (max_verts && !d_scratch)) {
        slhip::set_error("%s: null argument (assets, outputs, and templates / vertices / scratch unless their count is 0)", who);
        return -1;
    }
    k_fps<<<n_assets, FPS_BLOCK, 0, stream>>>(reinterpret_cast<const float4*>(d_pos), n_vertices, d_assets, d_templates, n_templates,
                                             n_fps, max_verts, (float*)d_scratch, reinterpret_cast<float4*>(d_keypoints), d_vertex);
    SLHIP_LAUNCH_CHECK();
    return 0;
}

int slhip::fps_host(const char* who, const char* what, uint32_t limit, const float* h_pos, uint64_t n_vertices,
                    const slhip_asset* h_assets, uint32_t n_assets, const slhip_draw* h_templates, uint32_t n_templates,
                    uint32_t n_fps, float* h_keypoints, int32_t* h_vertex)
{
    if (const int st = check_fps(who, what, limit, n_assets, n_fps)) return st;
    if (!h_assets || !h_keypoints || !h_vertex || (n_templates && !h_templates) || (n_vertices && !h_pos)) {
        slhip::set_error("%s: null argument", who);
        return -1;
    }
    std::vector<float> dmin;
    for (uint32_t c = 0; c < n_assets; ++c) {
        const slhip_asset& a = h_assets[c];
        uint64_t base;
        uint32_t n;
        class_vertices(a, h_templates, n_templates, n_vertices, ~0ull, &base, &n);
        const kp::P3 o = kp::bbox_centre(a.bbox_min, a.bbox_max);
        float* kout = h_keypoints + (size_t)c * n_fps * 4u;
        int32_t* vout = h_vertex + (size_t)c * n_fps;
        dmin.assign(n, 0.0f);
        kp::P3 last = o;
        for (uint32_t k = 0; k < n_fps; ++k) {
            int i = -1;
            if (n) {
                kp::Best best = kp::best_start();
                for (uint32_t v = 0; v < n; ++v) {
                    const float* q = h_pos + (base + v) * 4u;
                    const float d = kp::d2(kp::object_point(a.mesh_to_object, q[0], q[1], q[2]), last);
                    dmin[v] = k == 0u ? d : kp::keep_min(dmin[v], d);
                    best = kp::offer(best, dmin[v], (int)v);
                }
                i = kp::best_index(best);
                const float* q = h_pos + (base + (uint32_t)i) * 4u;
                last = kp::object_point(a.mesh_to_object, q[0], q[1], q[2]);
            }
            kout[4u * k] = last.x; kout[4u * k + 1u] = last.y; kout[4u * k + 2u] = last.z; kout[4u * k + 3u] = 1.0f;
            vout[k] = i;
        }
    }
    return 0;
}
