// Rigid fit (this project's addition, no counterpart in the reference): the pose of every set of N 3D-3D correspondences in the
// least-squares sense, by Horn's quaternion form -- the last step of PVN3D / FFB6D (bank keypoints onto voted keypoints) and the
// pose from predicted object coordinates plus depth (points.coord onto points.camera).  include/slhip.h "Rigid fit" and
// DESIGN.md "Rigid fit" are the contract; all arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through
// slhip_fit_rules.h on host and device alike, so slhip_pose_fit_host gives the kernel's outputs bit for bit.
//   k_pose_fit   one workgroup of 256 lanes per set.  Three passes over the set's correspondences from global memory (16 bytes a
//                side; a set is at most 128 KiB and stays in L2), lane l taking j = l, l + 256, ...: the count and the six sums of
//                the centroids, the nine sums of the moments, the sum of the squared residuals; every sum in pose_error's order.
//                Between them every lane runs the same 4 x 4 Jacobi in registers, so nothing is broadcast.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fit_rules.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_fit_params) == 64, "slhip_pose_fit_params layout");

using Params = slhip_pose_fit_params;
using Out = slhip_pose_fit_out;
namespace ft = slhip_fit;

constexpr uint32_t BLOCK = ft::BLOCK;
constexpr uint32_t NWAVES = BLOCK / ft::WAVE;
constexpr uint32_t SUMS = 9u;        // the most sums of one reduction (the moments')

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

// S[i] = the workgroup's sum of acc[i] in pose_error's order: the butterfly in a wave, then ((w0 + w1) + w2) + w3
template <int N>
__device__ __forceinline__ void block_sums(const float* acc, float* s_part, uint32_t wave, uint32_t lane, float* S)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float w = wave_sum(acc[i]);
        if (lane == 0u) s_part[wave * SUMS + i] = w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) S[i] = ((s_part[i] + s_part[SUMS + i]) + s_part[2u * SUMS + i]) + s_part[3u * SUMS + i];
    __syncthreads();      // the sums are read before the next reduction writes them
}

// lane 0 writes the set's outputs; pose == nullptr: NaN.  (Inlined and unrolled: the pose stays in registers.)
__device__ __forceinline__ void write_all(const Params& p, const Out& out, uint32_t set, const float* pose, uint32_t n_used, float rms, int flags)
{
    if (threadIdx.x) return;
    const uint32_t m = p.outputs;
    if (m & SLHIP_FIT_OUT_POSE)
#pragma unroll
        for (uint32_t i = 0u; i < 12u; ++i) out.pose[(size_t)set * 12u + i] = pose ? pose[i] : __builtin_nanf("");
    if (m & SLHIP_FIT_OUT_N_USED) out.n_used[set] = (int32_t)n_used;
    if (m & SLHIP_FIT_OUT_RMS) out.rms[set] = rms;
    if (m & SLHIP_FIT_OUT_FLAGS) out.flags[set] = flags;
}

__global__ __launch_bounds__(BLOCK) void k_pose_fit(Params p, const float4* __restrict__ src, const float4* __restrict__ dst, Out out)
{
    __shared__ float s_part[NWAVES * SUMS];
    __shared__ uint32_t s_cnt[NWAVES];
    const uint32_t N = p.n_points, tid = threadIdx.x, wave = tid / ft::WAVE, lane = tid % ft::WAVE, set = blockIdx.x;
    const float4* my_src = src + (size_t)set * N;
    const float4* my_dst = dst + (size_t)set * N;
    const float nan = __builtin_nanf("");

    // pass 1: the count and the centroids
    float c[6];
    uint32_t n_used;
    {
        float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, S[6];
        uint32_t mine = 0u;
        for (uint32_t j = tid; j < N; j += BLOCK) {
            const float4 a = my_src[j], b = my_dst[j];
            const float s[4] = {a.x, a.y, a.z, a.w}, d[4] = {b.x, b.y, b.z, b.w};
            if (!ft::used(s, d)) continue;
            ++mine;
            ft::accumulate_centroids(s, d, acc);
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) mine += (uint32_t)__shfl_xor((int)mine, off);
        if (lane == 0u) s_cnt[wave] = mine;
        block_sums<6>(acc, s_part, wave, lane, S);      // (its barriers order s_cnt too)
        n_used = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
        if (n_used < 3u) {      // the same for every lane
            write_all(p, out, set, nullptr, n_used, nan, SLHIP_FIT_INSUFFICIENT);
            return;
        }
        const float count = (float)n_used;
#pragma unroll
        for (int i = 0; i < 6; ++i) c[i] = S[i] / count;
    }

    // pass 2: the moments
    float M[9];
    {
        float acc[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t j = tid; j < N; j += BLOCK) {
            const float4 a = my_src[j], b = my_dst[j];
            const float s[4] = {a.x, a.y, a.z, a.w}, d[4] = {b.x, b.y, b.z, b.w};
            if (ft::used(s, d)) ft::accumulate_moments(s, d, c, acc);
        }
        block_sums<9>(acc, s_part, wave, lane, M);
    }

    // every lane: the same eigen decomposition, the same pose
    float A[4][4], V[4][4], pose[12];
    ft::horn(M, A);
    ft::jacobi(A, V);
    if (!ft::pose_of(A, V, c, p.min_gap, pose)) {      // the same for every lane
        write_all(p, out, set, nullptr, n_used, nan, SLHIP_FIT_DEGENERATE);
        return;
    }

    // pass 3: the residuals
    float rms = 0.0f;
    if (p.outputs & SLHIP_FIT_OUT_RMS) {
        float acc[1] = {0.0f}, S[1];
        for (uint32_t j = tid; j < N; j += BLOCK) {
            const float4 a = my_src[j], b = my_dst[j];
            const float s[4] = {a.x, a.y, a.z, a.w}, d[4] = {b.x, b.y, b.z, b.w};
            if (ft::used(s, d)) acc[0] = acc[0] + ft::residual2(pose, s, d);
        }
        block_sums<1>(acc, s_part, wave, lane, S);
        rms = sqrtf(S[0] / (float)n_used);
    }
    write_all(p, out, set, pose, n_used, rms, 0);
}

constexpr uint32_t ALL_OUTPUTS = SLHIP_FIT_OUT_POSE | SLHIP_FIT_OUT_N_USED | SLHIP_FIT_OUT_RMS | SLHIP_FIT_OUT_FLAGS;

// the checks that slhip_pose_fit and slhip_pose_fit_host share
int check_call(const char* who, const Params* params, const float* src, const float* dst, const Out* out)
{
    if (const int st = slhip_pose_fit_check_params(params)) return st;
    if (!src || !dst || !out) {
        slhip::set_error("%s: null argument (src, dst and the output record are required)", who);
        return -1;
    }
    const uint32_t m = params->outputs;
    if (((m & SLHIP_FIT_OUT_POSE) && !out->pose) || ((m & SLHIP_FIT_OUT_N_USED) && !out->n_used) ||
        ((m & SLHIP_FIT_OUT_RMS) && !out->rms) || ((m & SLHIP_FIT_OUT_FLAGS) && !out->flags)) {
        slhip::set_error("%s: an output named in `outputs` (0x%x) has a null pointer", who, m);
        return -1;
    }
    if (((uintptr_t)src & 15u) || ((uintptr_t)dst & 15u)) {
        slhip::set_error("%s: src and dst must be 16-byte aligned", who);
        return -1;
    }
    const uintptr_t all = ((m & SLHIP_FIT_OUT_POSE) ? (uintptr_t)out->pose : 0u) | ((m & SLHIP_FIT_OUT_N_USED) ? (uintptr_t)out->n_used : 0u) |
                          ((m & SLHIP_FIT_OUT_RMS) ? (uintptr_t)out->rms : 0u) | ((m & SLHIP_FIT_OUT_FLAGS) ? (uintptr_t)out->flags : 0u);
    if (all & 3u) {
        slhip::set_error("%s: every output must be 4-byte aligned", who);
        return -1;
    }
    return 0;
}

// optional HIP-event timing: events round the last call
slhip::StepTimer<1> g_timer;

}  // namespace

extern "C" int slhip_pose_fit_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_pose_fit_timings(float ms_out[1])
{
    if (!ms_out) {
        slhip::set_error("slhip_pose_fit_timings: null argument");
        return -1;
    }
    return std::min(g_timer.read(ms_out), 0);
}

extern "C" int slhip_pose_fit_check_params(const slhip_pose_fit_params* p)
{
    static const char* who = "slhip_pose_fit";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 1u, SLHIP_FIT_POINTS_MAX)) return st;
    if (!(p->min_gap >= 0.0f) || !(p->min_gap < 1.0f)) {
        slhip::set_error("%s: min_gap %g must lie in [0, 1)", who, (double)p->min_gap);
        return -1;
    }
    if (p->outputs == 0u || (p->outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of pose 1, n_used 2, rms 4, flags 8 and nothing else", who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_pose_fit(const slhip_pose_fit_params* params, const float* d_src, const float* d_dst, const slhip_pose_fit_out* out,
                              void* stream_)
{
    static const char* who = "slhip_pose_fit";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_src, d_dst, out)) return st;
    if (params->n_sets == 0u) return 0;
    if (const int st = g_timer.begin(0, stream)) return st;
    k_pose_fit<<<params->n_sets, BLOCK, 0, stream>>>(*params, reinterpret_cast<const float4*>(d_src), reinterpret_cast<const float4*>(d_dst), *out);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

extern "C" int slhip_pose_fit_host(const slhip_pose_fit_params* params, const float* h_src, const float* h_dst, const slhip_pose_fit_out* out)
{
    static const char* who = "slhip_pose_fit_host";
    if (const int st = check_call(who, params, h_src, h_dst, out)) return st;
    const Params& p = *params;
    const uint32_t N = p.n_points, mask = p.outputs;
    const float nan = __builtin_nanf("");
    for (uint32_t set = 0u; set < p.n_sets; ++set) {
        const float* src = h_src + (size_t)set * N * 4u;
        const float* dst = h_dst + (size_t)set * N * 4u;
        auto write = [&](const float* pose, uint32_t n_used, float rms, int flags) {
            if (mask & SLHIP_FIT_OUT_POSE)
                for (uint32_t i = 0u; i < 12u; ++i) out->pose[(size_t)set * 12u + i] = pose ? pose[i] : nan;
            if (mask & SLHIP_FIT_OUT_N_USED) out->n_used[set] = (int32_t)n_used;
            if (mask & SLHIP_FIT_OUT_RMS) out->rms[set] = rms;
            if (mask & SLHIP_FIT_OUT_FLAGS) out->flags[set] = flags;
        };
        // upwards: lane j % BLOCK meets its correspondences in rising order
        float lanes[9][BLOCK] = {};
        uint32_t n_used = 0u;
        for (uint32_t j = 0u; j < N; ++j) {
            if (!ft::used(src + 4u * j, dst + 4u * j)) continue;
            ++n_used;
            float acc[6];
            for (int s = 0; s < 6; ++s) acc[s] = lanes[s][j % BLOCK];
            ft::accumulate_centroids(src + 4u * j, dst + 4u * j, acc);
            for (int s = 0; s < 6; ++s) lanes[s][j % BLOCK] = acc[s];
        }
        if (n_used < 3u) {
            write(nullptr, n_used, nan, SLHIP_FIT_INSUFFICIENT);
            continue;
        }
        float c[6], M[9];
        for (int s = 0; s < 6; ++s) c[s] = slhip_pose::block_sum(lanes[s]) / (float)n_used;
        for (int s = 0; s < 9; ++s) std::fill(lanes[s], lanes[s] + BLOCK, 0.0f);
        for (uint32_t j = 0u; j < N; ++j) {
            if (!ft::used(src + 4u * j, dst + 4u * j)) continue;
            float acc[9];
            for (int s = 0; s < 9; ++s) acc[s] = lanes[s][j % BLOCK];
            ft::accumulate_moments(src + 4u * j, dst + 4u * j, c, acc);
            for (int s = 0; s < 9; ++s) lanes[s][j % BLOCK] = acc[s];
        }
        for (int s = 0; s < 9; ++s) M[s] = slhip_pose::block_sum(lanes[s]);
        float A[4][4], V[4][4], pose[12];
        ft::horn(M, A);
        ft::jacobi(A, V);
        if (!ft::pose_of(A, V, c, p.min_gap, pose)) {
            write(nullptr, n_used, nan, SLHIP_FIT_DEGENERATE);
            continue;
        }
        std::fill(lanes[0], lanes[0] + BLOCK, 0.0f);
        for (uint32_t j = 0u; j < N; ++j)
            if (ft::used(src + 4u * j, dst + 4u * j)) lanes[0][j % BLOCK] = lanes[0][j % BLOCK] + ft::residual2(pose, src + 4u * j, dst + 4u * j);
        write(pose, n_used, sqrtf(slhip_pose::block_sum(lanes[0]) / (float)n_used), 0);
    }
    return 0;
}
