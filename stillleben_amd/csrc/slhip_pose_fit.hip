// Rigid fit (this project's addition, no counterpart in the reference): the pose of every set of N 3D-3D correspondences in the
// least-squares sense, by Horn's quaternion form -- the last step of PVN3D / FFB6D (bank keypoints onto voted keypoints) and the
// pose from predicted object coordinates plus depth (points.coord onto points.camera).  include/slhip.h "Rigid fit" and
// DESIGN.md "Rigid fit" are the contract; all arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through
// slhip_fit_rules.h on host and device alike, so slhip_pose_fit_host gives the kernel's outputs bit for bit.
//   k_pose_fit   one workgroup of 256 lanes per set.  The three passes of slhip_fit_block.h over the set's correspondences from
//                global memory (16 bytes a side; a set is at most 128 KiB and stays in L2), lane l taking j = l, l + 256, ...: the
//                count and the six sums of the centroids, the nine sums of the moments, the sum of the squared residuals; every
//                sum in the order of slhip_block_sum.h.  Between them every lane runs the same 4 x 4 Jacobi in registers, so
//                nothing is broadcast.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fit_block.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_fit_params) == 64, "slhip_pose_fit_params layout");

using Params = slhip_pose_fit_params;
using Out = slhip_pose_fit_out;
namespace ft = slhip_fit;

constexpr uint32_t BLOCK = ft::BLOCK;
constexpr uint32_t NWAVES = BLOCK / ft::WAVE;

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
    __shared__ float s_part[NWAVES * ft::FIT_SUMS];
    __shared__ uint32_t s_cnt[NWAVES];
    const uint32_t N = p.n_points, tid = threadIdx.x, set = blockIdx.x;
    const float4* my_src = src + (size_t)set * N;
    const float4* my_dst = dst + (size_t)set * N;
    const float nan = __builtin_nanf("");

    // correspondence j of the set, from global memory
    auto pair = [&](uint32_t j, float* s, float* d) {
        const float4 a = my_src[j], b = my_dst[j];
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
        d[0] = b.x; d[1] = b.y; d[2] = b.z; d[3] = b.w;
        return ft::used(s, d);
    };
    float S[6], pose[12];
    const uint32_t mine = ft::fit_centroids(N, pair, s_part, S);
    const uint32_t n_used = slhip_pose::block_count(mine, s_cnt, tid / ft::WAVE, tid % ft::WAVE);
    if (n_used < 3u) {      // the same for every lane
        write_all(p, out, set, nullptr, n_used, nan, SLHIP_FIT_INSUFFICIENT);
        return;
    }
    if (!ft::fit_pose(N, pair, S, n_used, p.min_gap, s_part, pose)) {      // the same for every lane
        write_all(p, out, set, nullptr, n_used, nan, SLHIP_FIT_DEGENERATE);
        return;
    }
    const float rms = (p.outputs & SLHIP_FIT_OUT_RMS) ? ft::fit_rms(N, pair, pose, n_used, s_part) : 0.0f;
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
    const slhip::OutputList outputs = {
        {SLHIP_FIT_OUT_POSE, out->pose}, {SLHIP_FIT_OUT_N_USED, out->n_used}, {SLHIP_FIT_OUT_RMS, out->rms}, {SLHIP_FIT_OUT_FLAGS, out->flags}};
    if (const int st = slhip::check_outputs_present(who, m, outputs)) return st;
    if (((uintptr_t)src & 15u) || ((uintptr_t)dst & 15u)) {
        slhip::set_error("%s: src and dst must be 16-byte aligned", who);
        return -1;
    }
    return slhip::check_outputs_aligned(who, m, outputs);
}

// optional HIP-event timing: events round the last call
slhip::StepTimer<1> g_timer;

}  // namespace

extern "C" int slhip_pose_fit_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_pose_fit_timings(float ms_out[1]) { return g_timer.read_for("slhip_pose_fit_timings", ms_out); }

extern "C" int slhip_pose_fit_check_params(const slhip_pose_fit_params* p)
{
    static const char* who = "slhip_pose_fit";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 1u, SLHIP_FIT_POINTS_MAX)) return st;
    if (const int st = slhip::check_min_gap(who, p->min_gap)) return st;
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
        auto pair = [&](uint32_t j, float* s, float* d) {
            for (int i = 0; i < 4; ++i) {
                s[i] = src[4u * j + i];
                d[i] = dst[4u * j + i];
            }
            return ft::used(s, d);
        };
        float S[6], pose[12];
        const uint32_t n_used = ft::fit_centroids_host(N, pair, S);
        if (n_used < 3u)
            write(nullptr, n_used, nan, SLHIP_FIT_INSUFFICIENT);
        else if (!ft::fit_pose_host(N, pair, S, n_used, p.min_gap, pose))
            write(nullptr, n_used, nan, SLHIP_FIT_DEGENERATE);
        else
            write(pose, n_used, ft::fit_rms_host(N, pair, pose, n_used), 0);
    }
    return 0;
}
