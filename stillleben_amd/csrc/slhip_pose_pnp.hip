// Pose PnP (this project's addition, no counterpart in the reference): the pose of every set of K 2D-3D correspondences by P3P
// inside RANSAC, then Gauss-Newton on the inliers.  include/slhip.h "Pose PnP" and DESIGN.md "Pose PnP" are the contract; all
// arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through slhip_pnp_rules.h on host and device alike,
// so slhip_pose_pnp_host gives the kernel's outputs bit for bit.
//   k_pose_pnp   one workgroup of 256 lanes per set.  (1) the valid correspondences, in ascending order, into five LDS planes
//                (u, v, x, y, z) by ballot ranks;  (2) a lane per hypothesis in rounds of 256: Philox, P3P, then the score with
//                the twelve pose entries in registers and the points by 16-byte LDS reads at one address for all lanes (a
//                broadcast), no barrier inside a round;  (3) arg-max of (count, lowest index) by wave then workgroup;
//                (4) Gauss-Newton: lanes over points, 27 sums in the order of slhip_block_sum.h, every lane solves the 6 x 6;
//                (5) the final pass over the correspondences in their own order: ballot words, count, rms
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_pnp_rules.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_pnp_params) == 64, "slhip_pose_pnp_params layout");

using Params = slhip_pose_pnp_params;
using Out = slhip_pose_pnp_out;
namespace pn = slhip_pnp;

constexpr uint32_t BLOCK = pn::BLOCK;
constexpr uint32_t NWAVES = BLOCK / pn::WAVE;
constexpr uint32_t PLANES = 5u;      // u v x y z, each k_pad floats
constexpr int PART_STRIDE = pn::SUMS + 1;      // the words of a wave's row of partial sums

using slhip_pose::pad4;
using slhip_pose::words_of;

__device__ __forceinline__ pn::Camera camera_of(const Params& p, const float* intrinsics, uint32_t set)
{
    pn::Camera k = {p.fx, p.fy, p.cx, p.cy};
    if (intrinsics) {
        const float4 v = reinterpret_cast<const float4*>(intrinsics)[set];
        k.fx = v.x; k.fy = v.y; k.cx = v.z; k.cy = v.w;
    }
    return k;
}

// INSUFFICIENT / NO_MODEL: a NaN pose, 0 inliers, NaN rms, best -2, zero bits (lane 0, and the words by all lanes)
__device__ void write_none(const Params& p, const Out& out, uint32_t set, int flags)
{
    const uint32_t m = p.outputs, nw = words_of(p.n_points);
    if (m & SLHIP_PNP_OUT_INLIERS)
        for (uint32_t w = threadIdx.x; w < nw; w += BLOCK) out.inliers[(size_t)set * nw + w] = 0u;
    if (threadIdx.x) return;
    if (m & SLHIP_PNP_OUT_POSE)
        for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = __builtin_nanf("");
    if (m & SLHIP_PNP_OUT_N_INLIERS) out.n_inliers[set] = 0;
    if (m & SLHIP_PNP_OUT_RMS) out.rms[set] = __builtin_nanf("");
    if (m & SLHIP_PNP_OUT_BEST) out.best[set] = -2;
    if (m & SLHIP_PNP_OUT_FLAGS) out.flags[set] = flags;
}

// the score of one pose in registers against the n valid points: four per 16-byte read of each plane, then the ragged rest
__device__ __forceinline__ uint32_t score(const float* M, const pn::Camera& k, float thr2, const float* s_u, const float* s_v,
                                          const float* s_x, const float* s_y, const float* s_z, uint32_t n)
{
    uint32_t count = 0u;
    float e2;
    const uint32_t whole = n & ~3u;
#pragma unroll 1      // unrolled further the reads of several rounds pile up: 256 VGPRs and spills against 164 and none
    for (uint32_t j = 0u; j < whole; j += 4u) {
        const float4 U = *reinterpret_cast<const float4*>(s_u + j), V = *reinterpret_cast<const float4*>(s_v + j);
        const float4 X = *reinterpret_cast<const float4*>(s_x + j), Y = *reinterpret_cast<const float4*>(s_y + j);
        const float4 Z = *reinterpret_cast<const float4*>(s_z + j);
        count += pn::inlier(M, k, X.x, Y.x, Z.x, U.x, V.x, thr2, &e2) ? 1u : 0u;
        count += pn::inlier(M, k, X.y, Y.y, Z.y, U.y, V.y, thr2, &e2) ? 1u : 0u;
        count += pn::inlier(M, k, X.z, Y.z, Z.z, U.z, V.z, thr2, &e2) ? 1u : 0u;
        count += pn::inlier(M, k, X.w, Y.w, Z.w, U.w, V.w, thr2, &e2) ? 1u : 0u;
    }
    for (uint32_t j = whole; j < n; ++j) count += pn::inlier(M, k, s_x[j], s_y[j], s_z[j], s_u[j], s_v[j], thr2, &e2) ? 1u : 0u;
    return count;
}

// One block per set.  Dynamic LDS: PLANES * k_pad floats, k_pad = K rounded up to 4.
__global__ __launch_bounds__(BLOCK) void k_pose_pnp(Params p, const float* __restrict__ uv, const float* __restrict__ xyz,
                                                    const float* __restrict__ intrinsics, const float* __restrict__ init, Out out,
                                                    uint32_t k_pad)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    __shared__ uint32_t s_cnt[NWAVES];
    __shared__ uint32_t s_key[NWAVES];
    __shared__ float s_pose[12];
    __shared__ float s_part[NWAVES * PART_STRIDE];
    float* s_u = s_all;
    float* s_v = s_u + k_pad;
    float* s_x = s_v + k_pad;
    float* s_y = s_x + k_pad;
    float* s_z = s_y + k_pad;

    const uint32_t tid = threadIdx.x, wave = tid / pn::WAVE, lane = tid % pn::WAVE;
    const uint32_t set = blockIdx.x, K = p.n_points, Hy = p.n_hypotheses, mask = p.outputs;
    const pn::Camera cam = camera_of(p, intrinsics, set);
    const float thr2 = p.threshold_px * p.threshold_px;
    const float2* my_uv = reinterpret_cast<const float2*>(uv) + (size_t)set * K;
    const float4* my_xyz = reinterpret_cast<const float4*>(xyz) + (size_t)set * K;

    // (1) the valid list: ranks by ballot inside a wave, the waves' counts through LDS
    uint32_t n_valid = 0u;
    for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
        const uint32_t j = j0 + tid;
        float2 a = make_float2(0.0f, 0.0f);
        float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j < K) {
            a = my_uv[j];
            b = my_xyz[j];
        }
        const bool ok = j < K && pn::valid(a.x, a.y, b.x, b.y, b.z, b.w);
        const unsigned long long votes = __ballot(ok);
        if (lane == 0u) s_cnt[wave] = (uint32_t)__popcll(votes);
        __syncthreads();
        uint32_t at = n_valid + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        for (uint32_t w = 0u; w < NWAVES; ++w) {
            at += w < wave ? s_cnt[w] : 0u;
            n_valid += s_cnt[w];
        }
        if (ok) {      // at < n_valid <= K <= k_pad
            s_u[at] = a.x; s_v[at] = a.y;
            s_x[at] = b.x; s_y[at] = b.y; s_z[at] = b.z;
        }
        __syncthreads();
    }
    if (n_valid < 4u) {      // the same for every lane
        write_none(p, out, set, SLHIP_PNP_INSUFFICIENT);
        return;
    }

    // (2) a lane per hypothesis; slot 0 is the caller's pose, slot h + 1 hypothesis h
    auto pick = [&](uint32_t i, float* c) {
        c[0] = s_u[i]; c[1] = s_v[i]; c[2] = s_x[i]; c[3] = s_y[i]; c[4] = s_z[i];
    };
    uint32_t best_key = 0u;
    float best_pose[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) best_pose[i] = 0.0f;
    for (uint32_t slot0 = init ? 0u : 1u; slot0 <= Hy; slot0 += BLOCK) {
        const uint32_t slot = slot0 + tid;
        float M[12];
        bool have = false;
        if (slot == 0u) {
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = init[(size_t)set * 12u + i];
            have = pn::pose_finite(M);
        } else if (slot <= Hy) {
            have = pn::hypothesis(p.seed_lo, p.seed_hi, p.set_id_base + set, slot - 1u, n_valid, cam, pick, M);
        }
        if (!have) {
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = __builtin_nanf("");      // counts nothing
        }
        uint32_t count = 0u;
        if (__ballot(have)) count = score(M, cam, thr2, s_u, s_v, s_x, s_y, s_z, n_valid);      // a wave without a pose skips the walk
        const uint32_t key = slot <= Hy ? pn::key_of(count, slot) : 0u;
        if (key > best_key) {
            best_key = key;
#pragma unroll
            for (int i = 0; i < 12; ++i) best_pose[i] = M[i];
        }
    }

    // (3) the winner: highest count, then lowest slot; every real slot has a key of its own, so one lane owns the maximum
    const uint32_t wkey = slhip_pose::wave_max(best_key);
    if (lane == 0u) s_key[wave] = wkey;
    __syncthreads();
    const uint32_t win = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
    if (win != 0u && best_key == win) {
#pragma unroll
        for (int i = 0; i < 12; ++i) s_pose[i] = best_pose[i];
    }
    __syncthreads();
    const uint32_t win_count = pn::key_count(win);
    if (win == 0u || win_count < p.min_inliers) {
        write_none(p, out, set, SLHIP_PNP_NO_MODEL);
        return;
    }
    float W[12], M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) W[i] = M[i] = s_pose[i];
    int flags = 0;

    // (4) Gauss-Newton on the inliers of the current pose: lane l takes valid points l, l + 256, ...
    for (uint32_t it = 0u; it < p.refine_iters; ++it) {
        float acc[pn::SUMS], S[pn::SUMS];
#pragma unroll
        for (int i = 0; i < pn::SUMS; ++i) acc[i] = 0.0f;
        for (uint32_t i = tid; i < n_valid; i += BLOCK) {
            float e2;
            if (pn::inlier(M, cam, s_x[i], s_y[i], s_z[i], s_u[i], s_v[i], thr2, &e2))
                pn::accumulate(M, cam, s_x[i], s_y[i], s_z[i], s_u[i], s_v[i], acc);
        }
        slhip_pose::block_sums<pn::SUMS, PART_STRIDE>(acc, s_part, wave, lane, S);
        if (!pn::step(S, M)) {      // the same for every lane
            flags |= SLHIP_PNP_REFINE_STOPPED;
            break;
        }
    }

    // (5) inliers, count and rms of the refined pose over the correspondences in their own order; should it hold fewer
    // inliers than the winner, the same of the winner's pose
    const uint32_t nw = words_of(K);
    for (int pass = 0; pass < 2; ++pass) {
        float acc = 0.0f;
        uint32_t mine = 0u;      // lane 0 of a wave: the wave's count
        for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
            const uint32_t j = j0 + tid;
            bool in = false;
            if (j < K) {
                const float2 a = my_uv[j];
                const float4 b = my_xyz[j];
                float e2;
                in = pn::valid(a.x, a.y, b.x, b.y, b.z, b.w) && pn::inlier(M, cam, b.x, b.y, b.z, a.x, a.y, thr2, &e2);
                if (in) acc = acc + e2;
            }
            const unsigned long long votes = __ballot(in);
            mine += (uint32_t)__popcll(votes);
            if (lane == 0u && (mask & SLHIP_PNP_OUT_INLIERS)) {
                const uint32_t w0 = (j0 + wave * pn::WAVE) / 32u;
                if (w0 < nw) out.inliers[(size_t)set * nw + w0] = (uint32_t)votes;
                if (w0 + 1u < nw) out.inliers[(size_t)set * nw + w0 + 1u] = (uint32_t)(votes >> 32);
            }
        }
        // (the count is read between the barriers of its own: the next pass writes s_cnt with no barrier in front)
        const float w = slhip_pose::wave_sum(acc);
        if (lane == 0u) {
            s_part[wave * PART_STRIDE] = w;
            s_cnt[wave] = mine;
        }
        __syncthreads();
        const uint32_t count = slhip_pose::waves_sum(s_cnt);
        const float sum = slhip_pose::waves_sum(s_part, PART_STRIDE);
        __syncthreads();
        if (pass == 0 && count < win_count) {      // the same for every lane; only a refined pose can get here
            flags |= SLHIP_PNP_REFINE_REJECTED;
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = W[i];
            continue;
        }
        if (tid == 0u) {
            if (mask & SLHIP_PNP_OUT_POSE)
                for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = M[i];
            if (mask & SLHIP_PNP_OUT_N_INLIERS) out.n_inliers[set] = (int32_t)count;
            if (mask & SLHIP_PNP_OUT_RMS) out.rms[set] = sqrtf(sum / (float)count);
            if (mask & SLHIP_PNP_OUT_BEST) out.best[set] = pn::key_best(win);
            if (mask & SLHIP_PNP_OUT_FLAGS) out.flags[set] = flags;
        }
        break;
    }
}

constexpr uint32_t ALL_OUTPUTS = SLHIP_PNP_OUT_POSE | SLHIP_PNP_OUT_N_INLIERS | SLHIP_PNP_OUT_RMS | SLHIP_PNP_OUT_INLIERS |
                                 SLHIP_PNP_OUT_BEST | SLHIP_PNP_OUT_FLAGS;

// the checks that slhip_pose_pnp and slhip_pose_pnp_host share
int check_call(const char* who, const Params* params, const float* uv, const float* xyz, const float* intrinsics, const float* init,
               const Out* out)
{
    if (const int st = slhip_pose_pnp_check_params(params)) return st;
    if (!uv || !xyz || !out) {
        slhip::set_error("%s: null argument (uv, xyz and the output record are required)", who);
        return -1;
    }
    if (params->n_hypotheses == 0u && !init) {
        slhip::set_error("%s: n_hypotheses 0 needs an initial pose (a pure refinement); without one there is nothing to score", who);
        return -1;
    }
    const slhip::OutputList outputs = {{SLHIP_PNP_OUT_POSE, out->pose},       {SLHIP_PNP_OUT_N_INLIERS, out->n_inliers}, {SLHIP_PNP_OUT_RMS, out->rms},
                                       {SLHIP_PNP_OUT_INLIERS, out->inliers}, {SLHIP_PNP_OUT_BEST, out->best},           {SLHIP_PNP_OUT_FLAGS, out->flags}};
    if (const int st = slhip::check_outputs_present(who, params->outputs, outputs)) return st;
    if (((uintptr_t)uv & 7u) || ((uintptr_t)xyz & 15u) || ((uintptr_t)intrinsics & 15u) || ((uintptr_t)init & 3u)) {
        slhip::set_error("%s: uv must be 8-byte aligned, xyz and the intrinsics 16-byte, the initial poses 4-byte", who);
        return -1;
    }
    return 0;
}

// optional HIP-event timing (tools/time_pose_pnp.py): events round the last whole call [0] and the last call that sampled
// hypotheses (n_hypotheses > 0) [1]
slhip::StepTimer<2> g_timer;

}  // namespace

extern "C" int slhip_pose_pnp_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_pose_pnp_timings(float ms_out[2]) { return g_timer.read_for("slhip_pose_pnp_timings", ms_out); }

extern "C" int slhip_pose_pnp_check_params(const slhip_pose_pnp_params* p)
{
    static const char* who = "slhip_pose_pnp";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_intrinsics(who, p->fx, p->fy, p->cx, p->cy)) return st;
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 4u, SLHIP_PNP_POINTS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_hypotheses", p->n_hypotheses, 0u, SLHIP_PNP_HYPOTHESES_MAX)) return st;
    if (!(p->threshold_px > 0.0f) || !slhip::is_finite(p->threshold_px)) {
        slhip::set_error("%s: threshold_px %g must be positive and finite", who, (double)p->threshold_px);
        return -1;
    }
    if (const int st = slhip::check_range(who, "refine_iters", p->refine_iters, 0u, SLHIP_PNP_REFINE_MAX)) return st;
    if (const int st = slhip::check_range(who, "min_inliers", p->min_inliers, 4u, 0x7fffffffu)) return st;
    if (p->outputs == 0u || (p->outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of pose 1, n_inliers 2, rms 4, inliers 8, best 16, flags 32 and nothing else",
                         who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_pose_pnp(const slhip_pose_pnp_params* params, const float* d_uv, const float* d_xyz, const float* d_intrinsics,
                              const float* d_init, const slhip_pose_pnp_out* out, void* stream_)
{
    static const char* who = "slhip_pose_pnp";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_uv, d_xyz, d_intrinsics, d_init, out)) return st;
    if (params->n_sets == 0u) return 0;
    const uint32_t k_pad = pad4(params->n_points);
    const size_t lds = (size_t)PLANES * k_pad * sizeof(float);      // 5 KiB at K = 256, 20 KiB at 1024, 80 KiB at 4096
    if (lds > 64u * 1024u)      // more than a kernel may ask for without the attribute (per device, so not remembered)
        SLHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_pnp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int sampled = params->n_hypotheses > 0u;
    if (const int st = g_timer.begin(0, stream)) return st;
    if (sampled)
        if (const int st = g_timer.begin(1, stream)) return st;
    k_pose_pnp<<<params->n_sets, BLOCK, lds, stream>>>(*params, d_uv, d_xyz, d_intrinsics, d_init, *out, k_pad);
    SLHIP_LAUNCH_CHECK();
    if (sampled)
        if (const int st = g_timer.end(1, stream)) return st;
    return g_timer.end(0, stream);
}

extern "C" int slhip_pose_pnp_p3p_host(const float* uv, const float* xyz, const float* intrinsics, float* poses_out)
{
    if (!uv || !xyz || !intrinsics || !poses_out) {
        slhip::set_error("slhip_pose_pnp_p3p_host: null argument");
        return -1;
    }
    if (const int st = slhip::check_intrinsics("slhip_pose_pnp_p3p_host", intrinsics[0], intrinsics[1], intrinsics[2], intrinsics[3])) return st;
    float ab[3][2], P[3][3];
    for (int i = 0; i < 3; ++i) {
        ab[i][0] = (uv[2 * i] - intrinsics[2]) / intrinsics[0];
        ab[i][1] = (uv[2 * i + 1] - intrinsics[3]) / intrinsics[1];
        for (int k = 0; k < 3; ++k) P[i][k] = xyz[3 * i + k];
    }
    pn::Triangle t;
    pn::triangle(ab, P, t);
    int n = 0;
    for (int s = 0; s < 4; ++s)
        if (((t.found >> s) & 1u) && pn::solution(t, s, P, poses_out + 12 * n)) ++n;
    return n;
}

extern "C" int slhip_pose_pnp_host(const slhip_pose_pnp_params* params, const float* h_uv, const float* h_xyz,
                                   const float* h_intrinsics, const float* h_init, const slhip_pose_pnp_out* out)
{
    static const char* who = "slhip_pose_pnp_host";
    if (const int st = check_call(who, params, h_uv, h_xyz, h_intrinsics, h_init, out)) return st;
    const Params& p = *params;
    const uint32_t K = p.n_points, Hy = p.n_hypotheses, mask = p.outputs, nw = words_of(K);
    const float thr2 = p.threshold_px * p.threshold_px, nan = __builtin_nanf("");
    std::vector<float> list((size_t)K * 5u);
    for (uint32_t set = 0u; set < p.n_sets; ++set) {
        const float* uv = h_uv + (size_t)set * K * 2u;
        const float* xyz = h_xyz + (size_t)set * K * 4u;
        pn::Camera cam = {p.fx, p.fy, p.cx, p.cy};
        if (h_intrinsics) cam = {h_intrinsics[4 * set], h_intrinsics[4 * set + 1], h_intrinsics[4 * set + 2], h_intrinsics[4 * set + 3]};
        auto none = [&](int flags) {
            if (mask & SLHIP_PNP_OUT_INLIERS)
                for (uint32_t w = 0u; w < nw; ++w) out->inliers[(size_t)set * nw + w] = 0u;
            if (mask & SLHIP_PNP_OUT_POSE)
                for (int i = 0; i < 12; ++i) out->pose[(size_t)set * 12u + i] = nan;
            if (mask & SLHIP_PNP_OUT_N_INLIERS) out->n_inliers[set] = 0;
            if (mask & SLHIP_PNP_OUT_RMS) out->rms[set] = nan;
            if (mask & SLHIP_PNP_OUT_BEST) out->best[set] = -2;
            if (mask & SLHIP_PNP_OUT_FLAGS) out->flags[set] = flags;
        };
        uint32_t n_valid = 0u;
        for (uint32_t j = 0u; j < K; ++j)
            if (pn::valid(uv[2 * j], uv[2 * j + 1], xyz[4 * j], xyz[4 * j + 1], xyz[4 * j + 2], xyz[4 * j + 3])) {
                float* c = &list[(size_t)n_valid++ * 5u];
                c[0] = uv[2 * j]; c[1] = uv[2 * j + 1]; c[2] = xyz[4 * j]; c[3] = xyz[4 * j + 1]; c[4] = xyz[4 * j + 2];
            }
        if (n_valid < 4u) {
            none(SLHIP_PNP_INSUFFICIENT);
            continue;
        }
        auto pick = [&](uint32_t i, float* c) {
            for (int k = 0; k < 5; ++k) c[k] = list[(size_t)i * 5u + k];
        };
        uint32_t win = 0u;
        float W[12] = {}, M[12];
        for (uint32_t slot = h_init ? 0u : 1u; slot <= Hy; ++slot) {
            bool have = false;
            if (slot == 0u) {
                for (int i = 0; i < 12; ++i) M[i] = h_init[(size_t)set * 12u + i];
                have = pn::pose_finite(M);
            } else {
                have = pn::hypothesis(p.seed_lo, p.seed_hi, p.set_id_base + set, slot - 1u, n_valid, cam, pick, M);
            }
            uint32_t count = 0u;
            float e2;
            if (have)
                for (uint32_t i = 0u; i < n_valid; ++i) {
                    const float* c = &list[(size_t)i * 5u];
                    count += pn::inlier(M, cam, c[2], c[3], c[4], c[0], c[1], thr2, &e2) ? 1u : 0u;
                }
            const uint32_t key = pn::key_of(count, slot);
            if (key > win) {
                win = key;
                for (int i = 0; i < 12; ++i) W[i] = have ? M[i] : nan;
            }
        }
        const uint32_t win_count = pn::key_count(win);
        if (win == 0u || win_count < p.min_inliers) {
            none(SLHIP_PNP_NO_MODEL);
            continue;
        }
        for (int i = 0; i < 12; ++i) M[i] = W[i];
        int flags = 0;
        for (uint32_t it = 0u; it < p.refine_iters; ++it) {
            slhip_pose::LaneSums<pn::SUMS> sums;
            for (uint32_t i = 0u; i < n_valid; ++i) {
                const float* c = &list[(size_t)i * 5u];
                float e2;
                if (pn::inlier(M, cam, c[2], c[3], c[4], c[0], c[1], thr2, &e2))
                    sums.add(i, [&](float* acc) { pn::accumulate(M, cam, c[2], c[3], c[4], c[0], c[1], acc); });
            }
            float S[pn::SUMS];
            for (int s = 0; s < pn::SUMS; ++s) S[s] = sums.total(s);
            if (!pn::step(S, M)) {
                flags |= SLHIP_PNP_REFINE_STOPPED;
                break;
            }
        }
        for (int pass = 0; pass < 2; ++pass) {
            slhip_pose::LaneSums<1> sums;
            uint32_t count = 0u;
            std::vector<uint32_t> bits(nw, 0u);
            for (uint32_t j = 0u; j < K; ++j) {
                float e2;
                if (!pn::valid(uv[2 * j], uv[2 * j + 1], xyz[4 * j], xyz[4 * j + 1], xyz[4 * j + 2], xyz[4 * j + 3]) ||
                    !pn::inlier(M, cam, xyz[4 * j], xyz[4 * j + 1], xyz[4 * j + 2], uv[2 * j], uv[2 * j + 1], thr2, &e2))
                    continue;
                sums.add(j, [&](float* acc) { acc[0] = acc[0] + e2; });
                bits[j >> 5] |= 1u << (j & 31u);
                ++count;
            }
            if (pass == 0 && count < win_count) {
                flags |= SLHIP_PNP_REFINE_REJECTED;
                for (int i = 0; i < 12; ++i) M[i] = W[i];
                continue;
            }
            if (mask & SLHIP_PNP_OUT_INLIERS)
                for (uint32_t w = 0u; w < nw; ++w) out->inliers[(size_t)set * nw + w] = bits[w];
            if (mask & SLHIP_PNP_OUT_POSE)
                for (int i = 0; i < 12; ++i) out->pose[(size_t)set * 12u + i] = M[i];
            if (mask & SLHIP_PNP_OUT_N_INLIERS) out->n_inliers[set] = (int32_t)count;
            if (mask & SLHIP_PNP_OUT_RMS) out->rms[set] = sqrtf(sums.total(0) / (float)count);
            if (mask & SLHIP_PNP_OUT_BEST) out->best[set] = pn::key_best(win);
            if (mask & SLHIP_PNP_OUT_FLAGS) out->flags[set] = flags;
            break;
        }
    }
    return 0;
}
