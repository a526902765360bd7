// Robust alignment (this project's addition, no counterpart in the reference): the pose of every set of K 3D-3D correspondences
// with the most inliers -- Horn's fit of three picked pairs inside RANSAC, then the rigid fit on the inliers.  It is to
// slhip_pose_fit what slhip_pose_pnp is to a plain PnP: predicted object coordinates onto camera points, or bank keypoints onto
// voted ones, when some of them are wrong by the size of the object.  include/slhip.h "Robust alignment" and DESIGN.md "Robust
// alignment" are the contract; all arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through
// slhip_align_rules.h and slhip_fit_block.h on host and device alike, so slhip_pose_align_host gives the kernel's outputs bit for
// bit.
//   k_pose_align  one workgroup of 256 lanes per set.  (1) the valid correspondences, in ascending order, into six LDS planes
//                 (sx, sy, sz, dx, dy, dz) by ballot ranks;  (2) a lane per hypothesis in rounds of 256: Philox, three picks,
//                 Horn and the Jacobi sweeps in the lane's registers, then the score with the twelve pose entries in registers
//                 and the points by 16-byte LDS reads at one address for all lanes (a broadcast), no barrier inside a round;
//                 (3) arg-max of (count, lowest slot) by wave then workgroup;  (4) the refit: fit_centroids and fit_pose of
//                 slhip_fit_block.h over the valid list, the pair source "entry i, if an inlier of the current pose";
//                 (5) the final pass over the correspondences in their own order: ballot words, count, rms
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_align_rules.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fit_block.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_align_params) == 64, "slhip_pose_align_params layout");

using Params = slhip_pose_align_params;
using Out = slhip_pose_align_out;
namespace al = slhip_align;
namespace ft = slhip_fit;

constexpr uint32_t BLOCK = al::BLOCK;
constexpr uint32_t NWAVES = BLOCK / al::WAVE;
constexpr uint32_t PLANES = 6u;      // sx sy sz dx dy dz, each k_pad floats

using slhip_pose::pad4;
using slhip_pose::words_of;

// INSUFFICIENT / NO_MODEL: a NaN pose, 0 inliers, NaN rms, best -2, zero bits (lane 0, and the words by all lanes)
__device__ void write_none(const Params& p, const Out& out, uint32_t set, int flags)
{
    const uint32_t m = p.outputs, nw = words_of(p.n_points);
    if (m & SLHIP_ALIGN_OUT_INLIERS)
        for (uint32_t w = threadIdx.x; w < nw; w += BLOCK) out.inliers[(size_t)set * nw + w] = 0u;
    if (threadIdx.x) return;
    if (m & SLHIP_ALIGN_OUT_POSE)
        for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = __builtin_nanf("");
    if (m & SLHIP_ALIGN_OUT_N_INLIERS) out.n_inliers[set] = 0;
    if (m & SLHIP_ALIGN_OUT_RMS) out.rms[set] = __builtin_nanf("");
    if (m & SLHIP_ALIGN_OUT_BEST) out.best[set] = -2;
    if (m & SLHIP_ALIGN_OUT_FLAGS) out.flags[set] = flags;
}

// the score of one pose in registers against the n valid pairs: four per 16-byte read of each plane, then the ragged rest
__device__ __forceinline__ uint32_t score(const float* M, float thr2, const float* s_sx, const float* s_sy, const float* s_sz,
                                          const float* s_dx, const float* s_dy, const float* s_dz, uint32_t n)
{
    uint32_t count = 0u;
    float e2;
    const uint32_t whole = n & ~3u;
    // as k_pose_pnp's walk: unrolled further the reads of several rounds pile up in registers.  The loop vectoriser is kept off
    // both loops (-fno-slp-vectorize does not reach it): it packs the four tests into v_pk_* pairs, which the build avoids, and
    // widened the ragged rest by 16, which took 246 VGPRs against 105
#pragma clang loop vectorize(disable) interleave(disable)
#pragma unroll 1
    for (uint32_t j = 0u; j < whole; j += 4u) {
        const float4 SX = *reinterpret_cast<const float4*>(s_sx + j), SY = *reinterpret_cast<const float4*>(s_sy + j);
        const float4 SZ = *reinterpret_cast<const float4*>(s_sz + j), DX = *reinterpret_cast<const float4*>(s_dx + j);
        const float4 DY = *reinterpret_cast<const float4*>(s_dy + j), DZ = *reinterpret_cast<const float4*>(s_dz + j);
        count += al::inlier(M, SX.x, SY.x, SZ.x, DX.x, DY.x, DZ.x, thr2, &e2) ? 1u : 0u;
        count += al::inlier(M, SX.y, SY.y, SZ.y, DX.y, DY.y, DZ.y, thr2, &e2) ? 1u : 0u;
        count += al::inlier(M, SX.z, SY.z, SZ.z, DX.z, DY.z, DZ.z, thr2, &e2) ? 1u : 0u;
        count += al::inlier(M, SX.w, SY.w, SZ.w, DX.w, DY.w, DZ.w, thr2, &e2) ? 1u : 0u;
    }
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)      // at most three rounds
    for (uint32_t j = whole; j < n; ++j) count += al::inlier(M, s_sx[j], s_sy[j], s_sz[j], s_dx[j], s_dy[j], s_dz[j], thr2, &e2) ? 1u : 0u;
    return count;
}

// One block per set.  Dynamic LDS: PLANES * k_pad floats, k_pad = K rounded up to 4.
__global__ __launch_bounds__(BLOCK) void k_pose_align(Params p, const float4* __restrict__ src, const float4* __restrict__ dst,
                                                      const float* __restrict__ init, Out out, uint32_t k_pad)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    __shared__ uint32_t s_cnt[NWAVES];
    __shared__ uint32_t s_key[NWAVES];
    __shared__ float s_pose[12];
    __shared__ float s_part[NWAVES * ft::FIT_SUMS];
    float* s_sx = s_all;
    float* s_sy = s_sx + k_pad;
    float* s_sz = s_sy + k_pad;
    float* s_dx = s_sz + k_pad;
    float* s_dy = s_dx + k_pad;
    float* s_dz = s_dy + k_pad;

    const uint32_t tid = threadIdx.x, wave = tid / al::WAVE, lane = tid % al::WAVE;
    const uint32_t set = blockIdx.x, K = p.n_points, Hy = p.n_hypotheses, mask = p.outputs;
    const float thr2 = p.threshold * p.threshold;
    const float4* my_src = src + (size_t)set * K;
    const float4* my_dst = dst + (size_t)set * K;

    // correspondence j of the set in its own order, from global memory; false when it does not count
    auto row = [&](uint32_t j, float* s, float* d) {
        const float4 a = my_src[j], b = my_dst[j];
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
        d[0] = b.x; d[1] = b.y; d[2] = b.z; d[3] = b.w;
        return ft::used(s, d);
    };

    // (1) the valid list: ranks by ballot inside a wave, the waves' counts through LDS
    uint32_t n_valid = 0u;
    for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
        const uint32_t j = j0 + tid;
        float s[4], d[4];
        const bool ok = j < K && row(j, s, d);
        const unsigned long long votes = __ballot(ok);
        if (lane == 0u) s_cnt[wave] = (uint32_t)__popcll(votes);
        __syncthreads();
        uint32_t at = n_valid + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        for (uint32_t w = 0u; w < NWAVES; ++w) {
            at += w < wave ? s_cnt[w] : 0u;
            n_valid += s_cnt[w];
        }
        if (ok) {      // at < n_valid <= K <= k_pad
            s_sx[at] = s[0]; s_sy[at] = s[1]; s_sz[at] = s[2];
            s_dx[at] = d[0]; s_dy[at] = d[1]; s_dz[at] = d[2];
        }
        __syncthreads();
    }
    if (n_valid < 3u) {      // the same for every lane
        write_none(p, out, set, SLHIP_ALIGN_INSUFFICIENT);
        return;
    }

    // (2) a lane per hypothesis; slot 0 is the caller's pose, slot h + 1 hypothesis h
    auto pick = [&](uint32_t i, float* s, float* d) {      // i < n_valid
        s[0] = s_sx[i]; s[1] = s_sy[i]; s[2] = s_sz[i];
        d[0] = s_dx[i]; d[1] = s_dy[i]; d[2] = s_dz[i];
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
            have = al::pose_finite(M);
        } else if (slot <= Hy) {
            have = al::hypothesis(p.seed_lo, p.seed_hi, p.set_id_base + set, slot - 1u, n_valid, p.min_gap, pick, M);
        }
        if (!have) {
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = __builtin_nanf("");      // counts nothing
        }
        uint32_t count = 0u;
        if (__ballot(have)) count = score(M, thr2, s_sx, s_sy, s_sz, s_dx, s_dy, s_dz, n_valid);      // a wave without a pose skips the walk
        const uint32_t key = slot <= Hy ? al::key_of(count, slot) : 0u;
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
    const uint32_t win_count = al::key_count(win);
    if (win == 0u || win_count < p.min_inliers) {
        write_none(p, out, set, SLHIP_ALIGN_NO_MODEL);
        return;
    }
    float W[12], M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) W[i] = M[i] = s_pose[i];
    int flags = 0;

    // (4) the rigid fit of the inliers of the current pose among the valid list: lane l takes entries l, l + 256, ...
    auto pair = [&](uint32_t i, float* s, float* d) {
        pick(i, s, d);
        s[3] = d[3] = 1.0f;
        float e2;
        return al::inlier(M, s[0], s[1], s[2], d[0], d[1], d[2], thr2, &e2);
    };
    for (uint32_t it = 0u; it < p.refine_iters; ++it) {
        float S[6], N[12];
        const uint32_t mine = ft::fit_centroids(n_valid, pair, s_part, S);
        const uint32_t n_in = slhip_pose::block_count(mine, s_cnt, wave, lane);
        __syncthreads();      // s_cnt is written again by the final pass, which may come next
        if (n_in < 3u || !ft::fit_pose(n_valid, pair, S, n_in, p.min_gap, s_part, N)) {      // the same for every lane
            flags |= SLHIP_ALIGN_REFINE_STOPPED;
            break;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = N[i];
    }

    // (5) inliers, count and rms of the refitted pose over the correspondences in their own order; should it hold fewer
    // inliers than the winner, the same of the winner's pose
    const uint32_t nw = words_of(K);
    for (int pass = 0; pass < 2; ++pass) {
        float acc = 0.0f;
        uint32_t mine = 0u;      // lane 0 of a wave: the wave's count
        for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
            const uint32_t j = j0 + tid;
            bool in = false;
            if (j < K) {
                float s[4], d[4], e2;
                in = row(j, s, d) && al::inlier(M, s[0], s[1], s[2], d[0], d[1], d[2], thr2, &e2);
                if (in) acc = acc + e2;
            }
            const unsigned long long votes = __ballot(in);
            mine += (uint32_t)__popcll(votes);
            if (lane == 0u && (mask & SLHIP_ALIGN_OUT_INLIERS)) {
                const uint32_t w0 = (j0 + wave * al::WAVE) / 32u;
                if (w0 < nw) out.inliers[(size_t)set * nw + w0] = (uint32_t)votes;
                if (w0 + 1u < nw) out.inliers[(size_t)set * nw + w0 + 1u] = (uint32_t)(votes >> 32);
            }
        }
        // (the count is read between the barriers of its own: the next pass writes s_cnt with no barrier in front)
        const float w = slhip_pose::wave_sum(acc);
        if (lane == 0u) {
            s_part[wave * ft::FIT_SUMS] = w;
            s_cnt[wave] = mine;
        }
        __syncthreads();
        const uint32_t count = slhip_pose::waves_sum(s_cnt);
        const float sum = slhip_pose::waves_sum(s_part, (uint32_t)ft::FIT_SUMS);
        __syncthreads();
        if (pass == 0 && count < win_count) {      // the same for every lane; only a refitted pose can get here
            flags |= SLHIP_ALIGN_REFINE_REJECTED;
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = W[i];
            continue;
        }
        if (tid == 0u) {
            if (mask & SLHIP_ALIGN_OUT_POSE)
                for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = M[i];
            if (mask & SLHIP_ALIGN_OUT_N_INLIERS) out.n_inliers[set] = (int32_t)count;
            if (mask & SLHIP_ALIGN_OUT_RMS) out.rms[set] = sqrtf(sum / (float)count);
            if (mask & SLHIP_ALIGN_OUT_BEST) out.best[set] = al::key_best(win);
            if (mask & SLHIP_ALIGN_OUT_FLAGS) out.flags[set] = flags;
        }
        break;
    }
}

constexpr uint32_t ALL_OUTPUTS = SLHIP_ALIGN_OUT_POSE | SLHIP_ALIGN_OUT_N_INLIERS | SLHIP_ALIGN_OUT_RMS | SLHIP_ALIGN_OUT_INLIERS |
                                 SLHIP_ALIGN_OUT_BEST | SLHIP_ALIGN_OUT_FLAGS;

// the checks that slhip_pose_align and slhip_pose_align_host share
int check_call(const char* who, const Params* params, const float* src, const float* dst, const float* init, const Out* out)
{
    if (const int st = slhip_pose_align_check_params(params)) return st;
    if (!src || !dst || !out) {
        slhip::set_error("%s: null argument (src, dst and the output record are required)", who);
        return -1;
    }
    if (params->n_hypotheses == 0u && !init) {
        slhip::set_error("%s: n_hypotheses 0 needs an initial pose (a pure refit); without one there is nothing to score", who);
        return -1;
    }
    const slhip::OutputList outputs = {{SLHIP_ALIGN_OUT_POSE, out->pose},       {SLHIP_ALIGN_OUT_N_INLIERS, out->n_inliers},
                                       {SLHIP_ALIGN_OUT_RMS, out->rms},         {SLHIP_ALIGN_OUT_INLIERS, out->inliers},
                                       {SLHIP_ALIGN_OUT_BEST, out->best},       {SLHIP_ALIGN_OUT_FLAGS, out->flags}};
    if (const int st = slhip::check_outputs_present(who, params->outputs, outputs)) return st;
    if (((uintptr_t)src & 15u) || ((uintptr_t)dst & 15u) || ((uintptr_t)init & 3u)) {
        slhip::set_error("%s: src and dst must be 16-byte aligned, the initial poses 4-byte", who);
        return -1;
    }
    return slhip::check_outputs_aligned(who, params->outputs, outputs);
}

// optional HIP-event timing (tools/time_pose_align.py): events round the last call
slhip::StepTimer<1> g_timer;

}  // namespace

extern "C" int slhip_pose_align_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_pose_align_timings(float ms_out[1]) { return g_timer.read_for("slhip_pose_align_timings", ms_out); }

extern "C" int slhip_pose_align_check_params(const slhip_pose_align_params* p)
{
    static const char* who = "slhip_pose_align";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 3u, SLHIP_ALIGN_POINTS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_hypotheses", p->n_hypotheses, 0u, SLHIP_ALIGN_HYPOTHESES_MAX)) return st;
    if (!(p->threshold > 0.0f) || !slhip::is_finite(p->threshold)) {
        slhip::set_error("%s: threshold %g must be positive and finite", who, (double)p->threshold);
        return -1;
    }
    if (const int st = slhip::check_min_gap(who, p->min_gap)) return st;
    if (const int st = slhip::check_range(who, "refine_iters", p->refine_iters, 0u, SLHIP_ALIGN_REFINE_MAX)) return st;
    if (const int st = slhip::check_range(who, "min_inliers", p->min_inliers, 3u, 0x7fffffffu)) return st;
    if (p->outputs == 0u || (p->outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of pose 1, n_inliers 2, rms 4, inliers 8, best 16, flags 32 and nothing else",
                         who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_pose_align(const slhip_pose_align_params* params, const float* d_src, const float* d_dst, const float* d_init,
                                const slhip_pose_align_out* out, void* stream_)
{
    static const char* who = "slhip_pose_align";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_src, d_dst, d_init, out)) return st;
    if (params->n_sets == 0u) return 0;
    const uint32_t k_pad = pad4(params->n_points);
    const size_t lds = (size_t)PLANES * k_pad * sizeof(float);      // 6 KiB at K = 256, 24 KiB at 1024, 96 KiB at 4096
    if (lds > 64u * 1024u)      // more than a kernel may ask for without the attribute (per device, so not remembered)
        SLHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_align), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (const int st = g_timer.begin(0, stream)) return st;
    k_pose_align<<<params->n_sets, BLOCK, lds, stream>>>(*params, reinterpret_cast<const float4*>(d_src),
                                                         reinterpret_cast<const float4*>(d_dst), d_init, *out, k_pad);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

extern "C" int slhip_pose_align_host(const slhip_pose_align_params* params, const float* h_src, const float* h_dst, const float* h_init,
                                     const slhip_pose_align_out* out)
{
    static const char* who = "slhip_pose_align_host";
    if (const int st = check_call(who, params, h_src, h_dst, h_init, out)) return st;
    const Params& p = *params;
    const uint32_t K = p.n_points, Hy = p.n_hypotheses, mask = p.outputs, nw = words_of(K);
    const float thr2 = p.threshold * p.threshold, nan = __builtin_nanf("");
    std::vector<float> list((size_t)K * 6u);
    std::vector<uint32_t> bits(nw);
    for (uint32_t set = 0u; set < p.n_sets; ++set) {
        const float* src = h_src + (size_t)set * K * 4u;
        const float* dst = h_dst + (size_t)set * K * 4u;
        auto none = [&](int flags) {
            if (mask & SLHIP_ALIGN_OUT_INLIERS)
                for (uint32_t w = 0u; w < nw; ++w) out->inliers[(size_t)set * nw + w] = 0u;
            if (mask & SLHIP_ALIGN_OUT_POSE)
                for (int i = 0; i < 12; ++i) out->pose[(size_t)set * 12u + i] = nan;
            if (mask & SLHIP_ALIGN_OUT_N_INLIERS) out->n_inliers[set] = 0;
            if (mask & SLHIP_ALIGN_OUT_RMS) out->rms[set] = nan;
            if (mask & SLHIP_ALIGN_OUT_BEST) out->best[set] = -2;
            if (mask & SLHIP_ALIGN_OUT_FLAGS) out->flags[set] = flags;
        };
        uint32_t n_valid = 0u;
        for (uint32_t j = 0u; j < K; ++j)
            if (ft::used(src + 4u * j, dst + 4u * j)) {
                float* c = &list[(size_t)n_valid++ * 6u];
                for (int k = 0; k < 3; ++k) {
                    c[k] = src[4u * j + k];
                    c[3 + k] = dst[4u * j + k];
                }
            }
        if (n_valid < 3u) {
            none(SLHIP_ALIGN_INSUFFICIENT);
            continue;
        }
        auto pick = [&](uint32_t i, float* s, float* d) {
            for (int k = 0; k < 3; ++k) {
                s[k] = list[(size_t)i * 6u + k];
                d[k] = list[(size_t)i * 6u + 3u + k];
            }
        };
        uint32_t win = 0u;
        float W[12] = {}, M[12];
        for (uint32_t slot = h_init ? 0u : 1u; slot <= Hy; ++slot) {
            bool have = false;
            if (slot == 0u) {
                for (int i = 0; i < 12; ++i) M[i] = h_init[(size_t)set * 12u + i];
                have = al::pose_finite(M);
            } else {
                have = al::hypothesis(p.seed_lo, p.seed_hi, p.set_id_base + set, slot - 1u, n_valid, p.min_gap, pick, M);
            }
            uint32_t count = 0u;
            float e2;
            if (have)
                for (uint32_t i = 0u; i < n_valid; ++i) {
                    const float* c = &list[(size_t)i * 6u];
                    count += al::inlier(M, c[0], c[1], c[2], c[3], c[4], c[5], thr2, &e2) ? 1u : 0u;
                }
            const uint32_t key = al::key_of(count, slot);
            if (key > win) {
                win = key;
                for (int i = 0; i < 12; ++i) W[i] = have ? M[i] : nan;
            }
        }
        const uint32_t win_count = al::key_count(win);
        if (win == 0u || win_count < p.min_inliers) {
            none(SLHIP_ALIGN_NO_MODEL);
            continue;
        }
        for (int i = 0; i < 12; ++i) M[i] = W[i];
        int flags = 0;
        auto pair = [&](uint32_t i, float* s, float* d) {
            pick(i, s, d);
            s[3] = d[3] = 1.0f;
            float e2;
            return al::inlier(M, s[0], s[1], s[2], d[0], d[1], d[2], thr2, &e2);
        };
        for (uint32_t it = 0u; it < p.refine_iters; ++it) {
            float S[6], N[12];
            const uint32_t n_in = ft::fit_centroids_host(n_valid, pair, S);
            if (n_in < 3u || !ft::fit_pose_host(n_valid, pair, S, n_in, p.min_gap, N)) {
                flags |= SLHIP_ALIGN_REFINE_STOPPED;
                break;
            }
            for (int i = 0; i < 12; ++i) M[i] = N[i];
        }
        for (int pass = 0; pass < 2; ++pass) {
            slhip_pose::LaneSums<1> sums;
            uint32_t count = 0u;
            for (uint32_t w = 0u; w < nw; ++w) bits[w] = 0u;
            for (uint32_t j = 0u; j < K; ++j) {
                const float* s = src + 4u * j;
                const float* d = dst + 4u * j;
                float e2;
                if (!ft::used(s, d) || !al::inlier(M, s[0], s[1], s[2], d[0], d[1], d[2], thr2, &e2)) continue;
                sums.add(j, [&](float* acc) { acc[0] = acc[0] + e2; });
                bits[j >> 5] |= 1u << (j & 31u);
                ++count;
            }
            if (pass == 0 && count < win_count) {
                flags |= SLHIP_ALIGN_REFINE_REJECTED;
                for (int i = 0; i < 12; ++i) M[i] = W[i];
                continue;
            }
            if (mask & SLHIP_ALIGN_OUT_INLIERS)
                for (uint32_t w = 0u; w < nw; ++w) out->inliers[(size_t)set * nw + w] = bits[w];
            if (mask & SLHIP_ALIGN_OUT_POSE)
                for (int i = 0; i < 12; ++i) out->pose[(size_t)set * 12u + i] = M[i];
            if (mask & SLHIP_ALIGN_OUT_N_INLIERS) out->n_inliers[set] = (int32_t)count;
            if (mask & SLHIP_ALIGN_OUT_RMS) out->rms[set] = sqrtf(sums.total(0) / (float)count);
            if (mask & SLHIP_ALIGN_OUT_BEST) out->best[set] = al::key_best(win);
            if (mask & SLHIP_ALIGN_OUT_FLAGS) out->flags[set] = flags;
            break;
        }
    }
    return 0;
}
