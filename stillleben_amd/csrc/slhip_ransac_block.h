// slhip_ransac_block.h -- the RANSAC workgroup of slhip_pose_pnp.hip and slhip_pose_align.hip and its host restatement, side by
// side: one workgroup of 256 lanes per set on the device, one loop per set on the host, the same five steps (DESIGN.md "The
// RANSAC workgroup"):
//   (1) the valid correspondences, in ascending order, into PLANES LDS planes of k_pad floats by ballot ranks;
//   (2) a lane per hypothesis in rounds of 256, slot 0 the caller's pose, slot h + 1 hypothesis h: the minimal solver in the
//       lane's registers, then the score with the twelve pose entries in registers and the list by 16-byte LDS reads at one
//       address for all lanes (a broadcast), no barrier inside a round;
//   (3) the arg-max of (count, lowest slot) by wave, then by workgroup (slhip_ransac_rules.h);
//   (4) the refinement steps of the problem, until one stops;
//   (5) the final pass over the correspondences in their own order: ballot words, count, rms; a refined pose that holds fewer
//       inliers than the winner gives way to the winner.
// The two modules differ in the *problem* they hand in, a small class with
//   PLANES, MIN_VALID, PART_STRIDE   the floats of a list entry, the fewest valid entries, the row stride of s_part
//   bool load(j, row)                correspondence j of the set in its own order as row[PLANES]; false when it does not count
//   bool hypothesis(h, n_valid, pick, M)   the pose of hypothesis h; pick(i, row) hands out entry i < n_valid of the list
//   bool inlier(M, row, &e2)         the inlier test of one entry and its squared residual
//   bool refine(n_valid, pick, s_part, s_cnt, M)   device: one refinement step over the list; all lanes call it together, it
//                                    holds barriers and leaves none owed; false when the refinement stops (M is then unchanged)
//   bool refine(n_valid, pick, M)    host: the same step by LaneSums or the fit_*_host passes
// load, hypothesis and inlier are the same functions on host and device.  Every sum is a sum of slhip_block_sum.h.  The output
// bits, the flag values and the fields of the output record are those of both modules (each ties its public names to the ones
// here by static_assert); `Params` is the module's parameter record, of which n_points, n_hypotheses, refine_iters, min_inliers
// and outputs are read.
#pragma once

#include <stdint.h>

#include <array>
#include <vector>

#include "slhip_block_sum.h"
#include "slhip_checks.h"
#include "slhip_ransac_rules.h"

namespace slhip_ransac {

constexpr uint32_t OUT_POSE = 1u, OUT_N_INLIERS = 2u, OUT_RMS = 4u, OUT_INLIERS = 8u, OUT_BEST = 16u, OUT_FLAGS = 32u;
constexpr uint32_t ALL_OUTPUTS = OUT_POSE | OUT_N_INLIERS | OUT_RMS | OUT_INLIERS | OUT_BEST | OUT_FLAGS;
constexpr int INSUFFICIENT = 1, NO_MODEL = 2, REFINE_STOPPED = 4, REFINE_REJECTED = 8;

using slhip_pose::BLOCK;
using slhip_pose::WAVE;
using slhip_pose::words_of;
constexpr uint32_t NWAVES = BLOCK / WAVE;

// ---- the checks of the entries ------------------------------------------------------------------------------------------------
// slhip_*_check_params, first part: the sizes and the threshold (`threshold_name` is the field's name in the module's record)
inline int check_sizes(const char* who, uint32_t n_sets, uint32_t n_points, uint32_t min_points, uint32_t points_max,
                       uint32_t n_hypotheses, uint32_t hypotheses_max, const char* threshold_name, float threshold)
{
    if (const int st = slhip::check_range(who, "n_sets", n_sets, 0u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_points", n_points, min_points, points_max)) return st;
    if (const int st = slhip::check_range(who, "n_hypotheses", n_hypotheses, 0u, hypotheses_max)) return st;
    if (!(threshold > 0.0f) || !slhip::is_finite(threshold)) {
        slhip::set_error("%s: %s %g must be positive and finite", who, threshold_name, (double)threshold);
        return -1;
    }
    return 0;
}

// slhip_*_check_params, last part
inline int check_refine_and_outputs(const char* who, uint32_t refine_iters, uint32_t refine_max, uint32_t min_inliers,
                                    uint32_t min_points, uint32_t outputs)
{
    if (const int st = slhip::check_range(who, "refine_iters", refine_iters, 0u, refine_max)) return st;
    if (const int st = slhip::check_range(who, "min_inliers", min_inliers, min_points, 0x7fffffffu)) return st;
    if (outputs == 0u || (outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of pose 1, n_inliers 2, rms 4, inliers 8, best 16, flags 32 and nothing else",
                         who, outputs);
        return -1;
    }
    return 0;
}

// the output record as the list that slhip::check_outputs_present and slhip::check_outputs_aligned take
template <class Out>
std::array<slhip::NamedOutput, 6> output_list(const Out* out)
{
    return {{{OUT_POSE, out->pose}, {OUT_N_INLIERS, out->n_inliers}, {OUT_RMS, out->rms},
             {OUT_INLIERS, out->inliers}, {OUT_BEST, out->best}, {OUT_FLAGS, out->flags}}};
}

// ---- the host twin ------------------------------------------------------------------------------------------------------------
// INSUFFICIENT / NO_MODEL: a NaN pose, 0 inliers, NaN rms, best -2, zero bits
template <class Out>
void none_host(uint32_t mask, uint32_t nw, const Out& out, uint32_t set, int flags)
{
    const float nan = __builtin_nanf("");
    if (mask & OUT_INLIERS)
        for (uint32_t w = 0u; w < nw; ++w) out.inliers[(size_t)set * nw + w] = 0u;
    if (mask & OUT_POSE)
        for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = nan;
    if (mask & OUT_N_INLIERS) out.n_inliers[set] = 0;
    if (mask & OUT_RMS) out.rms[set] = nan;
    if (mask & OUT_BEST) out.best[set] = -2;
    if (mask & OUT_FLAGS) out.flags[set] = flags;
}

// One set on the host.  `list`: room for K * PLANES floats, `bits` for words_of(K) words.
template <class Problem, class Params, class Out>
void solve_set_host(const Problem& prob, const Params& p, const float* init, const Out& out, uint32_t set, float* list, uint32_t* bits)
{
    constexpr uint32_t PLANES = Problem::PLANES;
    const uint32_t K = p.n_points, Hy = p.n_hypotheses, mask = p.outputs, nw = words_of(K);
    const float nan = __builtin_nanf("");
    float row[PLANES], e2;

    // (1)
    uint32_t n_valid = 0u;
    for (uint32_t j = 0u; j < K; ++j)
        if (prob.load(j, row)) {
            for (uint32_t k = 0u; k < PLANES; ++k) list[(size_t)n_valid * PLANES + k] = row[k];
            ++n_valid;
        }
    if (n_valid < Problem::MIN_VALID) return none_host(mask, nw, out, set, INSUFFICIENT);
    auto pick = [&](uint32_t i, float* c) {
        for (uint32_t k = 0u; k < PLANES; ++k) c[k] = list[(size_t)i * PLANES + k];
    };

    // (2) and (3)
    uint32_t win = 0u;
    float W[12] = {}, M[12];
    for (uint32_t slot = init ? 0u : 1u; slot <= Hy; ++slot) {
        bool have = false;
        if (slot == 0u) {
            for (int i = 0; i < 12; ++i) M[i] = init[(size_t)set * 12u + i];
            have = pose_finite(M);
        } else {
            have = prob.hypothesis(slot - 1u, n_valid, pick, M);
        }
        uint32_t count = 0u;
        if (have)
            for (uint32_t i = 0u; i < n_valid; ++i) count += prob.inlier(M, &list[(size_t)i * PLANES], &e2) ? 1u : 0u;
        const uint32_t key = key_of(count, slot);
        if (key > win) {
            win = key;
            for (int i = 0; i < 12; ++i) W[i] = have ? M[i] : nan;
        }
    }
    const uint32_t win_count = key_count(win);
    if (win == 0u || win_count < p.min_inliers) return none_host(mask, nw, out, set, NO_MODEL);
    for (int i = 0; i < 12; ++i) M[i] = W[i];
    int flags = 0;

    // (4)
    for (uint32_t it = 0u; it < p.refine_iters; ++it)
        if (!prob.refine(n_valid, pick, M)) {
            flags |= REFINE_STOPPED;
            break;
        }

    // (5)
    for (int pass = 0; pass < 2; ++pass) {
        slhip_pose::LaneSums<1> sums;
        uint32_t count = 0u;
        for (uint32_t w = 0u; w < nw; ++w) bits[w] = 0u;
        for (uint32_t j = 0u; j < K; ++j) {
            if (!prob.load(j, row) || !prob.inlier(M, row, &e2)) continue;
            sums.add(j, [&](float* acc) { acc[0] = acc[0] + e2; });
            bits[j >> 5] |= 1u << (j & 31u);
            ++count;
        }
        if (pass == 0 && count < win_count) {      // only a refined pose can get here
            flags |= REFINE_REJECTED;
            for (int i = 0; i < 12; ++i) M[i] = W[i];
            continue;
        }
        if (mask & OUT_INLIERS)
            for (uint32_t w = 0u; w < nw; ++w) out.inliers[(size_t)set * nw + w] = bits[w];
        if (mask & OUT_POSE)
            for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = M[i];
        if (mask & OUT_N_INLIERS) out.n_inliers[set] = (int32_t)count;
        if (mask & OUT_RMS) out.rms[set] = sqrtf(sums.total(0) / (float)count);
        if (mask & OUT_BEST) out.best[set] = key_best(win);
        if (mask & OUT_FLAGS) out.flags[set] = flags;
        break;
    }
}

// every set on the host; a set's problem is Problem(p, inputs..., set)
template <class Problem, class Params, class Out, class... Inputs>
void solve_host(const Params& p, const float* init, const Out& out, Inputs... inputs)
{
    std::vector<float> list((size_t)p.n_points * Problem::PLANES);
    std::vector<uint32_t> bits(words_of(p.n_points));
    for (uint32_t set = 0u; set < p.n_sets; ++set)
        solve_set_host(Problem(p, inputs..., set), p, init, out, set, list.data(), bits.data());
}

#ifdef __HIPCC__

// the kernel's dynamic LDS for K points, and its launch's leave to use it: more than 64 KiB needs the attribute (per device, so
// not remembered)
template <class Kernel>
hipError_t reserve_lds(Kernel kernel, uint32_t planes, uint32_t k_pad, size_t* lds)
{
    *lds = (size_t)planes * k_pad * sizeof(float);
    if (*lds <= 64u * 1024u) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)*lds);
}

// INSUFFICIENT / NO_MODEL: a NaN pose, 0 inliers, NaN rms, best -2, zero bits (lane 0, and the words by all lanes)
template <class Out>
__device__ void write_none(uint32_t mask, uint32_t nw, const Out& out, uint32_t set, int flags)
{
    if (mask & OUT_INLIERS)
        for (uint32_t w = threadIdx.x; w < nw; w += BLOCK) out.inliers[(size_t)set * nw + w] = 0u;
    if (threadIdx.x) return;
    if (mask & OUT_POSE)
        for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = __builtin_nanf("");
    if (mask & OUT_N_INLIERS) out.n_inliers[set] = 0;
    if (mask & OUT_RMS) out.rms[set] = __builtin_nanf("");
    if (mask & OUT_BEST) out.best[set] = -2;
    if (mask & OUT_FLAGS) out.flags[set] = flags;
}

// the score of one pose in registers against the n entries of the list: four per 16-byte read of each plane, then the ragged rest
template <class Problem>
__device__ __forceinline__ uint32_t score(const Problem& prob, const float* M, const float* s_list, uint32_t k_pad, uint32_t n)
{
    constexpr uint32_t PLANES = Problem::PLANES;
    uint32_t count = 0u;
    float e2, r[PLANES];
    const uint32_t whole = n & ~3u;
    // unrolled further the reads of several rounds pile up in registers.  The loop vectoriser is kept off both loops
    // (-fno-slp-vectorize does not reach it): it packs the four tests into v_pk_* pairs, which the build avoids, and widened the
    // ragged rest by 16, which took 246 VGPRs against 105 in k_pose_align
    // the loop starts near the head of a 64-byte line of code: at K = 4096 a workgroup has a compute unit to itself, one wave per
    // SIMD, and k_pose_align's 592-byte loop took 1 % longer from byte 60 of a line (eleven lines) than from byte 16 (ten);
    // profiles/r23 has the three builds timed side by side
    asm volatile(".p2align 6");
#pragma clang loop vectorize(disable) interleave(disable)
#pragma unroll 1
    for (uint32_t j = 0u; j < whole; j += 4u) {
        float4 P[PLANES];
#pragma unroll
        for (uint32_t k = 0u; k < PLANES; ++k) P[k] = *reinterpret_cast<const float4*>(s_list + k * k_pad + j);
#pragma unroll
        for (uint32_t k = 0u; k < PLANES; ++k) r[k] = P[k].x;
        count += prob.inlier(M, r, &e2) ? 1u : 0u;
#pragma unroll
        for (uint32_t k = 0u; k < PLANES; ++k) r[k] = P[k].y;
        count += prob.inlier(M, r, &e2) ? 1u : 0u;
#pragma unroll
        for (uint32_t k = 0u; k < PLANES; ++k) r[k] = P[k].z;
        count += prob.inlier(M, r, &e2) ? 1u : 0u;
#pragma unroll
        for (uint32_t k = 0u; k < PLANES; ++k) r[k] = P[k].w;
        count += prob.inlier(M, r, &e2) ? 1u : 0u;
    }
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)      // at most three rounds
    for (uint32_t j = whole; j < n; ++j) {
#pragma unroll
        for (uint32_t k = 0u; k < PLANES; ++k) r[k] = s_list[k * k_pad + j];
        count += prob.inlier(M, r, &e2) ? 1u : 0u;
    }
    return count;
}

// One workgroup of BLOCK lanes per set.  s_list: PLANES * k_pad floats of dynamic LDS, 16-byte aligned, k_pad = pad4(K).
template <class Problem, class Params, class Out>
__device__ __forceinline__ void solve_set(const Problem& prob, const Params& p, const float* __restrict__ init, const Out& out,
                                          uint32_t set, float* s_list, uint32_t k_pad)
{
    constexpr uint32_t PLANES = Problem::PLANES;
    constexpr uint32_t PART_STRIDE = Problem::PART_STRIDE;
    __shared__ uint32_t s_cnt[NWAVES];
    __shared__ uint32_t s_key[NWAVES];
    __shared__ float s_pose[12];
    __shared__ float s_part[NWAVES * PART_STRIDE];

    const uint32_t tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const uint32_t K = p.n_points, Hy = p.n_hypotheses, mask = p.outputs, nw = words_of(K);

    // (1) the valid list: ranks by ballot inside a wave, the waves' counts through LDS
    uint32_t n_valid = 0u;
    for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
        const uint32_t j = j0 + tid;
        float row[PLANES];
        const bool ok = j < K && prob.load(j, row);
        const unsigned long long votes = __ballot(ok);
        if (lane == 0u) s_cnt[wave] = (uint32_t)__popcll(votes);
        __syncthreads();
        uint32_t at = n_valid + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        for (uint32_t w = 0u; w < NWAVES; ++w) {
            at += w < wave ? s_cnt[w] : 0u;
            n_valid += s_cnt[w];
        }
        if (ok) {      // at < n_valid <= K <= k_pad
#pragma unroll
            for (uint32_t k = 0u; k < PLANES; ++k) s_list[k * k_pad + at] = row[k];
        }
        __syncthreads();
    }
    if (n_valid < Problem::MIN_VALID) {      // the same for every lane
        write_none(mask, nw, out, set, INSUFFICIENT);
        return;
    }

    // (2) a lane per hypothesis; slot 0 is the caller's pose, slot h + 1 hypothesis h
    auto pick = [&](uint32_t i, float* c) {      // i < n_valid
#pragma unroll
        for (uint32_t k = 0u; k < PLANES; ++k) c[k] = s_list[k * k_pad + i];
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
            have = pose_finite(M);
        } else if (slot <= Hy) {
            have = prob.hypothesis(slot - 1u, n_valid, pick, M);
        }
        if (!have) {
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = __builtin_nanf("");      // counts nothing
        }
        uint32_t count = 0u;
        if (__ballot(have)) count = score(prob, M, s_list, k_pad, n_valid);      // a wave without a pose skips the walk
        const uint32_t key = slot <= Hy ? key_of(count, slot) : 0u;
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
    const uint32_t win_count = key_count(win);
    if (win == 0u || win_count < p.min_inliers) {
        write_none(mask, nw, out, set, NO_MODEL);
        return;
    }
    float W[12], M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) W[i] = M[i] = s_pose[i];
    int flags = 0;

    // (4) the problem's refinement on the inliers of the current pose among the valid list
    for (uint32_t it = 0u; it < p.refine_iters; ++it)
        if (!prob.refine(n_valid, pick, s_part, s_cnt, M)) {      // the same for every lane
            flags |= REFINE_STOPPED;
            break;
        }

    // (5) inliers, count and rms of the refined pose over the correspondences in their own order; should it hold fewer
    // inliers than the winner, the same of the winner's pose
    for (int pass = 0; pass < 2; ++pass) {
        float acc = 0.0f;
        uint32_t mine = 0u;      // lane 0 of a wave: the wave's count
        for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
            const uint32_t j = j0 + tid;
            bool in = false;
            if (j < K) {
                float row[PLANES], e2;
                in = prob.load(j, row) && prob.inlier(M, row, &e2);
                if (in) acc = acc + e2;
            }
            const unsigned long long votes = __ballot(in);
            mine += (uint32_t)__popcll(votes);
            if (lane == 0u && (mask & OUT_INLIERS)) {
                const uint32_t w0 = (j0 + wave * WAVE) / 32u;
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
            flags |= REFINE_REJECTED;
#pragma unroll
            for (int i = 0; i < 12; ++i) M[i] = W[i];
            continue;
        }
        if (tid == 0u) {
            if (mask & OUT_POSE)
                for (int i = 0; i < 12; ++i) out.pose[(size_t)set * 12u + i] = M[i];
            if (mask & OUT_N_INLIERS) out.n_inliers[set] = (int32_t)count;
            if (mask & OUT_RMS) out.rms[set] = sqrtf(sum / (float)count);
            if (mask & OUT_BEST) out.best[set] = key_best(win);
            if (mask & OUT_FLAGS) out.flags[set] = flags;
        }
        break;
    }
}

#endif      // __HIPCC__

}  // namespace slhip_ransac
