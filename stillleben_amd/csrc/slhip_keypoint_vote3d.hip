// Keypoint voting in 3D (this project's addition, no counterpart in the reference): one camera-frame position per (set, keypoint)
// from per-point predicted 3D offsets, by mean shift over the candidates camera_j + offset_jk and the mode with the most support,
// with the mean and covariance of its supporters -- the decoder of PVN3D / FFB6D.  include/slhip.h "Keypoint voting in 3D" and
// DESIGN.md "Keypoint voting in 3D" are the contract; all arithmetic is float32, one rounded operation at a time
// (-ffp-contract=off), through slhip_vote3d_rules.h on host and device alike, so slhip_keypoint_vote3d_host gives the kernel's
// outputs bit for bit.
//   k_keypoint_vote3d  one workgroup of 256 lanes per (set, keypoint).  (1) the valid candidates, in ascending order, into three
//                      LDS planes (x, y, z) by ballot ranks -- the only global read; every 64 voters' validity word and first
//                      rank stay in LDS for (4);  (2) a lane per seed (seeds beyond 256 in turn): the seed in registers, every
//                      step walks the whole list by 16-byte LDS reads at one address for all lanes (a broadcast) and sums
//                      sequentially -- no barrier and no cross-lane step inside; a lane whose seed has stopped idles;  (3) arg-max
//                      of (support, lowest seed) by wave then workgroup, the winner's lane leaves its mode in LDS;  (4) the
//                      supporters of the mode over the voters in their own order: ballot words and the count;  (5) mean and
//                      covariance of the supporters: lanes over the valid list, two passes of sums (slhip_block_sum.h).
// Every loop is bounded by max_iters, n_seeds and K; nothing waits on another workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_step_timer.h"
#include "slhip_vote3d_rules.h"

namespace {

static_assert(sizeof(slhip_keypoint_vote3d_params) == 64, "slhip_keypoint_vote3d_params layout");

using Params = slhip_keypoint_vote3d_params;
using Out = slhip_keypoint_vote3d_out;
namespace vt = slhip_vote3d;

constexpr uint32_t BLOCK = vt::BLOCK;
constexpr uint32_t NWAVES = BLOCK / vt::WAVE;
constexpr int SUMS = 6;            // the most sums of one reduction (the covariance's)
constexpr uint32_t SMALL = 2u * NWAVES + NWAVES * SUMS + 8u;      // the words behind the planes: counts, keys, partial sums, winner
constexpr uint32_t N_SETS_MAX = 0x7fffffffu / SLHIP_KEYPOINTS_MAX;      // the grid is n_sets * n_keypoints blocks

using slhip_pose::chunks_of;
using slhip_pose::pad4;
using slhip_pose::words_of;

// dynamic LDS in 4-byte words: 3 candidate planes, a validity word pair and a first rank (and a spare) per 64 voters, SMALL:
// 49 KiB + 1 KiB + 168 B at K = 4096, under the 64 KiB a kernel may ask for without an attribute
__host__ __device__ inline uint32_t lds_words(uint32_t K) { return 3u * pad4(K) + 4u * chunks_of(K) + SMALL; }

// INSUFFICIENT / NO_MODEL: NaN xyz, mean and cov, 0 supporters, best -2, 0 iterations, zero bits (lane 0, and the words by all lanes)
__device__ void write_none(const Params& p, const Out& out, uint32_t o, int flags)
{
    const uint32_t m = p.outputs, nw = words_of(p.n_points);
    const float nan = __builtin_nanf("");
    if (m & SLHIP_VOTE3D_OUT_SUPPORT)
        for (uint32_t w = threadIdx.x; w < nw; w += BLOCK) out.support[(size_t)o * nw + w] = 0u;
    if (threadIdx.x) return;
    if (m & SLHIP_VOTE3D_OUT_XYZ)
        for (uint32_t i = 0u; i < 3u; ++i) out.xyz[(size_t)o * 3u + i] = nan;
    if (m & SLHIP_VOTE3D_OUT_N_SUPPORT) out.n_support[o] = 0;
    if (m & SLHIP_VOTE3D_OUT_BEST) out.best[o] = -2;
    if (m & SLHIP_VOTE3D_OUT_ITERS) out.iters[o] = 0;
    if (m & SLHIP_VOTE3D_OUT_FLAGS) out.flags[o] = flags;
    if (m & SLHIP_VOTE3D_OUT_MEAN)
        for (uint32_t i = 0u; i < 3u; ++i) out.mean[(size_t)o * 3u + i] = nan;
    if (m & SLHIP_VOTE3D_OUT_COV)
        for (uint32_t i = 0u; i < 6u; ++i) out.cov[(size_t)o * 6u + i] = nan;
}

// the four sums of one step of seed x over the n valid candidates, one after the other: four per 16-byte read of each plane,
// then the ragged rest
__device__ __forceinline__ void shift_sums(const vt::P& x, float inv_h2, const float* s_cx, const float* s_cy, const float* s_cz,
                                           uint32_t n, float* acc)
{
    const uint32_t whole = n & ~3u;
#pragma unroll 2
    for (uint32_t j = 0u; j < whole; j += 4u) {
        const float4 X = *reinterpret_cast<const float4*>(s_cx + j), Y = *reinterpret_cast<const float4*>(s_cy + j);
        const float4 Z = *reinterpret_cast<const float4*>(s_cz + j);
        vt::accumulate_shift(x, X.x, Y.x, Z.x, inv_h2, acc);
        vt::accumulate_shift(x, X.y, Y.y, Z.y, inv_h2, acc);
        vt::accumulate_shift(x, X.z, Y.z, Z.z, inv_h2, acc);
        vt::accumulate_shift(x, X.w, Y.w, Z.w, inv_h2, acc);
    }
    for (uint32_t j = whole; j < n; ++j) vt::accumulate_shift(x, s_cx[j], s_cy[j], s_cz[j], inv_h2, acc);
}

__device__ __forceinline__ uint32_t support_of(const vt::P& x, float h2, const float* s_cx, const float* s_cy, const float* s_cz, uint32_t n)
{
    uint32_t count = 0u;
    const uint32_t whole = n & ~3u;
    for (uint32_t j = 0u; j < whole; j += 4u) {
        const float4 X = *reinterpret_cast<const float4*>(s_cx + j), Y = *reinterpret_cast<const float4*>(s_cy + j);
        const float4 Z = *reinterpret_cast<const float4*>(s_cz + j);
        count += vt::supports(x, X.x, Y.x, Z.x, h2) ? 1u : 0u;
        count += vt::supports(x, X.y, Y.y, Z.y, h2) ? 1u : 0u;
        count += vt::supports(x, X.z, Y.z, Z.z, h2) ? 1u : 0u;
        count += vt::supports(x, X.w, Y.w, Z.w, h2) ? 1u : 0u;
    }
    for (uint32_t j = whole; j < n; ++j) count += vt::supports(x, s_cx[j], s_cy[j], s_cz[j], h2) ? 1u : 0u;
    return count;
}

// One block per (set, keypoint).  Dynamic LDS: lds_words(K) words, nothing static in front of it (the planes are read 16 bytes
// at a time and must start 16-byte aligned).
__global__ __launch_bounds__(BLOCK) void k_keypoint_vote3d(Params p, const float4* __restrict__ camera, const float* __restrict__ offsets,
                                                           Out out)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    const uint32_t K = p.n_points, Kp = p.n_keypoints, mask = p.outputs;
    const uint32_t k_pad = pad4(K), n_chunks = chunks_of(K);
    float* s_cx = s_all;
    float* s_cy = s_cx + k_pad;
    float* s_cz = s_cy + k_pad;
    unsigned long long* s_valid = reinterpret_cast<unsigned long long*>(s_cz + k_pad);      // 16-byte aligned: every plane is
    uint32_t* s_first = reinterpret_cast<uint32_t*>(s_valid + n_chunks);
    uint32_t* s_cnt = s_first + 2u * n_chunks;      // (n_chunks of them are used; the rest keeps what follows 8-byte aligned)
    uint32_t* s_key = s_cnt + NWAVES;
    float* s_part = reinterpret_cast<float*>(s_key + NWAVES);
    float* s_win = s_part + NWAVES * SUMS;          // the winner's x, y, z, and as integers its steps and whether it stopped

    const uint32_t tid = threadIdx.x, wave = tid / vt::WAVE, lane = tid % vt::WAVE;
    const uint32_t set = blockIdx.x / Kp, kp = blockIdx.x % Kp, o = blockIdx.x;
    const float h2 = p.bandwidth * p.bandwidth, inv_h2 = vt::inv_h2_of(p.bandwidth), tol2 = p.tol * p.tol;

    // (1) the valid list: ranks by ballot inside a wave, the waves' counts through LDS
    uint32_t n_valid = 0u;
    for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
        const uint32_t j = j0 + tid;
        vt::P c = {0.0f, 0.0f, 0.0f};
        bool ok = false;
        if (j < K) {
            const float4 cam = camera[(size_t)set * K + j];
            const float* off = offsets + (((size_t)set * K + j) * Kp + kp) * 3u;
            ok = vt::candidate(cam.x, cam.y, cam.z, cam.w, off[0], off[1], off[2], &c);
        }
        const unsigned long long votes = __ballot(ok);
        if (lane == 0u) s_cnt[wave] = (uint32_t)__popcll(votes);
        __syncthreads();
        uint32_t first = n_valid;
        for (uint32_t w = 0u; w < NWAVES; ++w) {
            first += w < wave ? s_cnt[w] : 0u;
            n_valid += s_cnt[w];
        }
        const uint32_t chunk = j0 / vt::WAVE + wave;
        if (lane == 0u && chunk < n_chunks) {
            s_valid[chunk] = votes;
            s_first[chunk] = first;
        }
        if (ok) {      // at < n_valid <= K <= k_pad
            const uint32_t at = first + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
            s_cx[at] = c.x; s_cy[at] = c.y; s_cz[at] = c.z;
        }
        __syncthreads();
    }
    if (n_valid == 0u) {      // the same for every lane
        write_none(p, out, o, SLHIP_VOTE3D_INSUFFICIENT);
        return;
    }

    // (2) a lane per seed; the seeds of a lane in turn
    const uint32_t S_eff = vt::n_seeds_of(p.n_seeds, n_valid);
    uint32_t best_key = 0u, best_iters = 0u;
    bool best_stopped = false;
    vt::P best_x = {0.0f, 0.0f, 0.0f};
    for (uint32_t s = tid; s < S_eff; s += BLOCK) {
        const uint32_t r = vt::seed_rank(s, n_valid, S_eff);      // < n_valid
        vt::P x = {s_cx[r], s_cy[r], s_cz[r]};
        uint32_t iters = 0u;
        bool stopped = false;
        while (iters < p.max_iters && !stopped) {
            float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            shift_sums(x, inv_h2, s_cx, s_cy, s_cz, n_valid, acc);
            stopped = vt::advance(&x, acc, tol2);
            ++iters;
        }
        const uint32_t key = vt::key_of(support_of(x, h2, s_cx, s_cy, s_cz, n_valid), s);
        if (key > best_key) {
            best_key = key;
            best_x = x;
            best_iters = iters;
            best_stopped = stopped;
        }
    }

    // (3) the winner: highest support, then lowest s; every seed has a key of its own, so one lane owns the maximum
    const uint32_t wkey = slhip_pose::wave_max(best_key);
    if (lane == 0u) s_key[wave] = wkey;
    __syncthreads();
    const uint32_t win = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
    if (best_key == win) {      // win != 0: S_eff >= 1 and a key is never 0
        s_win[0] = best_x.x; s_win[1] = best_x.y; s_win[2] = best_x.z;
        reinterpret_cast<uint32_t*>(s_win)[3] = best_iters;
        reinterpret_cast<uint32_t*>(s_win)[4] = best_stopped ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t win_support = vt::key_support(win);
    if (win_support < p.min_support) {
        write_none(p, out, o, SLHIP_VOTE3D_NO_MODEL);
        return;
    }
    const vt::P mode = {s_win[0], s_win[1], s_win[2]};
    const uint32_t win_iters = reinterpret_cast<const uint32_t*>(s_win)[3];
    const int flags = reinterpret_cast<const uint32_t*>(s_win)[4] ? 0 : SLHIP_VOTE3D_NOT_CONVERGED;

    // (4) the supporters of the mode over the voters in their own order
    if (mask & SLHIP_VOTE3D_OUT_SUPPORT) {
        const uint32_t nw = words_of(K);
        for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
            const uint32_t chunk = j0 / vt::WAVE + wave;
            bool in = false;
            if (chunk < n_chunks) {
                const unsigned long long valid = s_valid[chunk];
                if ((valid >> lane) & 1ull) {
                    const uint32_t i = s_first[chunk] + (uint32_t)__popcll(valid & ((1ull << lane) - 1ull));      // i < n_valid
                    in = vt::supports(mode, s_cx[i], s_cy[i], s_cz[i], h2);
                }
            }
            const unsigned long long votes = __ballot(in);
            if (lane == 0u) {
                const uint32_t w0 = 2u * chunk;
                if (w0 < nw) out.support[(size_t)o * nw + w0] = (uint32_t)votes;
                if (w0 + 1u < nw) out.support[(size_t)o * nw + w0 + 1u] = (uint32_t)(votes >> 32);
            }
        }
    }

    // (5) mean and covariance of the supporters: lane l takes valid candidates l, l + 256, ...
    vt::P mean = {0.0f, 0.0f, 0.0f};
    float cov[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (mask & (SLHIP_VOTE3D_OUT_MEAN | SLHIP_VOTE3D_OUT_COV)) {
        const float count = (float)win_support;
        float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, S[6];
        for (uint32_t i = tid; i < n_valid; i += BLOCK)
            if (vt::supports(mode, s_cx[i], s_cy[i], s_cz[i], h2)) vt::accumulate_mean(s_cx[i], s_cy[i], s_cz[i], acc);
        slhip_pose::block_sums<3, SUMS>(acc, s_part, wave, lane, S);
        mean.x = S[0] / count; mean.y = S[1] / count; mean.z = S[2] / count;
        acc[0] = acc[1] = acc[2] = 0.0f;
        for (uint32_t i = tid; i < n_valid; i += BLOCK)
            if (vt::supports(mode, s_cx[i], s_cy[i], s_cz[i], h2)) vt::accumulate_cov(s_cx[i], s_cy[i], s_cz[i], mean, acc);
        slhip_pose::block_sums<6, SUMS>(acc, s_part, wave, lane, S);
#pragma unroll
        for (int i = 0; i < 6; ++i) cov[i] = S[i] / count;
    }

    if (tid == 0u) {
        if (mask & SLHIP_VOTE3D_OUT_XYZ) {
            out.xyz[(size_t)o * 3u] = mode.x; out.xyz[(size_t)o * 3u + 1u] = mode.y; out.xyz[(size_t)o * 3u + 2u] = mode.z;
        }
        if (mask & SLHIP_VOTE3D_OUT_N_SUPPORT) out.n_support[o] = (int32_t)win_support;
        if (mask & SLHIP_VOTE3D_OUT_BEST) out.best[o] = vt::key_best(win);
        if (mask & SLHIP_VOTE3D_OUT_ITERS) out.iters[o] = (int32_t)win_iters;
        if (mask & SLHIP_VOTE3D_OUT_FLAGS) out.flags[o] = flags;
        if (mask & SLHIP_VOTE3D_OUT_MEAN) {
            out.mean[(size_t)o * 3u] = mean.x; out.mean[(size_t)o * 3u + 1u] = mean.y; out.mean[(size_t)o * 3u + 2u] = mean.z;
        }
        if (mask & SLHIP_VOTE3D_OUT_COV)
            for (uint32_t i = 0u; i < 6u; ++i) out.cov[(size_t)o * 6u + i] = cov[i];
    }
}

constexpr uint32_t ALL_OUTPUTS = SLHIP_VOTE3D_OUT_XYZ | SLHIP_VOTE3D_OUT_N_SUPPORT | SLHIP_VOTE3D_OUT_BEST | SLHIP_VOTE3D_OUT_ITERS |
                                 SLHIP_VOTE3D_OUT_FLAGS | SLHIP_VOTE3D_OUT_MEAN | SLHIP_VOTE3D_OUT_COV | SLHIP_VOTE3D_OUT_SUPPORT;

// the checks that slhip_keypoint_vote3d and slhip_keypoint_vote3d_host share
int check_call(const char* who, const Params* params, const float* camera, const float* offsets, const Out* out)
{
    if (const int st = slhip_keypoint_vote3d_check_params(params)) return st;
    if (!camera || !offsets || !out) {
        slhip::set_error("%s: null argument (camera points, offsets and the output record are required)", who);
        return -1;
    }
    const uint32_t m = params->outputs;
    const slhip::OutputList outputs = {{SLHIP_VOTE3D_OUT_XYZ, out->xyz},     {SLHIP_VOTE3D_OUT_N_SUPPORT, out->n_support}, {SLHIP_VOTE3D_OUT_BEST, out->best},
                                       {SLHIP_VOTE3D_OUT_ITERS, out->iters}, {SLHIP_VOTE3D_OUT_FLAGS, out->flags},         {SLHIP_VOTE3D_OUT_MEAN, out->mean},
                                       {SLHIP_VOTE3D_OUT_COV, out->cov},     {SLHIP_VOTE3D_OUT_SUPPORT, out->support}};
    if (const int st = slhip::check_outputs_present(who, m, outputs)) return st;
    if (((uintptr_t)camera & 15u) || ((uintptr_t)offsets & 3u)) {
        slhip::set_error("%s: the camera points must be 16-byte aligned, the offsets 4-byte", who);
        return -1;
    }
    return slhip::check_outputs_aligned(who, m, outputs);
}

// optional HIP-event timing (tools/time_keypoint_vote3d.py): events round the last call
slhip::StepTimer<1> g_timer;

}  // namespace

extern "C" int slhip_keypoint_vote3d_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_keypoint_vote3d_timings(float ms_out[1]) { return g_timer.read_for("slhip_keypoint_vote3d_timings", ms_out); }

extern "C" int slhip_keypoint_vote3d_check_params(const slhip_keypoint_vote3d_params* p)
{
    static const char* who = "slhip_keypoint_vote3d";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, N_SETS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 1u, SLHIP_VOTE3D_POINTS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_keypoints", p->n_keypoints, 1u, SLHIP_KEYPOINTS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_seeds", p->n_seeds, 1u, SLHIP_VOTE3D_SEEDS_MAX)) return st;
    if (!(p->bandwidth > 0.0f) || !slhip::is_finite(p->bandwidth) || !(p->bandwidth * p->bandwidth > 0.0f) ||
        !slhip::is_finite(1.0f / (p->bandwidth * p->bandwidth))) {
        slhip::set_error("%s: bandwidth %g must be finite and > 0, and so must its square and the square's inverse", who, (double)p->bandwidth);
        return -1;
    }
    if (const int st = slhip::check_range(who, "max_iters", p->max_iters, 1u, SLHIP_VOTE3D_ITERS_MAX)) return st;
    if (!(p->tol >= 0.0f) || !slhip::is_finite(p->tol)) {
        slhip::set_error("%s: tol %g must be finite and >= 0", who, (double)p->tol);
        return -1;
    }
    if (const int st = slhip::check_range(who, "min_support", p->min_support, 1u, 0x7fffffffu)) return st;
    if (p->outputs == 0u || (p->outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of xyz 1, n_support 2, best 4, iters 8, flags 16, mean 32, cov 64, "
                         "support 128 and nothing else", who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_keypoint_vote3d(const slhip_keypoint_vote3d_params* params, const float* d_camera, const float* d_offsets,
                                     const slhip_keypoint_vote3d_out* out, void* stream_)
{
    static const char* who = "slhip_keypoint_vote3d";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_camera, d_offsets, out)) return st;
    if (params->n_sets == 0u) return 0;
    const size_t lds = (size_t)lds_words(params->n_points) * 4u;      // 12.4 KiB at K = 1024; 49.2 KiB at the limit
    if (const int st = g_timer.begin(0, stream)) return st;
    k_keypoint_vote3d<<<params->n_sets * params->n_keypoints, BLOCK, lds, stream>>>(*params, reinterpret_cast<const float4*>(d_camera),
                                                                                   d_offsets, *out);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

extern "C" int slhip_keypoint_vote3d_host(const slhip_keypoint_vote3d_params* params, const float* h_camera, const float* h_offsets,
                                          const slhip_keypoint_vote3d_out* out)
{
    static const char* who = "slhip_keypoint_vote3d_host";
    if (const int st = check_call(who, params, h_camera, h_offsets, out)) return st;
    const Params& p = *params;
    const uint32_t K = p.n_points, Kp = p.n_keypoints, mask = p.outputs, nw = words_of(K);
    const float h2 = p.bandwidth * p.bandwidth, inv_h2 = vt::inv_h2_of(p.bandwidth), tol2 = p.tol * p.tol, nan = __builtin_nanf("");
    std::vector<vt::P> list(K);
    std::vector<int32_t> rank(K);      // of voter j in the valid list, -1: not valid
    for (uint32_t set = 0u; set < p.n_sets; ++set)
        for (uint32_t kp = 0u; kp < Kp; ++kp) {
            const size_t o = (size_t)set * Kp + kp;
            auto none = [&](int flags) {
                if (mask & SLHIP_VOTE3D_OUT_SUPPORT)
                    for (uint32_t w = 0u; w < nw; ++w) out->support[o * nw + w] = 0u;
                if (mask & SLHIP_VOTE3D_OUT_XYZ)
                    for (uint32_t i = 0u; i < 3u; ++i) out->xyz[o * 3u + i] = nan;
                if (mask & SLHIP_VOTE3D_OUT_N_SUPPORT) out->n_support[o] = 0;
                if (mask & SLHIP_VOTE3D_OUT_BEST) out->best[o] = -2;
                if (mask & SLHIP_VOTE3D_OUT_ITERS) out->iters[o] = 0;
                if (mask & SLHIP_VOTE3D_OUT_FLAGS) out->flags[o] = flags;
                if (mask & SLHIP_VOTE3D_OUT_MEAN)
                    for (uint32_t i = 0u; i < 3u; ++i) out->mean[o * 3u + i] = nan;
                if (mask & SLHIP_VOTE3D_OUT_COV)
                    for (uint32_t i = 0u; i < 6u; ++i) out->cov[o * 6u + i] = nan;
            };
            uint32_t n_valid = 0u;
            for (uint32_t j = 0u; j < K; ++j) {
                rank[j] = -1;
                const float* cam = h_camera + ((size_t)set * K + j) * 4u;
                const float* off = h_offsets + (((size_t)set * K + j) * Kp + kp) * 3u;
                if (vt::candidate(cam[0], cam[1], cam[2], cam[3], off[0], off[1], off[2], &list[n_valid])) rank[j] = (int32_t)n_valid++;
            }
            if (n_valid == 0u) {
                none(SLHIP_VOTE3D_INSUFFICIENT);
                continue;
            }
            const uint32_t S_eff = vt::n_seeds_of(p.n_seeds, n_valid);
            uint32_t win = 0u, win_iters = 0u;
            bool win_stopped = false;
            vt::P mode = {0.0f, 0.0f, 0.0f};
            for (uint32_t s = 0u; s < S_eff; ++s) {
                vt::P x = list[vt::seed_rank(s, n_valid, S_eff)];
                uint32_t iters = 0u;
                bool stopped = false;
                while (iters < p.max_iters && !stopped) {
                    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    for (uint32_t i = 0u; i < n_valid; ++i) vt::accumulate_shift(x, list[i].x, list[i].y, list[i].z, inv_h2, acc);
                    stopped = vt::advance(&x, acc, tol2);
                    ++iters;
                }
                uint32_t support = 0u;
                for (uint32_t i = 0u; i < n_valid; ++i) support += vt::supports(x, list[i].x, list[i].y, list[i].z, h2) ? 1u : 0u;
                const uint32_t key = vt::key_of(support, s);
                if (key > win) {
                    win = key;
                    mode = x;
                    win_iters = iters;
                    win_stopped = stopped;
                }
            }
            const uint32_t win_support = vt::key_support(win);
            if (win_support < p.min_support) {
                none(SLHIP_VOTE3D_NO_MODEL);
                continue;
            }
            const float count = (float)win_support;
            slhip_pose::LaneSums<3> mean_sums;
            slhip_pose::LaneSums<6> cov_sums;
            for (uint32_t i = 0u; i < n_valid; ++i)
                if (vt::supports(mode, list[i].x, list[i].y, list[i].z, h2))
                    mean_sums.add(i, [&](float* acc) { vt::accumulate_mean(list[i].x, list[i].y, list[i].z, acc); });
            const vt::P mean = {mean_sums.total(0) / count, mean_sums.total(1) / count, mean_sums.total(2) / count};
            for (uint32_t i = 0u; i < n_valid; ++i)
                if (vt::supports(mode, list[i].x, list[i].y, list[i].z, h2))
                    cov_sums.add(i, [&](float* acc) { vt::accumulate_cov(list[i].x, list[i].y, list[i].z, mean, acc); });
            if (mask & SLHIP_VOTE3D_OUT_SUPPORT) {
                for (uint32_t w = 0u; w < nw; ++w) out->support[o * nw + w] = 0u;
                for (uint32_t j = 0u; j < K; ++j)
                    if (rank[j] >= 0 && vt::supports(mode, list[rank[j]].x, list[rank[j]].y, list[rank[j]].z, h2))
                        out->support[o * nw + (j >> 5)] |= 1u << (j & 31u);
            }
            if (mask & SLHIP_VOTE3D_OUT_XYZ) { out->xyz[o * 3u] = mode.x; out->xyz[o * 3u + 1u] = mode.y; out->xyz[o * 3u + 2u] = mode.z; }
            if (mask & SLHIP_VOTE3D_OUT_N_SUPPORT) out->n_support[o] = (int32_t)win_support;
            if (mask & SLHIP_VOTE3D_OUT_BEST) out->best[o] = vt::key_best(win);
            if (mask & SLHIP_VOTE3D_OUT_ITERS) out->iters[o] = (int32_t)win_iters;
            if (mask & SLHIP_VOTE3D_OUT_FLAGS) out->flags[o] = win_stopped ? 0 : SLHIP_VOTE3D_NOT_CONVERGED;
            if (mask & SLHIP_VOTE3D_OUT_MEAN) { out->mean[o * 3u] = mean.x; out->mean[o * 3u + 1u] = mean.y; out->mean[o * 3u + 2u] = mean.z; }
            if (mask & SLHIP_VOTE3D_OUT_COV)
                for (int s = 0; s < 6; ++s) out->cov[o * 6u + s] = cov_sums.total(s) / count;
        }
    return 0;
}
