// Keypoint voting (this project's addition, no counterpart in the reference): one 2D position per (set, keypoint) from a field of
// predicted unit vectors, by RANSAC over pairs of voters, a weighted mean and covariance of the hypotheses and one least-squares
// step on the winner's inliers -- PVNet's voting layer.  include/slhip.h "Keypoint voting" and DESIGN.md "Keypoint voting" are the
// contract; all arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through slhip_vote_rules.h on host and
// device alike, so slhip_keypoint_vote_host gives the kernel's outputs bit for bit.
//   k_keypoint_vote   one workgroup of 256 lanes per (set, keypoint).  (1) the valid voters, in ascending order, into four LDS
//                     planes (px, py, dx, dy) by ballot ranks -- the only global read of the field; every 64 voters' validity word
//                     and first rank stay in LDS for (6);  (2) a lane per hypothesis in rounds of 256: Philox, the meeting point,
//                     then the score with q in registers and the voters by 16-byte LDS reads at one address for all lanes (a
//                     broadcast), no barrier inside a round; (qx, qy, count) of every hypothesis into LDS;  (3) arg-max of
//                     (count, lowest index) by wave then workgroup;  (4) mean and covariance: lanes over hypotheses, two passes of
//                     three sums (slhip_block_sum.h);  (5) the fit: lanes over the valid list, five sums, every lane solves the
//                     2 x 2;  (6) the final pass over the voters in their own order from LDS: ballot words and the count
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_step_timer.h"
#include "slhip_vote_rules.h"

namespace {

static_assert(sizeof(slhip_keypoint_vote_params) == 64, "slhip_keypoint_vote_params layout");

using Params = slhip_keypoint_vote_params;
using Out = slhip_keypoint_vote_out;
namespace vt = slhip_vote;

constexpr uint32_t BLOCK = vt::BLOCK;
constexpr uint32_t NWAVES = BLOCK / vt::WAVE;
constexpr int SUMS = 5;            // the most sums of one reduction (the fit's)
constexpr uint32_t SMALL = 2u * NWAVES + NWAVES * SUMS + 2u;      // the words behind the planes: counts, keys, partial sums, q
constexpr uint32_t N_SETS_MAX = 0x7fffffffu / SLHIP_KEYPOINTS_MAX;      // the grid is n_sets * n_keypoints blocks

using slhip_pose::chunks_of;
using slhip_pose::pad4;
using slhip_pose::words_of;

// dynamic LDS in 4-byte words: 4 voter planes, 3 hypothesis planes, a validity word pair and a first rank per 64 voters, SMALL
__host__ __device__ inline uint32_t lds_words(uint32_t K, uint32_t Hy) { return 4u * pad4(K) + 3u * pad4(Hy) + 4u * chunks_of(K) + SMALL; }

// INSUFFICIENT / NO_MODEL: NaN uv, mean and cov, 0 inliers, best -2, zero bits (lane 0, and the words by all lanes)
__device__ void write_none(const Params& p, const Out& out, uint32_t o, int flags)
{
    const uint32_t m = p.outputs, nw = words_of(p.n_points);
    const float nan = __builtin_nanf("");
    if (m & SLHIP_VOTE_OUT_INLIERS)
        for (uint32_t w = threadIdx.x; w < nw; w += BLOCK) out.inliers[(size_t)o * nw + w] = 0u;
    if (threadIdx.x) return;
    if (m & SLHIP_VOTE_OUT_UV) out.uv[(size_t)o * 2u] = out.uv[(size_t)o * 2u + 1u] = nan;
    if (m & SLHIP_VOTE_OUT_N_INLIERS) out.n_inliers[o] = 0;
    if (m & SLHIP_VOTE_OUT_BEST) out.best[o] = -2;
    if (m & SLHIP_VOTE_OUT_FLAGS) out.flags[o] = flags;
    if (m & SLHIP_VOTE_OUT_MEAN) out.mean[(size_t)o * 2u] = out.mean[(size_t)o * 2u + 1u] = nan;
    if (m & SLHIP_VOTE_OUT_COV) out.cov[(size_t)o * 3u] = out.cov[(size_t)o * 3u + 1u] = out.cov[(size_t)o * 3u + 2u] = nan;
}

// the score of one q in registers against the n valid voters: four per 16-byte read of each plane, then the ragged rest
__device__ __forceinline__ uint32_t score(float qx, float qy, float cc, const float* s_px, const float* s_py, const float* s_dx,
                                          const float* s_dy, uint32_t n)
{
    uint32_t count = 0u;
    const uint32_t whole = n & ~3u;
#pragma unroll 2
    for (uint32_t j = 0u; j < whole; j += 4u) {
        const float4 X = *reinterpret_cast<const float4*>(s_px + j), Y = *reinterpret_cast<const float4*>(s_py + j);
        const float4 A = *reinterpret_cast<const float4*>(s_dx + j), B = *reinterpret_cast<const float4*>(s_dy + j);
        count += vt::inlier(qx, qy, X.x, Y.x, A.x, B.x, cc) ? 1u : 0u;
        count += vt::inlier(qx, qy, X.y, Y.y, A.y, B.y, cc) ? 1u : 0u;
        count += vt::inlier(qx, qy, X.z, Y.z, A.z, B.z, cc) ? 1u : 0u;
        count += vt::inlier(qx, qy, X.w, Y.w, A.w, B.w, cc) ? 1u : 0u;
    }
    for (uint32_t j = whole; j < n; ++j) count += vt::inlier(qx, qy, s_px[j], s_py[j], s_dx[j], s_dy[j], cc) ? 1u : 0u;
    return count;
}

// One block per (set, keypoint).  Dynamic LDS: lds_words(K, Hy) words, nothing static in front of it (the planes are read 16
// bytes at a time and must start 16-byte aligned).
__global__ __launch_bounds__(BLOCK) void k_keypoint_vote(Params p, const short2* __restrict__ pixel, const float2* __restrict__ vectors,
                                                         const int32_t* __restrict__ scene, uint32_t n_field_scenes, Out out)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    const uint32_t K = p.n_points, Hy = p.n_hypotheses, Kp = p.n_keypoints, mask = p.outputs;
    const uint32_t k_pad = pad4(K), h_pad = pad4(Hy), n_chunks = chunks_of(K);
    float* s_px = s_all;
    float* s_py = s_px + k_pad;
    float* s_dx = s_py + k_pad;
    float* s_dy = s_dx + k_pad;
    float* s_qx = s_dy + k_pad;
    float* s_qy = s_qx + h_pad;
    uint32_t* s_count = reinterpret_cast<uint32_t*>(s_qy + h_pad);
    unsigned long long* s_valid = reinterpret_cast<unsigned long long*>(s_count + h_pad);      // 16-byte aligned: every plane is
    uint32_t* s_first = reinterpret_cast<uint32_t*>(s_valid + n_chunks);
    uint32_t* s_cnt = s_first + 2u * n_chunks;      // (n_chunks of them are used; the rest keeps what follows 8-byte aligned)
    uint32_t* s_key = s_cnt + NWAVES;
    float* s_part = reinterpret_cast<float*>(s_key + NWAVES);
    float* s_q = s_part + NWAVES * SUMS;

    const uint32_t tid = threadIdx.x, wave = tid / vt::WAVE, lane = tid % vt::WAVE;
    const uint32_t set = blockIdx.x / Kp, kp = blockIdx.x % Kp, o = blockIdx.x;
    const float cc = p.inlier_cos * p.inlier_cos;
    const short2* my_pixel = pixel + (size_t)set * K;
    const int32_t sc = scene ? scene[set] : 0;
    const bool scene_ok = !scene || (sc >= 0 && (uint32_t)sc < n_field_scenes);

    // (1) the valid list: ranks by ballot inside a wave, the waves' counts through LDS
    uint32_t n_valid = 0u;
    for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
        const uint32_t j = j0 + tid;
        vt::Voter v = {0.0f, 0.0f, 0.0f, 0.0f};
        bool ok = false;
        if (j < K && scene_ok) {
            const short2 xy = my_pixel[j];
            if (vt::pixel_inside(xy.x, xy.y, p.W, p.H)) {      // a pixel outside the picture reads nothing
                const size_t at = scene ? (((size_t)sc * p.H + (uint32_t)xy.y) * p.W + (uint32_t)xy.x) * Kp + kp
                                        : ((size_t)set * K + j) * Kp + kp;
                const float2 f = vectors[at];
                ok = vt::voter(xy.x, xy.y, f.x, f.y, &v);
            }
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
            s_px[at] = v.px; s_py[at] = v.py; s_dx[at] = v.dx; s_dy[at] = v.dy;
        }
        __syncthreads();
    }
    if (n_valid < 2u) {      // the same for every lane
        write_none(p, out, o, SLHIP_VOTE_INSUFFICIENT);
        return;
    }

    // (2) a lane per hypothesis
    uint32_t best_key = 0u;
    float best_x = 0.0f, best_y = 0.0f;
    for (uint32_t h0 = 0u; h0 < Hy; h0 += BLOCK) {
        const uint32_t h = h0 + tid;
        vt::Q q = {__builtin_nanf(""), __builtin_nanf("")};      // a void hypothesis counts nothing
        bool have = false;
        if (h < Hy) {
            uint32_t a, b;
            vt::sample(p.seed_lo, p.seed_hi, p.set_id_base + set, h, kp, n_valid, &a, &b);
            const vt::Voter va = {s_px[a], s_py[a], s_dx[a], s_dy[a]}, vb = {s_px[b], s_py[b], s_dx[b], s_dy[b]};
            vt::Q got;
            have = vt::intersect(a == b, va, vb, p.min_sin, &got);
            if (have) q = got;
        }
        uint32_t count = 0u;
        if (__ballot(have)) count = score(q.x, q.y, cc, s_px, s_py, s_dx, s_dy, n_valid);      // a wave without a hypothesis skips the walk
        if (h < Hy) {
            s_qx[h] = q.x; s_qy[h] = q.y; s_count[h] = count;
            const uint32_t key = vt::key_of(count, h);
            if (key > best_key) {
                best_key = key;
                best_x = q.x; best_y = q.y;
            }
        }
    }

    // (3) the winner: highest count, then lowest h; every hypothesis has a key of its own, so one lane owns the maximum
    const uint32_t wkey = slhip_pose::wave_max(best_key);
    if (lane == 0u) s_key[wave] = wkey;
    __syncthreads();
    const uint32_t win = max(max(s_key[0], s_key[1]), max(s_key[2], s_key[3]));
    if (best_key == win) {      // win != 0: Hy >= 1
        s_q[0] = best_x; s_q[1] = best_y;
    }
    __syncthreads();      // (also: every hypothesis' (qx, qy, count) is in LDS)
    const uint32_t win_count = vt::key_count(win);
    if (win_count < p.min_inliers) {
        write_none(p, out, o, SLHIP_VOTE_NO_MODEL);
        return;
    }
    const float qx = s_q[0], qy = s_q[1];
    int flags = 0;

    // (4) the distribution of the non-void hypotheses: lane l takes h = l, l + 256, ...
    float mean_x = 0.0f, mean_y = 0.0f, cov[3] = {0.0f, 0.0f, 0.0f};
    if (mask & (SLHIP_VOTE_OUT_MEAN | SLHIP_VOTE_OUT_COV)) {
        float acc[3] = {0.0f, 0.0f, 0.0f}, S[3];
        for (uint32_t h = tid; h < Hy; h += BLOCK)
            if (s_qx[h] == s_qx[h]) vt::accumulate_mean(vt::weight(s_count[h], n_valid), s_qx[h], s_qy[h], acc);
        slhip_pose::block_sums<3, SUMS>(acc, s_part, wave, lane, S);
        const float sw = S[0];
        mean_x = S[1] / sw;
        mean_y = S[2] / sw;
        acc[0] = acc[1] = acc[2] = 0.0f;
        for (uint32_t h = tid; h < Hy; h += BLOCK)
            if (s_qx[h] == s_qx[h]) vt::accumulate_cov(vt::weight(s_count[h], n_valid), s_qx[h], s_qy[h], mean_x, mean_y, acc);
        slhip_pose::block_sums<3, SUMS>(acc, s_part, wave, lane, S);
        cov[0] = S[0] / sw; cov[1] = S[1] / sw; cov[2] = S[2] / sw;
    }

    // (5) one least-squares step on the inliers of q: lane l takes valid voters l, l + 256, ...
    vt::Q uv;
    {
        float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, S[5];
        for (uint32_t i = tid; i < n_valid; i += BLOCK)
            if (vt::inlier(qx, qy, s_px[i], s_py[i], s_dx[i], s_dy[i], cc)) vt::accumulate_fit(qx, qy, s_px[i], s_py[i], s_dx[i], s_dy[i], acc);
        slhip_pose::block_sums<5, SUMS>(acc, s_part, wave, lane, S);
        if (!vt::fit(S, qx, qy, &uv)) flags |= SLHIP_VOTE_REFINE_STOPPED;      // the same for every lane
    }

    // (6) inliers and count of uv over the voters in their own order; should it hold fewer than the winner, the same of q
    const uint32_t nw = words_of(K);
    for (int pass = 0; pass < 2; ++pass) {
        uint32_t mine = 0u;      // lane 0 of a wave: the wave's count
        for (uint32_t j0 = 0u; j0 < K; j0 += BLOCK) {
            const uint32_t chunk = j0 / vt::WAVE + wave;
            bool in = false;
            if (chunk < n_chunks) {
                const unsigned long long valid = s_valid[chunk];
                if ((valid >> lane) & 1ull) {
                    const uint32_t i = s_first[chunk] + (uint32_t)__popcll(valid & ((1ull << lane) - 1ull));      // i < n_valid
                    in = vt::inlier(uv.x, uv.y, s_px[i], s_py[i], s_dx[i], s_dy[i], cc);
                }
            }
            const unsigned long long votes = __ballot(in);
            mine += (uint32_t)__popcll(votes);
            if (lane == 0u && (mask & SLHIP_VOTE_OUT_INLIERS)) {
                const uint32_t w0 = 2u * chunk;
                if (w0 < nw) out.inliers[(size_t)o * nw + w0] = (uint32_t)votes;
                if (w0 + 1u < nw) out.inliers[(size_t)o * nw + w0 + 1u] = (uint32_t)(votes >> 32);
            }
        }
        if (lane == 0u) s_cnt[wave] = mine;
        __syncthreads();
        const uint32_t count = slhip_pose::waves_sum(s_cnt);
        __syncthreads();
        if (pass == 0 && count < win_count) {      // the same for every lane; only a refined position can get here
            flags |= SLHIP_VOTE_REFINE_REJECTED;
            uv.x = qx; uv.y = qy;
            continue;
        }
        if (tid == 0u) {
            if (mask & SLHIP_VOTE_OUT_UV) {
                out.uv[(size_t)o * 2u] = uv.x;
                out.uv[(size_t)o * 2u + 1u] = uv.y;
            }
            if (mask & SLHIP_VOTE_OUT_N_INLIERS) out.n_inliers[o] = (int32_t)count;
            if (mask & SLHIP_VOTE_OUT_BEST) out.best[o] = vt::key_best(win);
            if (mask & SLHIP_VOTE_OUT_FLAGS) out.flags[o] = flags;
            if (mask & SLHIP_VOTE_OUT_MEAN) {
                out.mean[(size_t)o * 2u] = mean_x;
                out.mean[(size_t)o * 2u + 1u] = mean_y;
            }
            if (mask & SLHIP_VOTE_OUT_COV) {
                out.cov[(size_t)o * 3u] = cov[0];
                out.cov[(size_t)o * 3u + 1u] = cov[1];
                out.cov[(size_t)o * 3u + 2u] = cov[2];
            }
        }
        break;
    }
}

constexpr uint32_t ALL_OUTPUTS = SLHIP_VOTE_OUT_UV | SLHIP_VOTE_OUT_N_INLIERS | SLHIP_VOTE_OUT_BEST | SLHIP_VOTE_OUT_FLAGS |
                                 SLHIP_VOTE_OUT_MEAN | SLHIP_VOTE_OUT_COV | SLHIP_VOTE_OUT_INLIERS;

// the checks that slhip_keypoint_vote and slhip_keypoint_vote_host share
int check_call(const char* who, const Params* params, const int16_t* pixel, const float* vectors, const int32_t* scene,
               uint32_t n_field_scenes, const Out* out)
{
    if (const int st = slhip_keypoint_vote_check_params(params)) return st;
    if (!pixel || !vectors || !out) {
        slhip::set_error("%s: null argument (pixels, vectors and the output record are required)", who);
        return -1;
    }
    if (scene && n_field_scenes < 1u) {
        slhip::set_error("%s: a dense field (the scene of every set is given) needs n_field_scenes >= 1", who);
        return -1;
    }
    const uint32_t m = params->outputs;
    const slhip::OutputList outputs = {{SLHIP_VOTE_OUT_UV, out->uv},       {SLHIP_VOTE_OUT_N_INLIERS, out->n_inliers}, {SLHIP_VOTE_OUT_BEST, out->best},
                                       {SLHIP_VOTE_OUT_FLAGS, out->flags}, {SLHIP_VOTE_OUT_MEAN, out->mean},           {SLHIP_VOTE_OUT_COV, out->cov},
                                       {SLHIP_VOTE_OUT_INLIERS, out->inliers}};
    if (const int st = slhip::check_outputs_present(who, m, outputs)) return st;
    if (((uintptr_t)pixel & 3u) || ((uintptr_t)vectors & 7u) || ((uintptr_t)scene & 3u)) {
        slhip::set_error("%s: the pixels and the scenes must be 4-byte aligned, the vectors 8-byte", who);
        return -1;
    }
    return slhip::check_outputs_aligned(who, m, outputs);
}

// optional HIP-event timing (tools/time_keypoint_vote.py): events round the last whole call [0] and the last call that read a
// dense field [1]
slhip::StepTimer<2> g_timer;

}  // namespace

extern "C" int slhip_keypoint_vote_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_keypoint_vote_timings(float ms_out[2]) { return g_timer.read_for("slhip_keypoint_vote_timings", ms_out); }

extern "C" int slhip_keypoint_vote_check_params(const slhip_keypoint_vote_params* p)
{
    static const char* who = "slhip_keypoint_vote";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (p->W < 1u || p->H < 1u || p->W > 32768u || p->H > 32768u) {      // (the pixels are int16)
        slhip::set_error("%s: bad picture size %u x %u (each side 1..32768)", who, p->W, p->H);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, N_SETS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 2u, SLHIP_VOTE_POINTS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_keypoints", p->n_keypoints, 1u, SLHIP_KEYPOINTS_MAX)) return st;
    if (const int st = slhip::check_range(who, "n_hypotheses", p->n_hypotheses, 1u, SLHIP_VOTE_HYPOTHESES_MAX)) return st;
    if (!(p->inlier_cos > 0.0f) || !(p->inlier_cos < 1.0f)) {
        slhip::set_error("%s: inlier_cos %g must lie in (0, 1)", who, (double)p->inlier_cos);
        return -1;
    }
    if (const int st = slhip::check_range(who, "min_inliers", p->min_inliers, 2u, 0x7fffffffu)) return st;
    if (!(p->min_sin >= 0.0f) || !slhip::is_finite(p->min_sin)) {
        slhip::set_error("%s: min_sin %g must be finite and >= 0", who, (double)p->min_sin);
        return -1;
    }
    if (p->outputs == 0u || (p->outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of uv 1, n_inliers 2, best 4, flags 8, mean 16, cov 32, inliers 64 and nothing else",
                         who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_keypoint_vote(const slhip_keypoint_vote_params* params, const int16_t* d_pixel, const float* d_vectors,
                                   const int32_t* d_scene, uint32_t n_field_scenes, const slhip_keypoint_vote_out* out, void* stream_)
{
    static const char* who = "slhip_keypoint_vote";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_pixel, d_vectors, d_scene, n_field_scenes, out)) return st;
    if (params->n_sets == 0u) return 0;
    const size_t lds = (size_t)lds_words(params->n_points, params->n_hypotheses) * 4u;      // 18 KiB at K = 1024, Hy = 128; 77 KiB at the limits
    if (lds > 64u * 1024u)      // more than a kernel may ask for without the attribute (per device, so not remembered)
        SLHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_keypoint_vote), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int dense = d_scene != nullptr;
    if (const int st = g_timer.begin(0, stream)) return st;
    if (dense)
        if (const int st = g_timer.begin(1, stream)) return st;
    k_keypoint_vote<<<params->n_sets * params->n_keypoints, BLOCK, lds, stream>>>(*params, reinterpret_cast<const short2*>(d_pixel),
                                                                                 reinterpret_cast<const float2*>(d_vectors), d_scene,
                                                                                 n_field_scenes, *out);
    SLHIP_LAUNCH_CHECK();
    if (dense)
        if (const int st = g_timer.end(1, stream)) return st;
    return g_timer.end(0, stream);
}

extern "C" int slhip_keypoint_vote_host(const slhip_keypoint_vote_params* params, const int16_t* h_pixel, const float* h_vectors,
                                        const int32_t* h_scene, uint32_t n_field_scenes, const slhip_keypoint_vote_out* out)
{
    static const char* who = "slhip_keypoint_vote_host";
    if (const int st = check_call(who, params, h_pixel, h_vectors, h_scene, n_field_scenes, out)) return st;
    const Params& p = *params;
    const uint32_t K = p.n_points, Hy = p.n_hypotheses, Kp = p.n_keypoints, mask = p.outputs, nw = words_of(K);
    const float cc = p.inlier_cos * p.inlier_cos, nan = __builtin_nanf("");
    std::vector<vt::Voter> list(K);
    std::vector<int32_t> rank(K);      // of voter j in the valid list, -1: not valid
    std::vector<vt::Q> hyp(Hy);
    std::vector<uint32_t> counts(Hy);
    std::vector<uint8_t> have(Hy);
    for (uint32_t set = 0u; set < p.n_sets; ++set)
        for (uint32_t kp = 0u; kp < Kp; ++kp) {
            const size_t o = (size_t)set * Kp + kp;
            auto none = [&](int flags) {
                if (mask & SLHIP_VOTE_OUT_INLIERS)
                    for (uint32_t w = 0u; w < nw; ++w) out->inliers[o * nw + w] = 0u;
                if (mask & SLHIP_VOTE_OUT_UV) out->uv[o * 2u] = out->uv[o * 2u + 1u] = nan;
                if (mask & SLHIP_VOTE_OUT_N_INLIERS) out->n_inliers[o] = 0;
                if (mask & SLHIP_VOTE_OUT_BEST) out->best[o] = -2;
                if (mask & SLHIP_VOTE_OUT_FLAGS) out->flags[o] = flags;
                if (mask & SLHIP_VOTE_OUT_MEAN) out->mean[o * 2u] = out->mean[o * 2u + 1u] = nan;
                if (mask & SLHIP_VOTE_OUT_COV) out->cov[o * 3u] = out->cov[o * 3u + 1u] = out->cov[o * 3u + 2u] = nan;
            };
            const int32_t sc = h_scene ? h_scene[set] : 0;
            const bool scene_ok = !h_scene || (sc >= 0 && (uint32_t)sc < n_field_scenes);
            uint32_t n_valid = 0u;
            for (uint32_t j = 0u; j < K; ++j) {
                rank[j] = -1;
                const int x = h_pixel[((size_t)set * K + j) * 2u], y = h_pixel[((size_t)set * K + j) * 2u + 1u];
                if (!scene_ok || !vt::pixel_inside(x, y, p.W, p.H)) continue;
                const size_t at = h_scene ? (((size_t)sc * p.H + (uint32_t)y) * p.W + (uint32_t)x) * Kp + kp : ((size_t)set * K + j) * Kp + kp;
                if (vt::voter(x, y, h_vectors[2u * at], h_vectors[2u * at + 1u], &list[n_valid])) rank[j] = (int32_t)n_valid++;
            }
            if (n_valid < 2u) {
                none(SLHIP_VOTE_INSUFFICIENT);
                continue;
            }
            auto count_of = [&](float x, float y) {
                uint32_t c = 0u;
                for (uint32_t i = 0u; i < n_valid; ++i) c += vt::inlier(x, y, list[i].px, list[i].py, list[i].dx, list[i].dy, cc) ? 1u : 0u;
                return c;
            };
            uint32_t win = 0u;
            for (uint32_t h = 0u; h < Hy; ++h) {
                uint32_t a, b;
                vt::sample(p.seed_lo, p.seed_hi, p.set_id_base + set, h, kp, n_valid, &a, &b);
                have[h] = vt::intersect(a == b, list[a], list[b], p.min_sin, &hyp[h]) ? 1u : 0u;
                counts[h] = have[h] ? count_of(hyp[h].x, hyp[h].y) : 0u;
                win = std::max(win, vt::key_of(counts[h], h));
            }
            const uint32_t win_count = vt::key_count(win);
            if (win_count < p.min_inliers) {
                none(SLHIP_VOTE_NO_MODEL);
                continue;
            }
            const int best = vt::key_best(win);
            const float qx = hyp[best].x, qy = hyp[best].y;
            int flags = 0;
            slhip_pose::LaneSums<3> mean_sums, cov_sums;
            for (uint32_t h = 0u; h < Hy; ++h)
                if (have[h]) mean_sums.add(h, [&](float* acc) { vt::accumulate_mean(vt::weight(counts[h], n_valid), hyp[h].x, hyp[h].y, acc); });
            const float sw = mean_sums.total(0);
            const float mean_x = mean_sums.total(1) / sw, mean_y = mean_sums.total(2) / sw;
            for (uint32_t h = 0u; h < Hy; ++h)
                if (have[h])
                    cov_sums.add(h, [&](float* acc) { vt::accumulate_cov(vt::weight(counts[h], n_valid), hyp[h].x, hyp[h].y, mean_x, mean_y, acc); });
            const float cov[3] = {cov_sums.total(0) / sw, cov_sums.total(1) / sw, cov_sums.total(2) / sw};
            slhip_pose::LaneSums<5> fit_sums;
            for (uint32_t i = 0u; i < n_valid; ++i) {
                const vt::Voter& v = list[i];
                if (vt::inlier(qx, qy, v.px, v.py, v.dx, v.dy, cc))
                    fit_sums.add(i, [&](float* acc) { vt::accumulate_fit(qx, qy, v.px, v.py, v.dx, v.dy, acc); });
            }
            float S[5];
            for (int s = 0; s < 5; ++s) S[s] = fit_sums.total(s);
            vt::Q uv;
            if (!vt::fit(S, qx, qy, &uv)) flags |= SLHIP_VOTE_REFINE_STOPPED;
            for (int pass = 0; pass < 2; ++pass) {
                uint32_t count = 0u;
                std::vector<uint32_t> bits(nw, 0u);
                for (uint32_t j = 0u; j < K; ++j) {
                    if (rank[j] < 0) continue;
                    const vt::Voter& v = list[rank[j]];
                    if (!vt::inlier(uv.x, uv.y, v.px, v.py, v.dx, v.dy, cc)) continue;
                    bits[j >> 5] |= 1u << (j & 31u);
                    ++count;
                }
                if (pass == 0 && count < win_count) {
                    flags |= SLHIP_VOTE_REFINE_REJECTED;
                    uv.x = qx; uv.y = qy;
                    continue;
                }
                if (mask & SLHIP_VOTE_OUT_INLIERS)
                    for (uint32_t w = 0u; w < nw; ++w) out->inliers[o * nw + w] = bits[w];
                if (mask & SLHIP_VOTE_OUT_UV) { out->uv[o * 2u] = uv.x; out->uv[o * 2u + 1u] = uv.y; }
                if (mask & SLHIP_VOTE_OUT_N_INLIERS) out->n_inliers[o] = (int32_t)count;
                if (mask & SLHIP_VOTE_OUT_BEST) out->best[o] = best;
                if (mask & SLHIP_VOTE_OUT_FLAGS) out->flags[o] = flags;
                if (mask & SLHIP_VOTE_OUT_MEAN) { out->mean[o * 2u] = mean_x; out->mean[o * 2u + 1u] = mean_y; }
                if (mask & SLHIP_VOTE_OUT_COV)
                    for (int s = 0; s < 3; ++s) out->cov[o * 3u + s] = cov[s];
                break;
            }
        }
    return 0;
}
