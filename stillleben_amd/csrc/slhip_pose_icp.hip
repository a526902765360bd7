// ICP (this project's addition, no counterpart in the reference): the pose of every set of K camera points refined against the
// points of its class in a model bank, point to point -- the refinement that DenseFusion, PVN3D, FFB6D, PoseCNN+ICP and the BOP
// baselines run after their estimate.  include/slhip.h "ICP" and DESIGN.md "ICP" are the contract; all arithmetic is float32, one
// rounded operation at a time (-ffp-contract=off), through slhip_icp_rules.h and slhip_fit_rules.h on host and device alike, so
// slhip_pose_icp_host gives the kernel's outputs bit for bit.
//   k_pose_icp   one workgroup of 256 lanes per set.  The class's points go into LDS once, as three padded float arrays; they are
//                never transformed.  Per iteration  (A) association: a lane holds up to four camera points in registers, in the
//                object frame of the current pose, and walks the bank by broadcast 16-byte LDS reads (the walk of
//                slhip_pose_error.hip (B), restated with the index of the minimum); the matched index of every point goes to LDS,
//                (B) the fit of slhip_fit_block.h over the pairs: the count and the centroids, the moments, then every lane the
//                same 4 x 4 Jacobi in registers,  (C) lane 0 writes the stop word, every lane reads it behind a barrier.  The
//                residuals are summed once, for the pose the loop ends with.  No float atomics; the loop runs max_iters times at
//                the most.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fit_block.h"
#include "slhip_icp_rules.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_icp_params) == 64, "slhip_pose_icp_params layout");

using Params = slhip_pose_icp_params;
using Bank = slhip_pose_bank;
using Out = slhip_pose_icp_out;
namespace ic = slhip_icp;
namespace ft = slhip_fit;
using slhip_pose::pad_to_block;

constexpr uint32_t BLOCK = ic::BLOCK;
constexpr uint32_t NWAVES = BLOCK / ic::WAVE;
constexpr uint32_t QUERIES = 4u;                       // camera points a lane holds in registers in the walk
constexpr uint32_t QUERY_TILE = BLOCK * QUERIES;       // camera points of a workgroup per walk over the bank

// dynamic LDS of a launch: the bank's three coordinate arrays and the K matched indices (at most 48 KiB + 16 KiB)
inline size_t lds_bytes(uint32_t bank_points, uint32_t K) { return ((size_t)3u * pad_to_block(bank_points) + K) * 4u; }

// rule 4 for NQ queries in registers: four bank points per 16-byte read of each coordinate (every lane reads the same address:
// a broadcast), then the ragged rest one by one; upwards, so the lowest index of the smallest distance stays
template <int NQ>
__device__ __forceinline__ void nearest_walk(const float* qx, const float* qy, const float* qz, float* best, int* at, const float* s_x,
                                             const float* s_y, const float* s_z, uint32_t count)
{
    const uint32_t whole = count & ~3u;
    for (uint32_t j = 0u; j < whole; j += 4u) {
        const float4 tx = *reinterpret_cast<const float4*>(s_x + j);
        const float4 ty = *reinterpret_cast<const float4*>(s_y + j);
        const float4 tz = *reinterpret_cast<const float4*>(s_z + j);
        const float ax[4] = {tx.x, tx.y, tx.z, tx.w}, ay[4] = {ty.x, ty.y, ty.z, ty.w}, az[4] = {tz.x, tz.y, tz.z, tz.w};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int k = 0; k < NQ; ++k) ic::take(ic::dist2(qx[k], qy[k], qz[k], ax[t], ay[t], az[t]), (int)j + t, best[k], at[k]);
    }
    for (uint32_t j = whole; j < count; ++j) {
        const float ax = s_x[j], ay = s_y[j], az = s_z[j];
#pragma unroll
        for (int k = 0; k < NQ; ++k) ic::take(ic::dist2(qx[k], qy[k], qz[k], ax, ay, az), (int)j, best[k], at[k]);
    }
}

// rules 2 to 5 for the camera points first + lane + k * BLOCK, k < NQ, of one set: s_near[point] = the bank point it pairs with,
// or -1; returns the lane's pairs.  A slot at or past K reads point 0 and its result is dropped.
template <int NQ>
__device__ __forceinline__ uint32_t associate(const float* pose, const float4* __restrict__ cam, uint32_t first, uint32_t K, float gate,
                                              const float* s_x, const float* s_y, const float* s_z, uint32_t count, int32_t* s_near)
{
    float qx[NQ], qy[NQ], qz[NQ], best[NQ];
    int at[NQ];
    bool ok[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const uint32_t i = first + threadIdx.x + (uint32_t)k * BLOCK;
        const float4 c = cam[i < K ? i : 0u];
        ok[k] = i < K && ic::counts(c.x, c.y, c.z, c.w);
        ic::to_object(pose, c.x, c.y, c.z, qx[k], qy[k], qz[k]);
        best[k] = __builtin_inff();
        at[k] = ic::NONE;
    }
    nearest_walk<NQ>(qx, qy, qz, best, at, s_x, s_y, s_z, count);
    uint32_t pairs = 0u;
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const uint32_t i = first + threadIdx.x + (uint32_t)k * BLOCK;
        if (i < K) {
            const bool pair = ic::paired(ok[k], at[k], best[k], gate);
            s_near[i] = pair ? at[k] : -1;
            pairs += pair ? 1u : 0u;
        }
    }
    return pairs;
}

__device__ __forceinline__ uint32_t associate_n(uint32_t nq, const float* pose, const float4* __restrict__ cam, uint32_t first, uint32_t K,
                                                float gate, const float* s_x, const float* s_y, const float* s_z, uint32_t count,
                                                int32_t* s_near)
{
    switch (nq) {      // the same for every lane of the workgroup
    case 1u: return associate<1>(pose, cam, first, K, gate, s_x, s_y, s_z, count, s_near);
    case 2u: return associate<2>(pose, cam, first, K, gate, s_x, s_y, s_z, count, s_near);
    case 3u: return associate<3>(pose, cam, first, K, gate, s_x, s_y, s_z, count, s_near);
    default: return associate<4>(pose, cam, first, K, gate, s_x, s_y, s_z, count, s_near);
    }
}

// Dynamic LDS: 3 * n_pad floats (the bank's x, y, z) and K int32 (the matched indices).
__global__ __launch_bounds__(BLOCK) void k_pose_icp(Params p, const float4* __restrict__ camera, const float* __restrict__ init,
                                                    const int32_t* __restrict__ classes, Bank bank, Out out, uint32_t n_pad)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    __shared__ float s_part[NWAVES * ft::FIT_SUMS];
    __shared__ uint32_t s_cnt[NWAVES];
    __shared__ int s_word[2];      // [0] the stop and failure decision of lane 0, [1] the class's count
    float* s_x = s_all;
    float* s_y = s_x + n_pad;
    float* s_z = s_y + n_pad;
    int32_t* s_near = reinterpret_cast<int32_t*>(s_z + n_pad);

    const uint32_t K = p.n_points, tid = threadIdx.x, wave = tid / ic::WAVE, lane = tid % ic::WAVE, set = blockIdx.x, mask = p.outputs;
    const float4* cam = camera + (size_t)set * K;
    const float nan = __builtin_nanf("");

    // the pair of camera point j: false when it has none
    auto pair = [&](uint32_t j, float* s, float* d) {
        const int32_t m = s_near[j];
        if (m < 0) return false;
        const float4 c = cam[j];
        s[0] = s_x[m]; s[1] = s_y[m]; s[2] = s_z[m]; s[3] = 1.0f;
        d[0] = c.x; d[1] = c.y; d[2] = c.z; d[3] = c.w;
        return true;
    };

    float pose[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = init[(size_t)set * 12u + i];
    const int32_t cls = classes[set];

    // rule 1, decided by lane 0 and read by all behind a barrier
    if (tid == 0u) {
        const uint32_t c = ic::class_count(cls, bank.n_assets, bank.count, bank.n_points);
        s_word[0] = c == 0u ? SLHIP_ICP_BAD_CLASS : ic::init_ok(pose) ? 0 : SLHIP_ICP_NO_INIT;
        s_word[1] = (int)c;
    }
    __syncthreads();
    int flags = __builtin_amdgcn_readfirstlane(s_word[0]);
    const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane(s_word[1]);      // <= bank.n_points <= n_pad
    uint32_t n_pairs = 0u, iters = 0u;
    float rms = nan;
    bool have_pose = false;

    if (flags == 0) {      // the same for every lane
        {
            const float4* src = reinterpret_cast<const float4*>(bank.points) + (size_t)cls * bank.n_points;
            for (uint32_t i = tid; i < pad_to_block(count); i += BLOCK) {      // zeros up to the next multiple of BLOCK (never candidates)
                const float4 v = i < count ? src[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                s_x[i] = v.x;
                s_y[i] = v.y;
                s_z[i] = v.z;
            }
        }
        __syncthreads();

        float gate = p.max_dist;
        for (uint32_t it = 0u; it < p.max_iters; ++it) {
            // (A) association with the current pose
            uint32_t mine = 0u;
            for (uint32_t first = 0u; first < K; first += QUERY_TILE) {
                if (first + wave * ic::WAVE >= K) break;      // nothing left for this wave, nor in any later tile (no barrier inside)
                const uint32_t nq = min(QUERIES, (K - first + BLOCK - 1u) / BLOCK);
                mine += associate_n(nq, pose, cam, first, K, gate, s_x, s_y, s_z, count, s_near);
            }

            // (B) the fit over the pairs (the barrier of the count also puts the matched indices in LDS)
            n_pairs = (uint32_t)__builtin_amdgcn_readfirstlane((int)slhip_pose::block_count(mine, s_cnt, wave, lane));
            if (n_pairs < p.min_pairs) {      // the same for every lane
                flags = SLHIP_ICP_INSUFFICIENT;
                have_pose = false;
                break;
            }
            float S[6], next[12];
            ft::fit_centroids(K, pair, s_part, S);
            const bool fitted = ft::fit_pose(K, pair, S, n_pairs, p.min_gap, s_part, next);

            // (C) lane 0 decides, every lane reads the decision behind a barrier
            if (tid == 0u) s_word[0] = !fitted ? SLHIP_ICP_DEGENERATE : ic::converged(pose, next, p.tol_rot, p.tol_trans) ? SLHIP_ICP_CONVERGED : 0;
            __syncthreads();
            const int stop = __builtin_amdgcn_readfirstlane(s_word[0]);      // (the next write lies behind the barriers of the next sums)
            if (stop & SLHIP_ICP_DEGENERATE) {
                flags = SLHIP_ICP_DEGENERATE;
                have_pose = false;
                break;
            }
#pragma unroll
            for (int i = 0; i < 12; ++i) pose[i] = next[i];
            have_pose = true;
            iters = it + 1u;
            gate = ic::next_gate(gate, p.dist_scale, p.min_dist);
            if ((stop & SLHIP_ICP_CONVERGED) || iters == p.max_iters) {
                flags = stop & SLHIP_ICP_CONVERGED;
                if (mask & SLHIP_ICP_OUT_RMS) rms = ft::fit_rms(K, pair, pose, n_pairs, s_part);      // rule 7, once: for the pose the loop ends with
                break;
            }
        }
    }

    // the outputs: the matched indices by every lane, the rest by lane 0
    if (mask & SLHIP_ICP_OUT_NEAREST) {
        const bool started = !(flags & (SLHIP_ICP_BAD_CLASS | SLHIP_ICP_NO_INIT));
        for (uint32_t j = tid; j < K; j += BLOCK) out.nearest[(size_t)set * K + j] = started ? s_near[j] : -1;
    }
    if (tid == 0u) {
        if (mask & SLHIP_ICP_OUT_POSE)
#pragma unroll
            for (uint32_t i = 0u; i < 12u; ++i) out.pose[(size_t)set * 12u + i] = have_pose ? pose[i] : nan;
        if (mask & SLHIP_ICP_OUT_N_PAIRS) out.n_pairs[set] = (int32_t)n_pairs;
        if (mask & SLHIP_ICP_OUT_RMS) out.rms[set] = rms;
        if (mask & SLHIP_ICP_OUT_ITERS) out.iters[set] = (int32_t)iters;
        if (mask & SLHIP_ICP_OUT_FLAGS) out.flags[set] = flags;
    }
}

constexpr uint32_t ALL_OUTPUTS = SLHIP_ICP_OUT_POSE | SLHIP_ICP_OUT_N_PAIRS | SLHIP_ICP_OUT_RMS | SLHIP_ICP_OUT_ITERS | SLHIP_ICP_OUT_FLAGS |
                                 SLHIP_ICP_OUT_NEAREST;

bool at_least_zero(float v) { return v >= 0.0f; }      // (a NaN is not)

// the checks that slhip_pose_icp and slhip_pose_icp_host share
int check_call(const char* who, const Params* params, const float* camera, const float* init, const int32_t* classes, const Bank* b,
               const Out* out)
{
    if (const int st = slhip_pose_icp_check_params(params)) return st;
    if (!camera || !init || !classes || !b || !out) {
        slhip::set_error("%s: null argument (camera, init, classes, the bank and the output record are required)", who);
        return -1;
    }
    if (!b->points || !b->count) {
        slhip::set_error("%s: null argument (the bank's points and count are required)", who);
        return -1;
    }
    const uint32_t m = params->outputs;
    const slhip::OutputList outputs = {{SLHIP_ICP_OUT_POSE, out->pose},   {SLHIP_ICP_OUT_N_PAIRS, out->n_pairs}, {SLHIP_ICP_OUT_RMS, out->rms},
                                       {SLHIP_ICP_OUT_ITERS, out->iters}, {SLHIP_ICP_OUT_FLAGS, out->flags},     {SLHIP_ICP_OUT_NEAREST, out->nearest}};
    if (const int st = slhip::check_outputs_present(who, m, outputs)) return st;
    if (((uintptr_t)camera & 15u) || ((uintptr_t)init & 15u) || ((uintptr_t)b->points & 15u)) {
        slhip::set_error("%s: camera, init and the bank's points must be 16-byte aligned", who);
        return -1;
    }
    if (((uintptr_t)classes & 3u) || ((uintptr_t)b->count & 3u)) {
        slhip::set_error("%s: classes and the bank's count must be 4-byte aligned", who);
        return -1;
    }
    if (const int st = slhip::check_outputs_aligned(who, m, outputs)) return st;
    if (const int st = slhip::check_range(who, "the bank's n_assets", b->n_assets, 1u, SLHIP_SYNTH_MAX_ASSETS)) return st;
    return slhip::check_range(who, "the bank's n_points", b->n_points, 1u, SLHIP_POSE_POINTS_MAX);
}

// optional HIP-event timing (tools/time_pose_icp.py): events round the last call
slhip::StepTimer<1> g_timer;

}  // namespace

extern "C" int slhip_pose_icp_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_pose_icp_timings(float ms_out[1]) { return g_timer.read_for("slhip_pose_icp_timings", ms_out); }

extern "C" int slhip_pose_icp_check_params(const slhip_pose_icp_params* p)
{
    static const char* who = "slhip_pose_icp";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 1u, SLHIP_ICP_POINTS_MAX)) return st;
    if (const int st = slhip::check_range(who, "max_iters", p->max_iters, 1u, SLHIP_ICP_ITERS_MAX)) return st;
    if (const int st = slhip::check_range(who, "min_pairs", p->min_pairs, 3u, 0xffffffffu)) return st;
    if (!at_least_zero(p->max_dist)) {
        slhip::set_error("%s: max_dist %g must be at least 0 (+inf: no gate)", who, (double)p->max_dist);
        return -1;
    }
    if (!(p->dist_scale > 0.0f) || !(p->dist_scale <= 1.0f)) {
        slhip::set_error("%s: dist_scale %g must lie in (0, 1]", who, (double)p->dist_scale);
        return -1;
    }
    if (!at_least_zero(p->min_dist)) {
        slhip::set_error("%s: min_dist %g must be at least 0", who, (double)p->min_dist);
        return -1;
    }
    if (const int st = slhip::check_min_gap(who, p->min_gap)) return st;
    if (!at_least_zero(p->tol_rot)) {
        slhip::set_error("%s: tol_rot %g must be at least 0", who, (double)p->tol_rot);
        return -1;
    }
    if (!at_least_zero(p->tol_trans)) {
        slhip::set_error("%s: tol_trans %g must be at least 0", who, (double)p->tol_trans);
        return -1;
    }
    if (p->outputs == 0u || (p->outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of pose 1, n_pairs 2, rms 4, iters 8, flags 16, nearest 32 and nothing else",
                         who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_pose_icp(const slhip_pose_icp_params* params, const float* d_camera, const float* d_init, const int32_t* d_classes,
                              const slhip_pose_bank* bank, const slhip_pose_icp_out* out, void* stream_)
{
    static const char* who = "slhip_pose_icp";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_camera, d_init, d_classes, bank, out)) return st;
    if (params->n_sets == 0u) return 0;
    const uint32_t n_pad = pad_to_block(bank->n_points);
    const size_t lds = lds_bytes(bank->n_points, params->n_points);      // 4 KiB at 256 x 256, 64 KiB at 4096 x 4096
    if (lds > 32u * 1024u)      // with the kernel's own words past what a kernel may ask for without the attribute (per device, so not remembered)
        SLHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_icp), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (const int st = g_timer.begin(0, stream)) return st;
    k_pose_icp<<<params->n_sets, BLOCK, lds, stream>>>(*params, reinterpret_cast<const float4*>(d_camera), d_init, d_classes, *bank, *out, n_pad);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

extern "C" int slhip_pose_icp_host(const slhip_pose_icp_params* params, const float* h_camera, const float* h_init, const int32_t* h_classes,
                                   const slhip_pose_bank* b, const slhip_pose_icp_out* out)
{
    static const char* who = "slhip_pose_icp_host";
    if (const int st = check_call(who, params, h_camera, h_init, h_classes, b, out)) return st;
    const Params& p = *params;
    const uint32_t K = p.n_points, mask = p.outputs;
    const float nan = __builtin_nanf("");
    std::vector<int32_t> near(K);
    for (uint32_t set = 0u; set < p.n_sets; ++set) {
        const float* cam = h_camera + (size_t)set * K * 4u;
        float pose[12];
        for (int i = 0; i < 12; ++i) pose[i] = h_init[(size_t)set * 12u + i];
        const int32_t cls = h_classes[set];
        const uint32_t count = ic::class_count(cls, b->n_assets, b->count, b->n_points);
        int flags = count == 0u ? SLHIP_ICP_BAD_CLASS : ic::init_ok(pose) ? 0 : SLHIP_ICP_NO_INIT;
        uint32_t n_pairs = 0u, iters = 0u;
        float rms = nan;
        bool have_pose = false;
        std::fill(near.begin(), near.end(), -1);
        if (flags == 0) {
            const float* pts = b->points + (size_t)cls * b->n_points * 4u;
            float gate = p.max_dist;
            // the pair of camera point j: false when it has none
            auto pair = [&](uint32_t j, float* s, float* d) {
                const int32_t m = near[j];
                if (m < 0) return false;
                s[0] = pts[4 * m]; s[1] = pts[4 * m + 1]; s[2] = pts[4 * m + 2]; s[3] = 1.0f;
                for (int i = 0; i < 4; ++i) d[i] = cam[4u * j + i];
                return true;
            };
            for (uint32_t it = 0u; it < p.max_iters; ++it) {
                n_pairs = 0u;
                for (uint32_t j = 0u; j < K; ++j) {
                    const float* c = cam + 4u * j;
                    float qx, qy, qz, best = __builtin_inff();
                    int at = ic::NONE;
                    ic::to_object(pose, c[0], c[1], c[2], qx, qy, qz);
                    for (uint32_t m = 0u; m < count; ++m) ic::take(ic::dist2(qx, qy, qz, pts[4 * m], pts[4 * m + 1], pts[4 * m + 2]), (int)m, best, at);
                    const bool pair = ic::paired(ic::counts(c[0], c[1], c[2], c[3]), at, best, gate);
                    near[j] = pair ? at : -1;
                    n_pairs += pair ? 1u : 0u;
                }
                if (n_pairs < p.min_pairs) {
                    flags = SLHIP_ICP_INSUFFICIENT;
                    have_pose = false;
                    break;
                }
                float S[6], next[12];
                ft::fit_centroids_host(K, pair, S);
                if (!ft::fit_pose_host(K, pair, S, n_pairs, p.min_gap, next)) {
                    flags = SLHIP_ICP_DEGENERATE;
                    have_pose = false;
                    break;
                }
                const bool conv = ic::converged(pose, next, p.tol_rot, p.tol_trans);
                for (int i = 0; i < 12; ++i) pose[i] = next[i];
                have_pose = true;
                iters = it + 1u;
                gate = ic::next_gate(gate, p.dist_scale, p.min_dist);
                if (conv || iters == p.max_iters) {
                    flags = conv ? SLHIP_ICP_CONVERGED : 0;
                    rms = ft::fit_rms_host(K, pair, pose, n_pairs);
                    break;
                }
            }
        }
        if (mask & SLHIP_ICP_OUT_NEAREST)
            for (uint32_t j = 0u; j < K; ++j) out->nearest[(size_t)set * K + j] = near[j];
        if (mask & SLHIP_ICP_OUT_POSE)
            for (uint32_t i = 0u; i < 12u; ++i) out->pose[(size_t)set * 12u + i] = have_pose ? pose[i] : nan;
        if (mask & SLHIP_ICP_OUT_N_PAIRS) out->n_pairs[set] = (int32_t)n_pairs;
        if (mask & SLHIP_ICP_OUT_RMS) out->rms[set] = rms;
        if (mask & SLHIP_ICP_OUT_ITERS) out->iters[set] = (int32_t)iters;
        if (mask & SLHIP_ICP_OUT_FLAGS) out->flags[set] = flags;
    }
    return 0;
}
