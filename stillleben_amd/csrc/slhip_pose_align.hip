// Robust alignment (this project's addition, no counterpart in the reference): the pose of every set of K 3D-3D correspondences
// with the most inliers -- Horn's fit of three picked pairs inside RANSAC, then the rigid fit on the inliers.  It is to
// slhip_pose_fit what slhip_pose_pnp is to a plain PnP: predicted object coordinates onto camera points, or bank keypoints onto
// voted ones, when some of them are wrong by the size of the object.  include/slhip.h "Robust alignment" and DESIGN.md "Robust
// alignment" are the contract; all arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through
// slhip_align_rules.h and slhip_fit_block.h on host and device alike, so slhip_pose_align_host gives the kernel's outputs bit for
// bit.
//   k_pose_align  the RANSAC workgroup of slhip_ransac_block.h over the problem below: an entry of the valid list is (sx, sy, sz,
//                 dx, dy, dz), a hypothesis Philox, three picks, Horn and the Jacobi sweeps, a refinement step fit_centroids and
//                 fit_pose of slhip_fit_block.h over the valid list, the pair source "entry i, if an inlier of the current pose"
#include <hip/hip_runtime.h>

#include <cstdint>

#include "slhip.h"
#include "slhip_align_rules.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fit_block.h"
#include "slhip_ransac_block.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_align_params) == 64, "slhip_pose_align_params layout");

using Params = slhip_pose_align_params;
using Out = slhip_pose_align_out;
namespace al = slhip_align;
namespace ft = slhip_fit;
namespace rs = slhip_ransac;

static_assert(SLHIP_ALIGN_OUT_POSE == rs::OUT_POSE && SLHIP_ALIGN_OUT_N_INLIERS == rs::OUT_N_INLIERS && SLHIP_ALIGN_OUT_RMS == rs::OUT_RMS &&
                  SLHIP_ALIGN_OUT_INLIERS == rs::OUT_INLIERS && SLHIP_ALIGN_OUT_BEST == rs::OUT_BEST && SLHIP_ALIGN_OUT_FLAGS == rs::OUT_FLAGS,
              "the output bits of slhip_ransac_block.h");
static_assert(SLHIP_ALIGN_INSUFFICIENT == rs::INSUFFICIENT && SLHIP_ALIGN_NO_MODEL == rs::NO_MODEL &&
                  SLHIP_ALIGN_REFINE_STOPPED == rs::REFINE_STOPPED && SLHIP_ALIGN_REFINE_REJECTED == rs::REFINE_REJECTED,
              "the flags of slhip_ransac_block.h");

constexpr uint32_t BLOCK = al::BLOCK;

// The problem of one set.  src and dst: the set's own K correspondences (16-byte aligned on host and device alike).
struct Align {
    static constexpr uint32_t PLANES = 6u;      // sx sy sz dx dy dz
    static constexpr uint32_t MIN_VALID = 3u;
    static constexpr uint32_t PART_STRIDE = ft::FIT_SUMS;

    const float4* src;
    const float4* dst;
    float thr2, min_gap;
    uint32_t seed_lo, seed_hi, set_id;

    SLHIP_HD Align(const Params& p, const float* src_, const float* dst_, uint32_t set)
        : src(reinterpret_cast<const float4*>(src_) + (size_t)set * p.n_points),
          dst(reinterpret_cast<const float4*>(dst_) + (size_t)set * p.n_points), thr2(p.threshold * p.threshold), min_gap(p.min_gap),
          seed_lo(p.seed_lo), seed_hi(p.seed_hi), set_id(p.set_id_base + set)
    {
    }

    SLHIP_HD bool load(uint32_t j, float* c) const
    {
        const float4 a = src[j], b = dst[j];
        const float s[4] = {a.x, a.y, a.z, a.w}, d[4] = {b.x, b.y, b.z, b.w};
        c[0] = a.x; c[1] = a.y; c[2] = a.z;
        c[3] = b.x; c[4] = b.y; c[5] = b.z;
        return ft::used(s, d);
    }

    template <class Pick>
    SLHIP_HD bool hypothesis(uint32_t h, uint32_t n_valid, Pick pick, float* M) const
    {
        auto points = [&](uint32_t i, float* s, float* d) {
            float c[PLANES];
            pick(i, c);
            s[0] = c[0]; s[1] = c[1]; s[2] = c[2];
            d[0] = c[3]; d[1] = c[4]; d[2] = c[5];
        };
        return al::hypothesis(seed_lo, seed_hi, set_id, h, n_valid, min_gap, points, M);
    }

    SLHIP_HD bool inlier(const float* M, const float* c, float* e2) const
    {
        return al::inlier(M, c[0], c[1], c[2], c[3], c[4], c[5], thr2, e2);
    }

    // the pair source of the refit: entry i of the valid list as s[4] and d[4], false when it is no inlier of M
    template <class Pick>
    SLHIP_HD bool pair(const float* M, Pick pick, uint32_t i, float* s, float* d) const
    {
        float c[PLANES], e2;
        pick(i, c);
        s[0] = c[0]; s[1] = c[1]; s[2] = c[2];
        d[0] = c[3]; d[1] = c[4]; d[2] = c[5];
        s[3] = d[3] = 1.0f;
        return inlier(M, c, &e2);
    }

    // the rigid fit of the inliers of M among the valid list: lane l takes entries l, l + 256, ...
    template <class Pick>
    __device__ __forceinline__ bool refine(uint32_t n_valid, Pick pick, float* s_part, uint32_t* s_cnt, float* M) const
    {
        auto inliers = [&](uint32_t i, float* s, float* d) { return pair(M, pick, i, s, d); };
        float S[6], N[12];
        const uint32_t mine = ft::fit_centroids(n_valid, inliers, s_part, S);
        const uint32_t n_in = slhip_pose::block_count(mine, s_cnt, threadIdx.x / al::WAVE, threadIdx.x % al::WAVE);
        __syncthreads();      // s_cnt is written again by the final pass, which may come next
        if (n_in < 3u || !ft::fit_pose(n_valid, inliers, S, n_in, min_gap, s_part, N)) return false;      // the same for every lane
#pragma unroll
        for (int i = 0; i < 12; ++i) M[i] = N[i];
        return true;
    }

    template <class Pick>
    bool refine(uint32_t n_valid, Pick pick, float* M) const
    {
        auto inliers = [&](uint32_t i, float* s, float* d) { return pair(M, pick, i, s, d); };
        float S[6], N[12];
        const uint32_t n_in = ft::fit_centroids_host(n_valid, inliers, S);
        if (n_in < 3u || !ft::fit_pose_host(n_valid, inliers, S, n_in, min_gap, N)) return false;
        for (int i = 0; i < 12; ++i) M[i] = N[i];
        return true;
    }
};

// One block per set.  Dynamic LDS: PLANES * k_pad floats, k_pad = K rounded up to 4.
__global__ __launch_bounds__(BLOCK) void k_pose_align(Params p, const float* __restrict__ src, const float* __restrict__ dst,
                                                      const float* __restrict__ init, Out out, uint32_t k_pad)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    rs::solve_set(Align(p, src, dst, blockIdx.x), p, init, out, blockIdx.x, s_all, k_pad);
}

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
    const auto outputs = rs::output_list(out);
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
    if (const int st = rs::check_sizes(who, p->n_sets, p->n_points, Align::MIN_VALID, SLHIP_ALIGN_POINTS_MAX, p->n_hypotheses,
                                       SLHIP_ALIGN_HYPOTHESES_MAX, "threshold", p->threshold))
        return st;
    if (const int st = slhip::check_min_gap(who, p->min_gap)) return st;
    return rs::check_refine_and_outputs(who, p->refine_iters, SLHIP_ALIGN_REFINE_MAX, p->min_inliers, Align::MIN_VALID, p->outputs);
}

extern "C" int slhip_pose_align(const slhip_pose_align_params* params, const float* d_src, const float* d_dst, const float* d_init,
                                const slhip_pose_align_out* out, void* stream_)
{
    static const char* who = "slhip_pose_align";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_src, d_dst, d_init, out)) return st;
    if (params->n_sets == 0u) return 0;
    const uint32_t k_pad = slhip_pose::pad4(params->n_points);
    size_t lds;      // 6 KiB at K = 256, 24 KiB at 1024, 96 KiB at 4096
    SLHIP_CHECK(rs::reserve_lds(k_pose_align, Align::PLANES, k_pad, &lds));
    if (const int st = g_timer.begin(0, stream)) return st;
    k_pose_align<<<params->n_sets, BLOCK, lds, stream>>>(*params, d_src, d_dst, d_init, *out, k_pad);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

extern "C" int slhip_pose_align_host(const slhip_pose_align_params* params, const float* h_src, const float* h_dst, const float* h_init,
                                     const slhip_pose_align_out* out)
{
    static const char* who = "slhip_pose_align_host";
    if (const int st = check_call(who, params, h_src, h_dst, h_init, out)) return st;
    rs::solve_host<Align>(*params, h_init, *out, h_src, h_dst);
    return 0;
}
