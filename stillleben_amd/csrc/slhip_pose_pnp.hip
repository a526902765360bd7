// Pose PnP (this project's addition, no counterpart in the reference): the pose of every set of K 2D-3D correspondences by P3P
// inside RANSAC, then Gauss-Newton on the inliers.  include/slhip.h "Pose PnP" and DESIGN.md "Pose PnP" are the contract; all
// arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through slhip_pnp_rules.h on host and device alike,
// so slhip_pose_pnp_host gives the kernel's outputs bit for bit.
//   k_pose_pnp   the RANSAC workgroup of slhip_ransac_block.h over the problem below: an entry of the valid list is (u, v, x, y,
//                z), a hypothesis Philox and P3P, a refinement step Gauss-Newton with lanes over points, 27 sums in the order of
//                slhip_block_sum.h, and every lane solves the 6 x 6
#include <hip/hip_runtime.h>

#include <cstdint>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_pnp_rules.h"
#include "slhip_ransac_block.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_pnp_params) == 64, "slhip_pose_pnp_params layout");

using Params = slhip_pose_pnp_params;
using Out = slhip_pose_pnp_out;
namespace pn = slhip_pnp;
namespace rs = slhip_ransac;

static_assert(SLHIP_PNP_OUT_POSE == rs::OUT_POSE && SLHIP_PNP_OUT_N_INLIERS == rs::OUT_N_INLIERS && SLHIP_PNP_OUT_RMS == rs::OUT_RMS &&
                  SLHIP_PNP_OUT_INLIERS == rs::OUT_INLIERS && SLHIP_PNP_OUT_BEST == rs::OUT_BEST && SLHIP_PNP_OUT_FLAGS == rs::OUT_FLAGS,
              "the output bits of slhip_ransac_block.h");
static_assert(SLHIP_PNP_INSUFFICIENT == rs::INSUFFICIENT && SLHIP_PNP_NO_MODEL == rs::NO_MODEL &&
                  SLHIP_PNP_REFINE_STOPPED == rs::REFINE_STOPPED && SLHIP_PNP_REFINE_REJECTED == rs::REFINE_REJECTED,
              "the flags of slhip_ransac_block.h");

constexpr uint32_t BLOCK = pn::BLOCK;

// The problem of one set.  uv and xyz: the set's own K correspondences (8- and 16-byte aligned on host and device alike).
struct Pnp {
    static constexpr uint32_t PLANES = 5u;      // u v x y z
    static constexpr uint32_t MIN_VALID = 4u;
    static constexpr uint32_t PART_STRIDE = pn::SUMS + 1;      // the words of a wave's row of partial sums

    const float2* uv;
    const float4* xyz;
    pn::Camera cam;
    float thr2;
    uint32_t seed_lo, seed_hi, set_id;

    SLHIP_HD Pnp(const Params& p, const float* uv_, const float* xyz_, const float* intrinsics, uint32_t set)
        : uv(reinterpret_cast<const float2*>(uv_) + (size_t)set * p.n_points),
          xyz(reinterpret_cast<const float4*>(xyz_) + (size_t)set * p.n_points), cam{p.fx, p.fy, p.cx, p.cy},
          thr2(p.threshold_px * p.threshold_px), seed_lo(p.seed_lo), seed_hi(p.seed_hi), set_id(p.set_id_base + set)
    {
        if (intrinsics) {
            const float4 v = reinterpret_cast<const float4*>(intrinsics)[set];
            cam = {v.x, v.y, v.z, v.w};
        }
    }

    SLHIP_HD bool load(uint32_t j, float* c) const
    {
        const float2 a = uv[j];
        const float4 b = xyz[j];
        c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y; c[4] = b.z;
        return pn::valid(a.x, a.y, b.x, b.y, b.z, b.w);
    }

    template <class Pick>
    SLHIP_HD bool hypothesis(uint32_t h, uint32_t n_valid, Pick pick, float* M) const
    {
        return pn::hypothesis(seed_lo, seed_hi, set_id, h, n_valid, cam, pick, M);
    }

    SLHIP_HD bool inlier(const float* M, const float* c, float* e2) const
    {
        return pn::inlier(M, cam, c[2], c[3], c[4], c[0], c[1], thr2, e2);
    }

    // the 27 terms of entry i, if an inlier of M
    template <class Pick>
    SLHIP_HD void accumulate(const float* M, Pick pick, uint32_t i, float* acc) const
    {
        float c[PLANES], e2;
        pick(i, c);
        if (inlier(M, c, &e2)) pn::accumulate(M, cam, c[2], c[3], c[4], c[0], c[1], acc);
    }

    // Gauss-Newton on the inliers of M among the valid list: lane l takes entries l, l + 256, ...
    template <class Pick>
    __device__ __forceinline__ bool refine(uint32_t n_valid, Pick pick, float* s_part, uint32_t*, float* M) const
    {
        float acc[pn::SUMS], S[pn::SUMS];
#pragma unroll
        for (int i = 0; i < pn::SUMS; ++i) acc[i] = 0.0f;
        for (uint32_t i = threadIdx.x; i < n_valid; i += BLOCK) accumulate(M, pick, i, acc);
        slhip_pose::block_sums<pn::SUMS, PART_STRIDE>(acc, s_part, threadIdx.x / pn::WAVE, threadIdx.x % pn::WAVE, S);
        return pn::step(S, M);
    }

    template <class Pick>
    bool refine(uint32_t n_valid, Pick pick, float* M) const
    {
        slhip_pose::LaneSums<pn::SUMS> sums;
        for (uint32_t i = 0u; i < n_valid; ++i) sums.add(i, [&](float* acc) { accumulate(M, pick, i, acc); });
        float S[pn::SUMS];
        for (int s = 0; s < pn::SUMS; ++s) S[s] = sums.total(s);
        return pn::step(S, M);
    }
};

// One block per set.  Dynamic LDS: PLANES * k_pad floats, k_pad = K rounded up to 4.
__global__ __launch_bounds__(BLOCK) void k_pose_pnp(Params p, const float* __restrict__ uv, const float* __restrict__ xyz,
                                                    const float* __restrict__ intrinsics, const float* __restrict__ init, Out out,
                                                    uint32_t k_pad)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    rs::solve_set(Pnp(p, uv, xyz, intrinsics, blockIdx.x), p, init, out, blockIdx.x, s_all, k_pad);
}

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
    const auto outputs = rs::output_list(out);
    if (const int st = slhip::check_outputs_present(who, params->outputs, outputs)) return st;
    if (((uintptr_t)uv & 7u) || ((uintptr_t)xyz & 15u) || ((uintptr_t)intrinsics & 15u) || ((uintptr_t)init & 3u)) {
        slhip::set_error("%s: uv must be 8-byte aligned, xyz and the intrinsics 16-byte, the initial poses 4-byte", who);
        return -1;
    }
    return slhip::check_outputs_aligned(who, params->outputs, outputs);
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
    if (const int st = rs::check_sizes(who, p->n_sets, p->n_points, Pnp::MIN_VALID, SLHIP_PNP_POINTS_MAX, p->n_hypotheses,
                                       SLHIP_PNP_HYPOTHESES_MAX, "threshold_px", p->threshold_px))
        return st;
    return rs::check_refine_and_outputs(who, p->refine_iters, SLHIP_PNP_REFINE_MAX, p->min_inliers, Pnp::MIN_VALID, p->outputs);
}

extern "C" int slhip_pose_pnp(const slhip_pose_pnp_params* params, const float* d_uv, const float* d_xyz, const float* d_intrinsics,
                              const float* d_init, const slhip_pose_pnp_out* out, void* stream_)
{
    static const char* who = "slhip_pose_pnp";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_uv, d_xyz, d_intrinsics, d_init, out)) return st;
    if (params->n_sets == 0u) return 0;
    const uint32_t k_pad = slhip_pose::pad4(params->n_points);
    size_t lds;      // 5 KiB at K = 256, 20 KiB at 1024, 80 KiB at 4096
    SLHIP_CHECK(rs::reserve_lds(k_pose_pnp, Pnp::PLANES, k_pad, &lds));
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
    rs::solve_host<Pnp>(*params, h_init, *out, h_uv, h_xyz, h_intrinsics);
    return 0;
}
