// Pose errors (this project's addition, no counterpart in the reference): ADD, ADD-S, MSSD and MSPD of pose estimates against a
// batch's ground truth, with the symmetries of every class.  include/slhip.h "Pose errors" and DESIGN.md "Pose errors" are the
// contract; all arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through slhip_pose_rules.h on host
// and device alike, so tests/pose_error_ref.py restates it and every output is bit-exact against it.
//   k_pose_error     one workgroup per (scene, object) and share of its hypotheses: the class's points in LDS once, then per
//                    hypothesis  (A) q = p + R_g^T (e - g) p into LDS, the ADD terms and the estimate's pixels,  (B) ADD-S: a lane holds up to
//                    four queries in registers and walks the targets by broadcast 16-byte LDS reads,  (C) the symmetry sweep:
//                    the symmetries dealt over the four waves, a lane takes four consecutive points per 16-byte read
//   k_pose_diameter  the tile loop of (B) with max in place of min, the queries split over workgroups, joined by an integer
//                    atomic max on the bits of the squared distance;  k_pose_sqrt finishes
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_pose_rules.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_pose_error_params) == 32, "slhip_pose_error_params layout");
static_assert(sizeof(slhip_pose_bank) == 48, "slhip_pose_bank layout");

using Params = slhip_pose_error_params;
using Bank = slhip_pose_bank;
using Out = slhip_pose_error_out;
namespace pr = slhip_pose;

constexpr uint32_t BLOCK = pr::BLOCK;
constexpr uint32_t NWAVES = BLOCK / pr::WAVE;
constexpr uint32_t QUERIES = 4u;                       // queries a lane holds in registers in the all-pairs loops
constexpr uint32_t QUERY_TILE = BLOCK * QUERIES;       // queries of a workgroup per walk over the targets
constexpr uint32_t LDS_ARRAYS = 8u;                    // p.x p.y p.z q.x q.y q.z u v, each n_pad floats

using pr::pad_to_block;
using pr::wave_max;
using pr::wave_sum;

// min (or max) over the targets [0, count) of dist2(query, target) for NQ queries in registers: four targets per 16-byte read
// of each coordinate (every lane reads the same address: a broadcast), then the ragged rest one by one
template <int NQ, bool IS_MAX>
__device__ __forceinline__ void all_pairs(const float* qx, const float* qy, const float* qz, float* best, const float* s_x,
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
            for (int k = 0; k < NQ; ++k) {
                const float d = pr::dist2(qx[k], qy[k], qz[k], ax[t], ay[t], az[t]);
                best[k] = IS_MAX ? fmaxf(best[k], d) : fminf(best[k], d);
            }
    }
    for (uint32_t j = whole; j < count; ++j) {
        const float ax = s_x[j], ay = s_y[j], az = s_z[j];
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
            const float d = pr::dist2(qx[k], qy[k], qz[k], ax, ay, az);
            best[k] = IS_MAX ? fmaxf(best[k], d) : fminf(best[k], d);
        }
    }
}

// queries first + lane + k * BLOCK, k < NQ, of (x, y, z) against the targets (t_x, t_y, t_z); a query at or past `count` is a
// copy of point 0 whose result the caller drops
template <int NQ, bool IS_MAX>
__device__ __forceinline__ void query_tile(const float* x, const float* y, const float* z, const float* t_x, const float* t_y,
                                           const float* t_z, uint32_t first, uint32_t count, float* best)
{
    float qx[NQ], qy[NQ], qz[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) {
        const uint32_t i = first + threadIdx.x + (uint32_t)k * BLOCK, at = i < count ? i : 0u;
        qx[k] = x[at];
        qy[k] = y[at];
        qz[k] = z[at];
    }
    all_pairs<NQ, IS_MAX>(qx, qy, qz, best, t_x, t_y, t_z, count);
}

template <bool IS_MAX>
__device__ __forceinline__ void query_tile_n(uint32_t nq, const float* x, const float* y, const float* z, const float* t_x,
                                             const float* t_y, const float* t_z, uint32_t first, uint32_t count, float* best)
{
    switch (nq) {      // the same for every lane of the workgroup
    case 1u: query_tile<1, IS_MAX>(x, y, z, t_x, t_y, t_z, first, count, best); break;
    case 2u: query_tile<2, IS_MAX>(x, y, z, t_x, t_y, t_z, first, count, best); break;
    case 3u: query_tile<3, IS_MAX>(x, y, z, t_x, t_y, t_z, first, count, best); break;
    default: query_tile<4, IS_MAX>(x, y, z, t_x, t_y, t_z, first, count, best); break;
    }
}

// the points of class `cls` into LDS, zeros up to the next multiple of BLOCK
__device__ __forceinline__ void load_points(const Bank& bank, uint32_t cls, uint32_t count, float* s_x, float* s_y, float* s_z)
{
    const float4* src = reinterpret_cast<const float4*>(bank.points) + (size_t)cls * bank.n_points;
    for (uint32_t i = threadIdx.x; i < pad_to_block(count); i += BLOCK) {
        const float4 v = i < count ? src[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_x[i] = v.x;
        s_y[i] = v.y;
        s_z[i] = v.z;
    }
}

__device__ __forceinline__ void write_all(const Out& out, uint32_t mask, size_t at, float v, int idx)
{
    if (mask & SLHIP_POSE_OUT_ADD) out.add[at] = v;
    if (mask & SLHIP_POSE_OUT_ADDS) out.adds[at] = v;
    if (mask & SLHIP_POSE_OUT_MSSD) {
        out.mssd[at] = v;
        out.mssd_sym[at] = idx;
    }
    if (mask & SLHIP_POSE_OUT_MSPD) {
        out.mspd[at] = v;
        out.mspd_sym[at] = idx;
    }
}

// Blocks (x, y): x = scene * O + object, y takes the hypotheses y, y + gridDim.y, ...  Dynamic LDS: LDS_ARRAYS * n_pad floats.
__global__ __launch_bounds__(BLOCK) void k_pose_error(Params p, Bank bank, const int32_t* __restrict__ classes,
                                                      uint32_t class_stride, const float* __restrict__ gt,
                                                      const float* __restrict__ est, Out out, uint32_t n_pad)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    __shared__ float s_sum[2][NWAVES];
    __shared__ float s_val[2][NWAVES];
    __shared__ int s_idx[2][NWAVES];
    __shared__ int s_behind;
    float* s_px = s_all;
    float* s_py = s_px + n_pad;
    float* s_pz = s_py + n_pad;
    float* s_qx = s_pz + n_pad;
    float* s_qy = s_qx + n_pad;
    float* s_qz = s_qy + n_pad;
    float* s_u = s_qz + n_pad;
    float* s_v = s_u + n_pad;

    const uint32_t tid = threadIdx.x, wave = tid / pr::WAVE, lane = tid % pr::WAVE;
    const uint32_t so = blockIdx.x, Hy = p.n_hypotheses, mask = p.outputs;
    const uint32_t cls = (uint32_t)classes[(size_t)so * class_stride];
    int32_t count_ = 0, n_sym_ = 0;
    if (cls < bank.n_assets) {
        count_ = bank.count[cls];
        n_sym_ = bank.n_sym[cls];
    }
    if (!pr::class_ok(count_, bank.n_points, n_sym_, bank.n_symmetries)) {      // +inf and -1, a hypothesis per lane
        for (uint32_t h = blockIdx.y + gridDim.y * tid; h < Hy; h += gridDim.y * BLOCK)
            write_all(out, mask, (size_t)so * Hy + h, __builtin_inff(), -1);
        return;
    }
    const uint32_t count = (uint32_t)count_, n_sym = (uint32_t)n_sym_;      // count <= n_points <= n_pad
    load_points(bank, cls, count, s_px, s_py, s_pz);
    float g[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) g[i] = gt[(size_t)so * 12u + i];
    const float* sym = bank.symmetries + (size_t)cls * bank.n_symmetries * 12u;

    for (uint32_t h = blockIdx.y; h < Hy; h += gridDim.y) {
        const size_t at = (size_t)so * Hy + h;
        float e[12], D[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) e[i] = est[at * 12u + i];
        pr::difference(g, e, D);
        if (!pr::all_finite(D)) {      // the same for every lane
            if (tid == 0u) write_all(out, mask, at, __builtin_nanf(""), -1);
            continue;
        }
        if (tid == 0u) s_behind = 0;
        __syncthreads();      // the points are in LDS; the sweep of the hypothesis before has read its q, u and v

        // (A) q = p + R_g^T (D p), the ADD terms, the estimate's pixels
        float acc_add = 0.0f, acc_adds = 0.0f;
        bool behind = false;
        for (uint32_t i = tid; i < count; i += BLOCK) {
            const float x = s_px[i], y = s_py[i], z = s_pz[i];
            const pr::Moved m = pr::move_point(g, D, x, y, z);
            s_qx[i] = m.qx;
            s_qy[i] = m.qy;
            s_qz[i] = m.qz;
            if (mask & SLHIP_POSE_OUT_ADD) acc_add = acc_add + sqrtf(m.add2);
            if (mask & SLHIP_POSE_OUT_MSPD) {
                const float X = pr::row_point(e, x, y, z), Y = pr::row_point(e + 4, x, y, z), Z = pr::row_point(e + 8, x, y, z);
                behind = behind || !(Z > 0.0f);
                s_u[i] = pr::pixel_u(p.fx, X, Z, p.cx);
                s_v[i] = pr::pixel_u(p.fy, Y, Z, p.cy);
            }
        }
        // (B) ADD-S: the lane's queries against every point of the class
        __syncthreads();      // (a query past the end is a copy of q_0, which lane 0 wrote)
        if (mask & SLHIP_POSE_OUT_ADDS) {
            for (uint32_t first = 0u; first < count; first += QUERY_TILE) {
                if (first + wave * pr::WAVE >= count) break;      // nothing left for this wave, nor in any later tile
                const uint32_t nq = min(QUERIES, (count - first + BLOCK - 1u) / BLOCK);
                float best[QUERIES] = {__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
                query_tile_n<false>(nq, s_qx, s_qy, s_qz, s_px, s_py, s_pz, first, count, best);
#pragma unroll
                for (uint32_t k = 0u; k < QUERIES; ++k)
                    if (k < nq && first + tid + k * BLOCK < count) acc_adds = acc_adds + sqrtf(best[k]);
            }
        }
        if (mask & SLHIP_POSE_OUT_ADD) {
            const float w = wave_sum(acc_add);
            if (lane == 0u) s_sum[0][wave] = w;
        }
        if (mask & SLHIP_POSE_OUT_ADDS) {
            const float w = wave_sum(acc_adds);
            if (lane == 0u) s_sum[1][wave] = w;
        }
        if (behind) s_behind = 1;
        __syncthreads();      // q, u and v of every point are in LDS

        // (C) the symmetry sweep: wave w takes s = w, w + 4, ...; a lane four consecutive points per read
        if (mask & (SLHIP_POSE_OUT_MSSD | SLHIP_POSE_OUT_MSPD)) {
            pr::Best b3 = pr::best_start(), b2 = pr::best_start();
            bool g_behind = false;
            for (uint32_t s = wave; s < n_sym; s += NWAVES) {
                float S[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) S[i] = sym[(size_t)s * 12u + i];
                float m3 = 0.0f, m2 = 0.0f;
                for (uint32_t i0 = lane * 4u; i0 < count; i0 += BLOCK) {      // i0 + 3 < pad_to_block(count) <= n_pad
                    const float4 X4 = *reinterpret_cast<const float4*>(s_px + i0), Y4 = *reinterpret_cast<const float4*>(s_py + i0);
                    const float4 Z4 = *reinterpret_cast<const float4*>(s_pz + i0);
                    const float4 QX = *reinterpret_cast<const float4*>(s_qx + i0), QY = *reinterpret_cast<const float4*>(s_qy + i0);
                    const float4 QZ = *reinterpret_cast<const float4*>(s_qz + i0);
                    const float px[4] = {X4.x, X4.y, X4.z, X4.w}, py[4] = {Y4.x, Y4.y, Y4.z, Y4.w}, pz[4] = {Z4.x, Z4.y, Z4.z, Z4.w};
                    const float qx[4] = {QX.x, QX.y, QX.z, QX.w}, qy[4] = {QY.x, QY.y, QY.z, QY.w}, qz[4] = {QZ.x, QZ.y, QZ.z, QZ.w};
                    float ue[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ve[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (mask & SLHIP_POSE_OUT_MSPD) {
                        const float4 U4 = *reinterpret_cast<const float4*>(s_u + i0), V4 = *reinterpret_cast<const float4*>(s_v + i0);
                        ue[0] = U4.x; ue[1] = U4.y; ue[2] = U4.z; ue[3] = U4.w;
                        ve[0] = V4.x; ve[1] = V4.y; ve[2] = V4.z; ve[3] = V4.w;
                    }
#pragma unroll
                    for (uint32_t t = 0u; t < 4u; ++t) {
                        const bool live = i0 + t < count;
                        const float yx = pr::row_point(S, px[t], py[t], pz[t]), yy = pr::row_point(S + 4, px[t], py[t], pz[t]);
                        const float yz = pr::row_point(S + 8, px[t], py[t], pz[t]);
                        if (mask & SLHIP_POSE_OUT_MSSD) {
                            const float d = pr::dist2(qx[t], qy[t], qz[t], yx, yy, yz);
                            m3 = fmaxf(m3, live ? d : 0.0f);
                        }
                        if (mask & SLHIP_POSE_OUT_MSPD) {
                            const float X = pr::row_point(g, yx, yy, yz), Y = pr::row_point(g + 4, yx, yy, yz);
                            const float Z = pr::row_point(g + 8, yx, yy, yz);
                            g_behind = g_behind || (live && !(Z > 0.0f));
                            const float d = pr::pixel_dist2(ue[t], ve[t], pr::pixel_u(p.fx, X, Z, p.cx), pr::pixel_u(p.fy, Y, Z, p.cy));
                            m2 = fmaxf(m2, live ? d : 0.0f);
                        }
                    }
                }
                pr::Best c;
                c.idx = (int)s;
                c.val = wave_max(m3);
                b3 = pr::join(b3, c);
                c.val = wave_max(m2);
                b2 = pr::join(b2, c);
            }
            if (g_behind) s_behind = 1;
            if (lane == 0u) {
                s_val[0][wave] = b3.val;
                s_idx[0][wave] = b3.idx;
                s_val[1][wave] = b2.val;
                s_idx[1][wave] = b2.idx;
            }
        }
        __syncthreads();
        if (tid == 0u) {
            const float n = (float)count;
            if (mask & SLHIP_POSE_OUT_ADD) out.add[at] = pr::waves_sum(s_sum[0]) / n;
            if (mask & SLHIP_POSE_OUT_ADDS) out.adds[at] = pr::waves_sum(s_sum[1]) / n;
            pr::Best b3 = pr::best_start(), b2 = pr::best_start();
            for (uint32_t w = 0u; w < NWAVES; ++w) {
                pr::Best c;
                c.val = s_val[0][w];
                c.idx = s_idx[0][w];
                b3 = pr::join(b3, c);
                c.val = s_val[1][w];
                c.idx = s_idx[1][w];
                b2 = pr::join(b2, c);
            }
            if (mask & SLHIP_POSE_OUT_MSSD) {
                out.mssd[at] = sqrtf(b3.val);
                out.mssd_sym[at] = pr::best_index(b3);
            }
            if (mask & SLHIP_POSE_OUT_MSPD) {
                const bool hidden = s_behind != 0;
                out.mspd[at] = hidden ? __builtin_inff() : sqrtf(b2.val);
                out.mspd_sym[at] = hidden ? -1 : pr::best_index(b2);
            }
        }
    }
}

// Blocks (x, y): class x, queries [y * QUERY_TILE, ...) against every point of the class.  Dynamic LDS: 3 * n_pad floats.
// d_bits: the squared diameters as the bit patterns of non-negative floats, zeroed by the entry.
__global__ __launch_bounds__(BLOCK) void k_pose_diameter(Bank bank, uint32_t* __restrict__ d_bits, uint32_t n_pad)
{
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    __shared__ float s_max[NWAVES];
    float* s_px = s_all;
    float* s_py = s_px + n_pad;
    float* s_pz = s_py + n_pad;
    const uint32_t cls = blockIdx.x, first = blockIdx.y * QUERY_TILE;
    const int32_t count_ = bank.count[cls];
    if (count_ < 1 || (uint32_t)count_ > bank.n_points || first >= (uint32_t)count_) return;      // the same for every lane
    const uint32_t count = (uint32_t)count_;
    load_points(bank, cls, count, s_px, s_py, s_pz);
    __syncthreads();
    const uint32_t nq = min(QUERIES, (count - first + BLOCK - 1u) / BLOCK);
    float best[QUERIES] = {0.0f, 0.0f, 0.0f, 0.0f};
    query_tile_n<true>(nq, s_px, s_py, s_pz, s_px, s_py, s_pz, first, count, best);      // (a query past the end is point 0 again)
    const float w = wave_max(fmaxf(fmaxf(best[0], best[1]), fmaxf(best[2], best[3])));
    if (threadIdx.x % pr::WAVE == 0u) s_max[threadIdx.x / pr::WAVE] = w;
    __syncthreads();
    if (threadIdx.x == 0u) atomicMax(d_bits + cls, __float_as_uint(fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]))));
}

__global__ __launch_bounds__(BLOCK) void k_pose_sqrt(float* __restrict__ d, uint32_t n)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) d[i] = sqrtf(d[i]);
}

int check_bank(const char* who, const Bank* b)
{
    if (!b || !b->points || !b->count || !b->symmetries || !b->n_sym) {
        slhip::set_error("%s: null argument (the bank and its points, count, symmetries and n_sym are required)", who);
        return -1;
    }
    if (((uintptr_t)b->points & 15u) || ((uintptr_t)b->symmetries & 15u)) {
        slhip::set_error("%s: the bank's points and symmetries must be 16-byte aligned", who);
        return -1;
    }
    if (((uintptr_t)b->count & 3u) || ((uintptr_t)b->n_sym & 3u)) {
        slhip::set_error("%s: the bank's count and n_sym must be 4-byte aligned", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_assets", b->n_assets, 1u, SLHIP_SYNTH_MAX_ASSETS)) return st;
    if (const int st = slhip::check_range(who, "n_points", b->n_points, 1u, SLHIP_POSE_POINTS_MAX)) return st;
    return slhip::check_range(who, "n_symmetries", b->n_symmetries, 1u, SLHIP_POSE_SYMMETRIES_MAX);
}

// the checks that slhip_pose_error and slhip_pose_error_host share
int check_call(const char* who, const Params* params, const Bank* bank, const int32_t* classes, uint32_t class_stride,
               const float* gt, const float* est, uint32_t n_scenes, const Out* out)
{
    if (const int st = slhip_pose_error_check_params(params)) return st;
    if (const int st = check_bank(who, bank)) return st;
    if (!classes || !gt || !est || !out) {
        slhip::set_error("%s: null argument (classes, ground truth, estimates and the output record are required)", who);
        return -1;
    }
    if (class_stride == 0u) {
        slhip::set_error("%s: class_stride must be at least 1 (1: a plain tensor, 4: slhip_synth_object records)", who);
        return -1;
    }
    const slhip::OutputList outputs = {{SLHIP_POSE_OUT_ADD, out->add},   {SLHIP_POSE_OUT_ADDS, out->adds},     {SLHIP_POSE_OUT_MSSD, out->mssd},
                                       {SLHIP_POSE_OUT_MSSD, out->mssd_sym}, {SLHIP_POSE_OUT_MSPD, out->mspd}, {SLHIP_POSE_OUT_MSPD, out->mspd_sym}};
    if (const int st = slhip::check_outputs_present(who, params->outputs, outputs)) return st;
    if (((uintptr_t)classes & 3u) || ((uintptr_t)gt & 3u) || ((uintptr_t)est & 3u)) {
        slhip::set_error("%s: classes, ground truth and estimates must be 4-byte aligned", who);
        return -1;
    }
    if ((uint64_t)n_scenes * params->n_objects > 0x7fffffffu) {
        slhip::set_error("%s: %u scenes x %u objects do not fit one launch", who, n_scenes, params->n_objects);
        return -1;
    }
    return 0;
}

// optional HIP-event timing (tools/time_pose_error.py): events round the last diameter and the last errors
slhip::StepTimer<2> g_timer;

}  // namespace

extern "C" int slhip_pose_error_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_pose_error_timings(float ms_out[2]) { return g_timer.read_for("slhip_pose_error_timings", ms_out); }

extern "C" int slhip_pose_error_check_params(const slhip_pose_error_params* p)
{
    static const char* who = "slhip_pose_error";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_intrinsics(who, p->fx, p->fy, p->cx, p->cy)) return st;
    if (const int st = slhip::check_range(who, "n_objects", p->n_objects, 1u, SLHIP_SYNTH_MAX_OBJECTS)) return st;
    if (const int st = slhip::check_range(who, "n_hypotheses", p->n_hypotheses, 1u, 0x7fffffffu)) return st;
    const uint32_t all = SLHIP_POSE_OUT_ADD | SLHIP_POSE_OUT_ADDS | SLHIP_POSE_OUT_MSSD | SLHIP_POSE_OUT_MSPD;
    if (p->outputs == 0u || (p->outputs & ~all)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of add 1, adds 2, mssd 4, mspd 8 and nothing else", who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_pose_error_diameter(const slhip_pose_bank* bank, float* d_diameter, void* stream_)
{
    static const char* who = "slhip_pose_error_diameter";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_bank(who, bank)) return st;
    if (!d_diameter || ((uintptr_t)d_diameter & 3u)) {
        slhip::set_error("%s: the diameters need a 4-byte aligned pointer", who);
        return -1;
    }
    const uint32_t n_pad = pad_to_block(bank->n_points);
    const size_t lds = (size_t)3u * n_pad * sizeof(float);      // at most 48 KiB
    if (const int st = g_timer.begin(0, stream)) return st;
    SLHIP_CHECK(hipMemsetAsync(d_diameter, 0, (size_t)bank->n_assets * sizeof(float), stream));
    const dim3 grid(bank->n_assets, (bank->n_points + QUERY_TILE - 1u) / QUERY_TILE);
    k_pose_diameter<<<grid, BLOCK, lds, stream>>>(*bank, reinterpret_cast<uint32_t*>(d_diameter), n_pad);
    SLHIP_LAUNCH_CHECK();
    k_pose_sqrt<<<(bank->n_assets + BLOCK - 1u) / BLOCK, BLOCK, 0, stream>>>(d_diameter, bank->n_assets);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

extern "C" int slhip_pose_error_diameter_host(const slhip_pose_bank* b, float* h_diameter)
{
    static const char* who = "slhip_pose_error_diameter_host";
    if (const int st = check_bank(who, b)) return st;
    if (!h_diameter) {
        slhip::set_error("%s: null argument", who);
        return -1;
    }
    for (uint32_t a = 0u; a < b->n_assets; ++a) {
        float best = 0.0f;
        const int32_t count = b->count[a];
        if (count >= 1 && (uint32_t)count <= b->n_points) {
            const float* p = b->points + (size_t)a * b->n_points * 4u;
            for (int32_t i = 0; i < count; ++i)
                for (int32_t j = 0; j < count; ++j)
                    best = fmaxf(best, pr::dist2(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * j], p[4 * j + 1], p[4 * j + 2]));
        }
        h_diameter[a] = sqrtf(best);
    }
    return 0;
}

extern "C" int slhip_pose_error(const slhip_pose_error_params* params, const slhip_pose_bank* bank, const int32_t* d_classes,
                                uint32_t class_stride, const float* d_gt, const float* d_est, uint32_t n_scenes,
                                const slhip_pose_error_out* out, void* stream_)
{
    static const char* who = "slhip_pose_error";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, bank, d_classes, class_stride, d_gt, d_est, n_scenes, out)) return st;
    if (n_scenes == 0u) return 0;
    const uint32_t n_pad = pad_to_block(bank->n_points);
    const size_t lds = (size_t)LDS_ARRAYS * n_pad * sizeof(float);      // 8 KiB at N <= 256, 32 KiB at 1024, 128 KiB at 4096
    if (lds > 64u * 1024u)      // more than a kernel may ask for without the attribute (N > 2048; per device, so not remembered)
        SLHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pose_error), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // an object's hypotheses over enough workgroups to fill the device when there are few objects (sl.diff: 1 x 64 x 32)
    const uint32_t pairs = n_scenes * params->n_objects;
    const uint32_t split = std::min<uint32_t>(std::min<uint32_t>(params->n_hypotheses, 65535u), std::max<uint32_t>(1u, 2048u / pairs));
    if (const int st = g_timer.begin(1, stream)) return st;
    k_pose_error<<<dim3(pairs, split), BLOCK, lds, stream>>>(*params, *bank, d_classes, class_stride, d_gt, d_est, *out, n_pad);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(1, stream);
}

extern "C" int slhip_pose_error_host(const slhip_pose_error_params* params, const slhip_pose_bank* b, const int32_t* h_classes,
                                     uint32_t class_stride, const float* h_gt, const float* h_est, uint32_t n_scenes,
                                     const slhip_pose_error_out* out)
{
    static const char* who = "slhip_pose_error_host";
    if (const int st = check_call(who, params, b, h_classes, class_stride, h_gt, h_est, n_scenes, out)) return st;
    const Params& p = *params;
    const uint32_t Hy = p.n_hypotheses, mask = p.outputs;
    const float inf = __builtin_inff(), nan = __builtin_nanf("");
    auto write_all = [&](size_t at, float v, int idx) {
        if (mask & SLHIP_POSE_OUT_ADD) out->add[at] = v;
        if (mask & SLHIP_POSE_OUT_ADDS) out->adds[at] = v;
        if (mask & SLHIP_POSE_OUT_MSSD) out->mssd[at] = v, out->mssd_sym[at] = idx;
        if (mask & SLHIP_POSE_OUT_MSPD) out->mspd[at] = v, out->mspd_sym[at] = idx;
    };
    std::vector<float> q, uv;
    for (size_t so = 0; so < (size_t)n_scenes * p.n_objects; ++so) {
        const uint32_t cls = (uint32_t)h_classes[so * class_stride];
        const int32_t count = cls < b->n_assets ? b->count[cls] : 0, n_sym = cls < b->n_assets ? b->n_sym[cls] : 0;
        const bool ok = pr::class_ok(count, b->n_points, n_sym, b->n_symmetries);
        const float* g = h_gt + so * 12u;
        const float* pts = ok ? b->points + (size_t)cls * b->n_points * 4u : nullptr;
        const float* sym = ok ? b->symmetries + (size_t)cls * b->n_symmetries * 12u : nullptr;
        for (uint32_t h = 0u; h < Hy; ++h) {
            const size_t at = so * Hy + h;
            if (!ok) {
                write_all(at, inf, -1);
                continue;
            }
            const float* e = h_est + at * 12u;
            float D[12];
            pr::difference(g, e, D);
            if (!pr::all_finite(D)) {
                write_all(at, nan, -1);
                continue;
            }
            q.assign((size_t)count * 3u, 0.0f);
            uv.assign((size_t)count * 2u, 0.0f);
            pr::LaneSums<1> sum_add, sum_adds;
            bool behind = false;
            for (int32_t i = 0; i < count; ++i) {
                const float x = pts[4 * i], y = pts[4 * i + 1], z = pts[4 * i + 2];
                float* qi = &q[3 * (size_t)i];
                const pr::Moved m = pr::move_point(g, D, x, y, z);
                qi[0] = m.qx;
                qi[1] = m.qy;
                qi[2] = m.qz;
                sum_add.add((uint32_t)i, [&](float* acc) { acc[0] = acc[0] + sqrtf(m.add2); });
                if (mask & SLHIP_POSE_OUT_MSPD) {
                    const float X = pr::row_point(e, x, y, z), Y = pr::row_point(e + 4, x, y, z), Z = pr::row_point(e + 8, x, y, z);
                    behind = behind || !(Z > 0.0f);
                    uv[2 * (size_t)i] = pr::pixel_u(p.fx, X, Z, p.cx);
                    uv[2 * (size_t)i + 1] = pr::pixel_u(p.fy, Y, Z, p.cy);
                }
                if (mask & SLHIP_POSE_OUT_ADDS) {
                    float best = inf;
                    for (int32_t j = 0; j < count; ++j)
                        best = fminf(best, pr::dist2(qi[0], qi[1], qi[2], pts[4 * j], pts[4 * j + 1], pts[4 * j + 2]));
                    sum_adds.add((uint32_t)i, [&](float* acc) { acc[0] = acc[0] + sqrtf(best); });
                }
            }
            if (mask & SLHIP_POSE_OUT_ADD) out->add[at] = sum_add.total(0) / (float)count;
            if (mask & SLHIP_POSE_OUT_ADDS) out->adds[at] = sum_adds.total(0) / (float)count;
            if (!(mask & (SLHIP_POSE_OUT_MSSD | SLHIP_POSE_OUT_MSPD))) continue;
            pr::Best b3 = pr::best_start(), b2 = pr::best_start();
            for (int32_t s = 0; s < n_sym; ++s) {
                const float* S = sym + (size_t)s * 12u;
                float m3 = 0.0f, m2 = 0.0f;
                for (int32_t i = 0; i < count; ++i) {
                    const float x = pts[4 * i], y = pts[4 * i + 1], z = pts[4 * i + 2];
                    const float yx = pr::row_point(S, x, y, z), yy = pr::row_point(S + 4, x, y, z), yz = pr::row_point(S + 8, x, y, z);
                    m3 = fmaxf(m3, pr::dist2(q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2], yx, yy, yz));
                    if (mask & SLHIP_POSE_OUT_MSPD) {
                        const float X = pr::row_point(g, yx, yy, yz), Y = pr::row_point(g + 4, yx, yy, yz), Z = pr::row_point(g + 8, yx, yy, yz);
                        behind = behind || !(Z > 0.0f);
                        m2 = fmaxf(m2, pr::pixel_dist2(uv[2 * (size_t)i], uv[2 * (size_t)i + 1], pr::pixel_u(p.fx, X, Z, p.cx),
                                                       pr::pixel_u(p.fy, Y, Z, p.cy)));
                    }
                }
                pr::Best c;
                c.idx = s;
                c.val = m3;
                b3 = pr::join(b3, c);
                c.val = m2;
                b2 = pr::join(b2, c);
            }
            if (mask & SLHIP_POSE_OUT_MSSD) {
                out->mssd[at] = sqrtf(b3.val);
                out->mssd_sym[at] = pr::best_index(b3);
            }
            if (mask & SLHIP_POSE_OUT_MSPD) {
                out->mspd[at] = behind ? inf : sqrtf(b2.val);
                out->mspd_sym[at] = behind ? -1 : pr::best_index(b2);
            }
        }
    }
    return 0;
}
