// Point k-NN (this project's addition, no counterpart in the reference): for every query point of a set its k nearest reference
// points of the same set, as sorted lists of indices and squared distances -- the neighbourhood graph that FFB6D and
// PVN3D-with-RandLA build per frame with a CPU kd-tree (cld_nei_idx, cld_interp_idx, r2p / p2r_ds_nei_idx) and that PointNet++ /
// DGCNN style refiners build per set.  include/slhip.h "Point neighbours" and DESIGN.md "Point neighbours" are the contract; all
// arithmetic is float32, one rounded operation at a time (-ffp-contract=off), through slhip_knn_rules.h on host and device alike,
// so slhip_point_knn_host gives the kernel's outputs bit for bit.
//   k_point_knn<K>  one workgroup of 256 lanes per set and block of 256 queries, a 1-D grid.  A lane holds one query and its list
//                   in two register arrays of K slots (K the rung of the ladder 1, 4, 8, 16, 32 at or above the run-time k); the
//                   set's references pass through LDS in tiles of SLHIP_KNN_TILE float4 in rising index order, a reference that
//                   does not count stored as NaNs (its distances are NaN and never enter).  The walk reads every reference by one
//                   16-byte LDS read at an address all lanes share (a broadcast), evaluates dist2 and compares it with the list's
//                   last distance; the rare entry is a fully unrolled compare-and-shift with static indices, which lists of 8
//                   slots and more run for the whole wave at once from per-lane queues in LDS (below).  Lanes past the last
//                   query, and lanes whose query does not count, hold a NaN query: they load tiles and reach every barrier like
//                   the others, and nothing ever enters their list.  The tile loop's trip count depends on n_refs alone.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_knn_rules.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_point_knn_params) == 48, "slhip_point_knn_params layout");

using Params = slhip_point_knn_params;
using Out = slhip_point_knn_out;
namespace kn = slhip_knn;

constexpr uint32_t BLOCK = kn::BLOCK;
constexpr uint32_t TILE = kn::TILE;
constexpr uint32_t STEP = 4u;      // references per round of the walk: their LDS reads are in flight together
static_assert(TILE % BLOCK == 0u && TILE % STEP == 0u, "a tile is whole rounds of the workgroup and of the walk");

constexpr uint32_t ALL_OUTPUTS = SLHIP_KNN_OUT_IDX | SLHIP_KNN_OUT_DIST2 | SLHIP_KNN_OUT_COUNT;
// what the kernel's 32-bit quantities address (include/slhip.h): elements of an output, floats of an input
constexpr uint64_t MAX_ELEMENTS = 0x7fffffffull;

// Lists of 8 slots and more do not insert where they find: a wave pays an insertion in full whenever one of its 64 lanes has one,
// and at k = 16 some lane has one at nearly every reference.  A lane queues what passes rule 3 and its stale last distance in LDS
// slots of its own (no lane reads another's, so no barrier), and the wave empties its queues together when one of them could
// overflow in the next round: the insertions of a wave then run with most lanes at work.  The last distance only falls, so the
// queue holds every reference that belongs in the list; insert() asks again.  A queue keeps the rising index order and is emptied
// before anything later is looked at, so the order of insertion -- the tie rule -- is the plain scan's.
constexpr uint32_t QUEUE = 8u;                  // slots of a lane's queue
constexpr uint32_t DRAIN_AT = QUEUE - STEP;     // a round adds STEP entries at the most
template <int K>
constexpr bool QUEUED = K >= 8;

template <int K>
__device__ __forceinline__ void drain(float (&d)[K], int (&r)[K], uint32_t& pending, const float (*s_qd)[BLOCK], const int (*s_qr)[BLOCK],
                                      uint32_t tid)
{
    for (uint32_t s = 0u; s < QUEUE; ++s) {
        if (__ballot(s < pending) == 0ull) break;      // (the same for every lane of the wave)
        if (s < pending) {
            const float x = s_qd[s][tid];
            if (kn::enters(x, d[K - 1])) kn::insert(d, r, x, s_qr[s][tid]);
        }
    }
    pending = 0u;
}

template <int K>
__global__ __launch_bounds__(BLOCK) void k_point_knn(Params p, const float4* __restrict__ queries, const float4* __restrict__ refs, Out out,
                                                     uint32_t blocks_per_set)
{
    __shared__ float4 s_ref[TILE];
    __shared__ float s_qd[QUEUED<K> ? QUEUE : 1u][BLOCK];      // the queued distances, slot by slot: lane l at [s][l]
    __shared__ int s_qr[QUEUED<K> ? QUEUE : 1u][BLOCK];        // and their references

    const uint32_t tid = threadIdx.x, set = blockIdx.x / blocks_per_set, q = (blockIdx.x % blocks_per_set) * BLOCK + tid;
    const uint32_t Q = p.n_queries, R = p.n_refs, k = p.k;
    const bool live = q < Q;
    const float nan = __builtin_nanf("");

    // the lane's query: NaNs when there is none or it does not count (rule 1), so that no distance of this lane enters
    const float4 c = queries[(size_t)set * p.query_stride + (live ? q : 0u)];
    const bool ok = live && kn::counts(c.x, c.y, c.z, c.w);
    const float qx = ok ? c.x : nan, qy = ok ? c.y : nan, qz = ok ? c.z : nan;
    const float g2 = kn::gate2(p.max_dist);
    const int self = p.skip_same ? (int)q : kn::EMPTY;

    float d[K];
    int r[K];
    kn::clear(d, r);
    uint32_t pending = 0u;      // the entries of the lane's queue, at most DRAIN_AT between two rounds

    const float4* src = refs + (size_t)set * p.ref_stride;
    for (uint32_t base = 0u; base < R; base += TILE) {      // (the same trips for every lane of the grid: R alone decides)
        if (base) __syncthreads();                            // the tile before is walked
#pragma unroll
        for (uint32_t i = tid; i < TILE; i += BLOCK) {
            const uint32_t j = base + i;
            float4 v = make_float4(nan, nan, nan, 0.0f);      // past n_refs, or not counting: never a candidate
            if (j < R) {
                const float4 t = src[j];
                if (kn::counts(t.x, t.y, t.z, t.w)) v = t;
            }
            s_ref[i] = v;
        }
        __syncthreads();
        const uint32_t m = min(TILE, (R - base + STEP - 1u) & ~(STEP - 1u));      // whole rounds: the rest of a round is NaNs
        for (uint32_t j = 0u; j < m; j += STEP) {
            float4 t[STEP];
#pragma unroll
            for (uint32_t s = 0u; s < STEP; ++s) t[s] = s_ref[j + s];
#pragma unroll
            for (uint32_t s = 0u; s < STEP; ++s) {
                const float x = kn::dist2(qx, qy, qz, t[s].x, t[s].y, t[s].z);
                const int ri = (int)(base + j + s);
                if (kn::enters(x, d[K - 1]))      // (a NaN and a +inf never do)
                    if (x <= g2 && ri != self) {
                        if constexpr (QUEUED<K>) {
                            s_qd[pending][tid] = x;      // pending < QUEUE: at most DRAIN_AT before the round, STEP in it
                            s_qr[pending][tid] = ri;
                            ++pending;
                        } else {
                            kn::insert(d, r, x, ri);
                        }
                    }
            }
            if constexpr (QUEUED<K>)
                if (__ballot(pending > DRAIN_AT) != 0ull) drain(d, r, pending, s_qd, s_qr, tid);
        }
    }
    if constexpr (QUEUED<K>) drain(d, r, pending, s_qd, s_qr, tid);

    // the outputs of the lane's query: the first k slots (slots k .. K - 1 were never part of the answer)
    if (live) {
        const uint32_t mask = p.outputs;
        const size_t row = (size_t)set * Q + q, at = row * k;
        int filled = 0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if ((uint32_t)j < k) {
                if (mask & SLHIP_KNN_OUT_IDX) out.idx[at + j] = r[j];
                if (mask & SLHIP_KNN_OUT_DIST2) out.dist2[at + j] = kn::slot_dist2(d[j], r[j]);
                filled += r[j] != kn::EMPTY ? 1 : 0;
            }
        if (mask & SLHIP_KNN_OUT_COUNT) out.count[row] = filled;
    }
}

// the checks that slhip_point_knn and slhip_point_knn_host share
int check_call(const char* who, const Params* params, const float* queries, const float* refs, const Out* out)
{
    if (const int st = slhip_point_knn_check_params(params)) return st;
    if (!queries || !refs || !out) {
        slhip::set_error("%s: null argument (queries, refs and the output record are required)", who);
        return -1;
    }
    const uint32_t m = params->outputs;
    const slhip::OutputList outputs = {{SLHIP_KNN_OUT_IDX, out->idx}, {SLHIP_KNN_OUT_DIST2, out->dist2}, {SLHIP_KNN_OUT_COUNT, out->count}};
    if (const int st = slhip::check_outputs_present(who, m, outputs)) return st;
    if (((uintptr_t)queries & 15u) || ((uintptr_t)refs & 15u)) {
        slhip::set_error("%s: queries and refs must be 16-byte aligned", who);
        return -1;
    }
    if (const int st = slhip::check_outputs_aligned(who, m, outputs)) return st;
    if (params->skip_same && queries != refs) {
        slhip::set_error("%s: skip_same is for a self-search: queries and refs must be the same pointer", who);
        return -1;
    }
    return 0;
}

template <int K>
void launch(const Params& p, const float* q, const float* r, const Out& out, hipStream_t stream)
{
    const uint32_t per_set = (p.n_queries + BLOCK - 1u) / BLOCK;      // n_sets * per_set <= n_sets * n_queries < 2^31
    k_point_knn<K><<<p.n_sets * per_set, BLOCK, 0, stream>>>(p, reinterpret_cast<const float4*>(q), reinterpret_cast<const float4*>(r), out, per_set);
}

// optional HIP-event timing (tools/time_point_knn.py): events round the last call
slhip::StepTimer<1> g_timer;

}  // namespace

extern "C" int slhip_point_knn_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_point_knn_timings(float ms_out[1]) { return g_timer.read_for("slhip_point_knn_timings", ms_out); }

extern "C" int slhip_point_knn_check_params(const slhip_point_knn_params* p)
{
    static const char* who = "slhip_point_knn";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_sets", p->n_sets, 0u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_queries", p->n_queries, 1u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "n_refs", p->n_refs, 1u, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "query_stride", p->query_stride, p->n_queries, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "ref_stride", p->ref_stride, p->n_refs, 0x7fffffffu)) return st;
    if (const int st = slhip::check_range(who, "k", p->k, 1u, SLHIP_KNN_K_MAX)) return st;
    if (!(p->max_dist >= 0.0f)) {
        slhip::set_error("%s: max_dist %g must be at least 0 (+inf: no gate)", who, (double)p->max_dist);
        return -1;
    }
    if (const int st = slhip::check_range(who, "skip_same", p->skip_same, 0u, 1u)) return st;
    if (p->skip_same && p->query_stride != p->ref_stride) {
        slhip::set_error("%s: skip_same is for a self-search: query_stride %u and ref_stride %u must be equal", who, p->query_stride,
                         p->ref_stride);
        return -1;
    }
    if (p->outputs == 0u || (p->outputs & ~ALL_OUTPUTS)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of idx 1, dist2 2, count 4 and nothing else", who, p->outputs);
        return -1;
    }
    if ((uint64_t)p->n_sets * p->n_queries * p->k > MAX_ELEMENTS) {
        slhip::set_error("%s: n_sets %u x n_queries %u x k %u: the lists may hold 2^31 - 1 elements at the most", who, p->n_sets, p->n_queries,
                         p->k);
        return -1;
    }
    const uint32_t stride = p->query_stride > p->ref_stride ? p->query_stride : p->ref_stride;
    if ((uint64_t)p->n_sets * stride * 4u > MAX_ELEMENTS) {
        slhip::set_error("%s: n_sets %u x stride %u x 4: an input may hold 2^31 - 1 floats at the most", who, p->n_sets, stride);
        return -1;
    }
    return 0;
}

extern "C" int slhip_point_knn(const slhip_point_knn_params* params, const float* d_queries, const float* d_refs, const slhip_point_knn_out* out,
                               void* stream_)
{
    static const char* who = "slhip_point_knn";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_call(who, params, d_queries, d_refs, out)) return st;
    if (params->n_sets == 0u) return 0;
    if (const int st = g_timer.begin(0, stream)) return st;
    const uint32_t k = params->k;      // the rung of the ladder at or above k
    if (k <= 1u) launch<1>(*params, d_queries, d_refs, *out, stream);
    else if (k <= 4u) launch<4>(*params, d_queries, d_refs, *out, stream);
    else if (k <= 8u) launch<8>(*params, d_queries, d_refs, *out, stream);
    else if (k <= 16u) launch<16>(*params, d_queries, d_refs, *out, stream);
    else launch<32>(*params, d_queries, d_refs, *out, stream);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(0, stream);
}

// the plain scan of rule 4, one query after the other
extern "C" int slhip_point_knn_host(const slhip_point_knn_params* params, const float* h_queries, const float* h_refs, const slhip_point_knn_out* out)
{
    static const char* who = "slhip_point_knn_host";
    if (const int st = check_call(who, params, h_queries, h_refs, out)) return st;
    const Params& p = *params;
    const uint32_t Q = p.n_queries, R = p.n_refs, k = p.k, mask = p.outputs;
    const float g2 = kn::gate2(p.max_dist);
    std::vector<float> d(k);
    std::vector<int> r(k);
    for (uint32_t set = 0u; set < p.n_sets; ++set) {
        const float* qs = h_queries + (size_t)set * p.query_stride * 4u;
        const float* rs = h_refs + (size_t)set * p.ref_stride * 4u;
        for (uint32_t q = 0u; q < Q; ++q) {
            const float* c = qs + 4u * q;
            const bool ok = kn::counts(c[0], c[1], c[2], c[3]);
            const int self = p.skip_same ? (int)q : kn::EMPTY;
            for (uint32_t j = 0u; j < k; ++j) {
                d[j] = __builtin_inff();
                r[j] = kn::EMPTY;
            }
            for (uint32_t j = 0u; j < R; ++j) {
                const float* t = rs + 4u * j;
                const float x = kn::dist2(c[0], c[1], c[2], t[0], t[1], t[2]);
                if (kn::candidate(ok, kn::counts(t[0], t[1], t[2], t[3]), x, g2, (int)j, self) && kn::enters(x, d[k - 1u]))
                    kn::insert_n(d.data(), r.data(), k, x, (int)j);
            }
            const size_t row = (size_t)set * Q + q, at = row * k;
            int filled = 0;
            for (uint32_t j = 0u; j < k; ++j) {
                if (mask & SLHIP_KNN_OUT_IDX) out->idx[at + j] = r[j];
                if (mask & SLHIP_KNN_OUT_DIST2) out->dist2[at + j] = kn::slot_dist2(d[j], r[j]);
                filled += r[j] != kn::EMPTY ? 1 : 0;
            }
            if (mask & SLHIP_KNN_OUT_COUNT) out->count[row] = filled;
        }
    }
    return 0;
}
