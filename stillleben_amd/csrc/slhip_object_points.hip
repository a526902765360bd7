// Object points (this project's addition, no counterpart in the reference): K pixels of every visible object of a render,
// drawn inside its visible mask, and the render's targets gathered there -- the input of a network that takes a fixed number of
// points per object.  include/slhip.h "Object points" and DESIGN.md "Object points" are the contract; the choice of the pixels is
// integer arithmetic and the camera point float32 without fma (-ffp-contract=off), so tests/object_points_ref.py restates both
// and every output is bit-exact against it.
//   select           the count / scan / emit pass of slhip_select.h under PointRule
//   k_points_gather  one workgroup per set: popcounts of the slot's kind-1 words summed per thread over a contiguous segment,
//                    the 256 segment prefixes in LDS, then per point a search of its rank in them and a walk of one segment
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_mask_select.h"
#include "slhip_rng.h"
#include "slhip_select.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_object_point_params) == 48, "slhip_object_point_params layout");
static_assert(sizeof(slhip_object_point_set) == 16, "slhip_object_point_set layout");
static_assert(sizeof(slhip_object_stats) == 40, "slhip_object_stats layout");
static_assert(sizeof(slhip_object_mask) == 56, "slhip_object_mask layout");

constexpr uint32_t STREAM_POINTS = 6u;      // "Randomness" of include/slhip.h
constexpr uint32_t BLOCK = 256u;            // threads of k_points_gather = segments of a slot's tiles
constexpr uint32_t MAX_SLOTS = 65536u;

using Params = slhip_object_point_params;

// the four draws of points 4 q .. 4 q + 3 of (scene, slot)
__host__ __device__ inline void point_draws(const Params& p, uint32_t scene, uint32_t slot, uint32_t q, uint32_t x[4])
{
    slhip::Philox ph;
    ph.c[0] = p.scene_id_base + scene; ph.c[1] = STREAM_POINTS; ph.c[2] = (slot << 12) | q; ph.c[3] = 0x51DE5EEDu;
    ph.k[0] = p.seed_lo; ph.k[1] = p.seed_hi;
    for (int i = 0; i < 10; ++i) ph.round();      // block() without its unroll pragma, under which k_points_gather takes 40 VGPRs for 36
    x[0] = ph.c[0]; x[1] = ph.c[1]; x[2] = ph.c[2]; x[3] = ph.c[3];
}

// the rank of point j of K among n visible pixels under the draw x: stratum [lo, hi) of the ranks, x picks inside it
__host__ __device__ inline uint64_t point_rank(uint32_t j, uint32_t n, uint32_t K, uint32_t x)
{
    const uint64_t lo = (uint64_t)j * n / K, hi = ((uint64_t)j + 1u) * n / K;
    return lo + (uint32_t)(((uint64_t)x * (hi - lo)) >> 32);
}

// the rule of slhip_select.h: a slot with enough visible pixels, a large enough visible share and a tile box gets a set
struct PointRule {
    typedef slhip_object_point_set Record;
    typedef slhip_object_point_params Params;
    Params p;
    const slhip_object_stats* stats;
    const slhip_object_mask* masks;

    __device__ __forceinline__ size_t row(uint32_t scene, uint32_t n_slots) const { return (size_t)scene * n_slots; }
    __device__ __forceinline__ bool eligible(size_t row, uint32_t slot) const
    {
        const slhip_object_stats& s = stats[row + slot];
        const slhip_object_mask& m = masks[row + slot];
        return s.px_visib >= p.min_px && (float)s.px_visib >= p.min_visib_fract * (float)s.px_all && m.tile_box[0] <= m.tile_box[2];
    }
    __device__ __forceinline__ Record make(size_t row, uint32_t scene, uint32_t slot) const
    {
        slhip_object_point_set r;
        r.scene = scene; r.slot = slot; r.n_visib = stats[row + slot].px_visib; r._pad = 0u;
        return r;
    }
};

struct Source {
    const uint32_t* rgb;        // the four bytes of a pixel as one word
    const float4* coord;
    const float4* normals;
    const float* depth;
    uint32_t depth_stride;
    const slhip_object_mask* masks;
    const unsigned long long* words;
};

struct Dest {
    uint32_t* pixel;            // (x, y) as one word: x in the low half
    float4* camera;
    float4* coord;
    float4* normals;
    uint32_t* rgb;
};

// Block b is set set0 + b: the record, the tile box and every branch on `outputs` are uniform over the block.  The words of the
// slot are read inside its tile box only, and the box is followed only when it lies inside the picture's tiles; every read of the
// picture is guarded by the picture's bounds; every write goes to the thread's own points.
__global__ __launch_bounds__(256) void k_points_gather(Params p, const slhip_object_point_set* __restrict__ sets,
                                                       unsigned long long set0, Source src, uint32_t n_scenes, uint32_t n_slots,
                                                       int W, int H, Dest dst)
{
    __shared__ uint32_t s_prefix[BLOCK];      // set pixels before segment i (W * H < 2^31, and a tile box holds < 2^32 bits)
    __shared__ uint32_t s_wave[BLOCK / 64u];
    const uint32_t tid = threadIdx.x;
    const unsigned long long set = set0 + blockIdx.x;
    const slhip_object_point_set r = sets[set];
    slhip_mask::TileBox box = {0, 0, -1, -1};
    const unsigned long long* words = nullptr;
    if (r.scene < n_scenes && r.slot < n_slots) {
        const slhip_object_mask* m = src.masks + (size_t)r.scene * n_slots + r.slot;
        const int tx0 = m->tile_box[0], ty0 = m->tile_box[1], tx1 = m->tile_box[2], ty1 = m->tile_box[3];
        if (tx0 >= 0 && ty0 >= 0 && tx0 <= tx1 && ty0 <= ty1 && tx1 <= (W - 1) >> 3 && ty1 <= (H - 1) >> 3) {
            box.tx0 = tx0; box.ty0 = ty0; box.tx1 = tx1; box.ty1 = ty1;
            words = src.words + m->word_offset[1];
        }
    }
    const uint32_t tiles = words ? (uint32_t)(box.tx1 - box.tx0 + 1) * (uint32_t)(box.ty1 - box.ty0 + 1) : 0u;
    const uint32_t per = (tiles + BLOCK - 1u) / BLOCK;      // words per segment; the last segments may be short or empty

    // pass A: the set pixels of this thread's segment, then the exclusive scan over the block
    const uint32_t first = min(tid * per, tiles), last = min(first + per, tiles);
    uint32_t mine = 0u;
    for (uint32_t t = first; t < last; ++t) mine += (uint32_t)__popcll(words[t]);
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    uint32_t incl = mine;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0u, total = 0u;
#pragma unroll
    for (uint32_t w = 0u; w < BLOCK / 64u; ++w) {
        const uint32_t c = s_wave[w];
        if (w < wave) before += c;
        total += c;
    }
    s_prefix[tid] = before + incl - mine;
    __syncthreads();

    // pass B: four points per thread and trip, one Philox block for the four
    const uint32_t K = p.n_points, n = r.n_visib;
    const size_t image = (size_t)r.scene * (size_t)H;
    for (uint32_t q = tid; 4u * q < K; q += BLOCK) {
        uint32_t x4[4];
        point_draws(p, r.scene, r.slot, q, x4);
#pragma unroll
        for (uint32_t c = 0u; c < 4u; ++c) {
            const uint32_t j = 4u * q + c;
            if (j >= K) break;
            const uint64_t rank = point_rank(j, n, K, x4[c]);
            int x = 0, y = 0;
            bool found = false;
            if (rank < (uint64_t)total) {
                // the last segment whose prefix is <= rank: it holds the rank, the empty segments before it do not win ties
                uint32_t seg = 0u;
#pragma unroll
                for (uint32_t step = BLOCK / 2u; step; step >>= 1)
                    if ((uint64_t)s_prefix[seg + step] <= rank) seg += step;
                const uint32_t f = min(seg * per, tiles), l = min(f + per, tiles);
                found = slhip_mask::select_pixel(words, box, f, l, s_prefix[seg], rank, &x, &y) && x < W && y < H;
            }
            if (!found) x = y = 0;
            const size_t out = (size_t)set * K + j;
            const size_t at = (image + (size_t)y) * (size_t)W + (size_t)x;      // followed only when `found`
            if (p.outputs & SLHIP_POINTS_PIXEL) dst.pixel[out] = (uint32_t)x | ((uint32_t)y << 16);
            if (p.outputs & SLHIP_POINTS_CAMERA) {
                float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (found) {
                    const float z = src.depth[at * src.depth_stride];
                    if (z > 0.0f && z - z == 0.0f)      // finite and positive
                        t = make_float4(((((float)x + 0.5f) - p.cx) * z) / p.fx, ((((float)y + 0.5f) - p.cy) * z) / p.fy, z, 1.0f);
                }
                dst.camera[out] = t;
            }
            if (p.outputs & SLHIP_POINTS_COORD) {
                float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (found) t = src.coord[at];
                dst.coord[out] = t;
            }
            if (p.outputs & SLHIP_POINTS_NORMALS) {
                float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (found) t = src.normals[at];
                dst.normals[out] = t;
            }
            if (p.outputs & SLHIP_POINTS_RGB) dst.rgb[out] = found ? src.rgb[at] : 0u;
        }
    }
}

// optional HIP-event timing (tools/time_object_points.py): events round the last select's kernels and the last gather's
slhip::StepTimer<2> g_timer;

int check_slots(const char* who, uint32_t n_slots)
{
    if (n_slots == 0u || n_slots > MAX_SLOTS) {
        slhip::set_error("%s: n_slots %u must be in [1, %u] (slot 0 is the background; the slot shares a counter word with the point)",
                         who, n_slots, MAX_SLOTS);
        return -1;
    }
    return 0;
}

}  // namespace

extern "C" int slhip_object_points_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_object_points_timings(float ms_out[2])
{
    if (!ms_out || !g_timer.all_timed()) {
        slhip::set_error("slhip_object_points_timings: no timed calls (slhip_object_points_timing_enable(1), then "
                         "slhip_object_points_select and slhip_object_points_gather)");
        return -1;
    }
    return g_timer.read_for("slhip_object_points_timings", ms_out);
}

extern "C" int slhip_object_points_check_params(const slhip_object_point_params* p, int W, int H)
{
    static const char* who = "slhip_object_points";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (!slhip::picture_fits(W, H, 32768, 0x7fffffffu)) {
        slhip::set_error("%s: bad picture size %d x %d (each side 1..32768: a pixel is two int16; fewer than 2^31 pixels)", who, W, H);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_points", p->n_points, 1u, SLHIP_OBJECT_POINTS_MAX)) return st;
    if (p->min_px < 1u) {
        slhip::set_error("%s: min_px %u must be at least 1", who, p->min_px);
        return -1;
    }
    if (!(p->min_visib_fract >= 0.0f && p->min_visib_fract <= 1.0f)) {
        slhip::set_error("%s: min_visib_fract %g must be in [0, 1]", who, (double)p->min_visib_fract);
        return -1;
    }
    if (const int st = slhip::check_intrinsics(who, p->fx, p->fy, p->cx, p->cy)) return st;
    const uint32_t all = SLHIP_POINTS_PIXEL | SLHIP_POINTS_CAMERA | SLHIP_POINTS_COORD | SLHIP_POINTS_NORMALS | SLHIP_POINTS_RGB;
    if (p->outputs == 0u || (p->outputs & ~all)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of pixel 1, camera 2, coord 4, normals 8, rgb 16 and nothing else",
                         who, p->outputs);
        return -1;
    }
    return 0;
}

extern "C" int slhip_object_points_scratch_bytes(uint32_t n_scenes, uint64_t* bytes)
{
    if (!bytes) {
        slhip::set_error("slhip_object_points_scratch_bytes: null argument");
        return -1;
    }
    *bytes = slhip::select_scratch_bytes(n_scenes);
    return 0;
}

extern "C" int slhip_object_points_select(const slhip_object_point_params* params, const slhip_object_stats* d_stats,
                                          const slhip_object_mask* d_masks, uint32_t n_scenes, uint32_t n_slots,
                                          slhip_object_point_set* d_sets, uint64_t capacity, void* d_scratch, uint64_t* n_out,
                                          void* stream_)
{
    static const char* who = "slhip_object_points_select";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = slhip_object_points_check_params(params, 1, 1)) return st;      // (select reads no picture)
    if (!d_stats || !d_masks || !d_scratch || !n_out || (!d_sets && capacity)) {
        slhip::set_error("%s: null argument (statistics, mask records, scratch and n_out are required, and d_sets unless its "
                         "capacity is 0)", who);
        return -1;
    }
    if (const int st = check_slots(who, n_slots)) return st;
    return slhip::select<PointRule>(*params, n_scenes, n_slots, d_sets, capacity, d_scratch, n_out, stream, SLHIP_OBJECT_POINTS_CAPACITY,
                                    who, "d_sets", g_timer, 0, d_stats, d_masks);
}

extern "C" int slhip_object_points_gather(const slhip_object_point_params* params, const slhip_object_point_set* d_sets,
                                          uint64_t n_sets, const slhip_render_out* buffers, const float* d_depth,
                                          uint32_t depth_stride, uint32_t n_scenes, int W, int H, const slhip_object_mask* d_masks,
                                          const uint64_t* d_words, uint32_t n_slots, const slhip_object_points_out* out,
                                          void* stream_)
{
    static const char* who = "slhip_object_points_gather";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = slhip_object_points_check_params(params, W, H)) return st;
    if (n_sets == 0u) return 0;
    if (!d_sets || !buffers || !out || !d_masks || !d_words) {
        slhip::set_error("%s: null argument (records, buffers, mask records, words and outputs are required)", who);
        return -1;
    }
    if (const int st = check_slots(who, n_slots)) return st;
    const uint32_t o = params->outputs;
    if (((o & SLHIP_POINTS_COORD) && !buffers->d_coord) || ((o & SLHIP_POINTS_NORMALS) && !buffers->d_normals) ||
        ((o & SLHIP_POINTS_RGB) && !buffers->d_rgb)) {
        slhip::set_error("%s: outputs 0x%x: a render target they read is NULL (coord, normals, rgb)", who, o);
        return -1;
    }
    if ((o & SLHIP_POINTS_CAMERA) && (!d_depth || depth_stride == 0u)) {
        slhip::set_error("%s: the camera output needs d_depth and a depth_stride of at least 1 (4: the w of d_coord, 1: a plane)", who);
        return -1;
    }
    if (((o & SLHIP_POINTS_PIXEL) && !out->d_pixel) || ((o & SLHIP_POINTS_CAMERA) && !out->d_camera) ||
        ((o & SLHIP_POINTS_COORD) && !out->d_coord) || ((o & SLHIP_POINTS_NORMALS) && !out->d_normals) ||
        ((o & SLHIP_POINTS_RGB) && !out->d_rgb)) {
        slhip::set_error("%s: outputs 0x%x: a requested output pointer is NULL", who, o);
        return -1;
    }
    Source src;
    src.rgb = reinterpret_cast<const uint32_t*>(buffers->d_rgb);
    src.coord = reinterpret_cast<const float4*>(buffers->d_coord);
    src.normals = reinterpret_cast<const float4*>(buffers->d_normals);
    src.depth = d_depth;
    src.depth_stride = depth_stride;
    src.masks = d_masks;
    src.words = reinterpret_cast<const unsigned long long*>(d_words);
    Dest dst;
    dst.pixel = reinterpret_cast<uint32_t*>(out->d_pixel);
    dst.camera = reinterpret_cast<float4*>(out->d_camera);
    dst.coord = reinterpret_cast<float4*>(out->d_coord);
    dst.normals = reinterpret_cast<float4*>(out->d_normals);
    dst.rgb = reinterpret_cast<uint32_t*>(out->d_rgb);
    const uint64_t per_launch = 0x7fffffffu;      // sets whose blocks fit the grid's x extent
    if (const int st = g_timer.begin(1, stream)) return st;
    for (uint64_t s0 = 0; s0 < n_sets; s0 += per_launch) {
        const uint64_t n = std::min<uint64_t>(per_launch, n_sets - s0);
        k_points_gather<<<dim3((uint32_t)n), BLOCK, 0, stream>>>(*params, d_sets, s0, src, n_scenes, n_slots, W, H, dst);
    }
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(1, stream);
}

extern "C" int slhip_object_points_host_pixels(const slhip_object_point_params* params, uint32_t scene, uint32_t slot,
                                               uint32_t n_visib, const int32_t tile_box[4], const uint64_t* h_words,
                                               int16_t* out_xy)
{
    static const char* who = "slhip_object_points_host_pixels";
    if (const int st = slhip_object_points_check_params(params, 1, 1)) return st;      // (no picture: the box alone bounds the walk)
    if (!tile_box || !h_words || !out_xy) {
        slhip::set_error("%s: null argument", who);
        return -1;
    }
    if (slot >= MAX_SLOTS) {
        slhip::set_error("%s: slot %u must be below %u", who, slot, MAX_SLOTS);
        return -1;
    }
    const slhip_mask::TileBox box = {tile_box[0], tile_box[1], tile_box[2], tile_box[3]};
    if (box.tx0 < 0 || box.ty0 < 0 || box.tx1 > 4095 || box.ty1 > 4095) {      // pixels must fit int16
        slhip::set_error("%s: tile box (%d, %d, %d, %d) must lie in [0, 4095]", who, box.tx0, box.ty0, box.tx1, box.ty1);
        return -1;
    }
    const uint64_t tiles = box.tx0 <= box.tx1 && box.ty0 <= box.ty1
                               ? (uint64_t)(box.tx1 - box.tx0 + 1) * (uint64_t)(box.ty1 - box.ty0 + 1) : 0u;
    const unsigned long long* words = reinterpret_cast<const unsigned long long*>(h_words);
    const uint32_t K = params->n_points;
    uint32_t x4[4] = {0u, 0u, 0u, 0u};
    for (uint32_t j = 0; j < K; ++j) {
        if ((j & 3u) == 0u) point_draws(*params, scene, slot, j >> 2, x4);
        int x = 0, y = 0;
        if (!slhip_mask::select_pixel(words, box, 0u, tiles, 0u, point_rank(j, n_visib, K, x4[j & 3u]), &x, &y)) x = y = 0;
        out_xy[2 * j] = (int16_t)x;
        out_xy[2 * j + 1] = (int16_t)y;
    }
    return 0;
}
