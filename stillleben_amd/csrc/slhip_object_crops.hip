// Object crops (this project's addition, no counterpart in the reference): one N x N window per visible object of a render,
// cut round the object's 2D box, enlarged, randomly scaled and shifted -- the input of an object-centric network.
// include/slhip.h "Object crops" and DESIGN.md "Object crops" are the contract; tests/object_crops_ref.py restates it in the
// same float32 operation order (IEEE add, mul, div, floor, compare under -ffp-contract=off), so records and windows are
// bit-exact against it.
//   select         the count / scan / emit pass of slhip_select.h under CropRule
//   k_crop_gather  one thread per output pixel, 256 consecutive pixels of one crop per block: a pure streaming kernel
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_rng.h"
#include "slhip_select.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_object_crop_params) == 64, "slhip_object_crop_params layout");
static_assert(sizeof(slhip_object_crop) == 48, "slhip_object_crop layout");
static_assert(sizeof(slhip_object_stats) == 40, "slhip_object_stats layout");
static_assert(sizeof(slhip_object_mask) == 56, "slhip_object_mask layout");

constexpr uint32_t STREAM_CROP = 5u;      // "Randomness" of include/slhip.h

using Params = slhip_object_crop_params;

__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// the rule of slhip_select.h: a slot with a box, enough visible pixels and a large enough visible share gets a window
struct CropRule {
    typedef slhip_object_crop Record;
    typedef slhip_object_crop_params Params;
    Params p;
    const slhip_object_stats* stats;

    __device__ __forceinline__ const slhip_object_stats* row(uint32_t scene, uint32_t n_slots) const
    {
        return stats + (size_t)scene * n_slots;
    }
    __device__ __forceinline__ bool eligible(const slhip_object_stats* row, uint32_t slot) const
    {
        const slhip_object_stats& s = row[slot];
        const int32_t* b = p.box ? s.bbox_obj : s.bbox_visib;
        return b[2] > 0 && b[3] > 0 && s.px_visib >= p.min_px && (float)s.px_visib >= p.min_visib_fract * (float)s.px_all;
    }
    __device__ Record make(const slhip_object_stats* row, uint32_t scene, uint32_t slot) const
    {
        const slhip_object_stats& s = row[slot];
        const int32_t* b = p.box ? s.bbox_obj : s.bbox_visib;
        const float w = (float)b[2], h = (float)b[3];
        slhip::Philox ph;
        ph.c[0] = p.scene_id_base + scene; ph.c[1] = STREAM_CROP; ph.c[2] = slot; ph.c[3] = 0x51DE5EEDu;
        ph.k[0] = p.seed_lo; ph.k[1] = p.seed_hi;
        ph.block();
        const float u0 = u01(ph.c[0]), u1 = u01(ph.c[1]), u2 = u01(ph.c[2]);
        const float side0 = (float)max(b[2], b[3]) * p.pad;
        const float side = side0 * (1.0f + p.jitter_scale * (2.0f * u0 - 1.0f));
        const float cxb = ((float)b[0] + 0.5f * w) + p.jitter_shift * w * (2.0f * u1 - 1.0f);
        const float cyb = ((float)b[1] + 0.5f * h) + p.jitter_shift * h * (2.0f * u2 - 1.0f);
        slhip_object_crop r;
        r.scene = scene; r.slot = slot;
        r.x0 = cxb - 0.5f * side;
        r.y0 = cyb - 0.5f * side;
        r.side = side;
        r.step = side / (float)p.size;
        r.K[0] = p.fx / r.step; r.K[1] = p.fy / r.step;
        r.K[2] = (p.cx - r.x0) / r.step; r.K[3] = (p.cy - r.y0) / r.step;
        r._pad[0] = r._pad[1] = 0u;
        return r;
    }
};

struct Source {
    const uint32_t* rgb;        // the four bytes of a pixel as one word
    const float4* coord;
    const float4* normals;
    const uint16_t* instance;
    const slhip_object_mask* masks;
    const unsigned long long* words;
};

struct Dest {
    uint32_t* rgb;
    float4* coord;
    float4* normals;
    int16_t* instance;
    uint8_t* mask;
};

__device__ __forceinline__ float lerp2(float ax, float ay, uint32_t p00, uint32_t p10, uint32_t p01, uint32_t p11, int shift)
{
    const float c00 = (float)((p00 >> shift) & 255u), c10 = (float)((p10 >> shift) & 255u);
    const float c01 = (float)((p01 >> shift) & 255u), c11 = (float)((p11 >> shift) & 255u);
    const float top = (1.0f - ax) * c00 + ax * c10;
    const float bot = (1.0f - ax) * c01 + ax * c11;
    const float val = (1.0f - ay) * top + ay * bot;
    return fminf(255.0f, floorf(val + 0.5f));
}

// Block b covers pixels [256 (b % bpc), ...) of crop crop0 + b / bpc in row-major order: the record, the mask record and every
// branch on `outputs` are uniform over the block.  Every read of the picture is guarded by the picture's bounds (and by the
// record's scene and slot lying inside the batch); every write goes to the thread's own output pixel.
__global__ __launch_bounds__(256) void k_crop_gather(Params p, const slhip_object_crop* __restrict__ crops,
                                                     unsigned long long crop0, uint32_t bpc, Source src, uint32_t n_scenes,
                                                     uint32_t n_slots, int W, int H, Dest dst)
{
    const unsigned long long c = crop0 + blockIdx.x / bpc;
    const uint32_t N = p.size, pix = (blockIdx.x % bpc) * 256u + threadIdx.x;
    if (pix >= N * N) return;
    const uint32_t v = pix / N, u = pix - v * N;
    const slhip_object_crop r = crops[c];
    const bool known = r.scene < n_scenes && r.slot < n_slots;
    const size_t image = (size_t)r.scene * (size_t)H;
    const size_t out = (size_t)c * N * N + pix;
    const float sx = r.x0 + ((float)u + 0.5f) * r.step;
    const float sy = r.y0 + ((float)v + 0.5f) * r.step;

    if (p.outputs & SLHIP_CROP_RGB) {
        const float tx = sx - 0.5f, ty = sy - 0.5f;
        const float bx = floorf(tx), by = floorf(ty);
        const float ax = tx - bx, ay = ty - by;
        // (clamped before the conversion: a window far outside the picture must not overflow the integer)
        const int jx = (int)fminf(fmaxf(bx, -2.0f), (float)W), jy = (int)fminf(fmaxf(by, -2.0f), (float)H);
        const bool x0in = known && jx >= 0 && jx < W, x1in = known && jx + 1 >= 0 && jx + 1 < W;
        const bool y0in = jy >= 0 && jy < H, y1in = jy + 1 >= 0 && jy + 1 < H;
        const size_t row0 = (image + (size_t)jy) * (size_t)W, row1 = (image + (size_t)(jy + 1)) * (size_t)W;
        const uint32_t p00 = x0in && y0in ? src.rgb[row0 + jx] : 0u;
        const uint32_t p10 = x1in && y0in ? src.rgb[row0 + jx + 1] : 0u;
        const uint32_t p01 = x0in && y1in ? src.rgb[row1 + jx] : 0u;
        const uint32_t p11 = x1in && y1in ? src.rgb[row1 + jx + 1] : 0u;
        uint32_t word = 0u;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) word |= (uint32_t)lerp2(ax, ay, p00, p10, p01, p11, 8 * ch) << (8 * ch);
        dst.rgb[out] = word;
    }
    if (!(p.outputs & ~SLHIP_CROP_RGB)) return;

    const float fx = floorf(sx), fy = floorf(sy);
    const bool inside = known && fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H;      // false for NaN
    const int ix = inside ? (int)fx : 0, iy = inside ? (int)fy : 0;
    const size_t at = (image + (size_t)iy) * (size_t)W + (size_t)ix;      // followed only when `inside`
    const uint32_t inst = inside && src.instance ? (uint32_t)src.instance[at] : 0u;
    const bool visible = inside && src.instance && inst == r.slot;
    const bool keep = inside && (!p.isolate || visible);
    // (the loads stay under their own branch: a select between the picture and a zero in memory would cost scratch)
    if (p.outputs & SLHIP_CROP_COORD) {
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (keep) t = src.coord[at];
        dst.coord[out] = t;
    }
    if (p.outputs & SLHIP_CROP_NORMALS) {
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (keep) t = src.normals[at];
        dst.normals[out] = t;
    }
    if (p.outputs & SLHIP_CROP_INSTANCE) dst.instance[out] = (int16_t)inst;
    if (p.outputs & SLHIP_CROP_MASK) {
        uint32_t amodal = 0u;
        if (src.masks && inside) {
            const slhip_object_mask* m = src.masks + (size_t)r.scene * n_slots + r.slot;      // (`inside` implies `known`)
            const int tx0 = m->tile_box[0], ty0 = m->tile_box[1], tx1 = m->tile_box[2], ty1 = m->tile_box[3];
            const int tx = ix >> 3, ty = iy >> 3;
            if (tx >= tx0 && tx <= tx1 && ty >= ty0 && ty <= ty1) {
                const unsigned long long w = src.words[m->word_offset[0] + (unsigned long long)(ty - ty0) * (unsigned long long)(tx1 - tx0 + 1)
                                                       + (unsigned long long)(tx - tx0)];
                amodal = (uint32_t)(w >> ((iy & 7) * 8 + (ix & 7))) & 1u;
            }
        }
        dst.mask[out] = (uint8_t)((visible ? 1u : 0u) | (amodal << 1));
    }
}

// optional HIP-event timing (tools/time_object_crops.py): events round the last select's kernels and the last gather's
slhip::StepTimer<2> g_timer;

}  // namespace

extern "C" int slhip_object_crops_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_object_crops_timings(float ms_out[2])
{
    if (!ms_out || !g_timer.all_timed()) {
        slhip::set_error("slhip_object_crops_timings: no timed calls (slhip_object_crops_timing_enable(1), then "
                         "slhip_object_crops_select and slhip_object_crops_gather)");
        return -1;
    }
    return g_timer.read_for("slhip_object_crops_timings", ms_out);
}

extern "C" int slhip_object_crops_check_params(const slhip_object_crop_params* p, int W, int H)
{
    static const char* who = "slhip_object_crops";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (!slhip::picture_fits(W, H, 0x7fffffff, 0x7fffffffu)) {
        slhip::set_error("%s: bad picture size %d x %d", who, W, H);
        return -1;
    }
    if (const int st = slhip::check_range(who, "size", p->size, 1u, SLHIP_OBJECT_CROPS_MAX_SIZE)) return st;
    if (p->box > 1u) {
        slhip::set_error("%s: box %u (0: bbox_visib, 1: bbox_obj)", who, p->box);
        return -1;
    }
    if (!(p->pad > 0.0f) || !slhip::is_finite(p->pad)) {
        slhip::set_error("%s: pad %g must be positive and finite", who, (double)p->pad);
        return -1;
    }
    if (!(p->jitter_scale >= 0.0f && p->jitter_scale < 1.0f)) {
        slhip::set_error("%s: jitter_scale %g must be in [0, 1)", who, (double)p->jitter_scale);
        return -1;
    }
    if (!(p->jitter_shift >= 0.0f && p->jitter_shift <= 1.0f)) {
        slhip::set_error("%s: jitter_shift %g must be in [0, 1]", who, (double)p->jitter_shift);
        return -1;
    }
    if (p->min_px < 1u) {
        slhip::set_error("%s: min_px %u must be at least 1", who, p->min_px);
        return -1;
    }
    if (!(p->min_visib_fract >= 0.0f && p->min_visib_fract <= 1.0f)) {
        slhip::set_error("%s: min_visib_fract %g must be in [0, 1]", who, (double)p->min_visib_fract);
        return -1;
    }
    if (const int st = slhip::check_intrinsics(who, p->fx, p->fy, p->cx, p->cy)) return st;
    const uint32_t all = SLHIP_CROP_RGB | SLHIP_CROP_COORD | SLHIP_CROP_NORMALS | SLHIP_CROP_INSTANCE | SLHIP_CROP_MASK;
    if (p->outputs == 0u || (p->outputs & ~all)) {
        slhip::set_error("%s: outputs 0x%x must name at least one of rgb 1, coord 2, normals 4, instance 8, mask 16 and nothing else",
                         who, p->outputs);
        return -1;
    }
    if (p->isolate > 1u) {
        slhip::set_error("%s: isolate %u must be 0 or 1", who, p->isolate);
        return -1;
    }
    return 0;
}

extern "C" int slhip_object_crops_scratch_bytes(uint32_t n_scenes, uint64_t* bytes)
{
    if (!bytes) {
        slhip::set_error("slhip_object_crops_scratch_bytes: null argument");
        return -1;
    }
    *bytes = slhip::select_scratch_bytes(n_scenes);
    return 0;
}

extern "C" int slhip_object_crops_select(const slhip_object_crop_params* params, const slhip_object_stats* d_stats,
                                         uint32_t n_scenes, uint32_t n_slots, int W, int H, slhip_object_crop* d_crops,
                                         uint64_t capacity, void* d_scratch, uint64_t* n_out, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = slhip_object_crops_check_params(params, W, H)) return st;
    if (!d_stats || !d_scratch || !n_out || (!d_crops && capacity)) {
        slhip::set_error("slhip_object_crops_select: null argument (statistics, scratch and n_out are required, and d_crops "
                         "unless its capacity is 0)");
        return -1;
    }
    if (n_slots == 0u) {
        slhip::set_error("slhip_object_crops_select: n_slots must be at least 1 (slot 0 is the background)");
        return -1;
    }
    return slhip::select<CropRule>(*params, n_scenes, n_slots, d_crops, capacity, d_scratch, n_out, stream, SLHIP_OBJECT_CROPS_CAPACITY,
                                   "slhip_object_crops_select", "d_crops", g_timer, 0, d_stats);
}

extern "C" int slhip_object_crops_gather(const slhip_object_crop_params* params, const slhip_object_crop* d_crops,
                                         uint64_t n_crops, const slhip_render_out* buffers, uint32_t n_scenes, int W, int H,
                                         const slhip_object_mask* d_masks, const uint64_t* d_words, uint32_t n_slots,
                                         const slhip_object_crops_out* out, void* stream_)
{
    static const char* who = "slhip_object_crops_gather";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = slhip_object_crops_check_params(params, W, H)) return st;
    if (n_crops == 0u) return 0;
    if (!d_crops || !buffers || !out) {
        slhip::set_error("%s: null argument (records, buffers and outputs are required)", who);
        return -1;
    }
    if ((d_masks == nullptr) != (d_words == nullptr)) {
        slhip::set_error("%s: d_masks and d_words go together (both, or both NULL)", who);
        return -1;
    }
    const uint32_t o = params->outputs;
    const bool need_instance = (o & (SLHIP_CROP_INSTANCE | SLHIP_CROP_MASK)) || (params->isolate && (o & (SLHIP_CROP_COORD | SLHIP_CROP_NORMALS)));
    if (((o & SLHIP_CROP_RGB) && !buffers->d_rgb) || ((o & SLHIP_CROP_COORD) && !buffers->d_coord) ||
        ((o & SLHIP_CROP_NORMALS) && !buffers->d_normals) || (need_instance && !buffers->d_instance)) {
        slhip::set_error("%s: outputs 0x%x, isolate %u: a render target they read is NULL (rgb, coord, normals; instance for "
                         "the instance and mask outputs and for isolate)", who, o, params->isolate);
        return -1;
    }
    if (((o & SLHIP_CROP_RGB) && !out->d_rgb) || ((o & SLHIP_CROP_COORD) && !out->d_coord) || ((o & SLHIP_CROP_NORMALS) && !out->d_normals) ||
        ((o & SLHIP_CROP_INSTANCE) && !out->d_instance) || ((o & SLHIP_CROP_MASK) && !out->d_mask)) {
        slhip::set_error("%s: outputs 0x%x: a requested output pointer is NULL", who, o);
        return -1;
    }
    Source src;
    src.rgb = reinterpret_cast<const uint32_t*>(buffers->d_rgb);
    src.coord = reinterpret_cast<const float4*>(buffers->d_coord);
    src.normals = reinterpret_cast<const float4*>(buffers->d_normals);
    src.instance = buffers->d_instance;
    src.masks = d_masks;
    src.words = reinterpret_cast<const unsigned long long*>(d_words);
    Dest dst;
    dst.rgb = reinterpret_cast<uint32_t*>(out->d_rgb);
    dst.coord = reinterpret_cast<float4*>(out->d_coord);
    dst.normals = reinterpret_cast<float4*>(out->d_normals);
    dst.instance = out->d_instance;
    dst.mask = out->d_mask;
    const uint32_t bpc = (params->size * params->size + 255u) / 256u;      // blocks per crop
    const uint64_t per_launch = 0x7fffffffu / bpc;                         // crops whose blocks fit the grid's x extent
    if (const int st = g_timer.begin(1, stream)) return st;
    for (uint64_t c0 = 0; c0 < n_crops; c0 += per_launch) {
        const uint64_t n = std::min<uint64_t>(per_launch, n_crops - c0);
        k_crop_gather<<<dim3((uint32_t)(n * bpc)), 256, 0, stream>>>(*params, d_crops, c0, bpc, src, n_scenes, n_slots, W, H, dst);
    }
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(1, stream);
}
