// slhip_render_masks.inc -- per-object masks of a finished render (slhip_render_object_masks, slhip_object_masks_expand,
// include/slhip.h): every slot's whole silhouette (kind 0, BOP's mask/) and visible part (kind 1, mask_visib/) as bit tiles in
// the caller's word pool, and as uncompressed column-major run lengths (COCO's RLE, scene_gt_coco.json).  Included at the end
// of slhip_render.hip after slhip_render_stats.inc: the silhouettes are the words os_run() rasterises for the statistics, kept
// instead of dropped.  See DESIGN.md section 4.
//
// The passes after os_run() (which has called om_save_layout: tile box and word offsets of both kinds into the mask records):
//   k_om_visible  the visibility keys of the render: key -> primitive -> draw -> slot (k_os_visible's rule), the pixel's bit
//                 into the slot's kind-1 words; neighbouring lanes that hit one word combine their bits before the atomicOr
//   k_om_count    one wave per (scene, slot, kind): the run boundaries of the mask in COCO order, lanes over image columns
//   k_om_scan     one block: exclusive scan of the run counts -> rle_offset, total to the host; a slot whose whole silhouette
//                 is empty gets the empty tile box
//   k_om_emit     the walk of k_om_count again; every lane writes the run lengths that end in its column
//   k_om_expand   (its own entry) bit tiles -> dense bytes
// Integers only; the atomics are `or` and nothing else: the same bits from run to run.

#include "slhip_mask_walk.h"

namespace {

struct OmRec {
    int tile_box[4];
    unsigned long long word_offset[2];
    unsigned long long rle_offset[2];
    unsigned rle_count[2];
};
static_assert(sizeof(OmRec) == sizeof(slhip_object_mask) && sizeof(OmRec) == 56, "slhip_object_mask layout");

__device__ __forceinline__ slhip_mask::TileBox om_box(const OmRec& r)
{
    return slhip_mask::TileBox{r.tile_box[0], r.tile_box[1], r.tile_box[2], r.tile_box[3]};
}

// after k_os_scan: the record's bbox_obj is the tile box, bbox_visib[0..1] the first word; kind 1 follows the `total` words of kind 0
__global__ __launch_bounds__(256) void k_om_save(OmRec* __restrict__ masks, const OsRec* __restrict__ out, size_t n, unsigned long long total)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const OsRec r = out[i];
        OmRec m;
        m.tile_box[0] = r.bbox_obj[0]; m.tile_box[1] = r.bbox_obj[1]; m.tile_box[2] = r.bbox_obj[2]; m.tile_box[3] = r.bbox_obj[3];
        const unsigned long long off = *reinterpret_cast<const unsigned long long*>(r.bbox_visib);
        m.word_offset[0] = off; m.word_offset[1] = total + off;
        m.rle_offset[0] = m.rle_offset[1] = 0ull;
        m.rle_count[0] = m.rle_count[1] = 0u;
        masks[i] = m;
    }
}

void om_save_layout(slhip_object_mask* d_masks, const OsRec* out, size_t n, unsigned long long total, hipStream_t stream)
{
    const unsigned gs = (unsigned)std::min<size_t>((n + 255) / 256, 4096);
    k_om_save<<<gs, 256, 0, stream>>>(reinterpret_cast<OmRec*>(d_masks), out, n, total);
}

constexpr unsigned long long kOmNoWord = ~0ull;

// grid (blocks per scene, scene): k_os_visible's pass over the keys, one pixel per lane and step, every lane of a wave in every
// step (the shuffles below need them all).  Lanes are consecutive pixels of a row, so the lanes of one word sit side by side,
// eight at the most: three shuffle steps gather their bits in the first of them -- the lane whose left neighbour has another
// word, or every eighth lane -- and that lane alone issues the atomicOr.  (A lane may gather bits that another head ORs as
// well; OR does not mind.)
__global__ __launch_bounds__(256) void k_om_visible(const slhip_scene* __restrict__ scenes, const slhip_draw* __restrict__ draws,
                                                    const unsigned long long* __restrict__ vis, int W, int H, unsigned n_slots,
                                                    const OmRec* __restrict__ masks, unsigned long long* __restrict__ pool_words)
{
    __shared__ unsigned s_prim[kOsLdsDraws];
    __shared__ unsigned s_slot[kOsLdsDraws];
    const unsigned scene = blockIdx.y;
    const slhip_scene* sc = scenes + scene;
    const unsigned nd = sc->draw_end - sc->draw_begin;
    const bool lds_draws = nd <= (unsigned)kOsLdsDraws;
    for (unsigned k = threadIdx.x; k < (unsigned)kOsLdsDraws; k += blockDim.x) {
        const bool in = lds_draws && k < nd;
        s_prim[k] = in ? draws[sc->draw_begin + k].prim_base : 0xFFFFFFFFu;
        s_slot[k] = in ? os_slot(draws + sc->draw_begin + k) : 0u;
    }
    __syncthreads();
    const OmRec* mrec = masks + (size_t)scene * n_slots;
    const size_t P = (size_t)W * H;
    const unsigned long long* v = vis + (size_t)scene * P;
    const unsigned lane = threadIdx.x & 63u;
    for (size_t base = (size_t)blockIdx.x * blockDim.x; base < P; base += (size_t)gridDim.x * blockDim.x) {
        const size_t p = base + threadIdx.x;
        unsigned long long word = kOmNoWord, bits = 0ull;
        const unsigned long long key = p < P ? v[p] : kVisEmpty;
        if (key != kVisEmpty && nd > 0u) {
            const unsigned prim = (unsigned)(key & 0xFFFFFFFFull);
            const unsigned k = draw_of_prim(s_prim, kOsLdsDraws, nd, sc, draws, prim);
            const unsigned slot = lds_draws ? s_slot[k] : os_slot(draws + sc->draw_begin + k);
            if (slot != 0u && slot < n_slots) {
                const OmRec* r = mrec + slot;
                const int x = (int)(p % (size_t)W), y = (int)(p / (size_t)W);
                const int tx = x >> 3, ty = y >> 3;
                const int tx0 = r->tile_box[0], ty0 = r->tile_box[1], tx1 = r->tile_box[2], ty1 = r->tile_box[3];
                // a visible pixel lies inside its slot's box (the box holds every vertex); a guard all the same
                if (tx >= tx0 && tx <= tx1 && ty >= ty0 && ty <= ty1) {
                    word = r->word_offset[1] + (unsigned long long)(ty - ty0) * (unsigned long long)(tx1 - tx0 + 1)
                         + (unsigned long long)(tx - tx0);
                    bits = 1ull << ((y & 7) * 8 + (x & 7));
                }
            }
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            const unsigned long long w2 = __shfl_down(word, o), b2 = __shfl_down(bits, o);
            if (w2 == word) bits |= b2;
        }
        const unsigned long long left = __shfl_up(word, 1);
        if (word != kOmNoWord && ((lane & 7u) == 0u || left != word)) atomicOr(pool_words + word, bits);
    }
}

// The masks in the order of the scan: record-major, kind minor.  One wave per mask.
__global__ __launch_bounds__(256) void k_om_count(OmRec* __restrict__ masks, size_t n_masks, int W, int H,
                                                  const unsigned long long* __restrict__ pool_words)
{
    const unsigned lane = threadIdx.x & 63u;
    const size_t wave0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    for (size_t m = wave0; m < n_masks; m += n_waves) {
        OmRec* rec = masks + (m >> 1);
        const unsigned kind = (unsigned)(m & 1u);
        const slhip_mask::TileBox box = om_box(*rec);
        unsigned cnt = 0u;
        if (box.tx0 <= box.tx1) {
            const unsigned long long* w = pool_words + rec->word_offset[kind];
            // the box's columns and the one after them (where a run that came down the last column ends)
            const int xs = 8 * box.tx0, xe = min(8 * box.tx1 + 8, W - 1);
            for (int x = xs + (int)lane; x <= xe; x += 64) cnt += slhip_mask::walk_column(w, box, x, H, [](unsigned) {});
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (lane == 0u) rec->rle_count[kind] = cnt + 1u;
    }
}

// k_os_scan's pattern over the run counts: one block of 1024 threads walks the masks in order
__global__ __launch_bounds__(1024) void k_om_scan(OmRec* __restrict__ masks, size_t n_masks, unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long s_wave[16];
    __shared__ unsigned long long s_carry;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0ull;
    __syncthreads();
    for (size_t base = 0; base < n_masks; base += 1024) {
        const size_t m = base + threadIdx.x;
        const unsigned long long cnt = m < n_masks ? (unsigned long long)masks[m >> 1].rle_count[m & 1u] : 0ull;
        unsigned long long inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long v = __shfl_up(inc, o);
            if ((int)lane >= o) inc += v;
        }
        if (lane == 63u) s_wave[wave] = inc;
        __syncthreads();
        unsigned long long before = s_carry;
        for (unsigned w = 0; w < wave; ++w) before += s_wave[w];
        if (m < n_masks) {
            OmRec* rec = masks + (m >> 1);
            rec->rle_offset[m & 1u] = before + inc - cnt;
            // A whole silhouette of one run length is empty (a full one has two: 0, W * H), and so is its visible part: the
            // record says "no tiles", whatever box the vertices gave it (an object behind the camera: the whole viewport).
            if ((m & 1u) == 0u && cnt == 1ull) { rec->tile_box[0] = 0; rec->tile_box[1] = 0; rec->tile_box[2] = -1; rec->tile_box[3] = -1; }
        }
        __syncthreads();
        if (threadIdx.x == 1023u) s_carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}

// One wave per mask, 64 image columns per step.  A lane counts the boundaries of its column, an exclusive scan over the lanes
// (plus what the steps before have emitted) gives the index of its first run length, a running maximum over the lanes the
// last boundary before its column; then it walks the column again and writes length = boundary - boundary before.  The last
// run, from the last boundary to W * H, is lane 0's.
__global__ __launch_bounds__(256) void k_om_emit(const OmRec* __restrict__ masks, size_t n_masks, int W, int H,
                                                 const unsigned long long* __restrict__ pool_words, unsigned* __restrict__ runs)
{
    const unsigned lane = threadIdx.x & 63u;
    const size_t wave0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((size_t)gridDim.x * blockDim.x) >> 6;
    const unsigned N = (unsigned)W * (unsigned)H;
    for (size_t m = wave0; m < n_masks; m += n_waves) {
        const OmRec* rec = masks + (m >> 1);
        const unsigned kind = (unsigned)(m & 1u);
        const slhip_mask::TileBox box = om_box(*rec);
        unsigned* out = runs + rec->rle_offset[kind];
        unsigned done = 0u;      // run lengths written by the steps so far
        unsigned last = 0u;      // the last boundary so far (0: none yet, or one at position 0 -- the same length either way)
        if (box.tx0 <= box.tx1) {
            const unsigned long long* w = pool_words + rec->word_offset[kind];
            const int xs = 8 * box.tx0, xe = min(8 * box.tx1 + 8, W - 1);
            for (int x0 = xs; x0 <= xe; x0 += 64) {
                const int x = x0 + (int)lane;
                unsigned mine_last = 0u;
                const unsigned cnt = x <= xe ? slhip_mask::walk_column(w, box, x, H, [&](unsigned pos) { mine_last = pos; }) : 0u;
                unsigned inc = cnt, mx = mine_last;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned v = __shfl_up(inc, o), q = __shfl_up(mx, o);
                    if ((int)lane >= o) { inc += v; mx = max(mx, q); }
                }
                unsigned before = __shfl_up(mx, 1);
                before = lane == 0u ? last : max(before, last);
                unsigned k = done + inc - cnt;
                if (cnt > 0u)
                    slhip_mask::walk_column(w, box, x, H, [&](unsigned pos) { out[k++] = pos - before; before = pos; });
                done += __shfl(inc, 63);
                last = max(last, __shfl(mx, 63));
            }
        }
        if (lane == 0u) out[done] = N - last;
    }
}

// one thread per (selected mask, image row, tile column): one row byte of a tile -> 8 output bytes, clipped to W
__global__ __launch_bounds__(256) void k_om_expand(const OmRec* __restrict__ masks, const unsigned long long* __restrict__ pool_words,
                                                   unsigned n_scenes, unsigned n_slots, int W, int H, unsigned kind,
                                                   const unsigned* __restrict__ select, size_t n_select, uint8_t* __restrict__ dense)
{
    const int tw = (W + 7) >> 3;
    const size_t total = n_select * (size_t)H * (size_t)tw;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int tx = (int)(i % (size_t)tw);
        const size_t row = i / (size_t)tw;
        const int y = (int)(row % (size_t)H);
        const size_t s = row / (size_t)H;
        const unsigned scene = select[2 * s], slot = select[2 * s + 1];
        unsigned b = 0u;
        if (scene < n_scenes && slot < n_slots) {
            const OmRec* r = masks + (size_t)scene * n_slots + slot;
            const int tx0 = r->tile_box[0], ty0 = r->tile_box[1], tx1 = r->tile_box[2], ty1 = r->tile_box[3];
            const int ty = y >> 3;
            if (tx >= tx0 && tx <= tx1 && ty >= ty0 && ty <= ty1) {
                const unsigned long long w = pool_words[r->word_offset[kind] + (unsigned long long)(ty - ty0) * (unsigned long long)(tx1 - tx0 + 1)
                                                        + (unsigned long long)(tx - tx0)];
                b = (unsigned)(w >> (8 * (y & 7))) & 0xFFu;
            }
        }
        // bit k of b -> byte k = 0 / 1 (byte k of the product holds b; the mask keeps its bit k; + 0x7F carries it into bit 7)
        unsigned long long e = ((unsigned long long)b * 0x0101010101010101ull) & 0x8040201008040201ull;
        e = ((e + 0x7F7F7F7F7F7F7F7Full) >> 7) & 0x0101010101010101ull;
        uint8_t* o = dense + row * (size_t)W + (size_t)tx * 8;
        const int nx = min(8, W - 8 * tx);
        if (nx == 8 && (W & 7) == 0) {
            *reinterpret_cast<unsigned long long*>(o) = e;
        } else {
            for (int k = 0; k < nx; ++k) o[k] = (uint8_t)((e >> (8 * k)) & 0xFFu);
        }
    }
}

}  // namespace

extern "C" int slhip_render_object_masks_bytes(uint32_t n_scenes, uint32_t n_slots, uint32_t width, uint32_t height,
                                               uint64_t* worst_words, uint64_t* worst_runs)
{
    if (!worst_words || !worst_runs) {
        slhip::set_error("slhip_render_object_masks_bytes: null argument");
        return -1;
    }
    const uint64_t objects = (uint64_t)n_scenes * (n_slots > 1u ? (uint64_t)(n_slots - 1u) : 0u);
    const uint64_t tiles = (uint64_t)((width + 7u) / 8u) * (uint64_t)((height + 7u) / 8u);
    *worst_words = 2u * objects * tiles;
    // slot 0 and every other empty mask is the single run [W * H]
    *worst_runs = 2u * ((uint64_t)n_scenes * n_slots + objects * (uint64_t)width * (uint64_t)height);
    return 0;
}

extern "C" int slhip_render_object_masks(const slhip_mesh_pool* pool, const slhip_scene* d_scenes, const slhip_draw* d_draws,
                                         const slhip_chunk* d_chunks, uint32_t n_scenes, uint32_t n_draws, uint32_t n_chunks,
                                         uint32_t width, uint32_t height, const slhip_render_scratch* scratch, uint32_t n_slots,
                                         uint64_t* d_words, uint64_t capacity_words, slhip_object_stats* d_out,
                                         uint64_t* words_needed, slhip_object_mask* d_masks, uint32_t* d_runs,
                                         uint64_t capacity_runs, uint64_t* runs_needed, void* stream_)
{
    (void)n_draws;
    static const char* who = "slhip_render_object_masks";
    hipStream_t stream = (hipStream_t)stream_;
    if (!d_masks || !d_runs) {
        slhip::set_error("%s: null argument (the mask records and the run pool are required)", who);
        return -1;
    }
    if ((uint64_t)width * (uint64_t)height > 0x7FFFFFFFull) {
        slhip::set_error("%s: %u x %u pixels do not fit the u32 run lengths", who, width, height);
        return -1;
    }
    if (runs_needed) *runs_needed = 0;
    const int st = os_run(who, SLHIP_OBJECT_MASKS_CAPACITY, pool, d_scenes, d_draws, d_chunks, n_scenes, n_chunks, width, height,
                          scratch, n_slots, d_words, capacity_words, 2u, d_out, d_masks, words_needed, stream);
    if (st != 0) return st;
    if (n_scenes == 0 || n_slots == 0 || width == 0 || height == 0) return 0;
    const int W = (int)width, H = (int)height;
    const size_t n_masks = 2 * (size_t)n_scenes * n_slots;
    OmRec* masks = reinterpret_cast<OmRec*>(d_masks);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(d_words);
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(scratch->d_queue);   // free again: k_os_large is done with it
    const size_t P = (size_t)W * H;
    const unsigned bps = (unsigned)std::min<size_t>((P + 255) / 256, 64);
    k_om_visible<<<dim3(bps, n_scenes), 256, 0, stream>>>(d_scenes, d_draws, reinterpret_cast<const unsigned long long*>(scratch->d_vis),
                                                          W, H, n_slots, masks, words);
    const unsigned gw = (unsigned)std::min<size_t>((n_masks + 3) / 4, 16384);   // 4 waves = 4 masks per block
    k_om_count<<<gw, 256, 0, stream>>>(masks, n_masks, W, H, words);
    k_om_scan<<<1, 1024, 0, stream>>>(masks, n_masks, d_total);
    SLHIP_LAUNCH_CHECK();
    unsigned long long total = 0;
    SLHIP_CHECK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, stream));
    SLHIP_CHECK(hipStreamSynchronize(stream));
    if (runs_needed) *runs_needed = total;
    if (total > capacity_runs) {
        slhip::set_error("%s: the run pool holds %llu run lengths, this batch needs %llu", who,
                         (unsigned long long)capacity_runs, total);
        return SLHIP_OBJECT_MASKS_CAPACITY;
    }
    k_om_emit<<<gw, 256, 0, stream>>>(masks, n_masks, W, H, words, d_runs);
    SLHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" int slhip_object_masks_expand(const slhip_object_mask* d_masks, const uint64_t* d_words, uint32_t n_scenes,
                                         uint32_t n_slots, uint32_t width, uint32_t height, uint32_t kind,
                                         const uint32_t* d_select, uint64_t n_select, uint8_t* d_dense, void* stream_)
{
    static const char* who = "slhip_object_masks_expand";
    if (!d_masks || !d_words || !d_select || !d_dense) {
        slhip::set_error("%s: null argument (mask records, word pool, selection and output are required)", who);
        return -1;
    }
    if (n_scenes == 0 || n_slots == 0 || width == 0 || height == 0 || n_select == 0) {
        slhip::set_error("%s: zero size (scenes, slots, width, height and the selection must not be empty)", who);
        return -1;
    }
    if (kind > 1u) {
        slhip::set_error("%s: kind %u (0: the whole silhouette, 1: the visible part)", who, kind);
        return -1;
    }
    const size_t total = (size_t)n_select * height * ((width + 7u) / 8u);
    const unsigned gs = (unsigned)std::min<size_t>((total + 255) / 256, 65535);
    k_om_expand<<<gs, 256, 0, (hipStream_t)stream_>>>(reinterpret_cast<const OmRec*>(d_masks),
                                                      reinterpret_cast<const unsigned long long*>(d_words), n_scenes, n_slots, (int)width,
                                                      (int)height, kind, d_select, (size_t)n_select, d_dense);
    SLHIP_LAUNCH_CHECK();
    return 0;
}
