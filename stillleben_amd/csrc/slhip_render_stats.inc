// slhip_render_stats.inc -- per-object visibility statistics of a finished render (slhip_render_object_stats, include/slhip.h):
// the pixel count and box of every object's whole silhouette ("as if drawn alone") and of its visible part, the numbers of the
// BOP toolkit's scene_gt_info.  Included at the end of slhip_render.hip, so that the silhouette raster runs the very set-up,
// clipping, fill rule and depth-range rules of the visibility pass (Setup, setup_tri, setup_from_screen, clip_near, raster_bbox,
// raster_or_enqueue) without moving any of that code.  See DESIGN.md section 4.
//
// Slot i of a scene is instance index i (slot 0: the background plane and other unindexed draws, always empty).  The passes:
//   k_os_bounds   per (scene, slot): min / max window coordinates of the slot's vertices (the dense plane of d_vattr; a vertex
//                 behind the near plane widens the box to the whole viewport)
//   k_os_scan     one block: the 8 x 8-tile box of each (scene, slot) and an exclusive scan of the tile counts -> the slot's run
//                 of u64 words in the caller's pool (one word per tile, bit (py & 7) * 8 + (px & 7) = one pixel)
//   k_os_raster   the chunk list over the object draws: MainTarget's depth rules, the alpha test of alpha-tested draws, then an
//   k_os_large    atomicOr of the pixel's bit (large triangles: one wave per (triangle, 8x8 tile) builds the whole word)
//   k_os_silhouette  popcount + box over each slot's words
//   k_os_visible  the visibility keys of the render: key -> primitive -> draw -> instance, count and box per slot
//   k_os_finish   boxes to BOP's (x, y, w, h)
// Everything is integer atomics (add / or / min / max): the results do not depend on the order of execution.
//
// Working space: until k_os_silhouette the output records hold the per-slot state -- bbox_obj the vertex box (window
// coordinates, 1/256 px), then the tile box; bbox_visib[0..1] the slot's first word in the pool (u64).

namespace {

constexpr int kOsLdsSlots = 256;    // slots accumulated in LDS by k_os_visible (beyond: global atomics per run)
constexpr int kOsLdsDraws = 256;    // draws of a scene whose first primitive ids k_os_visible keeps in LDS (beyond: global search)

struct OsRec {
    unsigned px_visib, px_all;
    int bbox_visib[4], bbox_obj[4];
};
static_assert(sizeof(OsRec) == sizeof(slhip_object_stats), "slhip_object_stats layout");

__device__ __forceinline__ unsigned os_slot(const slhip_draw* dr) { return dr->instance_index & 0xFFFFu; }

__device__ __forceinline__ unsigned long long& os_word_offset(OsRec* r) { return *reinterpret_cast<unsigned long long*>(r->bbox_visib); }

// every record: vertex box empty, no word run
__global__ __launch_bounds__(256) void k_os_init(OsRec* __restrict__ out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        OsRec r;
        r.px_visib = 0u; r.px_all = 0u;
        r.bbox_visib[0] = r.bbox_visib[1] = r.bbox_visib[2] = r.bbox_visib[3] = 0;
        r.bbox_obj[0] = r.bbox_obj[1] = INT_MAX;
        r.bbox_obj[2] = r.bbox_obj[3] = INT_MIN;
        out[i] = r;
    }
}

__device__ __forceinline__ int wave_min(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// grid (scene, slice): the block strides over the vertices of every object draw of its scene.  A vertex behind the near plane
// carries X = kScreenClipped = INT_MIN, so the minimum itself says "whole viewport"; its Y and the maxima ignore it.
__global__ __launch_bounds__(256) void k_os_bounds(const slhip_scene* __restrict__ scenes, const slhip_draw* __restrict__ draws,
                                                   const uint4* __restrict__ screen, unsigned n_slots, OsRec* __restrict__ out)
{
    const unsigned scene = blockIdx.x;
    const slhip_scene* sc = scenes + scene;
    for (unsigned d = sc->draw_begin; d < sc->draw_end; ++d) {
        const slhip_draw* dr = draws + d;
        const unsigned slot = os_slot(dr);
        if (slot == 0u || slot >= n_slots) continue;
        int xmn = INT_MAX, ymn = INT_MAX, xmx = INT_MIN, ymx = INT_MIN;
        for (unsigned v = blockIdx.y * blockDim.x + threadIdx.x; v < dr->n_verts; v += gridDim.y * blockDim.x) {
            const uint4 s = screen[dr->clip_base + v];
            const int X = (int)s.x, Y = (int)s.y;
            xmn = min(xmn, X);
            if (X != kScreenClipped) { ymn = min(ymn, Y); xmx = max(xmx, X); ymx = max(ymx, Y); }
        }
        xmn = wave_min(xmn); ymn = wave_min(ymn); xmx = wave_max(xmx); ymx = wave_max(ymx);
        if ((threadIdx.x & 63u) == 0u && xmn != INT_MAX) {
            OsRec* r = out + (size_t)scene * n_slots + slot;
            atomicMin(&r->bbox_obj[0], xmn); atomicMin(&r->bbox_obj[1], ymn);
            atomicMax(&r->bbox_obj[2], xmx); atomicMax(&r->bbox_obj[3], ymx);
        }
    }
}

// One block of 1024 threads walks the records in order: the vertex box becomes the 8 x 8-tile box (clamped to the viewport;
// the pixel box rule of setup_finish()), the tile counts are scanned into word offsets, the total goes to *total.
__global__ __launch_bounds__(1024) void k_os_scan(OsRec* __restrict__ out, size_t n, int W, int H,
                                                  unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long s_wave[16];
    __shared__ unsigned long long s_carry;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0ull;
    __syncthreads();
    for (size_t base = 0; base < n; base += 1024) {
        const size_t i = base + threadIdx.x;
        unsigned long long cnt = 0ull;
        int tb[4] = {0, 0, -1, -1};
        if (i < n) {
            const OsRec r = out[i];
            if (r.bbox_obj[0] != INT_MAX) {
                int x0, y0, x1, y1;
                if (r.bbox_obj[0] == kScreenClipped) {
                    x0 = 0; y0 = 0; x1 = W - 1; y1 = H - 1;
                } else {
                    x0 = max((r.bbox_obj[0] - 128 + 255) >> 8, 0); x1 = min((r.bbox_obj[2] - 128) >> 8, W - 1);
                    y0 = max((r.bbox_obj[1] - 128 + 255) >> 8, 0); y1 = min((r.bbox_obj[3] - 128) >> 8, H - 1);
                }
                if (x0 <= x1 && y0 <= y1) {
                    tb[0] = x0 >> 3; tb[1] = y0 >> 3; tb[2] = x1 >> 3; tb[3] = y1 >> 3;
                    cnt = (unsigned long long)(tb[2] - tb[0] + 1) * (unsigned long long)(tb[3] - tb[1] + 1);
                }
            }
        }
        // inclusive scan in the wave, then over the 16 wave totals
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
        if (i < n) {
            OsRec* r = out + i;
            r->bbox_obj[0] = tb[0]; r->bbox_obj[1] = tb[1]; r->bbox_obj[2] = tb[2]; r->bbox_obj[3] = tb[3];
            os_word_offset(r) = before + inc - cnt;
        }
        __syncthreads();
        if (threadIdx.x == 1023u) s_carry = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = s_carry;
}

// fragment emission into the slot's tile words: MainTarget's depth rules and its AlphaTest, no peel test, no key
struct StatsTarget {
    unsigned long long* words;   // the slot's run
    int tx0, ty0, tx1, ty1;      // its tile box
    AlphaTest alpha;             // pool_tex == nullptr: no alpha test

    __device__ __forceinline__ bool passes(const Setup& t, int px, int py, const float* l) const
    {
        const float z = interp(l, t.z[0], t.z[1], t.z[2]);
        if (!(z >= 0.0f && z <= 1.0f)) return false;
        if (depth24(z) >= 0xFFFFFFu) return false;   // a fragment AT the far plane loses (R6)
        if (alpha.pool_tex) {
            float b[3];
            alpha.persp_bary(t, l, b);
            if (alpha.discards(t, px, py, b)) return false;
        }
        return true;
    }
    // the tile's word, nullptr outside the slot's box (cannot happen: the box holds every vertex; a guard all the same)
    __device__ __forceinline__ unsigned long long* word(int px, int py) const
    {
        const int tx = px >> 3, ty = py >> 3;
        if (tx < tx0 || tx > tx1 || ty < ty0 || ty > ty1) return nullptr;
        return words + (size_t)(ty - ty0) * (size_t)(tx1 - tx0 + 1) + (size_t)(tx - tx0);
    }
    __device__ __forceinline__ void emit(const Setup& t, int px, int py, const float* l) const
    {
        if (!passes(t, px, py, l)) return;
        unsigned long long* w = word(px, py);
        if (w) atomicOr(w, 1ull << ((py & 7) * 8 + (px & 7)));
    }
};

__device__ __forceinline__ bool os_target(const OsRec* __restrict__ out, unsigned n_slots, unsigned scene, const slhip_draw* dr,
                                          unsigned long long* pool_words, StatsTarget& tgt)
{
    const unsigned slot = os_slot(dr);
    if (slot == 0u || slot >= n_slots) return false;
    const OsRec* r = out + (size_t)scene * n_slots + slot;
    tgt.tx0 = r->bbox_obj[0]; tgt.ty0 = r->bbox_obj[1]; tgt.tx1 = r->bbox_obj[2]; tgt.ty1 = r->bbox_obj[3];
    if (tgt.tx0 > tgt.tx1) return false;
    tgt.words = pool_words + *reinterpret_cast<const unsigned long long*>(r->bbox_visib);
    tgt.alpha.pool_tex = nullptr;
    return true;
}

// raster_chunk() with the silhouette target: the same triangles through the same definitions (for_each_setup, walk_attr_tri), the
// same queue for large triangles.  kAttr: the alpha-tested draws (per-pixel walk, as in raster_chunk<true>).
template <bool kAttr>
__global__ __launch_bounds__(256) SLHIP_LIGHT_KERNEL void k_os_raster(slhip_mesh_pool pool, const slhip_draw* __restrict__ draws,
                                                   const slhip_chunk* __restrict__ chunks, unsigned n_chunks, int W, int H,
                                                   const OsRec* __restrict__ out, unsigned n_slots,
                                                   unsigned long long* __restrict__ pool_words, unsigned* queue, unsigned capacity,
                                                   const float4* __restrict__ clipbuf, const uint4* __restrict__ screen)
{
    for (unsigned c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const slhip_chunk ch = chunks[c];
        if (threadIdx.x >= ch.count) continue;
        const slhip_draw* dr = draws + ch.draw;
        if (draw_alpha_tested(dr->flags) != kAttr) continue;
        StatsTarget tgt;
        if (!os_target(out, n_slots, ch.scene, dr, pool_words, tgt)) continue;
        const unsigned tri = ch.first_tri + threadIdx.x;
        const unsigned* ip = pool.d_idx + dr->idx_base + 3 * (size_t)tri;
        const unsigned vi[3] = {ip[0], ip[1], ip[2]};
        if constexpr (!kAttr) {
            const uint4 s0 = screen[dr->clip_base + vi[0]], s1 = screen[dr->clip_base + vi[1]], s2 = screen[dr->clip_base + vi[2]];
            for_each_setup<false>(s0, s1, s2, clipbuf, dr->clip_base, vi, W, H, [&](int sub, const Setup& t, const float*, const float*, const float*) {
                raster_or_enqueue(t, tgt, queue, capacity, ch.draw, tri | ((unsigned)sub << 31), ch.scene, kSmallArea);
                return true;
            });
        } else {
            ClipVert cv[3];
            clip_tri<true>(clipbuf, dr->clip_base, vi, cv);
            float uvs[6];
            tgt.alpha = AlphaTest::from_draw(pool, dr, vi, uvs);
            walk_attr_tri(cv, W, H, tgt);
        }
    }
}

// k_large with the silhouette target: one wave per contiguous run of the queue's tiles, lane == pixel of the 8 x 8 tile; the
// wave's ballot is the tile's word, one atomicOr per (triangle, tile).  Set-up and tile enumeration are wave-uniform, so every
// lane reaches the ballot.
__global__ __launch_bounds__(256) SLHIP_LIGHT_KERNEL void k_os_large(slhip_mesh_pool pool, const slhip_draw* __restrict__ draws, int W, int H,
                                                  const OsRec* __restrict__ out, unsigned n_slots,
                                                  unsigned long long* __restrict__ pool_words,
                                                  const unsigned* __restrict__ queue, unsigned capacity,
                                                  const float4* __restrict__ clipbuf, const uint4* __restrict__ screen)
{
    const QueueShare q(queue, capacity);
    const unsigned lane = threadIdx.x & 63;
    for (unsigned e = q.walk.e0; e < q.walk.e1; ++e) {
        const slhip_tq::Entry en = q.entries[e];
        if (q.walk.done(en)) break;
        unsigned k0, k1;
        if (!q.walk.tiles(en, k0, k1)) continue;
        Setup t;
        StatsTarget tgt;
        const slhip_draw* dr = draws + en.draw;
        if (!os_target(out, n_slots, en.scene_aux, dr, pool_words, tgt)) continue;
        unsigned tri;
        if (!entry_setup(en, dr, pool, screen, clipbuf, W, H, t, tri)) continue;
        TilePixels tp(en, k0, lane);
        for (unsigned k = k0; k < k1; ++k) {
            int px, py;
            tp.next(px, py);
            bool cov = !(px < t.xmin || px > t.xmax || py < t.ymin || py > t.ymax);
            float l[3];
            cov = cov && coverage(t, px, py, l);
            cov = cov && tgt.passes(t, px, py, l);
            const unsigned long long bits = __ballot(cov);   // bit lane == bit (py & 7) * 8 + (px & 7)
            if (lane == 0 && bits != 0ull) {
                unsigned long long* w = tgt.word(px, py);
                if (w) atomicOr(w, bits);
            }
        }
    }
}

// one block per (scene, slot), grid-stride: popcount and box of the slot's words.  Also readies the visible-part accumulators
// (count 0, box min = INT_MAX, max = -1).
__global__ __launch_bounds__(256) void k_os_silhouette(OsRec* __restrict__ out, size_t n, const unsigned long long* __restrict__ pool_words)
{
    __shared__ int s_red[5][4];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (size_t i = blockIdx.x; i < n; i += gridDim.x) {
        const OsRec r = out[i];
        const int tx0 = r.bbox_obj[0], ty0 = r.bbox_obj[1], tx1 = r.bbox_obj[2], ty1 = r.bbox_obj[3];
        const int tw = tx1 - tx0 + 1;
        const size_t nw = tx0 <= tx1 ? (size_t)tw * (size_t)(ty1 - ty0 + 1) : 0;
        const unsigned long long* w = pool_words + *reinterpret_cast<const unsigned long long*>(r.bbox_visib);
        int cnt = 0, xmn = INT_MAX, ymn = INT_MAX, xmx = -1, ymx = -1;
        for (size_t k = threadIdx.x; k < nw; k += blockDim.x) {
            const unsigned long long b = w[k];
            if (b == 0ull) continue;
            cnt += __popcll(b);
            unsigned cols = 0u, rows = 0u;
#pragma unroll
            for (int y = 0; y < 8; ++y) {
                const unsigned row = (unsigned)(b >> (8 * y)) & 0xFFu;
                cols |= row;
                rows |= (row != 0u ? 1u : 0u) << y;
            }
            const int tx = tx0 + (int)(k % (size_t)tw), ty = ty0 + (int)(k / (size_t)tw);
            xmn = min(xmn, tx * 8 + __ffs(cols) - 1); xmx = max(xmx, tx * 8 + 31 - __clz(cols));
            ymn = min(ymn, ty * 8 + __ffs(rows) - 1); ymx = max(ymx, ty * 8 + 31 - __clz(rows));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        xmn = wave_min(xmn); ymn = wave_min(ymn); xmx = wave_max(xmx); ymx = wave_max(ymx);
        if (lane == 0u) { s_red[0][wave] = cnt; s_red[1][wave] = xmn; s_red[2][wave] = ymn; s_red[3][wave] = xmx; s_red[4][wave] = ymx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int nwv = (int)(blockDim.x >> 6);
            for (int v = 1; v < nwv; ++v) {
                s_red[0][0] += s_red[0][v];
                s_red[1][0] = min(s_red[1][0], s_red[1][v]); s_red[2][0] = min(s_red[2][0], s_red[2][v]);
                s_red[3][0] = max(s_red[3][0], s_red[3][v]); s_red[4][0] = max(s_red[4][0], s_red[4][v]);
            }
            OsRec o;
            o.px_all = (unsigned)s_red[0][0];
            if (s_red[0][0] > 0) {
                o.bbox_obj[0] = s_red[1][0]; o.bbox_obj[1] = s_red[2][0];
                o.bbox_obj[2] = s_red[3][0] - s_red[1][0] + 1; o.bbox_obj[3] = s_red[4][0] - s_red[2][0] + 1;
            } else {
                o.bbox_obj[0] = o.bbox_obj[1] = o.bbox_obj[2] = o.bbox_obj[3] = -1;
            }
            o.px_visib = 0u;
            o.bbox_visib[0] = o.bbox_visib[1] = INT_MAX;
            o.bbox_visib[2] = o.bbox_visib[3] = -1;
            out[i] = o;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void os_flush(OsRec* __restrict__ grec, int* __restrict__ lds, unsigned slot, int cnt, int xmn, int ymn,
                                         int xmx, int ymx)
{
    if (slot < (unsigned)kOsLdsSlots) {
        int* a = lds + 5 * slot;
        atomicAdd(a, cnt); atomicMin(a + 1, xmn); atomicMin(a + 2, ymn); atomicMax(a + 3, xmx); atomicMax(a + 4, ymx);
    } else {
        OsRec* r = grec + slot;
        atomicAdd(&r->px_visib, (unsigned)cnt);
        atomicMin(&r->bbox_visib[0], xmn); atomicMin(&r->bbox_visib[1], ymn);
        atomicMax(&r->bbox_visib[2], xmx); atomicMax(&r->bbox_visib[3], ymx);
    }
}

// grid (blocks per scene, scene): one pass over the visibility keys.  A pixel's key -> primitive -> draw (the last of the scene's
// draws whose first primitive id is <= the primitive: draw_of_prim) -> slot.  Each thread walks pixels 256 apart and keeps a
// run of one slot in registers (pixels of slot 0 do not break it); a run goes to LDS (or to the record) when the slot changes.
__global__ __launch_bounds__(256) void k_os_visible(const slhip_scene* __restrict__ scenes, const slhip_draw* __restrict__ draws,
                                                    const unsigned long long* __restrict__ vis, int W, int H, unsigned n_slots,
                                                    OsRec* __restrict__ out)
{
    __shared__ unsigned s_prim[kOsLdsDraws];
    __shared__ unsigned s_slot[kOsLdsDraws];
    __shared__ int s_acc[5 * kOsLdsSlots];
    const unsigned scene = blockIdx.y;
    const slhip_scene* sc = scenes + scene;
    const unsigned nd = sc->draw_end - sc->draw_begin;
    const bool lds_draws = nd <= (unsigned)kOsLdsDraws;
    const unsigned ls = min(n_slots, (unsigned)kOsLdsSlots);
    for (unsigned k = threadIdx.x; k < (unsigned)kOsLdsDraws; k += blockDim.x) {
        const bool in = lds_draws && k < nd;
        s_prim[k] = in ? draws[sc->draw_begin + k].prim_base : 0xFFFFFFFFu;
        s_slot[k] = in ? os_slot(draws + sc->draw_begin + k) : 0u;
    }
    for (unsigned k = threadIdx.x; k < ls; k += blockDim.x) {
        s_acc[5 * k] = 0; s_acc[5 * k + 1] = INT_MAX; s_acc[5 * k + 2] = INT_MAX; s_acc[5 * k + 3] = -1; s_acc[5 * k + 4] = -1;
    }
    __syncthreads();
    OsRec* grec = out + (size_t)scene * n_slots;
    const size_t P = (size_t)W * H;
    const unsigned long long* v = vis + (size_t)scene * P;
    unsigned cur = 0u;
    int cnt = 0, xmn = INT_MAX, ymn = INT_MAX, xmx = -1, ymx = -1;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long key = v[p];
        if (key == kVisEmpty) continue;
        const unsigned prim = (unsigned)(key & 0xFFFFFFFFull);
        const unsigned k = draw_of_prim(s_prim, kOsLdsDraws, nd, sc, draws, prim);
        const unsigned slot = lds_draws ? s_slot[k] : os_slot(draws + sc->draw_begin + k);
        if (slot == 0u || slot >= n_slots) continue;
        if (slot != cur) {
            if (cnt > 0) os_flush(grec, s_acc, cur, cnt, xmn, ymn, xmx, ymx);
            cur = slot; cnt = 0; xmn = ymn = INT_MAX; xmx = ymx = -1;
        }
        const int x = (int)(p % (size_t)W), y = (int)(p / (size_t)W);
        ++cnt;
        xmn = min(xmn, x); xmx = max(xmx, x); ymn = min(ymn, y); ymx = max(ymx, y);
    }
    if (cnt > 0) os_flush(grec, s_acc, cur, cnt, xmn, ymn, xmx, ymx);
    __syncthreads();
    for (unsigned k = threadIdx.x; k < ls; k += blockDim.x) {
        const int c = s_acc[5 * k];
        if (c == 0) continue;
        OsRec* r = grec + k;
        atomicAdd(&r->px_visib, (unsigned)c);
        atomicMin(&r->bbox_visib[0], s_acc[5 * k + 1]); atomicMin(&r->bbox_visib[1], s_acc[5 * k + 2]);
        atomicMax(&r->bbox_visib[2], s_acc[5 * k + 3]); atomicMax(&r->bbox_visib[3], s_acc[5 * k + 4]);
    }
}

__global__ __launch_bounds__(256) void k_os_finish(OsRec* __restrict__ out, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        OsRec* r = out + i;
        if (r->px_visib > 0u) {
            const int x0 = r->bbox_visib[0], y0 = r->bbox_visib[1];
            r->bbox_visib[2] = r->bbox_visib[2] - x0 + 1;
            r->bbox_visib[3] = r->bbox_visib[3] - y0 + 1;
        } else {
            r->bbox_visib[0] = r->bbox_visib[1] = r->bbox_visib[2] = r->bbox_visib[3] = -1;
        }
    }
}

}  // namespace

extern "C" int slhip_render_object_stats_bytes(uint32_t n_scenes, uint32_t n_slots, uint32_t width, uint32_t height,
                                               uint64_t* worst_case_words)
{
    if (!worst_case_words) {
        slhip::set_error("slhip_render_object_stats_bytes: null argument");
        return -1;
    }
    const uint64_t tiles = (uint64_t)((width + 7u) / 8u) * (uint64_t)((height + 7u) / 8u);
    *worst_case_words = (uint64_t)n_scenes * (n_slots > 1u ? (uint64_t)(n_slots - 1u) : 0u) * tiles;
    return 0;
}

namespace {

// the layout hook of slhip_render_object_masks (slhip_render_masks.inc): keeps every slot's tile box and word offset before
// k_os_silhouette overwrites them
void om_save_layout(slhip_object_mask* d_masks, const OsRec* out, size_t n, unsigned long long total, hipStream_t stream);

// The body shared by slhip_render_object_stats and slhip_render_object_masks (`who` names the entry in error texts).  `kinds`
// word runs of the scanned size follow one another in the pool (1: the silhouettes; 2: the visible bits after them, all zero
// on return); `d_masks` (masks entry only) receives the layout; `capacity_status` is the entry's "pool too small" status.
int os_run(const char* who, int capacity_status, const slhip_mesh_pool* pool, const slhip_scene* d_scenes, const slhip_draw* d_draws,
           const slhip_chunk* d_chunks, uint32_t n_scenes, uint32_t n_chunks, uint32_t width, uint32_t height,
           const slhip_render_scratch* scratch, uint32_t n_slots, uint64_t* d_words, uint64_t capacity_words, unsigned kinds,
           slhip_object_stats* d_out, slhip_object_mask* d_masks, uint64_t* words_needed, hipStream_t stream)
{
    if (!pool || !d_scenes || !d_draws || !scratch || !d_words || !d_out) {
        slhip::set_error("%s: null argument (mesh pool, scenes, draws, scratch, word pool and output are required)", who);
        return -1;
    }
    if (n_chunks > 0 && !d_chunks) {
        slhip::set_error("%s: null chunk list", who);
        return -1;
    }
    if (words_needed) *words_needed = 0;
    if (n_scenes == 0 || n_slots == 0 || width == 0 || height == 0) return 0;
    if (!scratch->d_vis || !scratch->d_queue || (n_chunks > 0 && (!scratch->d_clip || !scratch->d_vattr || scratch->n_clip_verts == 0))) {
        slhip::set_error("%s: the render's d_vis, d_queue, d_clip and d_vattr scratch are required", who);
        return -1;
    }
    const int W = (int)width, H = (int)height;
    const size_t n = (size_t)n_scenes * n_slots;
    OsRec* out = reinterpret_cast<OsRec*>(d_out);
    const float4* clipbuf = reinterpret_cast<const float4*>(scratch->d_clip);
    const uint4* screen = reinterpret_cast<const uint4*>(scratch->d_vattr) + 4 * (size_t)scratch->n_clip_verts;
    unsigned long long* words = reinterpret_cast<unsigned long long*>(d_words);
    // the render's queue header doubles as the place of the scan total (the queue is free once slhip_render has returned)
    unsigned long long* d_total = reinterpret_cast<unsigned long long*>(scratch->d_queue);
    const unsigned gs = (unsigned)std::min<size_t>((n + 255) / 256, 4096);

    k_os_init<<<gs, 256, 0, stream>>>(out, n);
    if (n_chunks > 0) {
        const unsigned slices = std::min(std::max(scratch->n_clip_verts / (n_scenes * 2048u), 1u), 16u);
        k_os_bounds<<<dim3(n_scenes, slices), 256, 0, stream>>>(d_scenes, d_draws, screen, n_slots, out);
    }
    k_os_scan<<<1, 1024, 0, stream>>>(out, n, W, H, d_total);
    SLHIP_LAUNCH_CHECK();
    unsigned long long total = 0;
    SLHIP_CHECK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, stream));
    SLHIP_CHECK(hipStreamSynchronize(stream));
    if (words_needed) *words_needed = total * kinds;
    if (total * kinds > capacity_words) {
        slhip::set_error("%s: the word pool holds %llu words, this batch needs %llu", who,
                         (unsigned long long)capacity_words, total * kinds);
        return capacity_status;
    }
    if (total > 0) SLHIP_CHECK(hipMemsetAsync(words, 0, (size_t)total * kinds * 8, stream));
    SLHIP_CHECK(hipMemsetAsync(scratch->d_queue, 0, 16, stream));
    if (d_masks) om_save_layout(d_masks, out, n, total, stream);
    if (n_chunks > 0 && total > 0) {
        k_os_raster<false><<<n_chunks, 256, 0, stream>>>(*pool, d_draws, d_chunks, n_chunks, W, H, out, n_slots, words,
                                                         scratch->d_queue, scratch->queue_capacity, clipbuf, screen);
        k_os_raster<true><<<min(n_chunks, 4096u), 256, 0, stream>>>(*pool, d_draws, d_chunks, n_chunks, W, H, out, n_slots, words,
                                                                    scratch->d_queue, scratch->queue_capacity, clipbuf, screen);
        k_os_large<<<2048, 256, 0, stream>>>(*pool, d_draws, W, H, out, n_slots, words, scratch->d_queue, scratch->queue_capacity,
                                             clipbuf, screen);
    }
    k_os_silhouette<<<(unsigned)std::min<size_t>(n, 65535), 256, 0, stream>>>(out, n, words);
    const size_t P = (size_t)W * H;
    const unsigned bps = (unsigned)std::min<size_t>(std::max<size_t>((P + 256 * 64 - 1) / (256 * 64), 1), 64);   // ~64 pixels per thread
    k_os_visible<<<dim3(bps, n_scenes), 256, 0, stream>>>(d_scenes, d_draws, reinterpret_cast<const unsigned long long*>(scratch->d_vis),
                                                          W, H, n_slots, out);
    k_os_finish<<<gs, 256, 0, stream>>>(out, n);
    SLHIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int slhip_render_object_stats(const slhip_mesh_pool* pool, const slhip_scene* d_scenes, const slhip_draw* d_draws,
                                         const slhip_chunk* d_chunks, uint32_t n_scenes, uint32_t n_draws, uint32_t n_chunks,
                                         uint32_t width, uint32_t height, const slhip_render_scratch* scratch, uint32_t n_slots,
                                         uint64_t* d_words, uint64_t capacity_words, slhip_object_stats* d_out,
                                         uint64_t* words_needed, void* stream_)
{
    (void)n_draws;
    return os_run("slhip_render_object_stats", SLHIP_OBJECT_STATS_CAPACITY, pool, d_scenes, d_draws, d_chunks, n_scenes, n_chunks,
                  width, height, scratch, n_slots, d_words, capacity_words, 1u, d_out, nullptr, words_needed, (hipStream_t)stream_);
}
