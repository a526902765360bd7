// Object regions (this project's addition, no counterpart in the reference): the targets of pose networks that classify every
// pixel into a surface region of its object and regress inside it (GDR-Net, EPOS, SO-Pose, ZebraPose's coarse levels) -- a bank
// of R region centres per mesh class by the farthest point sampling of the keypoints, the region of every mesh vertex with
// per-region counts and extents, and per pixel of a render the region of its object coordinate.  include/slhip.h "Object
// regions" and DESIGN.md "Object regions" are the contract; all arithmetic is float32, one rounded operation at a time
// (-ffp-contract=off), through slhip_region_rules.h on host and device alike, so tests/object_regions_ref.py restates it and
// every output is bit-exact against it.
//   centres              k_fps of slhip_fps.hip with n_fps = R (slhip::fps_device)
//   k_regions_vertices   blocks (x, class): one thread per vertex of the class, the class's centres at block-uniform addresses;
//                        counts by integer adds, extents by integer maxima of the bit patterns
//   k_regions_label      one wave per 256 consecutive bytes of `region`; a wave without object pixels writes its bytes and
//                        leaves, the others walk the distinct classes of their lanes with the class's centres at wave-uniform
//                        addresses
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "slhip.h"
#include "slhip_checks.h"
#include "slhip_common.h"
#include "slhip_fps.h"
#include "slhip_region_rules.h"
#include "slhip_step_timer.h"

namespace {

static_assert(sizeof(slhip_object_region_params) == 32, "slhip_object_region_params layout");
static_assert(sizeof(slhip_synth_object) == 16, "slhip_synth_object layout");
static_assert(SLHIP_REGION_NONE == slhip_rg::NONE, "SLHIP_REGION_NONE");

using Params = slhip_object_region_params;
namespace kp = slhip_kp;
namespace rg = slhip_rg;

constexpr uint32_t MAX_R = SLHIP_REGIONS_MAX;
constexpr uint32_t VERT_BLOCK = 256u;
constexpr uint32_t LABEL_BLOCK = 256u;
constexpr uint32_t LABEL_TRIPS = 4u;                       // pixels of a lane: lane, lane + 64, lane + 128, lane + 192 of the wave's
constexpr uint32_t WAVE_BYTES = 64u * LABEL_TRIPS;         // 256 bytes of `region` per wave, four per lane when they are stored
constexpr uint32_t BLOCK_BYTES = WAVE_BYTES * (LABEL_BLOCK / 64u);
constexpr uint32_t KEY_NONE = 0xffffffffu;

// ---- vertices ----------------------------------------------------------------------------------------------------------------
// Block (x, c) is class c; the blocks of a class stride over its vertices.  The ranges of the classes above c that overlap c's
// are listed in LDS first (none, for a table of distinct meshes): a vertex inside one of them is labelled by that class's
// blocks, not by this one, so vertex_region has one writer per byte; count and extent of class c take every vertex of c.
// Every read of the pool is inside [base, base + n), which class_vertices bounds by n_vertices; centre reads are inside row c
// of the bank, c < n_assets; count / extent writes are at (c, r) with r < R.
__global__ __launch_bounds__(VERT_BLOCK) void k_regions_vertices(const float4* __restrict__ pos, uint64_t n_vertices,
                                                                 const slhip_asset* __restrict__ assets, uint32_t n_assets,
                                                                 const slhip_draw* __restrict__ templates, uint32_t n_templates,
                                                                 const float4* __restrict__ centres, uint32_t R,
                                                                 uint8_t* __restrict__ vertex_region, int32_t* __restrict__ count,
                                                                 uint32_t* __restrict__ extent)
{
    __shared__ uint32_t s_lo[SLHIP_SYNTH_MAX_ASSETS], s_hi[SLHIP_SYNTH_MAX_ASSETS];
    __shared__ uint32_t s_n;
    const uint32_t c = blockIdx.y, tid = threadIdx.x;
    const slhip_asset& a = assets[c];
    uint64_t base;
    uint32_t n;
    kp::class_vertices(a, templates, n_templates, n_vertices, ~0ull, &base, &n);
    if (n == 0u) return;      // uniform over the block
    if (tid == 0u) s_n = 0u;
    __syncthreads();
    for (uint32_t c2 = c + 1u + tid; c2 < n_assets; c2 += VERT_BLOCK) {
        uint64_t b2;
        uint32_t n2;
        kp::class_vertices(assets[c2], templates, n_templates, n_vertices, ~0ull, &b2, &n2);
        if (n2 != 0u && b2 < base + n && base < b2 + n2) {
            const uint32_t i = atomicAdd(&s_n, 1u);      // < n_assets - 1 - c: one slot per class above c at the most
            s_lo[i] = (uint32_t)b2;                      // n_vertices < 2^32 (checked by the entry)
            s_hi[i] = (uint32_t)(b2 + n2);
        }
    }
    __syncthreads();
    const uint32_t n_above = s_n;
    float m2o[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) m2o[i] = a.mesh_to_object[i];
    const float4* cc = centres + (size_t)c * R;
    for (uint32_t v = blockIdx.x * VERT_BLOCK + tid; v < n; v += gridDim.x * VERT_BLOCK) {
        const float4 q = pos[base + v];
        const kp::P3 p = kp::object_point(m2o, q.x, q.y, q.z);
        rg::Near best = rg::near_start();
        for (uint32_t r = 0u; r < R; ++r) {
            const float4 k = cc[r];
            kp::P3 kc;
            kc.x = k.x; kc.y = k.y; kc.z = k.z;
            best = rg::near_offer(best, kp::d2(p, kc), (int)r);
        }
        const uint32_t r = (uint32_t)best.idx;
        const float4 k = cc[r];
        kp::P3 kc;
        kc.x = k.x; kc.y = k.y; kc.z = k.z;
        const rg::Local l = rg::local_of(p, kc);
        const size_t slot = (size_t)c * R + r;
        atomicAdd(&count[slot], 1);
        atomicMax(&extent[4u * slot], rg::magnitude_bits(l.dx));
        atomicMax(&extent[4u * slot + 1u], rg::magnitude_bits(l.dy));
        atomicMax(&extent[4u * slot + 2u], rg::magnitude_bits(l.dz));
        atomicMax(&extent[4u * slot + 3u], rg::magnitude_bits(l.d2));
        const uint32_t g = (uint32_t)(base + v);
        bool mine = true;
        for (uint32_t i = 0u; i < n_above; ++i) mine = mine && !(g >= s_lo[i] && g < s_hi[i]);
        if (mine) vertex_region[g] = (uint8_t)r;
    }
}

// ---- label -------------------------------------------------------------------------------------------------------------------
// `base` = region - mis is 4-byte aligned (mis = the low two bits of the pointer); byte v of base is pixel v - mis.  A lane
// stores the four bytes v .. v + 3, v = v0 + 4 * lane, as one word when all four are pixels, and byte by byte at the two ragged
// ends of the buffer.  Nothing outside [mis, mis + total) is written.
__device__ __forceinline__ void store_region(uint8_t* base, uint32_t v, uint32_t word, uint32_t mis, uint32_t end)
{
    if (v >= mis && v + 4u <= end) {
        *reinterpret_cast<uint32_t*>(base + v) = word;
    } else {
#pragma unroll
        for (uint32_t j = 0u; j < 4u; ++j)
            if (v + j >= mis && v + j < end) base[v + j] = (uint8_t)(word >> (8u * j));
    }
}

// The lanes hold their pixels strided (pixel t * 64 + lane of the wave's 256 in byte t of `packed`) so that the loads are
// coalesced; the stores want bytes 4 * lane .. 4 * lane + 3.  Byte 4 * lane + j sits in lane (4 * lane + j) & 63, byte lane >> 4.
__device__ __forceinline__ uint32_t gather_region_word(uint32_t packed, uint32_t lane)
{
    const uint32_t shift = 8u * (lane >> 4);
    uint32_t word = 0u;
#pragma unroll
    for (uint32_t j = 0u; j < 4u; ++j) {
        const uint32_t from = (uint32_t)__shfl((int)packed, (int)((4u * lane + j) & 63u), 64);
        word |= ((from >> shift) & 0xffu) << (8u * j);
    }
    return word;
}

// The first of a lane's four values that is not `none`, or `none`.
__device__ __forceinline__ uint32_t first_of(const uint32_t (&v)[LABEL_TRIPS], uint32_t none)
{
    uint32_t c = none;
#pragma unroll
    for (int t = (int)LABEL_TRIPS - 1; t >= 0; --t) c = v[t] != none ? v[t] : c;
    return c;
}

// One wave per WAVE_BYTES bytes of base.  total = N * H * W and end = mis + total fit 32 bits with room for the last block
// (checked by the entry).  Reads: instance and coord at pixels < total; classes at (image * O + object) * stride with image < N
// and object < O; centres at (class, r) with class < A (checked per lane) and r < R; histogram at (image * O + object) * R + r.
__global__ __launch_bounds__(LABEL_BLOCK) void k_regions_label(Params p, const int16_t* __restrict__ instance,
                                                               const float4* __restrict__ coord, const int32_t* __restrict__ classes,
                                                               uint32_t stride, const float4* __restrict__ centres,
                                                               uint8_t* __restrict__ base, uint32_t mis, float4* __restrict__ local,
                                                               uint32_t* __restrict__ histogram)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t O = p.n_objects, R = p.n_regions, HW = (uint32_t)p.W * (uint32_t)p.H;
    const uint32_t total = p.n_images * HW, end = mis + total;
    const uint32_t v0 = (blockIdx.x * (LABEL_BLOCK / 64u) + (threadIdx.x >> 6)) * WAVE_BYTES;
    if (v0 >= end) return;      // uniform over the wave
    const bool want_local = (p.outputs & SLHIP_REGIONS_OUT_LOCAL) != 0u;

    uint32_t pix[LABEL_TRIPS];
    bool in[LABEL_TRIPS];
    int obj[LABEL_TRIPS];
    bool any = false;
#pragma unroll
    for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) {
        const uint32_t v = v0 + t * 64u + lane;
        in[t] = v >= mis && v < end;
        pix[t] = v - mis;
        obj[t] = in[t] ? rg::pixel_object((int)instance[pix[t]], O) : -1;
        any = any || obj[t] >= 0;
    }
    if (__ballot(any) == 0ull) {      // about 85 % of a picture: no centre, no class, no coordinate is read
        store_region(base, v0 + 4u * lane, 0xffffffffu, mis, end);
        if (want_local) {
#pragma unroll
            for (uint32_t t = 0u; t < LABEL_TRIPS; ++t)
                if (in[t]) local[pix[t]] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        return;
    }

    // the class and the point of every pixel that will get a region; NONE_CLASS for the others
    constexpr uint32_t NONE_CLASS = 0xffffffffu;
    uint32_t cls[LABEL_TRIPS], todo[LABEL_TRIPS], key[LABEL_TRIPS];
    kp::P3 q[LABEL_TRIPS];
#pragma unroll
    for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) {
        cls[t] = NONE_CLASS;
        key[t] = KEY_NONE;
        q[t].x = q[t].y = q[t].z = 0.0f;
        if (obj[t] >= 0) {
            const uint32_t slot = (pix[t] / HW) * O + (uint32_t)obj[t];      // (image, object): < N * O
            const int c = classes[(size_t)slot * stride];
            if (rg::class_ok(c, p.n_assets)) {
                const float4 f = coord[pix[t]];
                if (rg::point_ok(f.x, f.y, f.z)) {
                    cls[t] = (uint32_t)c;
                    key[t] = slot * R;      // + region below; N * O * R < 2^32 (checked by the entry)
                    q[t].x = f.x; q[t].y = f.y; q[t].z = f.z;
                }
            }
        }
        todo[t] = cls[t];
    }

    // The distinct classes of the wave, one after the other: c comes out of a lane, so it and the addresses of the class's centres
    // are wave-uniform (one class is at most 4 KB: it stays in the scalar / L1 path).  Every lane keeps its own running best.
    rg::Near best[LABEL_TRIPS];
#pragma unroll
    for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) best[t] = rg::near_start();
    for (;;) {
        const uint32_t cand = first_of(todo, NONE_CLASS);
        const uint64_t m = __ballot(cand != NONE_CLASS);
        if (m == 0ull) break;
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)__builtin_ctzll(m));
        const float4* cc = centres + (size_t)c * R;
        bool mine[LABEL_TRIPS];
#pragma unroll
        for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) mine[t] = todo[t] == c;
        // an object is a few dozen pixels of a row: most of the wave's four 64-pixel trips hold no pixel of class c, and a trip
        // without one is skipped by a scalar branch
        bool trip[LABEL_TRIPS];
#pragma unroll
        for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) trip[t] = __ballot(mine[t]) != 0ull;
        const auto offer = [&](const float4& k, uint32_t r) {
            kp::P3 kc;
            kc.x = k.x; kc.y = k.y; kc.z = k.z;
#pragma unroll
            for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) {
                if (!trip[t]) continue;      // wave-uniform
                const rg::Near b = rg::near_offer(best[t], kp::d2(q[t], kc), (int)r);
                best[t].val = mine[t] ? b.val : best[t].val;
                best[t].idx = mine[t] ? b.idx : best[t].idx;
            }
        };
        // four centres per wait, and the next four on their way while these are compared: the scalar loads' latency lies under
        // the arithmetic (the index of the last prefetch is clamped into the class's row)
        uint32_t r = 0u;
        if (R >= 4u) {
            float4 k0 = cc[0], k1 = cc[1], k2 = cc[2], k3 = cc[3];
            for (; r + 4u <= R; r += 4u) {
                const uint32_t n = min(r + 4u, R - 4u);
                const float4 n0 = cc[n], n1 = cc[n + 1u], n2 = cc[n + 2u], n3 = cc[n + 3u];
                offer(k0, r);
                offer(k1, r + 1u);
                offer(k2, r + 2u);
                offer(k3, r + 3u);
                k0 = n0; k1 = n1; k2 = n2; k3 = n3;
            }
        }
        for (; r < R; ++r) offer(cc[r], r);
        for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) todo[t] = mine[t] ? NONE_CLASS : todo[t];
    }

    uint32_t packed = 0u;
#pragma unroll
    for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) {
        const bool has = cls[t] != NONE_CLASS;
        const uint32_t r = has ? (uint32_t)best[t].idx : (uint32_t)rg::NONE;
        packed |= r << (8u * t);
        key[t] = has ? key[t] + r : KEY_NONE;
        if (want_local && in[t]) {
            float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (has) {
                const float4 k = centres[(size_t)cls[t] * R + r];
                kp::P3 kc;
                kc.x = k.x; kc.y = k.y; kc.z = k.z;
                const rg::Local l = rg::local_of(q[t], kc);
                out = make_float4(l.dx, l.dy, l.dz, l.d2);
            }
            local[pix[t]] = out;
        }
    }
    store_region(base, v0 + 4u * lane, gather_region_word(packed, lane), mis, end);

    // The histogram: the wave counts each of its distinct (image, object, region) among its 256 pixels and one lane adds the
    // count, so a picture filled by one region costs one atomic per wave, not one per pixel.
    if (p.outputs & SLHIP_REGIONS_OUT_HISTOGRAM) {
        for (;;) {
            const uint32_t cand = first_of(key, KEY_NONE);
            const uint64_t m = __ballot(cand != KEY_NONE);
            if (m == 0ull) break;
            const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)__builtin_ctzll(m));
            uint32_t n = 0u;
#pragma unroll
            for (uint32_t t = 0u; t < LABEL_TRIPS; ++t) {
                n += (uint32_t)__popcll(__ballot(key[t] == k));
                key[t] = key[t] == k ? KEY_NONE : key[t];
            }
            if (lane == 0u) atomicAdd(&histogram[k], n);
        }
    }
}

// optional HIP-event timing (tools/time_object_regions.py): events round the last call's work of each of the three steps
slhip::StepTimer<3> g_timer;

int check_bank(const char* who, uint32_t n_assets, uint32_t n_regions)
{
    return slhip::check_fps(who, "n_regions", MAX_R, n_assets, n_regions);
}

int check_vertices(const char* who, const void* pos, uint64_t n_vertices, const void* assets, uint32_t n_assets, const void* templates,
                   uint32_t n_templates, const void* centres, uint32_t n_regions, const void* vertex_region, const void* count,
                   const void* extent, bool device)
{
    if (const int st = check_bank(who, n_assets, n_regions)) return st;
    if (n_vertices > 0xffffffffull) {
        slhip::set_error("%s: a pool of %llu vertices: 2^32 or more", who, (unsigned long long)n_vertices);
        return -1;
    }
    if (!assets || !centres || !count || !extent || (n_templates && !templates) || (n_vertices && (!pos || !vertex_region))) {
        slhip::set_error("%s: null argument (assets, centres, count, extent, and templates / vertices / vertex_region unless their count is 0)", who);
        return -1;
    }
    if (device && (((uintptr_t)centres & 15u) || ((uintptr_t)pos & 15u) || ((uintptr_t)count & 3u) || ((uintptr_t)extent & 3u))) {
        slhip::set_error("%s: the pool and the centres must be 16-byte aligned, count and extent 4-byte aligned", who);
        return -1;
    }
    return 0;
}

int check_label(const char* who, const Params* p, const void* instance, const void* coord, const void* classes, uint32_t stride,
                const void* centres, const void* region, const void* local, const void* histogram, bool device)
{
    if (const int st = slhip_object_regions_check_params(p)) return st;
    if (p->n_images == 0u) return 0;
    if (!instance || !coord || !classes || !centres || !region || ((p->outputs & SLHIP_REGIONS_OUT_LOCAL) && !local) ||
        ((p->outputs & SLHIP_REGIONS_OUT_HISTOGRAM) && !histogram)) {
        slhip::set_error("%s: null argument (instance, coord, classes, centres, region, and the outputs the bits ask for)", who);
        return -1;
    }
    if (stride == 0u) {
        slhip::set_error("%s: class_stride must be at least 1 (1: an [N, O] tensor, 4: slhip_synth_object records)", who);
        return -1;
    }
    if (!device) return 0;      // host arrays: plain C++ reads, no vector access
    if (((uintptr_t)instance & 1u) || ((uintptr_t)coord & 15u) || ((uintptr_t)classes & 3u) || ((uintptr_t)centres & 15u) ||
        ((p->outputs & SLHIP_REGIONS_OUT_LOCAL) && ((uintptr_t)local & 15u)) ||
        ((p->outputs & SLHIP_REGIONS_OUT_HISTOGRAM) && ((uintptr_t)histogram & 3u))) {
        slhip::set_error("%s: coord, centres and local must be 16-byte aligned, classes and histogram 4-byte, instance 2-byte", who);
        return -1;
    }
    return 0;
}

}  // namespace

extern "C" int slhip_object_regions_timing_enable(int on) { return g_timer.enable(on); }

extern "C" int slhip_object_regions_timings(float ms_out[3]) { return g_timer.read_for("slhip_object_regions_timings", ms_out); }

extern "C" int slhip_object_regions_check_params(const slhip_object_region_params* p)
{
    static const char* who = "slhip_object_regions";
    if (!p) {
        slhip::set_error("%s: null parameter record", who);
        return -1;
    }
    if (const int st = slhip::check_picture_sides(who, p->W, p->H)) return st;
    if ((uint64_t)p->n_images * (uint64_t)p->W * (uint64_t)p->H >= 0xffffffffull - 2048u) {
        slhip::set_error("%s: n_images %u of %d x %d: the pixels of one call must stay below 2^32 - 2048", who, p->n_images, p->W, p->H);
        return -1;
    }
    if (const int st = slhip::check_range(who, "n_objects", p->n_objects, 1u, SLHIP_SYNTH_MAX_OBJECTS)) return st;
    if (const int st = slhip::check_range(who, "n_regions", p->n_regions, 1u, MAX_R)) return st;
    if (const int st = slhip::check_range(who, "n_assets", p->n_assets, 1u, SLHIP_SYNTH_MAX_ASSETS)) return st;
    if (p->outputs & ~(SLHIP_REGIONS_OUT_LOCAL | SLHIP_REGIONS_OUT_HISTOGRAM)) {
        slhip::set_error("%s: outputs 0x%x has bits other than local 1 and histogram 2", who, p->outputs);
        return -1;
    }
    if ((uint64_t)p->n_images * p->n_objects * p->n_regions > 0xfffffffeull) {
        slhip::set_error("%s: a histogram of %u x %u x %u counters: 2^32 or more", who, p->n_images, p->n_objects, p->n_regions);
        return -1;
    }
    return 0;
}

extern "C" int slhip_object_regions_centres_bytes(uint32_t n_assets, uint64_t max_verts, uint64_t* bytes)
{
    if (!bytes) {
        slhip::set_error("slhip_object_regions_centres_bytes: null argument");
        return -1;
    }
    *bytes = slhip::fps_scratch_bytes(n_assets, max_verts);
    return 0;
}

extern "C" int slhip_object_regions_centres(const float* d_pos, uint64_t n_vertices, const slhip_asset* d_assets, uint32_t n_assets,
                                            const slhip_draw* d_templates, uint32_t n_templates, uint32_t n_regions,
                                            uint64_t max_verts, void* d_scratch, float* d_centres, int32_t* d_vertex, void* stream_)
{
    static const char* who = "slhip_object_regions_centres";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_bank(who, n_assets, n_regions)) return st;
    if (const int st = g_timer.begin(0, stream)) return st;
    if (const int st = slhip::fps_device(who, "n_regions", MAX_R, d_pos, n_vertices, d_assets, n_assets, d_templates, n_templates,
                                         n_regions, max_verts, d_scratch, d_centres, d_vertex, stream))
        return st;
    return g_timer.end(0, stream);
}

extern "C" int slhip_object_regions_centres_host(const float* h_pos, uint64_t n_vertices, const slhip_asset* h_assets,
                                                 uint32_t n_assets, const slhip_draw* h_templates, uint32_t n_templates,
                                                 uint32_t n_regions, float* h_centres, int32_t* h_vertex)
{
    return slhip::fps_host("slhip_object_regions_centres_host", "n_regions", MAX_R, h_pos, n_vertices, h_assets, n_assets, h_templates,
                           n_templates, n_regions, h_centres, h_vertex);
}

extern "C" int slhip_object_regions_vertices(const float* d_pos, uint64_t n_vertices, const slhip_asset* d_assets, uint32_t n_assets,
                                             const slhip_draw* d_templates, uint32_t n_templates, const float* d_centres,
                                             uint32_t n_regions, uint8_t* d_vertex_region, int32_t* d_count, float* d_extent,
                                             void* stream_)
{
    static const char* who = "slhip_object_regions_vertices";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_vertices(who, d_pos, n_vertices, d_assets, n_assets, d_templates, n_templates, d_centres, n_regions,
                                      d_vertex_region, d_count, d_extent, true))
        return st;
    const size_t slots = (size_t)n_assets * n_regions;
    if (const int st = g_timer.begin(1, stream)) return st;
    if (n_vertices) SLHIP_CHECK(hipMemsetAsync(d_vertex_region, SLHIP_REGION_NONE, (size_t)n_vertices, stream));
    SLHIP_CHECK(hipMemsetAsync(d_count, 0, slots * 4u, stream));
    SLHIP_CHECK(hipMemsetAsync(d_extent, 0, slots * 16u, stream));
    if (n_vertices) {
        // the blocks of a class stride over its vertices: 64 of them cover 16 384 vertices in one trip
        const dim3 grid(64u, n_assets);
        k_regions_vertices<<<grid, VERT_BLOCK, 0, stream>>>(reinterpret_cast<const float4*>(d_pos), n_vertices, d_assets, n_assets,
                                                           d_templates, n_templates, reinterpret_cast<const float4*>(d_centres),
                                                           n_regions, d_vertex_region, d_count, reinterpret_cast<uint32_t*>(d_extent));
        SLHIP_LAUNCH_CHECK();
    }
    return g_timer.end(1, stream);
}

extern "C" int slhip_object_regions_vertices_host(const float* h_pos, uint64_t n_vertices, const slhip_asset* h_assets,
                                                  uint32_t n_assets, const slhip_draw* h_templates, uint32_t n_templates,
                                                  const float* h_centres, uint32_t n_regions, uint8_t* h_vertex_region,
                                                  int32_t* h_count, float* h_extent)
{
    static const char* who = "slhip_object_regions_vertices_host";
    if (const int st = check_vertices(who, h_pos, n_vertices, h_assets, n_assets, h_templates, n_templates, h_centres, n_regions,
                                      h_vertex_region, h_count, h_extent, false))
        return st;
    const uint32_t R = n_regions;
    if (n_vertices) std::memset(h_vertex_region, SLHIP_REGION_NONE, (size_t)n_vertices);
    std::memset(h_count, 0, (size_t)n_assets * R * 4u);
    uint32_t* extent = reinterpret_cast<uint32_t*>(h_extent);
    std::memset(extent, 0, (size_t)n_assets * R * 16u);
    for (uint32_t c = 0; c < n_assets; ++c) {      // upwards: the highest class writes a shared vertex last
        const slhip_asset& a = h_assets[c];
        uint64_t base;
        uint32_t n;
        kp::class_vertices(a, h_templates, n_templates, n_vertices, ~0ull, &base, &n);
        const float* cc = h_centres + (size_t)c * R * 4u;
        for (uint32_t v = 0; v < n; ++v) {
            const float* q = h_pos + (base + v) * 4u;
            const kp::P3 p = kp::object_point(a.mesh_to_object, q[0], q[1], q[2]);
            const uint32_t r = (uint32_t)rg::nearest(cc, R, p);
            kp::P3 kc;
            kc.x = cc[4u * r]; kc.y = cc[4u * r + 1u]; kc.z = cc[4u * r + 2u];
            const rg::Local l = rg::local_of(p, kc);
            const size_t slot = (size_t)c * R + r;
            h_count[slot] += 1;
            const uint32_t m[4] = {rg::magnitude_bits(l.dx), rg::magnitude_bits(l.dy), rg::magnitude_bits(l.dz), rg::magnitude_bits(l.d2)};
            for (int i = 0; i < 4; ++i)
                if (m[i] > extent[4u * slot + i]) extent[4u * slot + i] = m[i];
            h_vertex_region[base + v] = (uint8_t)r;
        }
    }
    return 0;
}

extern "C" int slhip_object_regions_label(const slhip_object_region_params* params, const int16_t* d_instance, const float* d_coord,
                                          const int32_t* d_classes, uint32_t class_stride, const float* d_centres, uint8_t* d_region,
                                          float* d_local, uint32_t* d_histogram, void* stream_)
{
    static const char* who = "slhip_object_regions_label";
    hipStream_t stream = (hipStream_t)stream_;
    if (const int st = check_label(who, params, d_instance, d_coord, d_classes, class_stride, d_centres, d_region, d_local, d_histogram, true))
        return st;
    if (params->n_images == 0u) return 0;
    const uint32_t total = params->n_images * (uint32_t)params->W * (uint32_t)params->H;      // < 2^32 - 2048
    const uint32_t mis = (uint32_t)((uintptr_t)d_region & 3u);
    const uint32_t blocks = (uint32_t)(((uint64_t)total + mis + BLOCK_BYTES - 1u) / BLOCK_BYTES);
    if (const int st = g_timer.begin(2, stream)) return st;
    if (params->outputs & SLHIP_REGIONS_OUT_HISTOGRAM)
        SLHIP_CHECK(hipMemsetAsync(d_histogram, 0, (size_t)params->n_images * params->n_objects * params->n_regions * 4u, stream));
    k_regions_label<<<blocks, LABEL_BLOCK, 0, stream>>>(*params, d_instance, reinterpret_cast<const float4*>(d_coord), d_classes,
                                                       class_stride, reinterpret_cast<const float4*>(d_centres), d_region - mis, mis,
                                                       reinterpret_cast<float4*>(d_local), d_histogram);
    SLHIP_LAUNCH_CHECK();
    return g_timer.end(2, stream);
}

extern "C" int slhip_object_regions_label_host(const slhip_object_region_params* params, const int16_t* h_instance,
                                               const float* h_coord, const int32_t* h_classes, uint32_t class_stride,
                                               const float* h_centres, uint8_t* h_region, float* h_local, uint32_t* h_histogram)
{
    static const char* who = "slhip_object_regions_label_host";
    if (const int st = check_label(who, params, h_instance, h_coord, h_classes, class_stride, h_centres, h_region, h_local, h_histogram, false))
        return st;
    const Params& p = *params;
    if (p.n_images == 0u) return 0;
    const uint32_t O = p.n_objects, R = p.n_regions, HW = (uint32_t)p.W * (uint32_t)p.H;
    const bool want_local = (p.outputs & SLHIP_REGIONS_OUT_LOCAL) != 0u, want_hist = (p.outputs & SLHIP_REGIONS_OUT_HISTOGRAM) != 0u;
    if (want_hist) std::memset(h_histogram, 0, (size_t)p.n_images * O * R * 4u);
    for (uint32_t n = 0; n < p.n_images; ++n) {
        for (uint32_t i = 0; i < HW; ++i) {
            const size_t px = (size_t)n * HW + i;
            int region = rg::NONE;
            rg::Local l = {0.0f, 0.0f, 0.0f, 0.0f};
            const int obj = rg::pixel_object((int)h_instance[px], O);
            if (obj >= 0) {
                const size_t slot = (size_t)n * O + (uint32_t)obj;
                const int c = h_classes[slot * class_stride];
                const float* f = h_coord + px * 4u;
                if (rg::class_ok(c, p.n_assets) && rg::point_ok(f[0], f[1], f[2])) {
                    kp::P3 q;
                    q.x = f[0]; q.y = f[1]; q.z = f[2];
                    const float* cc = h_centres + (size_t)c * R * 4u;
                    region = rg::nearest(cc, R, q);
                    kp::P3 kc;
                    kc.x = cc[4 * region]; kc.y = cc[4 * region + 1]; kc.z = cc[4 * region + 2];
                    l = rg::local_of(q, kc);
                    if (want_hist) h_histogram[slot * R + (uint32_t)region] += 1u;
                }
            }
            h_region[px] = (uint8_t)region;
            if (want_local) {
                float* o = h_local + px * 4u;
                o[0] = l.dx; o[1] = l.dy; o[2] = l.dz; o[3] = l.d2;
            }
        }
    }
    return 0;
}
