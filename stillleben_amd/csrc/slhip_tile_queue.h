// slhip_tile_queue.h -- the large-triangle queue of the rasterisers (slhip_render.hip, slhip_render_stats.inc): its layout and the
// index arithmetic of producer and consumers.  Plain integer C++ for host and device alike, like slhip_raster_walk.h, so that a
// host program can enumerate what the kernels enumerate (tests/test_tile_queue_host.py).
//
// A triangle whose pixel box is too large for its own thread is queued as ONE entry; the 8 x 8-pixel tiles of the box are a
// function of the entry and a counter, so the consumer enumerates them instead of reading one record per tile.
//
// LAYOUT.  A 16-byte header, then `capacity` 16-byte units (what slhip_render_scratch_bytes sizes); an entry takes two units.
//   header words 0, 1: ONE 64-bit counter, entries in its low word and tiles in its high word.  A producer adds
//                      1 | n_tiles << 32 with one atomic and so learns its entry index and the first tile of its range; as one
//                      atomic hands out both, the entries are ordered by tile_base.
//   header word 2:     set once a tile reservation carried out of 32 bits (below).
//   header word 3:     not the queue's: a flag word of the pass that owns the queue, zeroed with the header.  The visibility pass
//                      raises kFlagDiscardChunks in it when k_raster<false> meets a chunk of the discard-testing instantiation,
//                      and every block of k_raster<true> leaves at once while it is zero.  plan_of() never sees it.
// A triangle whose entry index is beyond the capacity is walked in place by its producer; its tile range stays reserved with no
// entry behind it (such ranges are the last of the queue).  A triangle whose range would carry out of 32 bits is walked in place
// as well and leaves a void entry (no tiles); it raises header word 2, because the tile counter has wrapped for every producer
// after it: tile_base then no longer orders the entries, and the consumers split the queue by entries instead of by tiles.
// (The entry counter is assumed not to wrap: fewer than 2^32 queued triangles per pass.)
//
// CONSUMERS.  Every wave takes an even share [t0, t1) of the tile total, finds the entry that holds t0 by binary search and walks
// entry by entry: of each it visits the tiles [max(t0, tile_base), min(t1, tile_base + n)) - tile_base, row-major over the box.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SLHIP_TQ_HD __host__ __device__ __forceinline__
#else
#define SLHIP_TQ_HD inline
#endif

namespace slhip_tq {

constexpr unsigned kHeaderWords = 4;      // 16 bytes
constexpr unsigned kUnitsPerEntry = 2;    // 32 bytes
constexpr unsigned kFlagWord = 3;         // header word 3 (above)
constexpr unsigned kFlagDiscardChunks = 1u;

struct Entry {
    unsigned draw;       // global draw index
    unsigned tri_sub;    // triangle | sub-triangle << 31
    unsigned scene_aux;  // scene | light << 24
    unsigned tile_base;  // first tile of the entry in the queue's tile numbering
    unsigned t0;         // tx0 | ty0 << 16: first 8 x 8 tile of the pixel box
    unsigned nt;         // ntx | nty << 16: tiles per row, tile rows (both < 2^16; 0: a void entry)
    unsigned spare[2];
};
static_assert(sizeof(Entry) == 16 * kUnitsPerEntry, "an entry is two 16-byte units");

SLHIP_TQ_HD unsigned entry_capacity(unsigned capacity_units) { return capacity_units / kUnitsPerEntry; }
SLHIP_TQ_HD unsigned ntx(const Entry& e) { return e.nt & 0xFFFFu; }
SLHIP_TQ_HD unsigned nty(const Entry& e) { return e.nt >> 16; }
SLHIP_TQ_HD unsigned n_tiles(const Entry& e) { return ntx(e) * nty(e); }

// what a producer adds to the 64-bit counter
SLHIP_TQ_HD unsigned long long reservation(unsigned n) { return 1ull | ((unsigned long long)n << 32); }

// What the counter's previous value means for the producer of n tiles.
struct Slot {
    unsigned index;      // entry index
    unsigned tile_base;
    bool fits;           // index < entry capacity: the entry is to be written (void if `carried`)
    bool carried;        // tile_base + n does not fit 32 bits: walk in place, raise header word 2
};
SLHIP_TQ_HD Slot slot_of(unsigned long long before, unsigned n, unsigned capacity_units)
{
    Slot s;
    s.index = (unsigned)before;
    s.tile_base = (unsigned)(before >> 32);
    s.fits = s.index < entry_capacity(capacity_units);
    s.carried = (unsigned long long)s.tile_base + n > 0xFFFFFFFFull;
    return s;
}

// What a consumer makes of the header: the entries it may read and how its `n_ranges` waves split the work.
struct Plan {
    unsigned count;      // entries behind the header (clamped by the capacity)
    unsigned total;      // what is split: tiles, or entries once a reservation carried
    bool by_entries;
};
SLHIP_TQ_HD Plan plan_of(unsigned entries, unsigned tiles, unsigned carried, unsigned capacity_units)
{
    Plan p;
    const unsigned cap = entry_capacity(capacity_units);
    p.count = entries < cap ? entries : cap;
    p.by_entries = carried != 0u;
    p.total = p.by_entries ? p.count : tiles;
    if (p.count == 0u) p.total = 0u;
    return p;
}

// range r of n_ranges over [0, total): contiguous, even (the last ones may be empty)
SLHIP_TQ_HD void range_of(unsigned total, unsigned n_ranges, unsigned r, unsigned& t0, unsigned& t1)
{
    const unsigned long long per = ((unsigned long long)total + n_ranges - 1) / n_ranges;
    const unsigned long long a = per * r, b = a + per;
    t0 = (unsigned)(a < total ? a : total);
    t1 = (unsigned)(b < total ? b : total);
}

// the last entry of [0, count) whose tile_base is <= t (0 if there is none); count >= 1, entries ordered by tile_base
SLHIP_TQ_HD unsigned find_entry(const Entry* entries, unsigned count, unsigned t)
{
    unsigned lo = 0, hi = count;         // invariant: the answer is in [lo, hi)
    while (hi - lo > 1u) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (entries[mid].tile_base <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// The walk of one range: first(), then for every entry e in [e0, e1): tiles(e, k0, k1) gives the tile indices [k0, k1) of the
// entry's box that belong to the range (k = ty * ntx + tx, box-relative); done(e) tells that no later entry has any.
struct Walk {
    unsigned t0, t1;     // the range (tiles; everything when split by entries)
    unsigned e0, e1;     // entries to look at
    bool by_entries;

    SLHIP_TQ_HD void first(const Plan& p, const Entry* entries, unsigned n_ranges, unsigned r)
    {
        by_entries = p.by_entries;
        unsigned a, b;
        range_of(p.total, n_ranges, r, a, b);
        if (by_entries) {
            e0 = a; e1 = b; t0 = 0u; t1 = 0xFFFFFFFFu;
        } else {
            t0 = a; t1 = b; e1 = p.count;
            e0 = a < b ? find_entry(entries, p.count, a) : p.count;
        }
    }
    SLHIP_TQ_HD bool done(const Entry& e) const { return !by_entries && e.tile_base >= t1; }
    SLHIP_TQ_HD bool tiles(const Entry& e, unsigned& k0, unsigned& k1) const
    {
        const unsigned n = n_tiles(e);
        if (by_entries) { k0 = 0u; k1 = n; return n != 0u; }
        const unsigned base = e.tile_base, end = base + n;      // no carry: a carrying producer leaves a void entry
        const unsigned lo = t0 > base ? t0 : base, hi = t1 < end ? t1 : end;
        if (lo >= hi) return false;
        k0 = lo - base; k1 = hi - base;
        return true;
    }
};

}  // namespace slhip_tq
