// Host check of stillleben_amd/csrc/slhip_tile_queue.h (compiled and run by tests/test_tile_queue_host.py).
//
// Queues are filled the way raster_or_enqueue() fills them (reservation() added to a 64-bit counter, slot_of() of the value before)
// or laid out by hand (gaps between entries), then consumed the way k_large, k_shadow_large and k_os_large consume them: every one of
// n_ranges waves takes Walk::first(), walks its entries and counts the tiles of each box by a column / row counter.  Checked:
// every triangle is either walked in place by its producer or has every tile of its box visited exactly once, over all ranges
// together; no tile outside a box is visited; no entry beyond the capacity is read.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "slhip_tile_queue.h"

using namespace slhip_tq;

struct Tri {             // one producer
    unsigned ntx, nty;
    bool in_place;       // what the producer decided
    long entry;          // index of its entry, -1: none
};

struct Queue {
    unsigned long long counter = 0;   // header words 0, 1
    unsigned carried = 0;             // header word 2
    unsigned capacity = 0;            // 16-byte units
    std::vector<Entry> entries;       // entry_capacity(capacity) of them, poisoned where unwritten
    std::vector<Tri> tris;
};

static const unsigned kPoison = 0xDEADBEEFu;

static Queue make_queue(unsigned capacity, unsigned long long counter0 = 0)
{
    Queue q;
    q.capacity = capacity;
    q.counter = counter0;
    Entry p;
    p.draw = p.tri_sub = p.scene_aux = p.tile_base = p.t0 = p.nt = kPoison;
    p.spare[0] = p.spare[1] = kPoison;
    q.entries.assign(entry_capacity(capacity), p);
    return q;
}

// raster_or_enqueue(): one atomic, one entry
static void produce(Queue& q, unsigned tx0, unsigned ty0, unsigned ntx_, unsigned nty_)
{
    const unsigned n = ntx_ * nty_;
    const unsigned long long before = q.counter;
    q.counter += reservation(n);
    const Slot s = slot_of(before, n, q.capacity);
    Tri t;
    t.ntx = ntx_; t.nty = nty_; t.entry = -1;
    if (s.carried) q.carried |= 1u;
    if (s.fits) {
        Entry& e = q.entries[s.index];
        e.draw = (unsigned)q.tris.size(); e.tri_sub = 0; e.scene_aux = 0; e.tile_base = s.tile_base;
        e.t0 = tx0 | (ty0 << 16);
        e.nt = s.carried ? 0u : (ntx_ | (nty_ << 16));
        t.entry = (long)s.index;
    }
    t.in_place = !s.fits || s.carried;
    q.tris.push_back(t);
}

// a reserved range with no entry behind it, anywhere in the queue (laid out by hand: the tile counter moves, the entry counter
// does not)
static void reserve_gap(Queue& q, unsigned n) { q.counter += (unsigned long long)n << 32; }

struct Totals {
    long long lists = 0, walks = 0, tiles = 0, visited = 0, in_place = 0, failures = 0;
    long long start_boundary = 0, start_midrow = 0, start_gap = 0, carried_lists = 0, clipped_lists = 0, empty_lists = 0;
};

static void fail(Totals& T, const char* what, unsigned n_ranges, unsigned r)
{
    if (T.failures < 20) std::printf("FAIL %s (list %lld, %u ranges, range %u)\n", what, T.lists, n_ranges, r);
    ++T.failures;
}

static void consume(const Queue& q, Totals& T)
{
    ++T.lists;
    const unsigned entries = (unsigned)q.counter, tiles = (unsigned)(q.counter >> 32);
    if (q.carried) ++T.carried_lists;
    if (entries > entry_capacity(q.capacity)) ++T.clipped_lists;
    if (entries == 0) ++T.empty_lists;
    static const unsigned kRanges[] = {1, 2, 3, 7, 64, 8192};
    for (unsigned n_ranges : kRanges) {
        ++T.walks;
        std::vector<std::vector<unsigned char>> seen(q.tris.size());
        for (size_t i = 0; i < q.tris.size(); ++i) seen[i].assign((size_t)q.tris[i].ntx * q.tris[i].nty, 0);
        const Plan p = plan_of(entries, tiles, q.carried, q.capacity);
        if (p.count > q.entries.size()) fail(T, "plan reads beyond the capacity", n_ranges, 0);
        unsigned prev_end = 0;
        for (unsigned r = 0; r < n_ranges; ++r) {
            Walk w;
            w.first(p, q.entries.data(), n_ranges, r);
            // the ranges tile [0, total) in order
            const unsigned a = p.by_entries ? w.e0 : w.t0, b = p.by_entries ? w.e1 : w.t1;
            if (a != prev_end || b < a || b > p.total) fail(T, "ranges do not follow each other", n_ranges, r);
            prev_end = b;
            if (r == n_ranges - 1 && b != p.total) fail(T, "ranges do not reach the total", n_ranges, r);
            if (!p.by_entries && a < b) {       // where does the range begin?
                bool inside = false;
                for (unsigned e = 0; e < p.count; ++e) {
                    const Entry& en = q.entries[e];
                    if (a == en.tile_base) { ++T.start_boundary; inside = true; break; }
                    if (a > en.tile_base && a - en.tile_base < n_tiles(en)) {
                        if ((a - en.tile_base) % ntx(en) != 0) ++T.start_midrow;
                        inside = true;
                        break;
                    }
                }
                if (!inside) ++T.start_gap;
            }
            for (unsigned e = w.e0; e < w.e1; ++e) {
                if (e >= p.count) { fail(T, "entry index beyond the count", n_ranges, r); break; }
                const Entry& en = q.entries[e];
                if (en.draw == kPoison) { fail(T, "unwritten entry read", n_ranges, r); break; }
                if (w.done(en)) break;
                unsigned k0, k1;
                if (!w.tiles(en, k0, k1)) continue;
                const Tri& t = q.tris[en.draw];
                if (t.in_place) { fail(T, "tiles of a triangle that was walked in place", n_ranges, r); continue; }
                // TilePixels of slhip_render.hip: one division, then a counter
                const unsigned nx = ntx(en);
                unsigned ty = k0 / nx, tx = k0 - ty * nx;
                for (unsigned k = k0; k < k1; ++k) {
                    if (tx >= t.ntx || ty >= t.nty) { fail(T, "tile outside the box", n_ranges, r); break; }
                    if (++seen[en.draw][(size_t)ty * t.ntx + tx] != 1) fail(T, "tile visited twice", n_ranges, r);
                    ++T.visited;
                    if (++tx == nx) { tx = 0; ++ty; }
                }
            }
        }
        for (size_t i = 0; i < q.tris.size(); ++i) {
            const Tri& t = q.tris[i];
            long long n = 0;
            for (unsigned char c : seen[i]) n += c;
            T.tiles += (long long)seen[i].size();
            if (t.in_place) {
                ++T.in_place;
                if (n != 0) fail(T, "in-place triangle visited", n_ranges, 0);
            } else if (n != (long long)seen[i].size()) {
                fail(T, "tiles of a queued triangle missed", n_ranges, 0);
            }
        }
    }
}

int main()
{
    Totals T;
    std::mt19937 rng(20261019u);
    auto rnd = [&](unsigned lo, unsigned hi) { return lo + (unsigned)(rng() % (hi - lo + 1)); };
    const unsigned kBig = 1u << 20;

    // the empty queue, with and without room
    for (unsigned cap : {0u, 1u, 2u, kBig}) { Queue q = make_queue(cap); consume(q, T); }

    // every box shape on its own and all of them together, in several orders
    const unsigned shapes[][2] = {{1, 1}, {1, 37}, {41, 1}, {80, 60}, {256, 256}, {3, 5}, {8, 8}};
    for (auto& s : shapes) { Queue q = make_queue(kBig); produce(q, 2, 3, s[0], s[1]); consume(q, T); }
    for (int rep = 0; rep < 4; ++rep) {
        Queue q = make_queue(kBig);
        for (int i = 0; i < 7; ++i) { auto& s = shapes[(i * (rep + 1) + rep) % 7]; produce(q, rnd(0, 9), rnd(0, 9), s[0], s[1]); }
        consume(q, T);
    }
    // many small boxes: ranges that hold several entries, ranges that begin on an entry's first tile
    for (int rep = 0; rep < 6; ++rep) {
        Queue q = make_queue(kBig);
        const unsigned n = rnd(1, 400);
        for (unsigned i = 0; i < n; ++i) produce(q, rnd(0, 100), rnd(0, 100), rnd(1, 9), rnd(1, 7));
        consume(q, T);
    }
    // 64 boxes of 8 x 8 tiles: 4096 tiles, so 64 ranges begin on an entry each and 8192 ranges mid-row
    { Queue q = make_queue(kBig); for (int i = 0; i < 64; ++i) produce(q, 0, 0, 8, 8); consume(q, T); }

    // gaps without an entry, before, between and behind the entries; ranges that begin inside them
    for (int rep = 0; rep < 8; ++rep) {
        Queue q = make_queue(kBig);
        if (rep & 1) reserve_gap(q, rnd(1, 5000));
        const unsigned n = rnd(1, 40);
        for (unsigned i = 0; i < n; ++i) {
            produce(q, rnd(0, 50), rnd(0, 50), rnd(1, 30), rnd(1, 30));
            if (rng() % 3 == 0) reserve_gap(q, rnd(1, 3000));
        }
        if (rep & 2) reserve_gap(q, 70000);
        consume(q, T);
    }
    { Queue q = make_queue(kBig); reserve_gap(q, 12345); consume(q, T); }      // nothing but a gap

    // a count clipped by the capacity: the triangles beyond it walk in place, their tiles stay reserved
    for (unsigned cap : {0u, 1u, 2u, 3u, 4u, 9u, 20u, 21u}) {
        Queue q = make_queue(cap);
        for (int i = 0; i < 12; ++i) produce(q, 1, 1, rnd(1, 90), rnd(1, 70));
        consume(q, T);
    }

    // the tile counter at its end: the carrying producer walks in place and leaves a void entry, the ones after it see a wrapped
    // counter; the consumers split by entries
    for (int rep = 0; rep < 4; ++rep) {
        const unsigned cap = rep == 3 ? 8u : kBig;
        Queue q = make_queue(cap, (unsigned long long)(0xFFFFFFFFu - 4000u - 100u * (unsigned)rep) << 32);
        produce(q, 0, 0, 50, 60);                       // 3000 tiles: fits below 2^32
        produce(q, 0, 0, rep == 1 ? 901 : 40, rep == 1 ? 1 : 40);   // 1600 tiles: carries; rep 1: 901 tiles still fit ...
        produce(q, 4, 4, 80, 60);                       // ... and this one carries (otherwise it follows the carry)
        for (int i = 0; i < 5; ++i) produce(q, rnd(0, 9), rnd(0, 9), rnd(1, 20), rnd(1, 20));
        if (!q.carried) { std::printf("FAIL the counter did not carry (list %lld)\n", T.lists); ++T.failures; }
        consume(q, T);
    }
    // exactly at the end: tile_base + n == 2^32 carries (the end of a range must fit 32 bits), one tile less does not
    {
        const Slot a = slot_of((unsigned long long)(0xFFFFFFFFu - 9u) << 32, 10u, kBig);
        const Slot b = slot_of((unsigned long long)(0xFFFFFFFFu - 9u) << 32, 9u, kBig);
        if (!a.carried || b.carried) { std::printf("FAIL carry at the boundary\n"); ++T.failures; }
    }

    // range_of with a total near 2^32 and many ranges: contiguous, no 32-bit overflow
    {
        unsigned prev = 0;
        for (unsigned r = 0; r < 8192; ++r) {
            unsigned a, b;
            range_of(0xFFFFFFF0u, 8192, r, a, b);
            if (a != prev || b < a) { std::printf("FAIL range_of near 2^32\n"); ++T.failures; break; }
            prev = b;
        }
        if (prev != 0xFFFFFFF0u) { std::printf("FAIL range_of does not reach the total\n"); ++T.failures; }
    }

    std::printf("lists %lld walks %lld tiles %lld visited %lld in_place %lld failures %lld\n", T.lists, T.walks, T.tiles, T.visited,
                T.in_place, T.failures);
    std::printf("starts boundary %lld midrow %lld gap %lld\n", T.start_boundary, T.start_midrow, T.start_gap);
    std::printf("kinds carried %lld clipped %lld empty %lld\n", T.carried_lists, T.clipped_lists, T.empty_lists);
    return T.failures == 0 ? 0 : 1;
}
