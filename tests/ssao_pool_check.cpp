// The index arithmetic of the pooled end-of-band drain of k_ssao_tiled (stillleben_amd/csrc/slhip_ssao_pool.h) against a plain
// enumeration: for a count vector (what each of the 4 waves holds of each of the 5 levels, fewer than 64 each), the common list is
// written out entry by entry -- level 5 of waves 0..3, then level 4, ... -- and every position, and some behind the end, must be
// located at that entry.  Then the runs as the kernel deals them out: every entry in exactly one run of one wave, a run's list at
// least every entry's level, only the last run part empty.  Plain C++, no GPU.  (tests/test_ssao_pool_host.py)
#include <cstdio>
#include <cstdint>
#include <vector>

#include "slhip_ssao_pool.h"

using namespace slhip_sp;

struct Entry { unsigned wave, level, slot; };

static unsigned long long g_vectors = 0, g_positions = 0, g_runs = 0, g_mixed = 0, g_failures = 0;
static unsigned long long g_empty_level = 0, g_level_over_64 = 0, g_multiple_of_64 = 0, g_zero = 0;

static void fail(const char* what, const unsigned* counts, unsigned pos)
{
    if (g_failures++ < 10) {
        std::printf("FAIL %s at position %u, counts", what, pos);
        for (unsigned i = 0; i < kSegments; ++i) std::printf(" %u", counts[i]);
        std::printf("\n");
    }
}

// counts[wave * kLevels + (level - 1)]
static void check(const unsigned* counts)
{
    std::vector<Entry> list;
    bool empty_level = false, over = false;
    for (unsigned level = kLevels; level >= 1; --level) {
        unsigned of_level = 0;
        for (unsigned wave = 0; wave < kWaves; ++wave) {
            const unsigned n = counts[wave * kLevels + (level - 1)];
            of_level += n;
            for (unsigned slot = 0; slot < n; ++slot) list.push_back({wave, level, slot});
        }
        empty_level |= of_level == 0;
        over |= of_level > 64;
    }
    const unsigned T = (unsigned)list.size();
    g_vectors += 1;
    g_empty_level += empty_level && T != 0;
    g_level_over_64 += over;
    g_multiple_of_64 += T != 0 && T % 64 == 0;
    g_zero += T == 0;
    if (total(counts) != T) fail("total", counts, T);
    for (unsigned pos = 0; pos < T + 130; ++pos) {
        unsigned level = 99, word = 99;
        const bool found = locate(counts, pos, level, word);
        g_positions += 1;
        if (found != (pos < T)) { fail("valid", counts, pos); continue; }
        if (!found) continue;
        const Entry& e = list[pos];
        // the word of s_q[wave][level - 1][128] as one array
        if (level != e.level || word != ((e.wave * kLevels + (e.level - 1)) * kQueueWords + e.slot)) fail("entry", counts, pos);
    }
    // the runs: wave w takes the runs w, w + 4, ...
    std::vector<unsigned> seen(T, 0);
    for (unsigned wave = 0; wave < kWaves; ++wave)
        for (unsigned first = 64 * wave; first < T; first += 64 * kWaves) {
            unsigned run_list = 0, w0 = 0, lowest = 0, lanes = 0;
            if (!locate(counts, first, run_list, w0)) fail("run start", counts, first);
            for (unsigned lane = 0; lane < 64; ++lane) {
                unsigned level = 0, word = 0;
                if (!locate(counts, first + lane, level, word)) continue;
                seen[first + lane] += 1;
                lanes += 1;
                lowest = level;
                if (level > run_list) fail("run list too short", counts, first + lane);
            }
            g_runs += 1;
            g_mixed += lowest != run_list;
            if (lanes != 64 && first + 64 < T) fail("an inner run is part empty", counts, first);
        }
    for (unsigned pos = 0; pos < T; ++pos)
        if (seen[pos] != 1) fail("not exactly once", counts, pos);
}

int main()
{
    unsigned c[kSegments];
    auto fill = [&](unsigned v) { for (unsigned i = 0; i < kSegments; ++i) c[i] = v; };
    // by hand: nothing at all; everything full; one entry; one level only; an empty level between others
    fill(0); check(c);
    fill(63); check(c);
    fill(0); c[0] = 1; check(c);
    fill(0); c[3 * kLevels + 4] = 1; check(c);
    fill(0); for (unsigned w = 0; w < kWaves; ++w) c[w * kLevels + 2] = 40; check(c);                 // level 3 alone: 160 > 64
    fill(7); for (unsigned w = 0; w < kWaves; ++w) c[w * kLevels + 3] = 0; check(c);                  // level 4 empty
    fill(0); for (unsigned w = 0; w < kWaves; ++w) { c[w * kLevels + 4] = 16; c[w * kLevels] = 32; } check(c);   // T = 192, runs end on level edges
    fill(16); check(c);                                                                             // T = 320 = 5 x 64
    fill(0); c[1 * kLevels + 4] = 63; c[2 * kLevels + 0] = 1; check(c);                               // T = 64: a full run of levels 5 and 1
    // at random (xorshift): sparse and dense vectors, fewer than 64 per queue
    uint32_t x = 2463534242u;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (int it = 0; it < 3000; ++it) {
        const unsigned density = rnd() % 4;
        for (unsigned i = 0; i < kSegments; ++i) {
            const unsigned r = rnd();
            c[i] = density == 0 ? (r % 8 == 0 ? (r >> 8) % 64 : 0) : density == 1 ? (r >> 8) % 8 : (r >> 8) % 64;
        }
        if (it % 5 == 0) for (unsigned w = 0; w < kWaves; ++w) c[w * kLevels + rnd() % kLevels] = 0;
        if (it % 7 == 0) {                                                                          // make T a multiple of 64
            unsigned T = total(c);
            for (unsigned i = 0; i < kSegments && T % 64 != 0; ++i)
                while (c[i] > 0 && T % 64 != 0) { c[i] -= 1; T -= 1; }
        }
        check(c);
    }
    std::printf("vectors %llu positions %llu runs %llu mixed %llu failures %llu\n", g_vectors, g_positions, g_runs, g_mixed, g_failures);
    std::printf("kinds empty_level %llu level_over_64 %llu multiple_of_64 %llu zero %llu\n", g_empty_level, g_level_over_64,
                g_multiple_of_64, g_zero);
    return g_failures ? 1 : 0;
}
