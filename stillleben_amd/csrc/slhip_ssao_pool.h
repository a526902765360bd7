// slhip_ssao_pool.h -- the pooled end-of-band drain of k_ssao_tiled (slhip_render.hip): where a position of the block's common
// list lies.  Plain integer C++ for host and device alike, like slhip_tile_queue.h, so that a host program can enumerate what the
// kernel enumerates (tests/test_ssao_pool_host.py).
//
// At the end of a band each of the block's kWaves waves holds, per level 1 .. kLevels, fewer than 64 queued pixels.  They stay
// where they are, in the wave's own queues; the block's COMMON LIST is their concatenation, the highest level first and within a
// level wave 0 .. kWaves - 1:
//     segment s = (kLevels - level) * kWaves + wave,      length counts[wave * kLevels + (level - 1)].
// Run r covers the positions [64 r, 64 r + 64) and runs the tap list of the level of its first entry: as the levels only fall
// along the list, no pixel of the run needs a longer one.
#pragma once

#if defined(__HIPCC__)
#define SLHIP_SP_HD __host__ __device__ __forceinline__
#else
#define SLHIP_SP_HD inline
#endif

namespace slhip_sp {

constexpr unsigned kWaves = 4;                      // waves of a block of k_ssao_tiled
constexpr unsigned kLevels = 5;                     // levels with taps: 1 .. 5 (level 0 runs nothing and is never queued)
constexpr unsigned kSegments = kWaves * kLevels;
constexpr unsigned kQueueWords = 128;               // words of one wave's queue of one level

SLHIP_SP_HD unsigned segment_wave(unsigned s) { return s % kWaves; }
SLHIP_SP_HD unsigned segment_level(unsigned s) { return kLevels - s / kWaves; }
// index into counts[] (as the waves publish them: wave-major) and word offset of the segment's queue in s_q[wave][level - 1][128]
SLHIP_SP_HD unsigned segment_count_index(unsigned s) { return segment_wave(s) * kLevels + (segment_level(s) - 1u); }
SLHIP_SP_HD unsigned segment_queue_offset(unsigned s) { return segment_count_index(s) * kQueueWords; }

SLHIP_SP_HD unsigned total(const unsigned* counts)
{
    unsigned t = 0;
    for (unsigned s = 0; s < kSegments; ++s) t += counts[s];
    return t;
}

// Position `pos` of the common list: false when it lies behind the list's end, otherwise its level and the word of s_q (all waves'
// queues as one array) that holds its pixel.  A walk over the segment lengths; in the kernel they are uniform values.
SLHIP_SP_HD bool locate(const unsigned* counts, unsigned pos, unsigned& level, unsigned& word)
{
    bool found = false;
    level = 0;
    word = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (unsigned s = 0; s < kSegments; ++s) {
        const unsigned len = counts[segment_count_index(s)];
        if (!found && pos < len) {
            found = true;
            level = segment_level(s);
            word = segment_queue_offset(s) + pos;
        }
        pos -= len;          // (wraps once found or behind the end: not looked at again)
    }
    return found;
}

}  // namespace slhip_sp
