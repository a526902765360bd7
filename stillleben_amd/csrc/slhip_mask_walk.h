// slhip_mask_walk.h -- the walk over one image column of a bit-tile mask that slhip_render_object_masks counts and emits
// COCO run lengths with (slhip_render_masks.inc).  Plain integer C++ for host and device alike, so that a host program can
// check it against a dense construction.
//
// A mask is a row-major box of 8 x 8 tiles [tx0..tx1] x [ty0..ty1], one u64 word per tile, bit (y & 7) * 8 + (x & 7) = pixel
// (x, y); everything outside the box is zero.  COCO's order is column-major: pixel (x, y) has position x * H + y, and a run goes
// on from (x, H - 1) to (x + 1, 0).  A BOUNDARY is a position whose pixel differs from the one before it (position 0: from 0);
// a mask with n boundaries b_0 < ... < b_{n-1} has the n + 1 run lengths b_0, b_1 - b_0, ..., W * H - b_{n-1}.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SLHIP_HD __host__ __device__ __forceinline__
#else
#define SLHIP_HD inline
#endif

namespace slhip_mask {

struct TileBox {
    int tx0, ty0, tx1, ty1;   // tx0 > tx1: no tiles
};

// rows 8 * ty .. 8 * ty + 7 of image column x as bits 0..7; rows >= H and tiles outside the box read as zero
SLHIP_HD unsigned column_bits(const unsigned long long* words, const TileBox& b, int x, int ty, int H)
{
    const int tx = x >> 3;
    if (tx < b.tx0 || tx > b.tx1 || ty < b.ty0 || ty > b.ty1) return 0u;
    const unsigned long long w = words[(size_t)(ty - b.ty0) * (size_t)(b.tx1 - b.tx0 + 1) + (size_t)(tx - b.tx0)];
    // bit 8 * r of (w >> (x & 7)) is row r of the column; the multiplication gathers the eight of them in the top byte
    // (term r lands on bit 56 + r, the exponents 8 r - 7 r' of all 64 products are distinct: no carries)
    unsigned c = (unsigned)((((w >> (x & 7)) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56);
    const int rows = H - 8 * ty;
    if (rows < 8) c &= (1u << rows) - 1u;
    return c;
}

// pixel (x, H - 1): what column x hands on to column x + 1 (0 for x < 0)
SLHIP_HD unsigned column_last_bit(const unsigned long long* words, const TileBox& b, int x, int H)
{
    if (x < 0) return 0u;
    return (column_bits(words, b, x, (H - 1) >> 3, H) >> ((H - 1) & 7)) & 1u;
}

// Calls f(position) for every boundary of image column x (0 <= x < W) in rising order and returns their number.
template <class F>
SLHIP_HD unsigned walk_column(const unsigned long long* words, const TileBox& b, int x, int H, F&& f)
{
    const unsigned base = (unsigned)x * (unsigned)H;
    unsigned prev = column_last_bit(words, b, x - 1, H);
    unsigned n = 0u;
    const int tx = x >> 3;
    if (tx < b.tx0 || tx > b.tx1) {   // a column of zeros: at most the end of a run that came down the column before
        if (prev) { f(base); n = 1u; }
        return n;
    }
    if (b.ty0 > 0 && prev) { f(base); n = 1u; prev = 0u; }   // row 0 is above the box
    for (int ty = b.ty0; ty <= b.ty1; ++ty) {
        const unsigned c = column_bits(words, b, x, ty, H);
        const int rows = H - 8 * ty < 8 ? H - 8 * ty : 8;
        unsigned d = (c ^ ((c << 1) | prev)) & ((1u << rows) - 1u);
        n += (unsigned)__builtin_popcount(d);
        while (d) {
            f(base + (unsigned)(8 * ty + __builtin_ctz(d)));
            d &= d - 1u;
        }
        prev = (c >> (rows - 1)) & 1u;
    }
    const int below = 8 * (b.ty1 + 1);
    if (below < H && prev) { f(base + (unsigned)below); ++n; }   // the box ends above the image's last row
    return n;
}

}  // namespace slhip_mask
