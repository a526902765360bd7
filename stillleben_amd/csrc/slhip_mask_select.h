// slhip_mask_select.h -- "the r-th set pixel" of a bit-tile mask, the lookup of the object points (slhip_object_points.hip).
// Plain integer C++ for host and device alike, so that a host program can check it against a dense construction.
//
// TILE ORDER of a mask (layout: slhip_mask_walk.h): the tiles of the box row-major, inside a tile the rising bit index of its
// word -- bit (y & 7) * 8 + (x & 7) is pixel (x, y), so a tile's pixels come row by row.  The RANK of a set pixel is the number
// of set pixels before it in that order.
#pragma once

#include "slhip_mask_walk.h"

namespace slhip_mask {

// index of the k-th set bit of w (k = 0: the lowest), by bisection on popcounts of the lower half.  Needs k < popcount(w).
SLHIP_HD unsigned nth_set_bit(unsigned long long w, unsigned k)
{
    unsigned pos = 0u;
    for (unsigned half = 32u; half; half >>= 1) {
        const unsigned below = (unsigned)__builtin_popcountll((w >> pos) & ((1ull << half) - 1ull));
        if (k >= below) {
            k -= below;
            pos += half;
        }
    }
    return pos;
}

// The pixel of rank `rank` among the tiles [first, last) of the box (tile t is word words[t], row-major over the box), where
// `before` set pixels precede tile `first`.  Returns false when those tiles end before the rank is reached (or the rank lies
// before them); x and y are then left alone.  The caller guarantees [first, last) lies inside the box.
SLHIP_HD bool select_pixel(const unsigned long long* words, const TileBox& b, unsigned long long first, unsigned long long last,
                           unsigned long long before, unsigned long long rank, int* x, int* y)
{
    if (rank < before) return false;
    unsigned long long left = rank - before;
    for (unsigned long long t = first; t < last; ++t) {
        const unsigned long long w = words[t];
        const unsigned n = (unsigned)__builtin_popcountll(w);
        if (left < n) {
            const unsigned bit = nth_set_bit(w, (unsigned)left);
            const unsigned long long tw = (unsigned long long)(b.tx1 - b.tx0 + 1);
            *x = 8 * (b.tx0 + (int)(t % tw)) + (int)(bit & 7u);
            *y = 8 * (b.ty0 + (int)(t / tw)) + (int)(bit >> 3);
            return true;
        }
        left -= n;
    }
    return false;
}

}  // namespace slhip_mask
