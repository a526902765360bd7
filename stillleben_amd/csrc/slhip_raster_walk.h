// slhip_raster_walk.h -- the edge-function arithmetic of the rasterisers (slhip_render.hip): start values, per-texel and
// per-row steps, the biased inside test and the barycentric numerators, as templates over the integer type they are carried
// in.  Plain integer C++ for host and device alike, so that a host program can hold the 32-bit form against the 64-bit one
// (tests/test_raster_walk_host.py instantiates it a third time, over a type that checks every intermediate for its range).
//
// Vertices are snapped to 1/256 px (X, Y); a pixel centre is (256 px + 128, 256 py + 128).  Edge i runs from vertex
// a = (i + 1) % 3 to b = (i + 2) % 3, and its function at a point c is
//     e_i(c) = (X_b - X_a) (c_y - Y_a) - (Y_b - Y_a) (c_x - X_a),          negated for a flipped triangle,
// an exact integer.  One texel to the right adds -256 (Y_b - Y_a), one row down adds 256 (X_b - X_a).
//
// THE NARROW BOUND.  Let ex = max X - min X and ey = max Y - min Y be the sub-pixel extents of the three VERTICES (not of the
// clamped pixel box).  Every pixel centre of the box lies inside the vertex extent: the box starts at ceil((min - 128) / 256)
// and ends at floor((max - 128) / 256), and clamping to the target only shrinks it.  For such a centre
//     |X_b - X_a| <= ex, |c_x - X_a| <= ex, |Y_b - Y_a| <= ey, |c_y - Y_a| <= ey
//     => each product <= ex ey,  |e_i| <= 2 ex ey,  area2 <= ex ey,  |steps| <= 256 max(ex, ey).
// The in-place walk takes one row step past the last row of the box (c_y up to 256 below the extent, |e_i| grows by at most
// 256 ex), and the biased value differs from e_i by at most 1.  With
//     ex ey <= kNarrowMax  and  256 max(ex, ey) <= kNarrowMax,   kNarrowMax = 2^29,
// every value the walk ever holds is at most 2 kNarrowMax + kNarrowMax + 1 = 3 * 2^29 + 1 < 2^31 - 1 in magnitude: no 32-bit
// intermediate overflows, so the 32-bit form holds the very integers of the 64-bit one, and (float) of them is the same float
// (the conversion rounds the value, not the type).  2^29 sub-pixel^2 is a vertex extent of 8192 texels, e.g. 90 x 90.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SLHIP_RW_HD __host__ __device__ __forceinline__
#else
#define SLHIP_RW_HD inline
#endif

namespace slhip_raster {

constexpr long long kNarrowMax = 1ll << 29;

// ex, ey: sub-pixel extents of the three vertices (>= 0).  Evaluated in 64 bits: the extents of a clipped-away giant do not fit
// the narrow form -- that is what is being decided.
SLHIP_RW_HD bool narrow_ok(long long ex, long long ey)
{
    const long long m = ex > ey ? ex : ey;
    return 256 * m <= kNarrowMax && ex * ey <= kNarrowMax;
}

// e_i at the sub-pixel point (cx, cy), without the bias.  I = long long: 32 x 32 -> 64-bit products, always exact.
// I = int: exact for a triangle that passes narrow_ok() and a point inside its vertex extent.
template <class I>
SLHIP_RW_HD I edge_value(const int* X, const int* Y, int flipped, int i, int cx, int cy)
{
    const int a = (i + 1) % 3, b = (i + 2) % 3;
    const I e = I(X[b] - X[a]) * I(cy - Y[a]) - I(Y[b] - Y[a]) * I(cx - X[a]);
    return flipped ? -e : e;
}

// the three biased edge values of one texel, stepped over a pixel box
template <class I>
struct Walk {
    I e[3];     // biased values at the current texel: covered iff all three are >= 0
    I row[3];   // ... at the first texel of the current row
    I sx[3];    // one texel to the right
    I sy[3];    // one row down
    int bias[3];

    // at texel (px, py); bias[i] is 0 for an owned edge, -1 otherwise
    SLHIP_RW_HD void start(const int* X, const int* Y, int flipped, const int* bias_, int px, int py)
    {
        const int cx = 256 * px + 128, cy = 256 * py + 128;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int a = (i + 1) % 3, b = (i + 2) % 3;
            const I dx = I(-256) * I(Y[b] - Y[a]), dy = I(256) * I(X[b] - X[a]);
            sx[i] = flipped ? -dx : dx;
            sy[i] = flipped ? -dy : dy;
            bias[i] = bias_[i];
            row[i] = edge_value<I>(X, Y, flipped, i, cx, cy) + I(bias_[i]);
            e[i] = row[i];
        }
    }
    SLHIP_RW_HD void step_x()
    {
        e[0] += sx[0]; e[1] += sx[1]; e[2] += sx[2];
    }
    SLHIP_RW_HD void next_row()
    {
        row[0] += sy[0]; row[1] += sy[1]; row[2] += sy[2];
        e[0] = row[0]; e[1] = row[1]; e[2] = row[2];
    }
    // n rows down in the same column (n >= 0): the strided walk of a pass in which every lane owns one texel of every n-th row
    // (k_vis_fill).  Carried in I = long long there: e_i is at most 2^55 in magnitude for vertices that snap() bounds by 2^26
    // and a pixel centre below 2^24, and a step of up to 2^16 rows at most 2^51.
    SLHIP_RW_HD void rows_down(int n)
    {
        row[0] += I(n) * sy[0]; row[1] += I(n) * sy[1]; row[2] += I(n) * sy[2];
        e[0] = row[0]; e[1] = row[1]; e[2] = row[2];
    }
    // all three biased values >= 0, i.e. the sign bit of their OR is clear
    SLHIP_RW_HD bool inside() const { return (e[0] | e[1] | e[2]) >= I(0); }
    // e_i of the current texel: the numerator of barycentric i over area2
    SLHIP_RW_HD I numerator(int i) const { return e[i] - I(bias[i]); }
};

// coverage from scratch at one texel: the inside test and the three numerators
template <class I>
SLHIP_RW_HD bool cover(const int* X, const int* Y, int flipped, const int* bias, int px, int py, I* num)
{
    const int cx = 256 * px + 128, cy = 256 * py + 128;
    bool in = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const I e = edge_value<I>(X, Y, flipped, i, cx, cy);
        in = in && (e + I(bias[i]) >= I(0));
        num[i] = e;
    }
    return in;
}

}  // namespace slhip_raster
