// slhip_vsd_rules.h -- the rules of the pose VSD (slhip_pose_vsd.hip) as plain C++ for host and device alike: the kernels and
// slhip_pose_vsd_host / slhip_pose_depth_host run the same functions, and tests/pose_vsd_ref.py restates them in NumPy.  Every
// float operation is one rounded IEEE operation (the build passes -ffp-contract=off, nothing here fuses); the parenthesisation
// is the contract (include/slhip.h, "Pose VSD").  The coverage is exact integer arithmetic on vertices snapped to 1/256 px,
// through slhip_raster::edge_value of slhip_raster_walk.h.
//
// 32 AND 64 BITS.  pixel_depth<I> evaluates the three edge functions from scratch at a pixel centre of the triangle's pixel box.
// The box starts at ceil((min - 128) / 256) and ends at floor((max - 128) / 256) of the vertices' sub-pixel extent, and clamping
// it only shrinks it, so every such centre lies inside the vertex extent (ex, ey).  slhip_raster_walk.h, "THE NARROW BOUND":
// then each product of edge_value is at most ex ey and |e_i| <= 2 ex ey; with narrow_ok (ex ey <= 2^29, 256 max(ex, ey) <= 2^29)
// that is at most 2^30 < 2^31, so I = int holds the very integers of I = long long, and (float) of an integer rounds the value,
// not the type: b_i, z and the coverage are the same bits in both forms.  Nothing is stepped, so the walk's extra row does not
// enter.  area2 <= ex ey likewise; it is converted once from 64 bits.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_keypoint_rules.h"      // row_point, is_finite, SLHIP_HD
#include "slhip_raster_walk.h"

namespace slhip_vsd {

using slhip_kp::is_finite;
using slhip_kp::row_point;

constexpr uint32_t BLOCK = 256u;
constexpr uint32_t WAVE = 64u;
constexpr uint32_t ABSENT = 0xFFFFFFFFu;      // a plane's value where the pose covers nothing: above the bits of every positive float

SLHIP_HD uint32_t float_bits(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

SLHIP_HD float bits_float(uint32_t u)
{
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}

SLHIP_HD bool pose_finite(const float* M)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && is_finite(M[i]);
    return ok;
}

// a class has a surface when it lies inside the bank and its triangles inside the table
SLHIP_HD bool surface_ok(uint32_t cls, uint32_t n_assets, uint32_t begin, uint32_t count, uint32_t n_triangles)
{
    return cls < n_assets && count >= 1u && (uint64_t)begin + count <= n_triangles;
}

// a screen coordinate in 1/256 px; a NaN gives 0
SLHIP_HD int snap(float c)
{
    float s = floorf(c * 256.0f + 0.5f);
    if (!(s == s)) s = 0.0f;
    s = fminf(fmaxf(s, -67108864.0f), 67108864.0f);
    return (int)s;
}

struct Vertex {
    int X, Y;      // snapped screen position
    float iz;      // 1 / Z
    bool ok;       // not clipped
};

SLHIP_HD Vertex project(const float* M, float x, float y, float z, float fx, float fy, float cx, float cy, float z_near)
{
    const float X = row_point(M, x, y, z), Y = row_point(M + 4, x, y, z), Z = row_point(M + 8, x, y, z);
    Vertex v;
    v.ok = is_finite(X) && is_finite(Y) && is_finite(Z) && Z > z_near;
    v.X = v.Y = 0;
    v.iz = 0.0f;
    if (v.ok) {
        v.X = snap((fx * X) / Z + cx);
        v.Y = snap((fy * Y) / Z + cy);
        v.iz = 1.0f / Z;
    }
    return v;
}

struct Tri {
    int X[3], Y[3];
    float iz[3];
    float fa;                  // (float)|area2|
    int flipped, narrow;
    int x0, x1, y0, y1;        // the pixel box, clamped
};

enum { TRI_OK = 0, TRI_EMPTY = 1, TRI_CLIPPED = 2 };

SLHIP_HD int imin(int a, int b) { return a < b ? a : b; }
SLHIP_HD int imax(int a, int b) { return a > b ? a : b; }

// the triangle of three projected vertices, its pixel box clamped to [wx0, wx1] x [wy0, wy1] (the picture, or a part of it)
SLHIP_HD int setup(const Vertex& a, const Vertex& b, const Vertex& c, int wx0, int wx1, int wy0, int wy1, Tri& t)
{
    if (!(a.ok && b.ok && c.ok)) return TRI_CLIPPED;
    t.X[0] = a.X; t.X[1] = b.X; t.X[2] = c.X;
    t.Y[0] = a.Y; t.Y[1] = b.Y; t.Y[2] = c.Y;
    t.iz[0] = a.iz; t.iz[1] = b.iz; t.iz[2] = c.iz;
    const long long area2 = (long long)(t.X[1] - t.X[0]) * (long long)(t.Y[2] - t.Y[0]) -
                            (long long)(t.Y[1] - t.Y[0]) * (long long)(t.X[2] - t.X[0]);
    if (area2 == 0) return TRI_EMPTY;
    t.flipped = area2 < 0;
    t.fa = (float)(area2 < 0 ? -area2 : area2);
    const int xmn = imin(t.X[0], imin(t.X[1], t.X[2])), xmx = imax(t.X[0], imax(t.X[1], t.X[2]));
    const int ymn = imin(t.Y[0], imin(t.Y[1], t.Y[2])), ymx = imax(t.Y[0], imax(t.Y[1], t.Y[2]));
    t.narrow = slhip_raster::narrow_ok((long long)xmx - xmn, (long long)ymx - ymn) ? 1 : 0;
    t.x0 = imax((xmn - 128 + 255) >> 8, wx0);
    t.x1 = imin((xmx - 128) >> 8, wx1);
    t.y0 = imax((ymn - 128 + 255) >> 8, wy0);
    t.y1 = imin((ymx - 128) >> 8, wy1);
    return (t.x0 > t.x1 || t.y0 > t.y1) ? TRI_EMPTY : TRI_OK;
}

// the bits of the triangle's depth at pixel (px, py) of its box; false: the centre is not covered
template <class I>
SLHIP_HD bool pixel_depth(const Tri& t, int px, int py, uint32_t* bits)
{
    const int cx = 256 * px + 128, cy = 256 * py + 128;
    const I e0 = slhip_raster::edge_value<I>(t.X, t.Y, t.flipped, 0, cx, cy);
    const I e1 = slhip_raster::edge_value<I>(t.X, t.Y, t.flipped, 1, cx, cy);
    const I e2 = slhip_raster::edge_value<I>(t.X, t.Y, t.flipped, 2, cx, cy);
    if ((e0 | e1 | e2) < I(0)) return false;
    const float b0 = (float)e0 / t.fa, b1 = (float)e1 / t.fa, b2 = (float)e2 / t.fa;
    *bits = float_bits(1.0f / ((b0 * t.iz[0] + b1 * t.iz[1]) + b2 * t.iz[2]));
    return true;
}

SLHIP_HD float ray_length(int px, int py, float fx, float fy, float cx, float cy)
{
    const float xn = (((float)px + 0.5f) - cx) / fx, yn = (((float)py + 0.5f) - cy) / fy;
    return sqrtf((xn * xn + yn * yn) + 1.0f);
}

struct Compared {
    bool vg, ve;       // V_g, V_e
    float diff;        // |D_g - D_e|, read only where both are visible
};

SLHIP_HD Compared compare(uint32_t g_bits, uint32_t e_bits, float t, float ray, float delta)
{
    const bool present_g = g_bits != ABSENT, present_e = e_bits != ABSENT;
    const bool absent_t = !(t > 0.0f) || (t - t != 0.0f);
    const float D_g = bits_float(g_bits) * ray, D_e = bits_float(e_bits) * ray, D_t = t * ray;
    Compared c;
    c.vg = present_g && (absent_t || (D_g - D_t) <= delta);
    c.ve = (present_e && (absent_t || (D_e - D_t) <= delta)) || (c.vg && present_e);
    c.diff = fabsf(D_g - D_e);
    return c;
}

SLHIP_HD float threshold(const slhip_pose_vsd_params& p, uint32_t t, float diameter)
{
    return (p.flags & SLHIP_VSD_NORMALIZED) ? p.taus[t] * diameter : p.taus[t];
}

SLHIP_HD float vsd_value(int32_t n_cost, int32_t n_inter, int32_t n_union)
{
    return n_union == 0 ? 1.0f : (float)(n_cost + (n_union - n_inter)) / (float)n_union;
}

}  // namespace slhip_vsd
