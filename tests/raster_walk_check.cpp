// Host check of stillleben_amd/csrc/slhip_raster_walk.h (compiled and run by tests/test_raster_walk_host.py).
//
// For every texel of a triangle's pixel box -- and the one row step the in-place walk takes past it -- the 32-bit form of the
// edge walk is held against the 64-bit one: start values, steps, biased inside test, numerators, and (float) of both.  The
// walk is instantiated a third time over Checked32, a 64-bit integer that records every intermediate leaving the int32 range,
// so an overflow is found by arithmetic, not by a sanitizer.  The triangle set-up (signed area, ownership, pixel box, clamp)
// restates setup_finish() of slhip_render.hip.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>

#include "slhip_raster_walk.h"

static long long g_out_of_range = 0;   // intermediates of Checked32 outside the int32 range

struct Checked32 {
    long long v;
    Checked32() : v(0) {}
    explicit Checked32(int x) : v(x) {}
    static Checked32 make(long long x)
    {
        if (x < (long long)INT32_MIN || x > (long long)INT32_MAX) ++g_out_of_range;
        Checked32 r;
        r.v = x;
        return r;
    }
    Checked32 operator*(const Checked32& o) const { return make(v * o.v); }
    Checked32 operator+(const Checked32& o) const { return make(v + o.v); }
    Checked32 operator-(const Checked32& o) const { return make(v - o.v); }
    Checked32 operator-() const { return make(-v); }
    Checked32 operator|(const Checked32& o) const { return make(v | o.v); }
    Checked32& operator+=(const Checked32& o) { *this = make(v + o.v); return *this; }
    bool operator>=(const Checked32& o) const { return v >= o.v; }
    explicit operator float() const { return (float)(int)v; }
};

struct Tri {
    int X[3], Y[3];
    int flipped, bias[3];
    long long area2;
    int xmin, xmax, ymin, ymax;
    bool narrow;
};

// setup_finish(): false if degenerate or outside the W x H target
static bool setup(Tri& t, int W, int H)
{
    long long area2 = (long long)(t.X[1] - t.X[0]) * (long long)(t.Y[2] - t.Y[0]) -
                      (long long)(t.Y[1] - t.Y[0]) * (long long)(t.X[2] - t.X[0]);
    if (area2 == 0) return false;
    t.flipped = area2 < 0;
    t.area2 = area2 < 0 ? -area2 : area2;
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        int dx = t.X[b] - t.X[a], dy = t.Y[b] - t.Y[a];
        if (t.flipped) { dx = -dx; dy = -dy; }
        const bool owned = (dy < 0) || (dy == 0 && dx < 0);
        t.bias[i] = owned ? 0 : -1;
    }
    const int xmn = std::min(t.X[0], std::min(t.X[1], t.X[2])), xmx = std::max(t.X[0], std::max(t.X[1], t.X[2]));
    const int ymn = std::min(t.Y[0], std::min(t.Y[1], t.Y[2])), ymx = std::max(t.Y[0], std::max(t.Y[1], t.Y[2]));
    t.narrow = slhip_raster::narrow_ok((long long)xmx - xmn, (long long)ymx - ymn);
    int x0 = (xmn - 128 + 255) >> 8, x1 = (xmx - 128) >> 8;
    int y0 = (ymn - 128 + 255) >> 8, y1 = (ymx - 128) >> 8;
    x0 = std::max(x0, 0); y0 = std::max(y0, 0);
    x1 = std::min(x1, W - 1); y1 = std::min(y1, H - 1);
    if (x0 > x1 || y0 > y1) return false;
    t.xmin = x0; t.xmax = x1; t.ymin = y0; t.ymax = y1;
    return true;
}

static bool same_float(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static long long g_texels = 0, g_covered = 0, g_failures = 0;

static void fail(const char* what, const Tri& t, int px, int py)
{
    if (++g_failures <= 10)
        std::printf("FAIL %s: X %d %d %d Y %d %d %d texel %d %d\n", what, t.X[0], t.X[1], t.X[2], t.Y[0], t.Y[1], t.Y[2], px, py);
}

// the whole box, as raster_bbox_as() walks it, in the three forms side by side
static void walk_box(const Tri& t, bool with_narrow)
{
    slhip_raster::Walk<long long> w64;
    slhip_raster::Walk<int> w32;
    slhip_raster::Walk<Checked32> wck;
    w64.start(t.X, t.Y, t.flipped, t.bias, t.xmin, t.ymin);
    if (with_narrow) {
        w32.start(t.X, t.Y, t.flipped, t.bias, t.xmin, t.ymin);
        wck.start(t.X, t.Y, t.flipped, t.bias, t.xmin, t.ymin);
        for (int i = 0; i < 3; ++i)
            if (w32.sx[i] != w64.sx[i] || w32.sy[i] != w64.sy[i] || wck.sx[i].v != w64.sx[i] || wck.sy[i].v != w64.sy[i])
                fail("steps", t, t.xmin, t.ymin);
    }
    const float fa64 = (float)t.area2, fa32 = (float)(int)t.area2;
    if (with_narrow && (t.area2 > INT32_MAX || !same_float(fa64, fa32))) fail("area2", t, t.xmin, t.ymin);
    const int bw = t.xmax - t.xmin + 1, n = bw * (t.ymax - t.ymin + 1);
    int px = t.xmin, py = t.ymin;
    for (int k = 0; k <= n; ++k) {      // k == n: the values after the row step past the last row (held, never used)
        // from scratch, 64-bit: what coverage() computes
        long long num[3];
        const bool in = slhip_raster::cover<long long>(t.X, t.Y, t.flipped, t.bias, px, py, num);
        for (int i = 0; i < 3; ++i)
            if (w64.e[i] != num[i] + t.bias[i] || w64.numerator(i) != num[i]) fail("walk64 vs scratch", t, px, py);
        if (k < n && w64.inside() != in) fail("inside64", t, px, py);
        if (with_narrow) {
            for (int i = 0; i < 3; ++i) {
                if ((long long)w32.e[i] != w64.e[i] || wck.e[i].v != w64.e[i]) fail("biased value", t, px, py);
                if ((long long)w32.numerator(i) != w64.numerator(i) || wck.numerator(i).v != w64.numerator(i)) fail("numerator", t, px, py);
                if (!same_float((float)w32.numerator(i), (float)w64.numerator(i))) fail("(float) numerator", t, px, py);
                if (!same_float((float)w32.numerator(i) / fa32, (float)w64.numerator(i) / fa64)) fail("lambda", t, px, py);
            }
            if (w32.inside() != w64.inside() || wck.inside() != w64.inside()) fail("inside", t, px, py);
            if (k < n) {
                int n32[3];
                Checked32 nck[3];
                const bool in32 = slhip_raster::cover<int>(t.X, t.Y, t.flipped, t.bias, px, py, n32);
                const bool inck = slhip_raster::cover<Checked32>(t.X, t.Y, t.flipped, t.bias, px, py, nck);
                if (in32 != in || inck != in) fail("cover inside", t, px, py);
                for (int i = 0; i < 3; ++i)
                    if ((long long)n32[i] != num[i] || nck[i].v != num[i]) fail("cover numerator", t, px, py);
            }
        }
        if (k == n) break;
        ++g_texels;
        g_covered += in ? 1 : 0;
        if (px == t.xmax) {
            px = t.xmin; ++py;
            w64.next_row();
            if (with_narrow) { w32.next_row(); wck.next_row(); }
        } else {
            ++px;
            w64.step_x();
            if (with_narrow) { w32.step_x(); wck.step_x(); }
        }
    }
}

struct Counts { long long tris = 0, narrow = 0, wide = 0, culled = 0; };

// sets the triangle up both ways round; walks it in the narrow forms iff it qualifies.  expect: -1 any, 0 must not qualify,
// 1 must qualify
static void check(Counts& c, const int* X, const int* Y, int W, int H, int expect, bool walk_wide_too = true)
{
    for (int winding = 0; winding < 2; ++winding) {
        Tri t;
        for (int i = 0; i < 3; ++i) { t.X[i] = X[winding ? 2 - i : i]; t.Y[i] = Y[winding ? 2 - i : i]; }
        ++c.tris;
        if (!setup(t, W, H)) { ++c.culled; continue; }
        if (expect >= 0 && (int)t.narrow != expect) fail(expect ? "should qualify" : "should not qualify", t, 0, 0);
        if (t.narrow) { ++c.narrow; walk_box(t, true); }
        else { ++c.wide; if (walk_wide_too) walk_box(t, false); }
    }
}

int main()
{
    std::mt19937 rng(20260929u);
    auto uni = [&](int lo, int hi) { return (int)(lo + (long long)(rng() % (unsigned)(hi - lo + 1))); };
    const long long K = slhip_raster::kNarrowMax;
    Counts random_c, bound_c, sliver_c, zero_c, far_c, border_c;

    // random triangles of up to 40 x 40 texels anywhere in (and around) a 2048^2 target
    for (int k = 0; k < 4000; ++k) {
        const int ox = uni(-30 * 256, 2078 * 256), oy = uni(-30 * 256, 2078 * 256), s = 256 * uni(1, 40);
        int X[3], Y[3];
        for (int i = 0; i < 3; ++i) { X[i] = ox + uni(0, s); Y[i] = oy + uni(0, s); }
        check(random_c, X, Y, 2048, 2048, -1);
    }
    // ex * ey just below, at and just above the bound: ex = 2^15 (128 texels), ey = 2^14 -1 / +0 / +1 sub-pixels, and the square
    // floor(sqrt(K)) = 23170: 23170^2 <= K < 23170 * 23171
    {
        const int ex = 1 << 15;
        const int eys[3] = {(int)(K / ex) - 1, (int)(K / ex), (int)(K / ex) + 1};
        for (int j = 0; j < 3; ++j)
            for (int shape = 0; shape < 4; ++shape) {
                const int ox = 256 * 300 + uni(0, 255), oy = 256 * 200 + uni(0, 255), ey = eys[j];
                // right-angled in each corner, and one with the third vertex inside the span
                const int X[4][3] = {{0, ex, 0}, {0, ex, ex}, {0, ex, ex / 3}, {ex, 0, ex / 2}};
                const int Y[4][3] = {{0, 0, ey}, {0, ey, 0}, {0, ey / 2, ey}, {0, ey / 5, ey}};
                int Xs[3], Ys[3];
                for (int i = 0; i < 3; ++i) { Xs[i] = ox + X[shape][i]; Ys[i] = oy + Y[shape][i]; }
                check(bound_c, Xs, Ys, 2048, 2048, (long long)ex * ey <= K ? 1 : 0);
            }
        const int sq[3][2] = {{23170, 23170}, {23170, 23171}, {23171, 23171}};
        for (int j = 0; j < 3; ++j) {
            const int Xs[3] = {1000, 1000 + sq[j][0], 1000 + sq[j][0] / 2}, Ys[3] = {777, 777 + sq[j][1] / 3, 777 + sq[j][1]};
            check(bound_c, Xs, Ys, 2048, 2048, (long long)sq[j][0] * sq[j][1] <= K ? 1 : 0);
        }
    }
    // slivers: ex at its own limit K / 256 = 2^21 sub-pixels (8192 texels) -1 / +0 / +1, ey one sub-pixel (and two, and ey at the
    // limit with ex one sub-pixel), placed so that the single row / column of centres is hit
    {
        const int lim = (int)(K / 256);
        for (int d = -1; d <= 1; ++d)
            for (int ey = 1; ey <= 2; ++ey) {
                const int e = lim + d;
                const int Xa[3] = {128, 128 + e, 128 + e / 2}, Ya[3] = {128 + 256 * 5, 128 + 256 * 5, 128 + 256 * 5 + ey};
                check(sliver_c, Xa, Ya, 16384, 16384, e <= lim ? 1 : 0);
                const int Xb[3] = {128 + 256 * 7, 128 + 256 * 7 - ey, 128 + 256 * 7}, Yb[3] = {128, 128 + e / 3, 128 + e};
                check(sliver_c, Xb, Yb, 16384, 16384, e <= lim ? 1 : 0);
            }
    }
    // zero area: rejected by the set-up, both ways round
    {
        const int X1[3] = {100, 300, 500}, Y1[3] = {100, 300, 500};
        const int X2[3] = {4000, 4000, 4000}, Y2[3] = {4000, 4000, 9000};
        check(zero_c, X1, Y1, 2048, 2048, -1);
        check(zero_c, X2, Y2, 2048, 2048, -1);
        if (zero_c.culled != zero_c.tris) { std::printf("FAIL zero area accepted\n"); ++g_failures; }
    }
    // vertices far outside the target, the clamped box a few texels: judged by the box they would qualify, by the vertex extent
    // they do not -- and the 32-bit form would overflow on them
    {
        for (int k = 0; k < 200; ++k) {
            const int far = uni(1 << 22, 1 << 26);
            const int X[3] = {-far, far, uni(-far, far)}, Y[3] = {uni(-256 * 4, 256 * 2), uni(-256 * 4, 256 * 2), far};
            check(far_c, X, Y, 4, 3, 0);
        }
        // the same triangles, forced through the checked 32-bit form: the range check must fire (the test can see an overflow)
        const int X[3] = {-(1 << 25), 1 << 25, 0}, Y[3] = {-512, -300, 1 << 25};
        Tri t;
        for (int i = 0; i < 3; ++i) { t.X[i] = X[i]; t.Y[i] = Y[i]; }
        const long long seen = g_out_of_range;
        if (setup(t, 4, 3)) {
            slhip_raster::Walk<Checked32> w;
            w.start(t.X, t.Y, t.flipped, t.bias, t.xmin, t.ymin);
        }
        if (g_out_of_range == seen) { std::printf("FAIL the range check did not see a giant overflow\n"); ++g_failures; }
        g_out_of_range = seen;
    }
    // boxes touching each border of a 130 x 98 target (and crossing it: the clamp)
    {
        const int W = 130, H = 98;
        for (int k = 0; k < 400; ++k) {
            const int side = k & 3, s = 256 * uni(1, 12);
            int ox = uni(0, (W - 12) * 256), oy = uni(0, (H - 12) * 256);
            if (side == 0) ox = -uni(0, s);
            if (side == 1) ox = W * 256 - uni(0, s);
            if (side == 2) oy = -uni(0, s);
            if (side == 3) oy = H * 256 - uni(0, s);
            int X[3], Y[3];
            for (int i = 0; i < 3; ++i) { X[i] = ox + uni(0, s); Y[i] = oy + uni(0, s); }
            check(border_c, X, Y, W, H, 1);
        }
    }
    const Counts* all[6] = {&random_c, &bound_c, &sliver_c, &zero_c, &far_c, &border_c};
    const char* names[6] = {"random", "bound", "sliver", "zero", "far", "border"};
    for (int i = 0; i < 6; ++i)
        std::printf("%s: triangles %lld narrow %lld wide %lld culled %lld\n", names[i], all[i]->tris, all[i]->narrow, all[i]->wide, all[i]->culled);
    std::printf("texels %lld covered %lld out_of_range %lld failures %lld\n", g_texels, g_covered, g_out_of_range, g_failures);
    return (g_failures == 0 && g_out_of_range == 0) ? 0 : 1;
}
