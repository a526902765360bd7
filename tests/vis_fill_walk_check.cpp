// Host check of the strided edge walk of k_vis_fill (stillleben_amd/csrc/slhip_raster_walk.h, Walk::rows_down; compiled and run
// by tests/test_vis_fill_walk_host.py).
//
// The fill pass owns every pixel of a W x H target: a block takes a strip of 64 columns and rows_per_block rows, wave w of its
// four the rows w, w + 4, ... of the strip, lane == column.  For every triangle and every run of 8 of its rows a lane forms the
// three biased edge values at its first row by products (Walk<long long>::start) and steps them four rows down seven times.
// This program walks whole targets in exactly that order -- with the pass's skip of a wave whose texels lie outside the
// triangle's pixel box -- and holds every value against cover<long long>, the from-scratch form of coverage(), pixel by pixel:
// the biased values, the numerators, (float) of them, and the verdict "inside the box and covered".  The triangle set-up restates
// setup_finish() of slhip_render.hip.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <vector>

#include "slhip_raster_walk.h"

struct Tri {
    int X[3], Y[3];
    int flipped, bias[3];
    long long area2;
    int xmin, xmax, ymin, ymax;
};

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
    int x0 = (xmn - 128 + 255) >> 8, x1 = (xmx - 128) >> 8;
    int y0 = (ymn - 128 + 255) >> 8, y1 = (ymx - 128) >> 8;
    x0 = std::max(x0, 0); y0 = std::max(y0, 0);
    x1 = std::min(x1, W - 1); y1 = std::min(y1, H - 1);
    if (x0 > x1 || y0 > y1) return false;
    t.xmin = x0; t.xmax = x1; t.ymin = y0; t.ymax = y1;
    return true;
}

static bool same_float(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

static long long g_pixels = 0, g_covered = 0, g_failures = 0, g_skipped_waves = 0, g_walked_waves = 0;

static void fail(const char* what, const Tri& t, int px, int py)
{
    if (++g_failures <= 10)
        std::printf("FAIL %s: X %d %d %d Y %d %d %d pixel %d %d\n", what, t.X[0], t.X[1], t.X[2], t.Y[0], t.Y[1], t.Y[2], px, py);
}

constexpr int kFillRows = 8;   // as in slhip_render.hip

// One triangle over the whole target, in the order of k_vis_fill.  visits[p] counts the lanes that own pixel p (must end as 1).
static void fill_target(const Tri& t, int W, int H, int rows_per_block)
{
    std::vector<unsigned char> verdict((size_t)W * H, 2);   // 2: no lane has been here
    const int col_strips = (W + 63) / 64, row_strips = (H + rows_per_block - 1) / rows_per_block;
    const float fa = (float)t.area2;
    for (int rs = 0; rs < row_strips; ++rs)
        for (int cs = 0; cs < col_strips; ++cs) {
            const int x0 = cs * 64, row_begin = rs * rows_per_block, row_end = std::min(H, row_begin + rows_per_block);
            for (int r0 = row_begin; r0 < row_end; r0 += 4 * kFillRows)
                for (int wave = 0; wave < 4; ++wave) {
                    const int py0 = r0 + wave, py_last = py0 + 4 * (kFillRows - 1);
                    const bool skip = x0 + 63 < t.xmin || x0 > t.xmax || py_last < t.ymin || py0 > t.ymax;
                    ++(skip ? g_skipped_waves : g_walked_waves);
                    for (int lane = 0; lane < 64; ++lane) {
                        const int px = x0 + lane;
                        slhip_raster::Walk<long long> w;
                        if (!skip) w.start(t.X, t.Y, t.flipped, t.bias, px, py0);
                        for (int k = 0; k < kFillRows; ++k) {
                            const int py = py0 + 4 * k;
                            bool covered = false;
                            if (!skip) {
                                long long num[3];
                                const bool in = slhip_raster::cover<long long>(t.X, t.Y, t.flipped, t.bias, px, py, num);
                                for (int i = 0; i < 3; ++i) {
                                    if (w.e[i] != num[i] + t.bias[i] || w.numerator(i) != num[i]) fail("stepped value", t, px, py);
                                    if (!same_float((float)w.numerator(i) / fa, (float)num[i] / fa)) fail("lambda", t, px, py);
                                }
                                if (w.inside() != in) fail("inside", t, px, py);
                                covered = px >= t.xmin && px <= t.xmax && py >= t.ymin && py <= t.ymax && w.inside();
                                w.rows_down(4);
                            }
                            if (px < W && py < row_end) {
                                unsigned char& v = verdict[(size_t)py * W + px];
                                if (v != 2) fail("a pixel with two owners", t, px, py);
                                v = covered ? 1 : 0;
                            }
                        }
                    }
                }
        }
    // every pixel has exactly one owner, and its verdict is that of the from-scratch form inside the pixel box
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            long long num[3];
            const bool in = px >= t.xmin && px <= t.xmax && py >= t.ymin && py <= t.ymax &&
                            slhip_raster::cover<long long>(t.X, t.Y, t.flipped, t.bias, px, py, num);
            const unsigned char v = verdict[(size_t)py * W + px];
            if (v == 2) fail("a pixel without an owner", t, px, py);
            else if ((v == 1) != in) fail("verdict", t, px, py);
            ++g_pixels;
            g_covered += in ? 1 : 0;
        }
}

struct Counts { long long tris = 0, walked = 0, flipped = 0, culled = 0; };

static void check(Counts& c, const int* X, const int* Y, int W, int H, int rows_per_block)
{
    for (int winding = 0; winding < 2; ++winding) {
        Tri t;
        for (int i = 0; i < 3; ++i) { t.X[i] = X[winding ? 2 - i : i]; t.Y[i] = Y[winding ? 2 - i : i]; }
        ++c.tris;
        if (!setup(t, W, H)) { ++c.culled; continue; }
        ++c.walked;
        c.flipped += t.flipped ? 1 : 0;
        fill_target(t, W, H, rows_per_block);
    }
}

int main()
{
    std::mt19937 rng(20261019u);
    auto uni = [&](int lo, int hi) { return (int)(lo + (long long)(rng() % (unsigned)(hi - lo + 1))); };
    Counts random_c, sliver_c, border_c, far_c, corner_c, plane_c;
    // targets: partial strips at the right and bottom edge, a single strip, several row strips, rows_per_block 32 and 96
    const int targets[5][3] = {{24, 16, 96}, {40, 12, 96}, {36, 20, 32}, {130, 98, 32}, {200, 150, 96}};

    for (int k = 0; k < 300; ++k) {
        const int* g = targets[k % 5];
        int X[3], Y[3];
        for (int i = 0; i < 3; ++i) { X[i] = uni(-20 * 256, (g[0] + 20) * 256); Y[i] = uni(-20 * 256, (g[1] + 20) * 256); }
        check(random_c, X, Y, g[0], g[1], g[2]);
    }
    // slivers: a sub-pixel or two high (wide), across the whole target and far beyond it
    for (int k = 0; k < 60; ++k) {
        const int* g = targets[k % 5];
        const int y = 128 + 256 * uni(0, g[1] - 1), e = uni(1, 3), far = k & 1 ? 1 << 24 : g[0] * 256;
        const int Xa[3] = {-far, far, uni(-far, far)}, Ya[3] = {y, y, y + e};
        check(sliver_c, Xa, Ya, g[0], g[1], g[2]);
        const int x = 128 + 256 * uni(0, g[0] - 1);
        const int Xb[3] = {x, x - e, x}, Yb[3] = {-far, uni(-far, far), far};
        check(sliver_c, Xb, Yb, g[0], g[1], g[2]);
    }
    // boxes touching and crossing each border of the target: the clamp
    for (int k = 0; k < 200; ++k) {
        const int* g = targets[k % 5];
        const int W = g[0], H = g[1], side = (k / 5) & 3, s = 256 * uni(1, 12);
        int ox = uni(0, std::max(W - 12, 1) * 256), oy = uni(0, std::max(H - 12, 1) * 256);
        if (side == 0) ox = -uni(0, s);
        if (side == 1) ox = W * 256 - uni(0, s);
        if (side == 2) oy = -uni(0, s);
        if (side == 3) oy = H * 256 - uni(0, s);
        int X[3], Y[3];
        for (int i = 0; i < 3; ++i) { X[i] = ox + uni(0, s); Y[i] = oy + uni(0, s); }
        check(border_c, X, Y, W, H, g[2]);
    }
    // vertices far outside the target, up to the 2^26 sub-pixels snap() allows: the plane seen from close above
    for (int k = 0; k < 100; ++k) {
        const int* g = targets[k % 5];
        const int far = uni(1 << 22, 1 << 26);
        const int X[3] = {-far, far, uni(-far, far)}, Y[3] = {uni(-256 * 4, 256 * g[1]), uni(-256 * 4, 256 * g[1]), far};
        check(far_c, X, Y, g[0], g[1], g[2]);
    }
    {
        const int m = 1 << 26;   // the extreme: all three at the bound
        const int X[3] = {-m, m, -m}, Y[3] = {-m, -m, m};
        check(far_c, X, Y, 200, 150, 96);
        const int X2[3] = {m, -m, m}, Y2[3] = {m, m, -m};
        check(far_c, X2, Y2, 200, 150, 96);
    }
    // pixel boxes that begin or end exactly at the origin of a wave's texels: columns 64 and 128, rows 32, 96, 97 (a vertex on a
    // pixel centre puts the box edge on that pixel)
    {
        const int xs[4] = {63, 64, 127, 128}, ys[6] = {31, 32, 35, 95, 96, 97};
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 6; ++b)
                for (int d = 0; d < 2; ++d) {
                    const int cx = 256 * xs[a] + 128, cy = 256 * ys[b] + 128, s = 256 * uni(3, 40);
                    // the box starts at (xs, ys) / ends there
                    const int X[3] = {cx, d ? cx - s : cx + s, d ? cx - s / 2 : cx + s / 3};
                    const int Y[3] = {cy, d ? cy - s / 4 : cy + s / 2, d ? cy - s : cy + s};
                    check(corner_c, X, Y, 200, 150, 32);
                    check(corner_c, X, Y, 200, 150, 96);
                }
    }
    // two triangles that share a diagonal and cover the target (the background plane): every pixel is in exactly one
    {
        const int W = 200, H = 150, m = 256 * 40;
        const int Xa[3] = {-m, W * 256 + m, W * 256 + m}, Ya[3] = {-m, -m, H * 256 + m};
        const int Xb[3] = {-m, W * 256 + m, -m}, Yb[3] = {-m, H * 256 + m, H * 256 + m};
        const long long before = g_covered;
        Tri ta, tb;
        for (int i = 0; i < 3; ++i) { ta.X[i] = Xa[i]; ta.Y[i] = Ya[i]; tb.X[i] = Xb[i]; tb.Y[i] = Yb[i]; }
        plane_c.tris = 2;
        if (setup(ta, W, H) && setup(tb, W, H)) {
            plane_c.walked = 2;
            plane_c.flipped = ta.flipped + tb.flipped;
            fill_target(ta, W, H, 96);
            fill_target(tb, W, H, 96);
        }
        if (g_covered - before != (long long)W * H) { std::printf("FAIL the two halves of a plane cover %lld of %d pixels\n", g_covered - before, W * H); ++g_failures; }
    }
    const Counts* all[6] = {&random_c, &sliver_c, &border_c, &far_c, &corner_c, &plane_c};
    const char* names[6] = {"random", "sliver", "border", "far", "corner", "plane"};
    for (int i = 0; i < 6; ++i)
        std::printf("%s: triangles %lld walked %lld flipped %lld culled %lld\n", names[i], all[i]->tris, all[i]->walked, all[i]->flipped, all[i]->culled);
    std::printf("pixels %lld covered %lld waves_walked %lld waves_skipped %lld failures %lld\n", g_pixels, g_covered, g_walked_waves,
                g_skipped_waves, g_failures);
    return g_failures == 0 ? 0 : 1;
}
