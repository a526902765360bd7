// slhip_vote_rules.h -- the rules of the keypoint voting (slhip_keypoint_vote.hip) as plain float32 C++ for host and device alike:
// k_keypoint_vote and slhip_keypoint_vote_host run the same functions, so every output agrees bit for bit.  Every operation is one
// rounded IEEE operation (the build passes -ffp-contract=off); only + - * /, sqrtf, fabsf and comparisons appear.  The
// parenthesisation is the contract (include/slhip.h "Keypoint voting", DESIGN.md "Keypoint voting").
//
// A voter is a pixel centre p and a unit vector d: the keypoint lies, the network says, on the ray p + s d, s > 0.  Two voters
// give a hypothesis q, the meeting point of their lines; a voter agrees with q when the angle between d and q - p has a cosine
// of at least inlier_cos, tested as dot > 0 && dot^2 >= cos^2 |q - p|^2 without a root or a division.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_pose_rules.h"      // is_finite, BLOCK, WAVE, block_sum
#include "slhip_rng.h"             // Philox

namespace slhip_vote {

using slhip_pose::is_finite;

constexpr uint32_t BLOCK = slhip_pose::BLOCK;
constexpr uint32_t WAVE = slhip_pose::WAVE;
constexpr uint32_t STREAM = 8u;         // the Philox stream of the samples ("Randomness")
constexpr int H_BITS = 11;              // arg-max key: (count << 11) | (1024 - h)

struct Voter {
    float px, py, dx, dy;
};

struct Q {
    float x, y;
};

// rule 1, the pixel's part: inside the picture
SLHIP_HD bool pixel_inside(int x, int y, uint32_t W, uint32_t H) { return x >= 0 && y >= 0 && (uint32_t)x < W && (uint32_t)y < H; }

// rule 1, the vector's part: finite and of a length > 0; the voter of pixel (x, y)
SLHIP_HD bool voter(int x, int y, float vx, float vy, Voter* v)
{
    if (!is_finite(vx) || !is_finite(vy)) return false;
    const float l = sqrtf(vx * vx + vy * vy);
    if (!(l > 0.0f)) return false;
    v->px = (float)x + 0.5f;
    v->py = (float)y + 0.5f;
    v->dx = vx / l;
    v->dy = vy / l;
    return true;
}

SLHIP_HD float uniform(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// rule 2: the two picks of hypothesis h of keypoint k among n_valid
SLHIP_HD void sample(uint32_t key0, uint32_t key1, uint32_t set_id, uint32_t h, uint32_t k, uint32_t n_valid, uint32_t* a, uint32_t* b)
{
    slhip::Philox p;
    p.c[0] = set_id; p.c[1] = STREAM; p.c[2] = h; p.c[3] = k;
    p.k[0] = key0; p.k[1] = key1;
    p.block();
    const uint32_t i = (uint32_t)(uniform(p.c[0]) * (float)n_valid), j = (uint32_t)(uniform(p.c[1]) * (float)n_valid);
    *a = i < n_valid - 1u ? i : n_valid - 1u;
    *b = j < n_valid - 1u ? j : n_valid - 1u;
}

// rule 2: the meeting point of the lines of voters a and b (a_is_b: the picks coincide); false when the hypothesis is void
SLHIP_HD bool intersect(bool a_is_b, const Voter& a, const Voter& b, float min_sin, Q* q)
{
    if (a_is_b || (a.px == b.px && a.py == b.py)) return false;
    const float det = a.dx * b.dy - a.dy * b.dx;
    if (fabsf(det) <= min_sin) return false;
    const float s = ((b.px - a.px) * b.dy - (b.py - a.py) * b.dx) / det;
    q->x = a.px + s * a.dx;
    q->y = a.py + s * a.dy;
    return is_finite(q->x) && is_finite(q->y);      // (a NaN det passes the comparison above and stops here)
}

// rule 3: voter (px, py, dx, dy) agrees with q; cc = inlier_cos * inlier_cos
SLHIP_HD bool inlier(float qx, float qy, float px, float py, float dx, float dy, float cc)
{
    const float ex = qx - px, ey = qy - py;
    const float dot = ex * dx + ey * dy, n2 = ex * ex + ey * ey;
    return n2 == 0.0f || (dot > 0.0f && dot * dot >= cc * n2);
}

SLHIP_HD uint32_t key_of(uint32_t count, uint32_t h) { return (count << H_BITS) | (1024u - h); }
SLHIP_HD uint32_t key_count(uint32_t key) { return key >> H_BITS; }
SLHIP_HD int key_best(uint32_t key) { return (int)(1024u - (key & ((1u << H_BITS) - 1u))); }

// rule 4: the weight of a hypothesis, and its terms of the two passes: acc[..] = acc[..] + term
SLHIP_HD float weight(uint32_t count, uint32_t n_valid) { return (float)count / (float)n_valid; }

SLHIP_HD void accumulate_mean(float w, float qx, float qy, float* acc)
{
    acc[0] = acc[0] + w;
    acc[1] = acc[1] + w * qx;
    acc[2] = acc[2] + w * qy;
}

SLHIP_HD void accumulate_cov(float w, float qx, float qy, float mx, float my, float* acc)
{
    const float gx = qx - mx, gy = qy - my;
    acc[0] = acc[0] + (w * gx) * gx;
    acc[1] = acc[1] + (w * gx) * gy;
    acc[2] = acc[2] + (w * gy) * gy;
}

// Error-free pieces of rule 5 (Dekker, Veltkamp): each is a handful of rounded + - *, no fma, and returns the rounded result with
// what the rounding lost in *err, exactly (barring overflow).
SLHIP_HD float two_sum(float a, float b, float* err)
{
    const float s = a + b, bb = s - a;
    *err = (a - (s - bb)) + (b - bb);
    return s;
}

SLHIP_HD void split(float a, float* hi, float* lo)
{
    const float c = 4097.0f * a;      // 2^12 + 1: two halves of 12 bits
    *hi = c - (c - a);
    *lo = a - *hi;
}

SLHIP_HD float two_product(float a, float b, float* err)
{
    const float p = a * b;
    float ah, al, bh, bl;
    split(a, &ah, &al);
    split(b, &bh, &bl);
    *err = ((ah * bh - p) + ah * bl + al * bh) + al * bl;
    return p;
}

// rule 5: c = n . (p - q), the signed distance of q from the voter's line.  q lies ON the lines of its pair and near those of its
// inliers, so c is the small rest of two products of the size of |p - q|: evaluated plainly it keeps their rounding, 2^-24 |p - q|,
// which is as large as c itself when the field is a good one.  Here the two differences, the two products and their sum are
// formed error-free and the lost parts are added back, smallest first: c is right to a rounding of ITSELF.
SLHIP_HD float line_offset(float nx, float ny, float px, float py, float qx, float qy)
{
    float fx, fy, e1, e2, t;
    const float ex = two_sum(px, -qx, &fx), ey = two_sum(py, -qy, &fy);
    const float p1 = two_product(nx, ex, &e1), p2 = two_product(ny, ey, &e2);
    const float s = two_sum(p1, p2, &t);
    return s + ((t + (e1 + e2)) + (nx * fx + ny * fy));
}

// rule 5: the five terms of an inlier of q
SLHIP_HD void accumulate_fit(float qx, float qy, float px, float py, float dx, float dy, float* acc)
{
    const float nx = -dy, ny = dx;
    const float c = line_offset(nx, ny, px, py, qx, qy);
    acc[0] = acc[0] + nx * nx;
    acc[1] = acc[1] + nx * ny;
    acc[2] = acc[2] + ny * ny;
    acc[3] = acc[3] + nx * c;
    acc[4] = acc[4] + ny * c;
}

// rule 5: uv = q + A^-1 b by Cramer; false, uv = q, when the determinant is not finite or not > 0
SLHIP_HD bool fit(const float* S, float qx, float qy, Q* uv)
{
    const float det = S[0] * S[2] - S[1] * S[1];
    uv->x = qx;
    uv->y = qy;
    if (!is_finite(det) || !(det > 0.0f)) return false;
    uv->x = qx + (S[3] * S[2] - S[1] * S[4]) / det;
    uv->y = qy + (S[0] * S[4] - S[1] * S[3]) / det;
    return true;
}

}  // namespace slhip_vote
