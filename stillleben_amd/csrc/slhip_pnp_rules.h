// slhip_pnp_rules.h -- the rules of the pose from correspondences (slhip_pose_pnp.hip) as plain float32 C++ for host and device
// alike: k_pose_pnp and slhip_pose_pnp_host run the same functions, so every output agrees bit for bit.  Every operation is one
// rounded IEEE operation (the build passes -ffp-contract=off); only + - * /, sqrtf, fabsf, fminf / fmaxf and comparisons appear:
// no sin, cos, acos, cbrt or pow, which the device and host libraries round differently.  The parenthesisation is the contract
// (include/slhip.h "Pose PnP", DESIGN.md "Pose PnP").
//
// The minimal solver.  Points P1, P2, P3 seen along the unit bearings f1, f2, f3 at the distances s1, s2, s3:
//   (si - sj)^2 + si sj e_ij = d_ij^2,   e_ij = |fi - fj|^2 (= 2 - 2 cos, formed without the cosine),  d_ij = |Pi - Pj|
// With s1 = (1 + xi) s3, s2 = (1 + eta) s3 and the pair (1, 3) dividing the other two, A = d23^2 / d13^2, C = d12^2 / d13^2:
//   q(xi) = xi^2 + (1 + xi) e13                                   (= d13^2 / s3^2)
//   eta^2 + e23 eta + P(xi) = 0,            P = e23 - A q          (pair 2, 3)
//   eta L(xi) + M(xi) = 0,                  L = (e23 - e12) + (2 - e12) xi,  M = (e23 - e12) - e12 xi - xi^2 + (C - A) q
// (the second is the difference of pairs (2, 3) and (1, 2)), hence the quartic G(xi) = M^2 - e23 M L + P L^2 = 0.  Every term
// is a small quantity when the depths are alike: nothing of the size of 1 cancels, which the cosine form does in float32.
// xi in (-1, inf) is mapped to tau in (-1, 1) by xi = 2 tau / (1 - tau); the real roots in tau come from sign changes between
// the roots of the derivative, each by BISECT halvings, the derivative's roots the same way down to the linear one.  Per root:
// eta from the (2, 3) quadratic (the root that serves pair (1, 2) better), the distances, POLISH Newton steps on the three
// equations above, a rotation from the two triangles' edge frames, t = X1 - R P1.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_pose_rules.h"      // row_point, is_finite, pixel_u, BLOCK, WAVE, block_sum
#include "slhip_ransac_rules.h"    // pick, key_of, key_count, key_best
#include "slhip_rng.h"             // Philox

namespace slhip_pnp {

using slhip_pose::is_finite;
using slhip_pose::pixel_u;
using slhip_pose::row_point;
using slhip_ransac::key_best;
using slhip_ransac::key_count;
using slhip_ransac::key_of;
using slhip_ransac::pose_finite;

constexpr uint32_t BLOCK = slhip_pose::BLOCK;
constexpr uint32_t WAVE = slhip_pose::WAVE;
constexpr uint32_t STREAM = 7u;               // the Philox stream of the samples ("Randomness")
constexpr int BISECT = 24;                    // halvings per root of the cascade
constexpr int POLISH = 3;                     // Newton steps on the three distances per solution
constexpr float SIDE_TOL = 1.0f / 1024.0f;    // a polished solution may miss a squared side by this share of it
constexpr int SUMS = 27;                      // 21 of J^T J (upper triangle, rows upwards), 6 of J^T r

struct Camera {
    float fx, fy, cx, cy;
};

// rule 1: a correspondence counts when u, v, x, y, z are finite and w > 0
SLHIP_HD bool valid(float u, float v, float x, float y, float z, float w)
{
    return is_finite(u) && is_finite(v) && is_finite(x) && is_finite(y) && is_finite(z) && w > 0.0f;
}

// rule 2: the four picks of hypothesis h among n_valid; false when two of them coincide (the hypothesis is void)
SLHIP_HD bool sample(uint32_t key0, uint32_t key1, uint32_t set_id, uint32_t h, uint32_t n_valid, uint32_t* idx)
{
    slhip::Philox p;
    p.c[0] = set_id; p.c[1] = STREAM; p.c[2] = h; p.c[3] = 0x51DE5EEDu;
    p.k[0] = key0; p.k[1] = key1;
    p.block();
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = slhip_ransac::pick(p.c[k], n_valid);
    return idx[0] != idx[1] && idx[0] != idx[2] && idx[0] != idx[3] && idx[1] != idx[2] && idx[1] != idx[3] && idx[2] != idx[3];
}

// ---- rule 3: the minimal solver -------------------------------------------------------------------------------------------------
template <int N>
SLHIP_HD float horner(const float* c, float t)
{
    float v = c[N];
#pragma unroll
    for (int i = N - 1; i >= 0; --i) v = v * t + c[i];
    return v;
}

// The real roots in [-1, 1] of c[0] + c[1] t + .. + c[N] t^N.  out[0 .. N) rises; bit i of the result: out[i] is a root, found
// in the i-th interval between the knots -1, (the derivative's out), 1; without the bit out[i] repeats the interval's upper end.
// A sign is `value > 0`, so a zero (or a NaN) sits on the negative side and is met once.
template <int N>
struct Roots {
    SLHIP_HD static unsigned run(const float* c, float* out)
    {
        float d[N], knot[N];
#pragma unroll
        for (int i = 0; i < N; ++i) d[i] = (float)(i + 1) * c[i + 1];
        Roots<N - 1>::run(d, knot);
        knot[N - 1] = 1.0f;
        unsigned found = 0u;
        float lo = -1.0f;
        bool slo = horner<N>(c, lo) > 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float hi = knot[i];
            const bool shi = horner<N>(c, hi) > 0.0f;
            float r = hi;
            if (slo != shi) {
                float a = lo, b = hi;
                for (int it = 0; it < BISECT; ++it) {
                    const float mid = 0.5f * (a + b);
                    if ((horner<N>(c, mid) > 0.0f) == slo) a = mid; else b = mid;
                }
                r = 0.5f * (a + b);
                found |= 1u << i;
            }
            out[i] = r;
            lo = hi;
            slo = shi;
        }
        return found;
    }
};

template <>
struct Roots<0> {
    SLHIP_HD static unsigned run(const float*, float*) { return 0u; }
};

struct Triangle {
    float f[3][3];          // unit bearings
    float e12, e13, e23;    // |fi - fj|^2
    float d12, d13, d23;    // |Pi - Pj|^2
    float root[4];          // tau
    unsigned found;
};

SLHIP_HD float dist2(const float* a, const float* b)
{
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// bearings ab[i] = (a, b) of rule 1, points P[i]: the quartic's roots
SLHIP_HD void triangle(const float ab[3][2], const float P[3][3], Triangle& t)
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float n = sqrtf((ab[i][0] * ab[i][0] + ab[i][1] * ab[i][1]) + 1.0f);
        t.f[i][0] = ab[i][0] / n;
        t.f[i][1] = ab[i][1] / n;
        t.f[i][2] = 1.0f / n;
    }
    t.e12 = dist2(t.f[0], t.f[1]); t.e13 = dist2(t.f[0], t.f[2]); t.e23 = dist2(t.f[1], t.f[2]);
    t.d12 = dist2(P[0], P[1]); t.d13 = dist2(P[0], P[2]); t.d23 = dist2(P[1], P[2]);
    const float A = t.d23 / t.d13, C = t.d12 / t.d13, ca = C - A;
    const float l0 = t.e23 - t.e12, l1 = 2.0f - t.e12;
    const float m0 = l0 + ca * t.e13, m1 = ca * t.e13 - t.e12, m2 = ca - 1.0f;
    const float p0 = t.e23 - A * t.e13, p1 = -(A * t.e13), p2 = -A;
    const float ll0 = l0 * l0, ll1 = 2.0f * (l0 * l1), ll2 = l1 * l1;
    float g[5];
    g[0] = (m0 * m0 - t.e23 * (m0 * l0)) + p0 * ll0;
    g[1] = (2.0f * (m0 * m1) - t.e23 * (m0 * l1 + m1 * l0)) + (p0 * ll1 + p1 * ll0);
    g[2] = ((2.0f * (m0 * m2) + m1 * m1) - t.e23 * (m1 * l1 + m2 * l0)) + ((p0 * ll2 + p1 * ll1) + p2 * ll0);
    g[3] = (2.0f * (m1 * m2) - t.e23 * (m2 * l1)) + (p1 * ll2 + p2 * ll1);
    g[4] = m2 * m2 + p2 * ll2;
    // xi = 2 tau / (1 - tau):  H(tau) = sum_k g_k (2 tau)^k (1 - tau)^(4 - k)
    float h[5];
    h[0] = g[0];
    h[1] = 2.0f * g[1] - 4.0f * g[0];
    h[2] = (6.0f * g[0] - 6.0f * g[1]) + 4.0f * g[2];
    h[3] = ((6.0f * g[1] - 4.0f * g[0]) - 8.0f * g[2]) + 8.0f * g[3];
    h[4] = (((g[0] - 2.0f * g[1]) + 4.0f * g[2]) - 8.0f * g[3]) + 16.0f * g[4];
    t.found = Roots<4>::run(h, t.root);
}

SLHIP_HD float det3(float a, float b, float c, float d, float e, float f, float g, float h, float i)
{
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}

// the pose of root `slot` of the triangle (P the same points): false when it is not kept
SLHIP_HD bool solution(const Triangle& t, int slot, const float P[3][3], float* pose)
{
    const float tau = slot == 0 ? t.root[0] : slot == 1 ? t.root[1] : slot == 2 ? t.root[2] : t.root[3];
    const float xi = (2.0f * tau) / (1.0f - tau);
    const float A = t.d23 / t.d13, C = t.d12 / t.d13;
    const float q = xi * xi + (1.0f + xi) * t.e13;
    // eta of pair (2, 3), the root that leaves pair (1, 2) the smaller rest
    const float disc = fmaxf(t.e23 * t.e23 - 4.0f * (t.e23 - A * q), 0.0f), sq = sqrtf(disc);
    const float ea = 0.5f * (sq - t.e23), eb = 0.5f * (-sq - t.e23);
    const float ra = fabsf((((xi - ea) * (xi - ea)) + ((1.0f + xi) * (1.0f + ea)) * t.e12) - C * q);
    const float rb = fabsf((((xi - eb) * (xi - eb)) + ((1.0f + xi) * (1.0f + eb)) * t.e12) - C * q);
    const float eta = rb < ra ? eb : ea;
    float s3 = sqrtf(t.d13 / q), s1 = (1.0f + xi) * s3, s2 = (1.0f + eta) * s3;
    float r12 = 0.0f, r13 = 0.0f, r23 = 0.0f;
    for (int it = 0; it <= POLISH; ++it) {
        const float a = s1 - s2, b = s1 - s3, c = s2 - s3;
        r12 = (a * a + (s1 * s2) * t.e12) - t.d12;
        r13 = (b * b + (s1 * s3) * t.e13) - t.d13;
        r23 = (c * c + (s2 * s3) * t.e23) - t.d23;
        if (it == POLISH) break;
        const float a1 = 2.0f * a + s2 * t.e12, a2 = s1 * t.e12 - 2.0f * a;
        const float b1 = 2.0f * b + s3 * t.e13, b3 = s1 * t.e13 - 2.0f * b;
        const float c2 = 2.0f * c + s3 * t.e23, c3 = s2 * t.e23 - 2.0f * c;
        const float det = det3(a1, a2, 0.0f, b1, 0.0f, b3, 0.0f, c2, c3);
        s1 = s1 - det3(r12, a2, 0.0f, r13, 0.0f, b3, r23, c2, c3) / det;
        s2 = s2 - det3(a1, r12, 0.0f, b1, r13, b3, 0.0f, r23, c3) / det;
        s3 = s3 - det3(a1, a2, r12, b1, 0.0f, r13, 0.0f, c2, r23) / det;
    }
    if (!(s1 > 0.0f) || !(s2 > 0.0f) || !(s3 > 0.0f)) return false;
    if (!(fabsf(r12) <= SIDE_TOL * t.d12) || !(fabsf(r13) <= SIDE_TOL * t.d13) || !(fabsf(r23) <= SIDE_TOL * t.d23)) return false;
    // X_i = s_i f_i;  R maps the frame (P2 - P1, P3 - P1, their cross product) onto that of the X
    float X1[3], u[3], v[3], p[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        X1[k] = s1 * t.f[0][k];
        u[k] = s2 * t.f[1][k] - X1[k];
        v[k] = s3 * t.f[2][k] - X1[k];
        p[k] = P[1][k] - P[0][k];
        r[k] = P[2][k] - P[0][k];
    }
    const float w[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
    const float n[3] = {p[1] * r[2] - p[2] * r[1], p[2] * r[0] - p[0] * r[2], p[0] * r[1] - p[1] * r[0]};
    const float k1[3] = {r[1] * n[2] - r[2] * n[1], r[2] * n[0] - r[0] * n[2], r[0] * n[1] - r[1] * n[0]};
    const float k2[3] = {n[1] * p[2] - n[2] * p[1], n[2] * p[0] - n[0] * p[2], n[0] * p[1] - n[1] * p[0]};
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) pose[4 * i + j] = ((u[i] * k1[j] + v[i] * k2[j]) + w[i] * n[j]) / nn;
        pose[4 * i + 3] = X1[i] - ((pose[4 * i] * P[0][0] + pose[4 * i + 1] * P[0][1]) + pose[4 * i + 2] * P[0][2]);
#pragma unroll
        for (int j = 0; j < 4; ++j) ok = ok && is_finite(pose[4 * i + j]);
    }
    return ok;
}

// ---- rule 4: the score ----------------------------------------------------------------------------------------------------------
// squared pixel error of point (x, y, z) seen at (u, v) under the pose M; *front: Z > 0
SLHIP_HD float reproject2(const float* M, const Camera& k, float x, float y, float z, float u, float v, bool* front)
{
    const float X = row_point(M, x, y, z), Y = row_point(M + 4, x, y, z), Z = row_point(M + 8, x, y, z);
    const float du = pixel_u(k.fx, X, Z, k.cx) - u, dv = pixel_u(k.fy, Y, Z, k.cy) - v;
    *front = Z > 0.0f;
    return du * du + dv * dv;
}

SLHIP_HD bool inlier(const float* M, const Camera& k, float x, float y, float z, float u, float v, float thr2, float* e2)
{
    bool front;
    *e2 = reproject2(M, k, x, y, z, u, v, &front);
    return front && *e2 <= thr2;
}

// rule 3's choice among the kept solutions and rule 2's picks: the pose of hypothesis h, false when it is void.
// pick(i, uvxyz) hands out valid correspondence i as (u, v, x, y, z)
template <class Pick>
SLHIP_HD bool hypothesis(uint32_t key0, uint32_t key1, uint32_t set_id, uint32_t h, uint32_t n_valid, const Camera& k, Pick pick,
                         float* pose)
{
    uint32_t idx[4];
    if (!sample(key0, key1, set_id, h, n_valid, idx)) return false;
    float ab[3][2], P[3][3], c[5];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        pick(idx[i], c);
        ab[i][0] = (c[0] - k.cx) / k.fx;
        ab[i][1] = (c[1] - k.cy) / k.fy;
        P[i][0] = c[2]; P[i][1] = c[3]; P[i][2] = c[4];
    }
    pick(idx[3], c);
    Triangle t;
    triangle(ab, P, t);
    bool have = false;
    float best = 0.0f;
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
        float m[12];
        if (!((t.found >> s) & 1u) || !solution(t, s, P, m)) continue;
        bool front;
        float e = reproject2(m, k, c[2], c[3], c[4], c[0], c[1], &front);
        if (!front || !(e == e)) e = __builtin_inff();
        if (!have || e < best) {
            have = true;
            best = e;
#pragma unroll
            for (int i = 0; i < 12; ++i) pose[i] = m[i];
        }
    }
    return have;
}

// ---- rule 5: the refinement -----------------------------------------------------------------------------------------------------
// the 27 terms of an inlier: acc[..] = acc[..] + term
SLHIP_HD void accumulate(const float* M, const Camera& k, float x, float y, float z, float u, float v, float* acc)
{
    const float X = row_point(M, x, y, z), Y = row_point(M + 4, x, y, z), Z = row_point(M + 8, x, y, z);
    const float iz = 1.0f / Z, xn = X * iz, yn = Y * iz;
    const float ru = pixel_u(k.fx, X, Z, k.cx) - u, rv = pixel_u(k.fy, Y, Z, k.cy) - v;
    const float ju[6] = {-(k.fx * (xn * yn)), k.fx * (1.0f + xn * xn), -(k.fx * yn), k.fx * iz, 0.0f, -(k.fx * (xn * iz))};
    const float jv[6] = {-(k.fy * (1.0f + yn * yn)), k.fy * (xn * yn), k.fy * xn, 0.0f, k.fy * iz, -(k.fy * (yn * iz))};
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++at) acc[at] = acc[at] + (ju[i] * ju[j] + jv[i] * jv[j]);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + (ju[i] * ru + jv[i] * rv);
}

// (J^T J) delta = -(J^T r) by L D L^T without pivoting, then M <- [R(c) R | R(c) t + dt], c = omega / 2 (Cayley).
// false, M unchanged, when a pivot is not positive and finite.
SLHIP_HD bool step(const float* S, float* M)
{
    float A[6][6], L[6][6], D[6], x[6];
    int at = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++at) A[i][j] = A[j][i] = S[at];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        float d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - (L[j][k] * L[j][k]) * D[k];
        ok = ok && d > 0.0f && is_finite(d);
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            float v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * D[k];
            L[i][j] = v / d;
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 6; ++i) {      // L z = -b
        float v = -S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * x[k];
        x[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) x[i] = x[i] / D[i];
#pragma unroll
    for (int i = 5; i >= 0; --i) {     // L^T delta = z / D
        float v = x[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
        x[i] = v;
    }
    const float c0 = 0.5f * x[0], c1 = 0.5f * x[1], c2 = 0.5f * x[2];
    const float cc = (c0 * c0 + c1 * c1) + c2 * c2, a = 1.0f - cc, b = 1.0f + cc;
    const float R[9] = {(a + 2.0f * (c0 * c0)) / b,        (2.0f * (c0 * c1) - 2.0f * c2) / b, (2.0f * (c0 * c2) + 2.0f * c1) / b,
                        (2.0f * (c0 * c1) + 2.0f * c2) / b, (a + 2.0f * (c1 * c1)) / b,        (2.0f * (c1 * c2) - 2.0f * c0) / b,
                        (2.0f * (c0 * c2) - 2.0f * c1) / b, (2.0f * (c1 * c2) + 2.0f * c0) / b, (a + 2.0f * (c2 * c2)) / b};
    float N[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) N[4 * i + j] = (R[3 * i] * M[j] + R[3 * i + 1] * M[4 + j]) + R[3 * i + 2] * M[8 + j];
        N[4 * i + 3] = N[4 * i + 3] + x[3 + i];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = N[i];
    return true;
}

}  // namespace slhip_pnp
