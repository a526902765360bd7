// slhip_fit_rules.h -- the rules of the rigid fit (slhip_pose_fit.hip) as plain float32 C++ for host and device alike: k_pose_fit
// and slhip_pose_fit_host run the same functions, so every output agrees bit for bit.  Every operation is one rounded IEEE
// operation (the build passes -ffp-contract=off); only + - * /, sqrtf, fabsf and comparisons appear.  The parenthesisation is
// the contract (include/slhip.h "Rigid fit", DESIGN.md "Rigid fit").
//
// Horn's closed form (Horn 1987, "Closed-form solution of absolute orientation using unit quaternions"): the rotation that takes
// the centred src onto the centred dst in the least-squares sense is the unit quaternion that is the eigenvector of the largest
// eigenvalue of a symmetric 4 x 4 matrix N built from the nine sums M = sum (src - cs)(dst - cd)^T.  A quaternion always gives a
// proper rotation: there is no reflection to correct, flat point sets included.  The eigenvectors come from cyclic Jacobi with a
// fixed number of sweeps -- straight-line code, the same on every lane and on the host.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_pose_rules.h"      // is_finite, row_point, BLOCK, WAVE, block_sum

namespace slhip_fit {

using slhip_pose::is_finite;
using slhip_pose::row_point;

constexpr uint32_t BLOCK = slhip_pose::BLOCK;      // the lanes of a set's sums: lane l takes correspondences l, l + 256, ... upwards
constexpr uint32_t WAVE = slhip_pose::WAVE;
constexpr int SWEEPS = 8;      // cyclic Jacobi sweeps over the six pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a 4 x 4 converges
                               // quadratically after the first two or three, and tests/test_host_pose_fit.py checks that what is
                               // left off the diagonal after 8 lies below float32 rounding of the diagonal

// rule 1: correspondence (s, d) counts
SLHIP_HD bool used(const float* s, const float* d)
{
    return s[3] > 0.0f && d[3] != 0.0f && is_finite(s[0]) && is_finite(s[1]) && is_finite(s[2]) && is_finite(d[0]) && is_finite(d[1]) &&
           is_finite(d[2]);
}

// rule 2, first pass: the six terms of the centroids
SLHIP_HD void accumulate_centroids(const float* s, const float* d, float* acc)
{
    acc[0] = acc[0] + s[0]; acc[1] = acc[1] + s[1]; acc[2] = acc[2] + s[2];
    acc[3] = acc[3] + d[0]; acc[4] = acc[4] + d[1]; acc[5] = acc[5] + d[2];
}

// rule 2, second pass: M[3 i + j] += (s_i - cs_i) * (d_j - cd_j); c = {cs, cd}
SLHIP_HD void accumulate_moments(const float* s, const float* d, const float* c, float* acc)
{
    const float a[3] = {s[0] - c[0], s[1] - c[1], s[2] - c[2]}, b[3] = {d[0] - c[3], d[1] - c[4], d[2] - c[5]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 * i + j] = acc[3 * i + j] + a[i] * b[j];
}

// rule 3: Horn's matrix, quaternion order (w, x, y, z); M = (Sxx Sxy Sxz Syx Syy Syz Szx Szy Szz)
SLHIP_HD void horn(const float* M, float N[4][4])
{
    const float Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
    N[0][0] = (Sxx + Syy) + Szz;
    N[1][1] = (Sxx - Syy) - Szz;
    N[2][2] = (Syy - Sxx) - Szz;
    N[3][3] = (Szz - Sxx) - Syy;
    N[0][1] = N[1][0] = Syz - Szy;
    N[0][2] = N[2][0] = Szx - Sxz;
    N[0][3] = N[3][0] = Sxy - Syx;
    N[1][2] = N[2][1] = Sxy + Syx;
    N[1][3] = N[3][1] = Szx + Sxz;
    N[2][3] = N[3][2] = Syz + Szy;
}

// rule 3: one rotation of the pair (p, q), p < q, of symmetric A with the eigenvector columns in V.  An off-diagonal of exactly
// 0 is skipped.  theta = (aqq - app) / (2 apq), t = sign(theta) / (|theta| + sqrtf(theta * theta + 1)) (sign(0) = +1; an
// infinite theta gives t = 0: nothing turns), c = 1 / sqrtf(t * t + 1), s = t * c.
template <int p, int q>
SLHIP_HD void rotate(float A[4][4], float V[4][4])
{
    const float apq = A[p][q];
    if (apq == 0.0f) return;
    const float theta = (A[q][q] - A[p][p]) / (2.0f * apq);
    const float r = fabsf(theta) + sqrtf(theta * theta + 1.0f);
    const float t = (theta < 0.0f ? -1.0f : 1.0f) / r;
    const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
    A[p][p] = A[p][p] - t * apq;
    A[q][q] = A[q][q] + t * apq;
    A[p][q] = A[q][p] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k != p && k != q) {
            const float akp = A[k][p], akq = A[k][q];
            A[k][p] = A[p][k] = c * akp - s * akq;
            A[k][q] = A[q][k] = s * akp + c * akq;
        }
        const float vkp = V[k][p], vkq = V[k][q];
        V[k][p] = c * vkp - s * vkq;
        V[k][q] = s * vkp + c * vkq;
    }
}

// rule 3: SWEEPS cyclic sweeps; on return the diagonal of A holds the eigenvalues and column i of V the eigenvector of A[i][i]
SLHIP_HD void jacobi(float A[4][4], float V[4][4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) V[i][j] = i == j ? 1.0f : 0.0f;
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        rotate<0, 1>(A, V);
        rotate<0, 2>(A, V);
        rotate<0, 3>(A, V);
        rotate<1, 2>(A, V);
        rotate<1, 3>(A, V);
        rotate<2, 3>(A, V);
    }
}

// rules 4 to 6 (quaternion, pose, degeneracy): the pose from the eigen decomposition and the centroids c = {cs, cd}.  False
// (the pose is not written) when the two largest eigenvalues differ by no more than min_gap times the sum of the four absolute eigenvalues (collinear or coincident
// points: the rotation about their line is free), or when that comparison involves a NaN.
SLHIP_HD bool pose_of(const float A[4][4], const float V[4][4], const float* c, float min_gap, float* pose)
{
    const float e[4] = {A[0][0], A[1][1], A[2][2], A[3][3]};
    int best = 0;
    float largest = e[0];      // (kept beside its index: no array is indexed by a value known only at run time)
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (e[i] > largest) {      // the largest, ties to the lowest column
            largest = e[i];
            best = i;
        }
    float second = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i != best && e[i] > second) second = e[i];
    const float scale = ((fabsf(e[0]) + fabsf(e[1])) + fabsf(e[2])) + fabsf(e[3]);
    if (!(largest - second > min_gap * scale)) return false;
    float q[4];      // column `best` of V, picked value by value (a pointer picked at run time would send V to memory)
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = best == 0 ? V[k][0] : best == 1 ? V[k][1] : best == 2 ? V[k][2] : V[k][3];
    const float n = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const float sgn = q[0] < 0.0f ? -1.0f : 1.0f;
    const float w = (q[0] / n) * sgn, x = (q[1] / n) * sgn, y = (q[2] / n) * sgn, z = (q[3] / n) * sgn;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    pose[0] = 1.0f - 2.0f * (yy + zz); pose[1] = 2.0f * (xy - wz);        pose[2] = 2.0f * (xz + wy);
    pose[4] = 2.0f * (xy + wz);        pose[5] = 1.0f - 2.0f * (xx + zz); pose[6] = 2.0f * (yz - wx);
    pose[8] = 2.0f * (xz - wy);        pose[9] = 2.0f * (yz + wx);        pose[10] = 1.0f - 2.0f * (xx + yy);
#pragma unroll
    for (int i = 0; i < 3; ++i) pose[4 * i + 3] = c[3 + i] - ((pose[4 * i] * c[0] + pose[4 * i + 1] * c[1]) + pose[4 * i + 2] * c[2]);
    return true;
}

// rule 7: |R s + t - d|^2 of one correspondence
SLHIP_HD float residual2(const float* pose, const float* s, const float* d)
{
    const float rx = row_point(pose, s[0], s[1], s[2]) - d[0], ry = row_point(pose + 4, s[0], s[1], s[2]) - d[1];
    const float rz = row_point(pose + 8, s[0], s[1], s[2]) - d[2];
    return (rx * rx + ry * ry) + rz * rz;
}

}  // namespace slhip_fit
