// slhip_align_rules.h -- the rules of the robust alignment (slhip_pose_align.hip) as plain float32 C++ for host and device alike:
// k_pose_align and slhip_pose_align_host run the same functions, so every output agrees bit for bit.  Every operation is one
// rounded IEEE operation (the build passes -ffp-contract=off); only + - * /, sqrtf, fabsf and comparisons appear.  The
// parenthesisation is the contract (include/slhip.h "Robust alignment", DESIGN.md "Robust alignment").
//
// RANSAC round the rigid fit of slhip_fit_rules.h: a hypothesis is Horn's fit of three picked correspondences, its score the
// number of valid correspondences whose squared residual lies within the threshold, and the winner is refitted on its inliers
// by slhip_fit_block.h.  What is new here is only the sample (rule 2), the fit of exactly three pairs in a fixed order (rule 3)
// and the inlier test (rule 4); which correspondences count, Horn's matrix, the Jacobi sweeps, the quaternion, min_gap and the
// residual are the fit's own functions, called as they stand.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_fit_rules.h"         // used, horn, jacobi, pose_of, residual2
#include "slhip_ransac_rules.h"      // pick, key_of, key_count, key_best
#include "slhip_rng.h"               // Philox

namespace slhip_align {

using slhip_fit::is_finite;
using slhip_ransac::key_best;
using slhip_ransac::key_count;
using slhip_ransac::key_of;
using slhip_ransac::pose_finite;

constexpr uint32_t BLOCK = slhip_fit::BLOCK;
constexpr uint32_t WAVE = slhip_fit::WAVE;
constexpr uint32_t STREAM = 9u;      // the Philox stream of the samples ("Randomness")

// rule 2: the three picks of hypothesis h among n_valid; false when two of them coincide (the hypothesis is void)
SLHIP_HD bool sample(uint32_t key0, uint32_t key1, uint32_t set_id, uint32_t h, uint32_t n_valid, uint32_t* idx)
{
    slhip::Philox p;
    p.c[0] = set_id; p.c[1] = STREAM; p.c[2] = h; p.c[3] = 0x51DE5EEDu;
    p.k[0] = key0; p.k[1] = key1;
    p.block();
    idx[0] = slhip_ransac::pick(p.c[0], n_valid);
    idx[1] = slhip_ransac::pick(p.c[1], n_valid);
    idx[2] = slhip_ransac::pick(p.c[2], n_valid);
    return idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2];
}

// rule 3: the fit's rules 2 to 6 on the three pairs (s[k], d[k]), every sum ((p0 + p1) + p2) from the first term on.  False when
// the sample is collinear or coincident (pose_of) or an entry of the pose is not finite.
SLHIP_HD bool minimal_fit(const float s[3][3], const float d[3][3], float min_gap, float* pose)
{
    float c[6], M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        c[i] = ((s[0][i] + s[1][i]) + s[2][i]) / 3.0f;
        c[3 + i] = ((d[0][i] + d[1][i]) + d[2][i]) / 3.0f;
    }
    float a[3][3], b[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a[k][i] = s[k][i] - c[i];
            b[k][i] = d[k][i] - c[3 + i];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = (a[0][i] * b[0][j] + a[1][i] * b[1][j]) + a[2][i] * b[2][j];
    float A[4][4], V[4][4];
    slhip_fit::horn(M, A);
    slhip_fit::jacobi(A, V);
    return slhip_fit::pose_of(A, V, c, min_gap, pose) && pose_finite(pose);
}

// rules 2 and 3: the pose of hypothesis h, false when it is void.  pick(i, s, d) hands out entry i of the valid list as the
// points s[3] and d[3]
template <class Pick>
SLHIP_HD bool hypothesis(uint32_t key0, uint32_t key1, uint32_t set_id, uint32_t h, uint32_t n_valid, float min_gap, Pick pick,
                         float* pose)
{
    uint32_t idx[3];
    if (!sample(key0, key1, set_id, h, n_valid, idx)) return false;
    float s[3][3], d[3][3];
    pick(idx[0], s[0], d[0]);
    pick(idx[1], s[1], d[1]);
    pick(idx[2], s[2], d[2]);
    return minimal_fit(s, d, min_gap, pose);
}

// rule 4: |R s + t - d|^2 <= threshold^2; a NaN residual (a NaN pose) compares false.  *e2: the squared residual
SLHIP_HD bool inlier(const float* M, float sx, float sy, float sz, float dx, float dy, float dz, float thr2, float* e2)
{
    const float s[3] = {sx, sy, sz}, d[3] = {dx, dy, dz};
    *e2 = slhip_fit::residual2(M, s, d);
    return *e2 <= thr2;
}

}  // namespace slhip_align
