// slhip_icp_rules.h -- the rules of the ICP refinement (slhip_pose_icp.hip) as plain float32 C++ for host and device alike:
// k_pose_icp and slhip_pose_icp_host run the same functions, so every output agrees bit for bit.  Every operation is one rounded
// IEEE operation (the build passes -ffp-contract=off); only + - * /, sqrtf, fabsf and comparisons appear.  The parenthesisation
// is the contract (include/slhip.h "ICP", DESIGN.md "ICP").
//
// ICP is the loop round two rules that exist: the nearest bank point of the pose errors' ADD-S (slhip_pose_rules.h: dist2, the
// scan upwards with a strict <) and Horn's closed-form fit (slhip_fit_rules.h, used unchanged).  The bank stays where it is: the
// camera points go into the object frame with the current pose, and every fit gives a new absolute pose from the pairs -- poses
// are never composed, so rounding cannot accumulate into a rotation that is no rotation.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_fit_rules.h"       // the fit: accumulate_centroids, accumulate_moments, horn, jacobi, pose_of, residual2
#include "slhip_pose_rules.h"      // dist2, is_finite, NONE, BLOCK, WAVE, block_sum

namespace slhip_icp {

using slhip_pose::dist2;
using slhip_pose::is_finite;

constexpr uint32_t BLOCK = slhip_pose::BLOCK;      // the lanes of a set's sums: lane l takes camera points l, l + 256, ... upwards
constexpr uint32_t WAVE = slhip_pose::WAVE;
constexpr int NONE = slhip_pose::NONE;             // no index has won yet

// rule 1: the number of points of class `cls`, 0 when the set cannot start for its class
SLHIP_HD uint32_t class_count(int32_t cls, uint32_t n_assets, const int32_t* count, uint32_t n_points)
{
    if (cls < 0 || (uint32_t)cls >= n_assets) return 0u;
    const int32_t c = count[cls];
    return (c >= 1 && (uint32_t)c <= n_points) ? (uint32_t)c : 0u;
}

// rule 1: the 12 entries of the initial pose are finite
SLHIP_HD bool init_ok(const float* init)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && is_finite(init[i]);
    return ok;
}

// rule 2: camera point c = (x, y, z, w) counts
SLHIP_HD bool counts(float x, float y, float z, float w) { return w != 0.0f && is_finite(x) && is_finite(y) && is_finite(z); }

// rule 3: q = R^T (c - t), the camera point in the object frame of pose (3 x 4 row-major)
SLHIP_HD void to_object(const float* pose, float x, float y, float z, float& qx, float& qy, float& qz)
{
    const float d0 = x - pose[3], d1 = y - pose[7], d2 = z - pose[11];
    qx = (pose[0] * d0 + pose[4] * d1) + pose[8] * d2;
    qy = (pose[1] * d0 + pose[5] * d1) + pose[9] * d2;
    qz = (pose[2] * d0 + pose[6] * d1) + pose[10] * d2;
}

// rule 4: one step of the scan upwards over the bank points: point m at squared distance d replaces the best on a strict <
// (a NaN and a +inf never win; among equals the lowest index stays).  A scan starts from best = +inf, at = NONE.
SLHIP_HD void take(float d, int m, float& best, int& at)
{
    if (d < best) {
        best = d;
        at = m;
    }
}

// rule 5: the pair counts (gate = +inf passes every distance that won; a NaN gate fails)
SLHIP_HD bool paired(bool point_counts, int at, float best, float gate) { return point_counts && at != NONE && best <= gate * gate; }

// rule 5: the gate of the next association
SLHIP_HD float next_gate(float gate, float dist_scale, float min_dist)
{
    const float g = gate * dist_scale;
    return g > min_dist ? g : min_dist;
}

// rule 8: no entry moved by more than its tolerance (a NaN entry: not converged)
SLHIP_HD bool converged(const float* before, const float* after, float tol_rot, float tol_trans)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && fabsf(after[i] - before[i]) <= ((i & 3) == 3 ? tol_trans : tol_rot);
    return ok;
}

}  // namespace slhip_icp
