// slhip_pose_rules.h -- the rules of the pose errors (slhip_pose_error.hip) as plain float32 C++ for host and device alike: the
// kernels and slhip_pose_error_host / slhip_pose_error_diameter_host run the same functions, and tests/pose_error_ref.py restates
// them in NumPy.  Every operation is one rounded IEEE operation (the build passes -ffp-contract=off, nothing here fuses); the
// parenthesisation is the contract (include/slhip.h, "Pose errors").
//
// The frame of the float32 arithmetic is the ground truth's object frame, reached through the difference of the two poses: per
// pose pair (g = ground truth, e = estimate, both 3 x 4 row-major)
//   D = e - g, all twelve entries: the rotations' difference and, in column 3, t_e - t_g -- the translations cancel before
//       anything is multiplied, and so do the rotations where they agree
//   w = D p, each row ((D0 * x + D1 * y) + D2 * z) + D3 (row_point of slhip_keypoint_rules.h): the camera-frame displacement
//       x_e(p) - x_g(p) of a bank point.  |w| is the ADD term: sqrt((w0 * w0 + w1 * w1) + w2 * w2)
//   v_i = (g[0][i] * w0 + g[1][i] * w1) + g[2][i] * w2: the displacement in the object frame (R_g^T w, R_g orthonormal: it
//       comes from the batch),  q = p + v per component: the point R_g^T (x_e(p) - t_g)
// ADD-S compares q_i with every p_j, MSSD with S_s p_i -- in that frame.  MSPD needs the camera: it projects e p_i and
// g (S_s p_i).  An estimate equal to the ground truth has D = 0, so w = v = 0 and q = p to the bit: every error is exactly 0.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_block_sum.h"           // BLOCK, WAVE, block_sum: the two means are sums in its order, / (float)count
#include "slhip_keypoint_rules.h"      // row_point, is_finite

namespace slhip_pose {

using slhip_kp::is_finite;
using slhip_kp::row_point;

constexpr int NONE = 0x7fffffff;

SLHIP_HD void difference(const float* g, const float* e, float* D)
{
#pragma unroll
    for (int i = 0; i < 12; ++i) D[i] = e[i] - g[i];
}

// a pose pair whose difference holds a NaN or an infinity has NaN errors and -1 indices
SLHIP_HD bool all_finite(const float* D)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && is_finite(D[i]);
    return ok;
}

struct Moved {
    float qx, qy, qz;      // q = p + R_g^T (D p)
    float add2;            // |D p|^2, the squared ADD term
};

SLHIP_HD Moved move_point(const float* g, const float* D, float x, float y, float z)
{
    const float w0 = row_point(D, x, y, z), w1 = row_point(D + 4, x, y, z), w2 = row_point(D + 8, x, y, z);
    Moved m;
    m.add2 = (w0 * w0 + w1 * w1) + w2 * w2;
    m.qx = x + ((g[0] * w0 + g[4] * w1) + g[8] * w2);
    m.qy = y + ((g[1] * w0 + g[5] * w1) + g[9] * w2);
    m.qz = z + ((g[2] * w0 + g[6] * w1) + g[10] * w2);
    return m;
}

// a class has points and symmetries when its counts lie inside the bank's rows; every other class gives +inf and -1
SLHIP_HD bool class_ok(int32_t count, uint32_t n_points, int32_t n_sym, uint32_t n_symmetries)
{
    return count >= 1 && (uint32_t)count <= n_points && n_sym >= 1 && (uint32_t)n_sym <= n_symmetries;
}

SLHIP_HD float dist2(float ax, float ay, float az, float bx, float by, float bz)
{
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

SLHIP_HD float pixel_u(float f, float X, float Z, float c) { return (f * X) / Z + c; }

SLHIP_HD float pixel_dist2(float ua, float va, float ub, float vb)
{
    const float du = ua - ub, dv = va - vb;
    return du * du + dv * dv;
}

// The arg-min over the symmetries: the smallest value, among equals the lowest index (a scan upwards with a strict <, in any
// grouping).  A scan starts from {+inf, NONE}; when nothing wins the index reads -1.
struct Best {
    float val;
    int idx;
};

SLHIP_HD Best best_start()
{
    Best b;
    b.val = __builtin_inff();
    b.idx = NONE;
    return b;
}

SLHIP_HD Best join(const Best& a, const Best& b) { return (b.val < a.val || (b.val == a.val && b.idx < a.idx)) ? b : a; }

SLHIP_HD int best_index(const Best& b) { return b.idx == NONE ? -1 : b.idx; }

}  // namespace slhip_pose
