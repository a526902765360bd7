// slhip_flow_rules.h -- the rules of the render flow (slhip_render_flow.hip) as plain float32 C++ for host and device alike:
// k_render_flow, k_flow_motion and their _host twins run the same functions, and tests/render_flow_ref.py restates them in NumPy.
// Every operation is one rounded IEEE operation (the build passes -ffp-contract=off); the parenthesisation is the contract
// (include/slhip.h, "Render flow").  row_point, project, is_finite and unoccluded are the keypoints' (slhip_keypoint_rules.h).
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"                    // slhip_render_flow_params, SLHIP_FLOW_*
#include "slhip_keypoint_rules.h"

namespace slhip_flow {

namespace kp = slhip_kp;

SLHIP_HD bool all_finite(const float* m, int n)
{
    for (int k = 0; k < n; ++k)
        if (!kp::is_finite(m[k])) return false;
    return true;
}

// (a*b + c*d) + e*f: the one order of every 3-term dot product here
SLHIP_HD float dot3(float a, float b, float c, float d, float e, float f) { return (a * b + c * d) + e * f; }

// The motion of one rigid frame between two pictures: out = to o inv_rigid(from), all three row-major 3 x 4 (rows 0-2 of a
// 4 x 4).  inv_rigid(R, t) = (R^T, -(R^T t)); the product's rotation by dot3, its translation by row_point.  `from` and `to` are
// ASSUMED rigid (R orthonormal) and not checked: for anything else R^T is not the inverse and the result is not a motion.  A
// non-finite entry among the 24 gives 12 NaNs, so that the pixels of that slot are not VALID.
SLHIP_HD void motion(const float* from, const float* to, float* out)
{
    if (!all_finite(from, 12) || !all_finite(to, 12)) {
        for (int k = 0; k < 12; ++k) out[k] = __builtin_nanf("");
        return;
    }
    float Ri[9], ti[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Ri[3 * r + c] = from[4 * c + r];
        ti[r] = -dot3(from[r], from[3], from[4 + r], from[7], from[8 + r], from[11]);
    }
    for (int r = 0; r < 3; ++r) {
        const float* m = to + 4 * r;
        for (int c = 0; c < 3; ++c) out[4 * r + c] = dot3(m[0], Ri[c], m[1], Ri[3 + c], m[2], Ri[6 + c]);
        out[4 * r + 3] = kp::row_point(m, ti[0], ti[1], ti[2]);
    }
}

// what one pixel of picture a gets
struct Pixel {
    float u, v;            // flow, pixels
    float x, y, z;         // scene flow, the unit of the depth
    unsigned flags;        // SLHIP_FLOW_VALID | _INSIDE | _VISIBLE
};

// Pixel (x, y) of picture a with depth z and instance i.  `table`: the scene's motion table [n_slots, 3, 4] (LDS on the
// device).  depth_b / inst_b: pixel 0 of the same scene of picture b (NULL: no VISIBLE / no instance condition), depth_b read
// at pixel * stride_b.
SLHIP_HD Pixel pixel(const slhip_render_flow_params& p, int x, int y, float z, unsigned i, const float* table, const float* depth_b,
                     unsigned stride_b, const uint16_t* inst_b)
{
    Pixel r;
    r.u = r.v = r.x = r.y = r.z = 0.0f;
    r.flags = 0u;
    if (!(kp::is_finite(z) && z > 0.0f && z < p.max_depth) || i >= p.n_slots) return r;
    const float* M = table + 12u * i;
    if (!all_finite(M, 12)) return r;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float X = ((px - p.cx) * z) / p.fx;
    const float Y = ((py - p.cy) * z) / p.fy;
    const kp::Projected q = kp::project(M, X, Y, z, p.fx, p.fy, p.cx, p.cy, p.W, p.H);
    if (!(q.flags & 1u)) return r;
    r.flags = SLHIP_FLOW_VALID;
    r.u = q.u - px;
    r.v = q.v - py;
    r.x = q.X - X;
    r.y = q.Y - Y;
    r.z = q.Z - z;
    if (!(q.flags & 2u)) return r;
    r.flags |= SLHIP_FLOW_INSIDE;
    if (!depth_b) return r;
    // the bilinear footprint of (u, v): 0 <= u < W gives -1 <= x0 <= W - 1, so only the four tests below clip it
    const int x0 = (int)floorf(q.u - 0.5f), y0 = (int)floorf(q.v - 0.5f);
    const float tol = p.depth_tol + p.depth_rel * q.Z;
    const bool match = (p.flags & SLHIP_FLOW_MATCH_INSTANCE) && inst_b;
    for (int k = 0; k < 4; ++k) {      // (0,0), (1,0), (0,1), (1,1)
        const int xx = x0 + (k & 1), yy = y0 + (k >> 1);
        if (xx < 0 || xx >= p.W || yy < 0 || yy >= p.H) continue;
        const size_t at = (size_t)yy * (size_t)p.W + (size_t)xx;
        if (match && inst_b[at] != i) continue;
        if (kp::unoccluded(q.Z, depth_b[at * stride_b], tol)) {
            r.flags |= SLHIP_FLOW_VISIBLE;
            break;
        }
    }
    return r;
}

}  // namespace slhip_flow
