// slhip_keypoint_rules.h -- the rules of the object keypoints (slhip_object_keypoints.hip) as plain float32 C++ for host and
// device alike: the kernels and slhip_object_keypoints_fps_host run the same functions, and tests/object_keypoints_ref.py restates
// them in NumPy.  Every operation is one rounded IEEE operation (the build passes -ffp-contract=off); the parenthesisation is the
// contract (include/slhip.h, "Object keypoints").
#pragma once

#include <stdint.h>

#include "slhip.h"                // slhip_asset, slhip_draw
#include "slhip_mask_walk.h"      // SLHIP_HD

namespace slhip_kp {

struct P3 {
    float x, y, z;
};

// row r of a row-major 4 x 4 (or 3 x 4) matrix applied to (x, y, z, 1)
SLHIP_HD float row_point(const float* m, float x, float y, float z) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3]; }

// a mesh vertex in the object frame, the frame of the `coord` target
SLHIP_HD P3 object_point(const float* mesh_to_object, float x, float y, float z)
{
    P3 p;
    p.x = row_point(mesh_to_object, x, y, z);
    p.y = row_point(mesh_to_object + 4, x, y, z);
    p.z = row_point(mesh_to_object + 8, x, y, z);
    return p;
}

// The vertices of class a: [*base, *base + *n) of the pool, none when the class has no draw, its template or its vertices lie
// outside the tables, or it has more vertices than the scratch row holds.
SLHIP_HD void class_vertices(const slhip_asset& a, const slhip_draw* templates, uint32_t n_templates, uint64_t n_vertices,
                             uint64_t max_verts, uint64_t* base, uint32_t* n)
{
    *base = 0u;
    *n = 0u;
    if (a.draw_count == 0u || a.n_verts == 0u || a.draw_begin >= n_templates) return;
    const uint64_t b = templates[a.draw_begin].vtx_base;
    if (b + a.n_verts > n_vertices || a.n_verts > max_verts) return;
    *base = b;
    *n = a.n_verts;
}

SLHIP_HD P3 bbox_centre(const float* bbox_min, const float* bbox_max)
{
    P3 o;
    o.x = (bbox_min[0] + bbox_max[0]) * 0.5f;
    o.y = (bbox_min[1] + bbox_max[1]) * 0.5f;
    o.z = (bbox_min[2] + bbox_max[2]) * 0.5f;
    return o;
}

SLHIP_HD float d2(const P3& a, const P3& b)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// min(a, b) of the FPS update: b only when it is smaller, so a NaN on either side changes nothing
SLHIP_HD float keep_min(float a, float b) { return b < a ? b : a; }

// The farthest vertex so far: the largest value, among equals the lowest index.  A scan starts from {-inf, NONE}; a vertex
// enters by `offer`, two partial scans join by `join` -- both give what one scan upwards with a strict > gives, in any order.
// A NaN is never larger, so it never wins; when nothing was offered (or only NaNs) the answer is vertex 0.
constexpr int NONE = 0x7fffffff;

struct Best {
    float val;
    int idx;
};

SLHIP_HD Best best_start()
{
    Best b;
    b.val = -__builtin_inff();
    b.idx = NONE;
    return b;
}

SLHIP_HD Best join(const Best& a, const Best& b) { return (b.val > a.val || (b.val == a.val && b.idx < a.idx)) ? b : a; }

SLHIP_HD Best offer(const Best& a, float val, int idx)
{
    Best b;
    b.val = val;
    b.idx = idx;
    return join(a, b);
}

SLHIP_HD int best_index(const Best& b) { return b.idx == NONE ? 0 : b.idx; }

SLHIP_HD bool is_finite(float v) { return v - v == 0.0f; }

// projection of a bank point by rows 0-2 of object_to_camera and the intrinsics
struct Projected {
    float X, Y, Z, u, v;
    unsigned flags;      // SLHIP_KEYPOINT_IN_FRONT | SLHIP_KEYPOINT_INSIDE (the depth test is the caller's)
};

SLHIP_HD Projected project(const float* o2c, float x, float y, float z, float fx, float fy, float cx, float cy, int W, int H)
{
    Projected r;
    r.X = row_point(o2c, x, y, z);
    r.Y = row_point(o2c + 4, x, y, z);
    r.Z = row_point(o2c + 8, x, y, z);
    r.u = r.v = 0.0f;
    r.flags = 0u;
    if (is_finite(r.X) && is_finite(r.Y) && is_finite(r.Z) && r.Z > 0.0f) {
        r.flags = 1u;
        r.u = (fx * r.X) / r.Z + cx;
        r.v = (fy * r.Y) / r.Z + cy;
        if (r.u >= 0.0f && r.u < (float)W && r.v >= 0.0f && r.v < (float)H) r.flags |= 2u;
    } else {
        r.X = r.Y = r.Z = 0.0f;
    }
    return r;
}

// unoccluded: the plane's z under the keypoint is finite and positive and the keypoint is not behind it by more than tol
SLHIP_HD bool unoccluded(float Z, float z_plane, float tol) { return is_finite(z_plane) && z_plane > 0.0f && Z <= z_plane + tol; }

}  // namespace slhip_kp
