// slhip_region_rules.h -- the rules of the object regions (slhip_object_regions.hip) as plain float32 C++ for host and device
// alike: the kernels and the _host entries run the same functions, and tests/object_regions_ref.py restates them in NumPy.
// Every operation is one rounded IEEE operation (the build passes -ffp-contract=off); the parenthesisation is the contract
// (include/slhip.h, "Object regions").  Distances are slhip_kp::d2(point, centre), the one of the keypoint FPS.
#pragma once

#include "slhip_keypoint_rules.h"

namespace slhip_rg {

namespace kp = slhip_kp;

constexpr int NONE = 255;      // SLHIP_REGION_NONE

// The nearest centre so far: a scan upwards from region 0 that takes a centre only on a strict <, so among equals -- duplicated
// centres included -- the lowest index stays.  A NaN distance is never smaller, so it never wins; when nothing wins (every
// distance NaN or +inf) the answer is region 0.
struct Near {
    float val;
    int idx;
};

SLHIP_HD Near near_start()
{
    Near b;
    b.val = __builtin_inff();
    b.idx = 0;
    return b;
}

SLHIP_HD Near near_offer(const Near& a, float d, int r)
{
    Near b;
    const bool win = d < a.val;
    b.val = win ? d : a.val;
    b.idx = win ? r : a.idx;
    return b;
}

// centres: the R float4 of one class
SLHIP_HD int nearest(const float* centres, unsigned R, const kp::P3& p)
{
    Near b = near_start();
    for (unsigned r = 0u; r < R; ++r) {
        kp::P3 c;
        c.x = centres[4u * r];
        c.y = centres[4u * r + 1u];
        c.z = centres[4u * r + 2u];
        b = near_offer(b, kp::d2(p, c), (int)r);
    }
    return b.idx;
}

// the object of a pixel, -1 for background and instances outside [1, n_objects]
SLHIP_HD int pixel_object(int instance, unsigned n_objects) { return instance >= 1 && (unsigned)instance <= n_objects ? instance - 1 : -1; }

SLHIP_HD bool class_ok(int cls, unsigned n_assets) { return cls >= 0 && (unsigned)cls < n_assets; }

SLHIP_HD bool point_ok(float x, float y, float z) { return kp::is_finite(x) && kp::is_finite(y) && kp::is_finite(z); }

// (x - cx, y - cy, z - cz, d2) against the winning centre: d2 is the very value the scan compared
struct Local {
    float dx, dy, dz, d2;
};

SLHIP_HD Local local_of(const kp::P3& p, const kp::P3& c)
{
    Local l;
    l.dx = p.x - c.x;
    l.dy = p.y - c.y;
    l.dz = p.z - c.z;
    l.d2 = kp::d2(p, c);
    return l;
}

// The extent of a region is a maximum over |dx|, |dy|, |dz| and d2 of its vertices, taken on the bit patterns with the sign
// cleared: for non-negative floats the order of the patterns is the order of the values, a NaN sorts above +inf, and an
// integer maximum does not depend on the order of its operands.
SLHIP_HD unsigned magnitude_bits(float v) { return __builtin_bit_cast(unsigned, v) & 0x7fffffffu; }

}  // namespace slhip_rg
