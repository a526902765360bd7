// slhip_checks.h -- the argument checks that the per-object outputs share (slhip_object_*_check_params and their entries): one
// place per rule and per error text.  Host code; a failed check sets the error text and returns -1.
#pragma once

#include <stdint.h>

#include "slhip_common.h"

namespace slhip {

inline bool is_finite(float v) { return v - v == 0.0f; }

inline int check_intrinsics(const char* who, float fx, float fy, float cx, float cy)
{
    if (!(fx > 0.0f) || !(fy > 0.0f) || !is_finite(fx) || !is_finite(fy) || !is_finite(cx) || !is_finite(cy)) {
        set_error("%s: intrinsics (fx %g, fy %g, cx %g, cy %g): fx and fy must be positive, all four finite", who, (double)fx,
                  (double)fy, (double)cx, (double)cy);
        return -1;
    }
    return 0;
}

// a count `what` = v outside [lo, hi]
inline int check_range(const char* who, const char* what, uint32_t v, uint32_t lo, uint32_t hi)
{
    if (v < lo || v > hi) {
        set_error("%s: %s %u must be in [%u, %u]", who, what, v, lo, hi);
        return -1;
    }
    return 0;
}

// sides in [1, max_side] and at most max_pixels pixels (the modules word the failure differently: the text stays with them)
inline bool picture_fits(int W, int H, int max_side, uint64_t max_pixels)
{
    return W >= 1 && H >= 1 && W <= max_side && H <= max_side && (uint64_t)W * (uint64_t)H <= max_pixels;
}

// the picture of the keypoints and the regions
inline int check_picture_sides(const char* who, int W, int H)
{
    if (!picture_fits(W, H, 32768, ~0ull)) {
        set_error("%s: bad picture size %d x %d (each side 1..32768)", who, W, H);
        return -1;
    }
    return 0;
}

}  // namespace slhip
