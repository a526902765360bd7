// slhip_checks.h -- the argument checks that the per-object outputs and the pose family share (slhip_*_check_params and their
// entries): one place per rule and per error text.  Host code; a failed check sets the error text and returns -1.
#pragma once

#include <stdint.h>

#include <initializer_list>

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

// the fit's min_gap: in [0, 1), and no NaN
inline int check_min_gap(const char* who, float min_gap)
{
    if (!(min_gap >= 0.0f) || !(min_gap < 1.0f)) {
        set_error("%s: min_gap %g must lie in [0, 1)", who, (double)min_gap);
        return -1;
    }
    return 0;
}

// One optional output of a module's output record: the bit of `outputs` that names it and its pointer.  The two checks below take
// the whole record as a brace list: const slhip::OutputList outputs = {{SLHIP_X_OUT_A, out->a}, {SLHIP_X_OUT_B, out->b}, ...};
// (or as any other range of NamedOutput, such as a std::array that a function returns)
struct NamedOutput {
    uint32_t bit;
    const void* ptr;
};
using OutputList = std::initializer_list<NamedOutput>;

template <class List>
int check_outputs_present(const char* who, uint32_t outputs, const List& all)
{
    for (const NamedOutput& o : all)
        if ((outputs & o.bit) && !o.ptr) {
            set_error("%s: an output named in `outputs` (0x%x) has a null pointer", who, outputs);
            return -1;
        }
    return 0;
}

template <class List>
int check_outputs_aligned(const char* who, uint32_t outputs, const List& all)
{
    for (const NamedOutput& o : all)
        if ((outputs & o.bit) && ((uintptr_t)o.ptr & 3u)) {
            set_error("%s: every output must be 4-byte aligned", who);
            return -1;
        }
    return 0;
}

}  // namespace slhip
