// slhip_ransac_rules.h -- the rules that the RANSAC workgroup (slhip_ransac_block.h) and its two problems share, as plain C++ for
// host and device alike: the uniform of a Philox word, the pick of one of n list entries by it, the arg-max key of a scored slot
// and the test of a caller's pose.
// Slot 0 is the caller's pose, slot h + 1 hypothesis h; the key orders by the highest count, then the lowest slot, so the
// caller's pose wins ties and every real slot has a key of its own (include/slhip.h "Pose PnP", "Robust alignment").
#pragma once

#include <stdint.h>

#include "slhip_mask_walk.h"      // SLHIP_HD

namespace slhip_ransac {

constexpr int SLOT_BITS = 13;      // arg-max key: (count << 13) | (4097 - slot); counts reach 4096, slots 4096

// include/slhip.h "Randomness": uniform = ((x >> 8) + 0.5) * 2^-24
SLHIP_HD float uniform(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// the pick rule: min(n - 1, (uint32_t)(uniform(x) * (float)n)), float32 throughout
SLHIP_HD uint32_t pick(uint32_t x, uint32_t n)
{
    const uint32_t i = (uint32_t)(uniform(x) * (float)n);
    return i < n - 1u ? i : n - 1u;
}

SLHIP_HD uint32_t key_of(uint32_t count, uint32_t slot) { return (count << SLOT_BITS) | (4097u - slot); }
SLHIP_HD uint32_t key_count(uint32_t key) { return key >> SLOT_BITS; }
SLHIP_HD int key_best(uint32_t key) { return (int)(4097u - (key & ((1u << SLOT_BITS) - 1u))) - 1; }

// every entry of a pose is finite
SLHIP_HD bool pose_finite(const float* M)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 12; ++i) ok = ok && M[i] - M[i] == 0.0f;
    return ok;
}

}  // namespace slhip_ransac
