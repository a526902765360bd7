// slhip_vote3d_rules.h -- the rules of the keypoint voting in 3D (slhip_keypoint_vote3d.hip) as plain float32 C++ for host and
// device alike: k_keypoint_vote3d and slhip_keypoint_vote3d_host run the same functions, so every output agrees bit for bit.
// Every operation is one rounded IEEE operation (the build passes -ffp-contract=off); only + - * / and comparisons appear
// -- no expf: the kernel of the mean shift is the compact w = 1 - t, not a Gaussian.  The parenthesisation is the contract
// (include/slhip.h "Keypoint voting in 3D", DESIGN.md "Keypoint voting in 3D").
//
// A voter is a point of the object in the camera frame with a predicted offset to a keypoint; its candidate is their sum.  The
// candidates of one (set, keypoint) are clustered by mean shift from seeds that are candidates themselves, every sum of a step
// taken over the valid candidates one after the other in rising order -- which is what lets a lane be a seed.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slhip.h"
#include "slhip_pose_rules.h"      // is_finite, BLOCK, WAVE, block_sum

namespace slhip_vote3d {

using slhip_pose::is_finite;

constexpr uint32_t BLOCK = slhip_pose::BLOCK;
constexpr uint32_t WAVE = slhip_pose::WAVE;
constexpr int S_BITS = 11;              // arg-max key: (support << 11) | (1024 - s); support <= 4096, so the key fits 24 bits

struct P {
    float x, y, z;
};

// rule 1: the candidate of a voter; false when the voter does not count
SLHIP_HD bool candidate(float cam_x, float cam_y, float cam_z, float cam_w, float ox, float oy, float oz, P* c)
{
    if (!(cam_w != 0.0f)) return false;
    c->x = cam_x + ox;
    c->y = cam_y + oy;
    c->z = cam_z + oz;
    return is_finite(c->x) && is_finite(c->y) && is_finite(c->z);
}

// rule 2: the seeds.  (2 s + 1) n_valid <= 2047 * 4096 fits 32 bits; the rank is < n_valid because 2 s + 1 < 2 S_eff
SLHIP_HD uint32_t n_seeds_of(uint32_t S, uint32_t n_valid) { return S < n_valid ? S : n_valid; }
SLHIP_HD uint32_t seed_rank(uint32_t s, uint32_t n_valid, uint32_t S_eff) { return ((2u * s + 1u) * n_valid) / (2u * S_eff); }

SLHIP_HD float inv_h2_of(float h) { return 1.0f / (h * h); }

// rule 3: the four terms of candidate c in the step of seed x: acc = {sum w, sum w dx, sum w dy, sum w dz}
SLHIP_HD void accumulate_shift(const P& x, float cx, float cy, float cz, float inv_h2, float* acc)
{
    const float dx = cx - x.x, dy = cy - x.y, dz = cz - x.z;
    const float t = ((dx * dx + dy * dy) + dz * dz) * inv_h2;
    const float w = t < 1.0f ? 1.0f - t : 0.0f;
    acc[0] = acc[0] + w;
    acc[1] = acc[1] + w * dx;
    acc[2] = acc[2] + w * dy;
    acc[3] = acc[3] + w * dz;
}

// rule 3: x' = x + m, m = (sum w d) / (sum w); true when the seed stops: |m|^2 <= tol^2 (|x' - x|^2 is taken on m itself, before
// it is added).  sum w > 0 in exact arithmetic: the first step has the seed's own candidate at t = 0, w = 1; after a step, x' is
// the weighted mean of the candidates inside the band round x, so sum w |c - x'|^2 <= sum w |c - x|^2 < (sum w) h^2 and at least
// one of them has |c - x'|^2 < h^2, t < 1, w > 0.  Rounding could defeat this only with every weighted candidate within a
// rounding of the band's edge; then m is 0 / 0 = NaN, x stays NaN, no comparison holds, the seed runs its max_iters steps and
// ends with support 0 -- nothing is divided that a loop or an index depends on.
SLHIP_HD bool advance(P* x, const float* acc, float tol2)
{
    const float mx = acc[1] / acc[0], my = acc[2] / acc[0], mz = acc[3] / acc[0];
    x->x = x->x + mx;
    x->y = x->y + my;
    x->z = x->z + mz;
    return (mx * mx + my * my) + mz * mz <= tol2;
}

// rule 4: candidate c supports x; h2 = h * h
SLHIP_HD bool supports(const P& x, float cx, float cy, float cz, float h2)
{
    const float dx = cx - x.x, dy = cy - x.y, dz = cz - x.z;
    return (dx * dx + dy * dy) + dz * dz <= h2;
}

SLHIP_HD uint32_t key_of(uint32_t support, uint32_t s) { return (support << S_BITS) | (1024u - s); }
SLHIP_HD uint32_t key_support(uint32_t key) { return key >> S_BITS; }
SLHIP_HD int key_best(uint32_t key) { return (int)(1024u - (key & ((1u << S_BITS) - 1u))); }

// rule 5: the terms of a supporter.  The sums of rule 5 run in the order of the pose errors' means over the valid list: lane
// i % 256 takes its supporters i in rising order from 0.0f, the butterfly in a wave, ((w0 + w1) + w2) + w3.
SLHIP_HD void accumulate_mean(float cx, float cy, float cz, float* acc)
{
    acc[0] = acc[0] + cx;
    acc[1] = acc[1] + cy;
    acc[2] = acc[2] + cz;
}

// xx, xy, xz, yy, yz, zz about the mean
SLHIP_HD void accumulate_cov(float cx, float cy, float cz, const P& mean, float* acc)
{
    const float gx = cx - mean.x, gy = cy - mean.y, gz = cz - mean.z;
    acc[0] = acc[0] + gx * gx;
    acc[1] = acc[1] + gx * gy;
    acc[2] = acc[2] + gx * gz;
    acc[3] = acc[3] + gy * gy;
    acc[4] = acc[4] + gy * gz;
    acc[5] = acc[5] + gz * gz;
}

}  // namespace slhip_vote3d
