// slhip_fit_block.h -- the rigid fit of slhip_fit_rules.h over the pairs of one set, host and device side by side: k_pose_fit,
// k_pose_icp and their *_host twins differ only in where a pair comes from.  `pair` is bool pair(uint32_t j, float* s, float* d):
// the correspondence of item j < n as s[4] (source) and d[4] (destination), false when j has none.  The three passes are called
// one by one, because the callers differ between them: the fit counts its pairs in the first pass, ICP knows the count from its
// association; the fit sums the residuals of every pose, ICP of the last one only.
//   fit_centroids   rule 2, first pass: S[6] = the sums of s and of d over the pairs; returns the pairs the caller (a lane on the
//                   device, the whole set on the host) met
//   fit_pose        rule 2, second pass, and rules 3 to 6: the pose from S and the count of pairs; false when degenerate
//   fit_rms         rule 7: sqrt(sum |R s + t - d|^2 / count)
// Every sum is a sum of slhip_block_sum.h.  On the device all lanes of the workgroup call a pass together (it holds barriers) and
// all get the same result; s_part is FIT_SUMS * 4 words of LDS.
#pragma once

#include "slhip_block_sum.h"
#include "slhip_fit_rules.h"

namespace slhip_fit {

constexpr int FIT_SUMS = 9;      // the most sums of one reduction (the moments'), and the row stride of s_part

template <class Pair>
uint32_t fit_centroids_host(uint32_t n, Pair pair, float* S)
{
    slhip_pose::LaneSums<6> sums;
    uint32_t count = 0u;
    float s[4], d[4];
    for (uint32_t j = 0u; j < n; ++j) {
        if (!pair(j, s, d)) continue;
        ++count;
        sums.add(j, [&](float* acc) { accumulate_centroids(s, d, acc); });
    }
    for (int i = 0; i < 6; ++i) S[i] = sums.total(i);
    return count;
}

template <class Pair>
bool fit_pose_host(uint32_t n, Pair pair, const float* S, uint32_t count, float min_gap, float* pose)
{
    float c[6], M[9], s[4], d[4];
    for (int i = 0; i < 6; ++i) c[i] = S[i] / (float)count;
    slhip_pose::LaneSums<9> sums;
    for (uint32_t j = 0u; j < n; ++j)
        if (pair(j, s, d)) sums.add(j, [&](float* acc) { accumulate_moments(s, d, c, acc); });
    for (int i = 0; i < 9; ++i) M[i] = sums.total(i);
    float A[4][4], V[4][4];
    horn(M, A);
    jacobi(A, V);
    return pose_of(A, V, c, min_gap, pose);
}

template <class Pair>
float fit_rms_host(uint32_t n, Pair pair, const float* pose, uint32_t count)
{
    slhip_pose::LaneSums<1> sums;
    float s[4], d[4];
    for (uint32_t j = 0u; j < n; ++j)
        if (pair(j, s, d)) sums.add(j, [&](float* acc) { acc[0] = acc[0] + residual2(pose, s, d); });
    return sqrtf(sums.total(0) / (float)count);
}

#ifdef __HIPCC__

// lane l takes j = l, l + BLOCK, ... upwards
template <class Pair>
__device__ __forceinline__ uint32_t fit_centroids(uint32_t n, Pair pair, float* s_part, float* S)
{
    float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, s[4], d[4];
    uint32_t mine = 0u;
    for (uint32_t j = threadIdx.x; j < n; j += BLOCK) {
        if (!pair(j, s, d)) continue;
        ++mine;
        accumulate_centroids(s, d, acc);
    }
    slhip_pose::block_sums<6, FIT_SUMS>(acc, s_part, threadIdx.x / WAVE, threadIdx.x % WAVE, S);
    return mine;
}

// every lane runs the same eigen decomposition in registers and gets the same pose: nothing is broadcast
template <class Pair>
__device__ __forceinline__ bool fit_pose(uint32_t n, Pair pair, const float* S, uint32_t count, float min_gap, float* s_part, float* pose)
{
    float c[6], M[9], s[4], d[4];
#pragma unroll
    for (int i = 0; i < 6; ++i) c[i] = S[i] / (float)count;
    float acc[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t j = threadIdx.x; j < n; j += BLOCK)
        if (pair(j, s, d)) accumulate_moments(s, d, c, acc);
    slhip_pose::block_sums<9, FIT_SUMS>(acc, s_part, threadIdx.x / WAVE, threadIdx.x % WAVE, M);
    float A[4][4], V[4][4];
    horn(M, A);
    jacobi(A, V);
    return pose_of(A, V, c, min_gap, pose);
}

template <class Pair>
__device__ __forceinline__ float fit_rms(uint32_t n, Pair pair, const float* pose, uint32_t count, float* s_part)
{
    float acc[1] = {0.0f}, S[1], s[4], d[4];
    for (uint32_t j = threadIdx.x; j < n; j += BLOCK)
        if (pair(j, s, d)) acc[0] = acc[0] + residual2(pose, s, d);
    slhip_pose::block_sums<1, FIT_SUMS>(acc, s_part, threadIdx.x / WAVE, threadIdx.x % WAVE, S);
    return sqrtf(S[0] / (float)count);
}

#endif      // __HIPCC__

}  // namespace slhip_fit
