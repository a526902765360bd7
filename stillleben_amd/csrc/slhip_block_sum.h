// slhip_block_sum.h -- the sums of a workgroup of the pose family (pose_error, pose_pnp, keypoint_vote, keypoint_vote3d, pose_fit,
// pose_icp), host and device side by side.  The order is the arithmetic contract that makes every *_host twin equal its kernel
// bit for bit, and it is stated here once:
//   lane l of BLOCK starts from 0.0f and adds the terms of its items l, l + BLOCK, l + 2 BLOCK, ... in that order; a lane without
//   items keeps 0.0f.  The 64 lanes of a wave combine by the butterfly
//     for off = 32, 16, 8, 4, 2, 1:  v[l] = v[l] + v[l ^ off]      (all lanes at once: every lane ends with the wave's sum)
//   and the four waves as ((w0 + w1) + w2) + w3.
// Every operation is one rounded IEEE operation (the build passes -ffp-contract=off).
#pragma once

#include <stdint.h>

#include "slhip_mask_walk.h"      // SLHIP_HD

namespace slhip_pose {

constexpr uint32_t BLOCK = 256u;      // the lanes of a workgroup's sums
constexpr uint32_t WAVE = 64u;
static_assert(BLOCK / WAVE == 4u, "the sums combine four waves");

// the layouts that the kernels and their launches share
SLHIP_HD uint32_t pad4(uint32_t n) { return (n + 3u) & ~3u; }
SLHIP_HD uint32_t words_of(uint32_t K) { return (K + 31u) / 32u; }       // 32-bit words of K bits
SLHIP_HD uint32_t chunks_of(uint32_t K) { return (K + 63u) / 64u; }      // waves of K lanes
SLHIP_HD uint32_t pad_to_block(uint32_t n) { return (n + BLOCK - 1u) / BLOCK * BLOCK; }

// ((w0 + w1) + w2) + w3 of the four waves' values, `stride` words apart
template <class T>
SLHIP_HD T waves_sum(const T* w, uint32_t stride = 1u)
{
    return ((w[0] + w[stride]) + w[2u * stride]) + w[3u * stride];
}

// host: the workgroup's sum of lanes[BLOCK]
inline float block_sum(const float* lanes)
{
    float w[BLOCK / WAVE];
    for (uint32_t k = 0; k < BLOCK / WAVE; ++k) {
        float v[WAVE], n[WAVE];
        for (uint32_t l = 0; l < WAVE; ++l) v[l] = lanes[k * WAVE + l];
        for (uint32_t off = WAVE / 2u; off; off >>= 1) {
            for (uint32_t l = 0; l < WAVE; ++l) n[l] = v[l] + v[l ^ off];
            for (uint32_t l = 0; l < WAVE; ++l) v[l] = n[l];
        }
        w[k] = v[0];
    }
    return waves_sum(w);
}

// host: the N running sums of every lane.  add(j, f) lets item j meet its lane: f(acc) accumulates into the N sums of lane
// j % BLOCK; call it upwards in j, as a lane meets its items.  total(i) is the workgroup's sum i.
template <int N>
struct LaneSums {
    float lanes[N][BLOCK] = {};

    template <class F>
    void add(uint32_t j, F&& f)
    {
        float acc[N];
        for (int i = 0; i < N; ++i) acc[i] = lanes[i][j % BLOCK];
        f(acc);
        for (int i = 0; i < N; ++i) lanes[i][j % BLOCK] = acc[i];
    }
    float total(int i) const { return block_sum(lanes[i]); }
};

#ifdef __HIPCC__

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int off = 32; off; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}

// S[i] = the workgroup's sum of acc[i], i < N, through s_part[4 * STRIDE] (wave w writes row w of STRIDE words).  Two barriers: the
// sums are read before the next reduction writes them.
template <int N, int STRIDE>
__device__ __forceinline__ void block_sums(const float* acc, float* s_part, uint32_t wave, uint32_t lane, float* S)
{
    static_assert(N <= STRIDE, "a row of s_part holds the N sums");
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float w = wave_sum(acc[i]);
        if (lane == 0u) s_part[wave * STRIDE + i] = w;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) S[i] = waves_sum(s_part + i, STRIDE);
    __syncthreads();
}

// the workgroup's sum of every lane's count `mine` through s_cnt[4].  One barrier, behind the write: everything the workgroup
// wrote to LDS before the call can be read after it, and a barrier must lie between the return and the next write of s_cnt.
__device__ __forceinline__ uint32_t block_count(uint32_t mine, uint32_t* s_cnt, uint32_t wave, uint32_t lane)
{
    mine = wave_sum(mine);
    if (lane == 0u) s_cnt[wave] = mine;
    __syncthreads();
    return waves_sum(s_cnt);
}

#endif      // __HIPCC__

}  // namespace slhip_pose
