// slhip_scan.h -- the scan step of the device-side compactions (slhip_object_crops_select, slhip_object_points_select): per-scene
// counts to the offsets at which the scenes write their records.  Device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slhip {

// counts[0 .. n) -> exclusive offsets in place, counts[n] = the total.  One block of 1024; n may exceed it (carry).
// (a template only so that every file that launches it may hold a copy)
template <int BLOCK = 1024>
__global__ __launch_bounds__(BLOCK) void k_scan_counts(unsigned long long* __restrict__ counts, uint32_t n)
{
    __shared__ unsigned long long s[BLOCK];
    unsigned long long carry = 0ull;
    for (uint32_t i0 = 0u; i0 < n; i0 += (uint32_t)BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        const unsigned long long v = i < n ? counts[i] : 0ull;
        s[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1u; d < (uint32_t)BLOCK; d <<= 1) {
            const unsigned long long add = threadIdx.x >= d ? s[threadIdx.x - d] : 0ull;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n) counts[i] = carry + s[threadIdx.x] - v;
        carry += s[BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0u) counts[n] = carry;
}

}  // namespace slhip
