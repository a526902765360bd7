// slhip_rng.h -- counter-based RNG of the sensor models (slhip_camera.hip, slhip_depth_sensor.hip): Philox4x32-10 keyed by
// the image's seed, counted by (pixel, image), with the uniform / normal / Poisson draws on top.  Philox (also the jitter of
// slhip_object_crops.hip and the draws of slhip_object_points.hip) runs on host and device; Rng is device code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slhip {

struct Philox {
    uint32_t c[4], k[2];
    __host__ __device__ void round()
    {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1];
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    __host__ __device__ void block()
    {
#pragma unroll
        for (int i = 0; i < 10; ++i) round();
    }
};

struct Rng {
    uint32_t key0, key1, ctr0, ctr1, sub;
    uint32_t buf[4];
    int left;
    __device__ Rng(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1) : key0(k0), key1(k1), ctr0(c0), ctr1(c1), sub(0), left(0) {}
    __device__ uint32_t next()
    {
        if (left == 0) {
            Philox p;
            p.c[0] = ctr0; p.c[1] = ctr1; p.c[2] = sub++; p.c[3] = 0x5114EBE2u;
            p.k[0] = key0; p.k[1] = key1;
            p.block();
            buf[0] = p.c[0]; buf[1] = p.c[1]; buf[2] = p.c[2]; buf[3] = p.c[3];
            left = 4;
        }
        return buf[--left];
    }
    __device__ float uniform() { return ((float)(next() >> 8) + 0.5f) * (1.0f / 16777216.0f); }   // (0, 1]: 1 for the largest word
    __device__ float normal()
    {
        const float u1 = uniform(), u2 = uniform();
        return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
    }
    // log of the Poisson weight, -lambda + k log(lambda) - log(k!), for a whole k >= 0 and lambda >= 10.  Term by term its three
    // parts are of the size of lambda log(lambda) and cancel to O(1): in float32 that is noise from a rate of about 1e5 on (at 1e6
    // the variance of the draws came out 2 % low).  From k = 10 on it is therefore taken as a difference, with Stirling's series
    // for log(k!): k log(lambda / k) + (k - lambda) - log(2 pi k) / 2 - 1 / (12 k) + 1 / (360 k^3); the next term is below 1e-8.
    // Below 10 the terms are small and log(k!) is a table.
    __device__ static float log_weight(float k, float lambda)
    {
        const bool small = k < 10.0f;
        const float l = logf(small ? lambda : 6.28318530717958647692f * k);      // one logf for both branches of a wave
        if (small) {
            constexpr float log_factorial[10] = {0.0f,        0.0f,        0.693147182f, 1.79175949f, 3.17805386f,
                                                 4.7874918f,  6.57925129f, 8.52516174f,  10.6046028f, 12.8018274f};
            return -lambda + k * l - log_factorial[(int)k];
        }
        const float d = lambda - k, ik = 1.0f / k;
        const float series = ik * (0.0833333333f - 0.00277777778f * (ik * ik));
        return ((k * log1pf(d * ik) - d) - 0.5f * l) - series;
    }
    // Poisson(lambda): multiplication method below 10, Hoermann's transformed rejection (PTRS) above
    __device__ float poisson(float lambda)
    {
        if (!(lambda > 0.0f)) return 0.0f;
        if (lambda < 10.0f) {
            const float limit = expf(-lambda);
            float prod = uniform();
            int k = 0;
            while (prod > limit && k < 200) { prod *= uniform(); ++k; }
            return (float)k;
        }
        const float slam = sqrtf(lambda);
        const float b = 0.931f + 2.53f * slam, a = -0.059f + 0.02483f * b;
        const float inv_alpha = 1.1239f + 1.1328f / (b - 3.4f), vr = 0.9277f - 3.6224f / (b - 2.0f);
        for (int it = 0; it < 64; ++it) {
            const float U = uniform() - 0.5f, V = uniform();
            const float us = 0.5f - fabsf(U);
            const float k = floorf((2.0f * a / us + b) * U + lambda + 0.43f);
            if (us >= 0.07f && V <= vr) return k;
            if (k < 0.0f || (us < 0.013f && V > us)) continue;
            if (logf(V * inv_alpha / (a / (us * us) + b)) <= log_weight(k, lambda)) return k;   // V >= 2^-25, us too: no underflow
        }
        return floorf(lambda + 0.5f);
    }
};

}  // namespace slhip
