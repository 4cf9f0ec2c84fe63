// philox.h -- Philox4x32-10, the counter-based generator of the synthetic-matrix generator
// (synth.hip) and of the FlexMF negative sampler (flexmf.hip): 128-bit counter + 64-bit key ->
// 4 x 32 random bits, a pure function of (key, counter), so a draw never depends on scheduling.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace lk {

struct Philox {
    uint32_t k0, k1;
    __device__ __forceinline__ void round(uint32_t (&c)[4], uint32_t ka, uint32_t kb) const
    {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ ka;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ kb;
        c[1] = (uint32_t)p1;
        c[3] = (uint32_t)p0;
        c[0] = n0;
        c[2] = n2;
    }
    // Philox4x32-10: 128-bit counter -> 4 x 32 random bits
    __device__ __forceinline__ void operator()(uint32_t (&c)[4]) const
    {
        uint32_t a = k0, b = k1;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            round(c, a, b);
            a += 0x9E3779B9u;
            b += 0xBB67AE85u;
        }
    }
};

}  // namespace lk
