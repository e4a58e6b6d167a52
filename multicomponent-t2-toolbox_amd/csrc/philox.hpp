// philox.hpp -- the counter-based generator of the Monte-Carlo kernels (met2_bootstrap.hip, met2_eval.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace met2 {

// Philox4x32-10 (Salmon et al., SC'11; the constants of Random123): 10 rounds, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ void philox4x32_10(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    }
}

// 53-bit uniforms from two 32-bit words: in [0, 1), and in (0, 1] (the Box-Muller radius takes its log)
__device__ __forceinline__ double u01_co(uint32_t a, uint32_t b) { return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * 0x1p-53; }
__device__ __forceinline__ double u01_oc(uint32_t a, uint32_t b) { return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 1.0) * 0x1p-53; }

}  // namespace met2
