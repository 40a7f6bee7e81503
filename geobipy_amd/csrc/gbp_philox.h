// Philox4x32-10 (Salmon et al., SC'11) and the 53-bit uniform made of two of its words: the one definition the sampler
// (gbp_rjmcmc.h: counter = (chain, iteration, stream, draw)) and the section draws (gbp_section.h: counter = (realisation, row key low,
// row key high, 0)) share.  key = seed.  tests/rj_emul.py and geobipy_amd/sections.py philox_uniform state the same arithmetic.
#pragma once

#include <cstdint>

namespace rng {

struct U4 { uint32_t x, y, z, w; };

__host__ __device__ inline U4 philox(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

__host__ __device__ inline double u53(uint32_t a, uint32_t b)      // [0, 1) with 53 random bits
{
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

}  // namespace rng
