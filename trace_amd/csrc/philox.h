// Stateless Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) for the device sampler.
// One call = one 10-round block of the counter (c0, c1, c2, c3) under the 64-bit key `seed`; the sampler uses word x of the counter
// (step, 0, row, 0), which is exactly the first rocrand() after rocrand_init(seed, row, 4 * step) of rocrand_philox4x32_10.h
// (tests/test_sampling_cpu.py checks that on the host).  Plain C++: compiles for the host and for gfx950.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define TRACE_HD __host__ __device__
#else
#define TRACE_HD
#endif

TRACE_HD inline uint32_t philox4x32_10_x(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)m1; c3 = (uint32_t)m0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// the sampler's uniform draw in [0, 1): 24 random bits of word x of counter (step, 0, row, 0)
TRACE_HD inline float philox_uniform(uint64_t seed, uint32_t step, uint32_t row) {
    return (float)(philox4x32_10_x(seed, step, 0u, row, 0u) >> 8) * (1.0f / 16777216.0f);
}
