// philox.h -- Philox4x32-10, the counter-based generator behind the Poisson sampler (poisson.hip) and the HMC sampler (hmc.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ctpvae {

struct Philox4 {
    unsigned w[4];
};

__host__ __device__ inline void mulhilo32(unsigned a, unsigned b, unsigned &hi, unsigned &lo)
{
    const unsigned long long p = (unsigned long long)a * b;
    hi = (unsigned)(p >> 32);
    lo = (unsigned)p;
}

// Philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__host__ __device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        unsigned hi0, lo0, hi1, lo1;
        mulhilo32(0xD2511F53u, c0, hi0, lo0);
        mulhilo32(0xCD9E8D57u, c2, hi1, lo1);
        const unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0;
        c1 = n1;
        c2 = n2;
        c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

}  // namespace ctpvae
