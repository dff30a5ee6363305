// Counter-based random numbers for libfgcn: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
// SC'11).  One call maps a 128-bit counter and a 64-bit key to four 32-bit words; it has no state, so a kernel forms the words of
// element i from i alone and the host recomputes them bit for bit (fgcn_philox4x32_10, include/fgcn.h).
#pragma once
#include <hip/hip_runtime.h>

namespace fgcn {

struct philox4 {
    unsigned w[4];
};

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // the round multipliers
constexpr unsigned PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // the key increments (golden ratio, sqrt(3) - 1)

// (c0, c1, c2, c3), (k0, k1) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), ten times, the key bumped after each round
__host__ __device__ inline philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0, p1 = (unsigned long long)PHILOX_M1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return philox4{{c0, c1, c2, c3}};
}

}  // namespace fgcn
