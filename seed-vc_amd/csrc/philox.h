// Philox4x32-10 (Salmon et al., SC'11): the counter-based generator behind every seeded draw of the library -- the AR
// sampler's Exp(1) race (ar_sampler.h) and the sampler / HiFT noise (noise.h).  Four 32-bit words per call, a pure function
// of the 128-bit counter and the 64-bit key.
#pragma once
#include <hip/hip_runtime.h>

namespace svc {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace svc
