// Seeded draws of everything after the AR model: the sampler's z (flow_matching.py:50) and HiFT's SineGen draws
// (generator.py:208-222), made inside the kernels that consume them and exported by svc_cfm_noise_draws /
// svc_hift_noise_draws (capi.hip) through the SAME device functions, so the two agree bit for bit.
//
// One rule: key = (seed low word, seed high word), counter = (pos, row / 4, domain, 0); output word row % 4 of that
// Philox4x32-10 call belongs to element (row, pos).  A draw is a pure function of (seed, domain, row, pos): batch row,
// padding, micro-batch, slot and neighbours never enter, and the first n positions of a row do not depend on the length
// asked for.  Domain 0 is the AR sampler's layout (ar_sampler.h, third counter word 0), so one seed may be handed to
// every stage of a request without a draw being used twice.
//   uniform  u = ((word >> 8) + 1) * 2^-24 in (0, 1], exact in fp32 (as the AR's)
//   normals  Box-Muller on word pairs: words (0, 1) -> rows 4q, 4q + 1 = r cos(2 pi u1), r sin(2 pi u1), r = sqrt(-2 ln u0);
//            words (2, 3) -> rows 4q + 2, 4q + 3.  |n| <= sqrt(48 ln 2) = 5.77
//   phase0   (2 u - 1) pi
#pragma once
#include "philox.h"

namespace svc {

enum { NOISE_CFM_Z = 1, NOISE_HIFT_SOURCE = 2, NOISE_HIFT_PHASE0 = 3 };

// The value as a rounded fp32 number: the consuming kernels go on computing with a draw (namp * noise, theta + phase0) where
// the exporter stores it, and a product contracted into the consumer's next operation would round differently.
__device__ __forceinline__ float noise_rounded(float v) {
    asm("" : "+v"(v));
    return v;
}

__device__ __forceinline__ float noise_uniform(unsigned word) { return (float)((word >> 8) + 1u) * 5.9604644775390625e-8f; }

// n[j] = the normal of (seed, domain, row 4 q + j, pos)
__device__ __forceinline__ void noise_normal4(unsigned long long seed, unsigned domain, unsigned q, unsigned pos, float (&n)[4]) {
    unsigned w[4];
    philox4x32_10(pos, q, domain, 0u, (unsigned)seed, (unsigned)(seed >> 32), w);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u0 = noise_uniform(w[2 * p]), u1 = noise_uniform(w[2 * p + 1]);
        const float r = sqrtf(-2.f * logf(u0));
        // cospif / sinpif of 2 u1 (exact in fp32): the argument of cosf(2 pi u1) would be rounded first
        n[2 * p] = noise_rounded(r * cospif(2.f * u1));
        n[2 * p + 1] = noise_rounded(r * sinpif(2.f * u1));
    }
}

// HiFT's SineGen phase of harmonic h (the entry of harmonic 0 is drawn and ignored, as generator.py:208-210 zeroes it)
__device__ __forceinline__ float noise_phase0(unsigned long long seed, int h) {
    unsigned w[4];
    philox4x32_10(0u, (unsigned)h >> 2, NOISE_HIFT_PHASE0, 0u, (unsigned)seed, (unsigned)(seed >> 32), w);
    const unsigned word = (h & 3) == 0 ? w[0] : (h & 3) == 1 ? w[1] : (h & 3) == 2 ? w[2] : w[3];
    return noise_rounded((2.f * noise_uniform(word) - 1.f) * 3.14159265358979323846f);     // 2 u - 1 is exact
}

namespace {

// out[b][h] = phase0 of (seeds[b], h); seeds null: B = 1 and the seed is `seed`
__global__ void noise_phase0_kernel(const unsigned long long* __restrict__ seeds, unsigned long long seed, int B, int NH,
                                    float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * NH) return;
    const int b = i / NH, h = i - b * NH;
    out[i] = noise_phase0(seeds ? seeds[b] : seed, h);
}

}  // namespace

}  // namespace svc
