// The polyphase dot product of the resampler, shared by `svc_resample` (resample.hip), `svc_rt_push`
// (rt_audio.hip) and `svc_rt_out` (sola.hip): the handle, the tile geometry and the ONE statement of an output's FMA chain.  All
// three kernels stage an input span in LDS and call `rs_dot4` on it, so a sample of a real-time context and the same sample of a one-shot conversion run
// the same instructions in the same order.
#pragma once
#include "model_util.h"

namespace svc {

constexpr int RS_THREADS = 256;
constexpr int RS_ROWS = 4;                  // outputs per work item, one phase in four periods

struct RsGeom {
    int o, n, width, ntaps;
    int G;                                  // periods per row group: a tile is RS_ROWS * G periods = RS_ROWS * G * n outputs
    int fmin;                               // min first[j]: the tile's span starts at period * o + fmin - width
    int span;                               // floats of LDS: (RS_ROWS G - 1) o + (fmax - fmin) + ntaps + 3, rounded up to 4
};

// Work item w = g n + j of a tile: phase j of the periods g + G r, r = 0 .. 3 (S = G n work items; its outputs lie S apart).
// xs holds the tile's span from input position (first period) * o + fmin - width - shift on; taps_kn is [ntaps][n], so adjacent
// lanes read adjacent words.  One tap load feeds four chains; every chain is ascending k, one fmaf per tap, from 0.0f.
__device__ __forceinline__ void rs_dot4(const float* __restrict__ xs, int shift, const RsGeom& q, const float* __restrict__ taps_kn,
                                        const int* __restrict__ first, int w, float& a0, float& a1, float& a2, float& a3) {
    const int g = w / q.n, j = w - g * q.n;
    const int step = q.G * q.o;
    const float* s0 = xs + g * q.o + first[j] - q.fmin + shift;
    const float* tp = taps_kn + j;
    a0 = 0.f; a1 = 0.f; a2 = 0.f; a3 = 0.f;
#pragma unroll 4
    for (int k = 0; k < q.ntaps; ++k) {                     // ascending k, one FMA chain per output
        const float t = tp[(long)k * q.n];
        a0 = fmaf(t, s0[k], a0);
        a1 = fmaf(t, s0[k + step], a1);
        a2 = fmaf(t, s0[k + 2 * step], a2);
        a3 = fmaf(t, s0[k + 3 * step], a3);
    }
}

}  // namespace svc

struct svc_resampler {
    svc::RsGeom q;
    svc::Arena mem;
    float* taps_kn = nullptr;               // device [ntaps][n]
    int* first = nullptr;                   // device [n]
};
