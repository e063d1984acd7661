// Shared by the AR device headers (ar_prefill.h, ar_decode1.h, ar_batch.h, ar_sampler.h) and by ar.hip, the one translation
// unit that includes them: the generate loop's device-resident state, the batch and vocabulary limits, the cross-lane
// sums and the compile-time size dispatch.
#pragma once
#include <math.h>

#include <type_traits>

#include "model_util.h"

using namespace svc;

namespace {

// Device-resident state of the generate loop: the captured per-token graph (decode step -> rank -> sample, which also
// embeds the drawn token and advances the positions) reads everything that changes from token to token from here, so one graph replay per token needs no host argument.
struct GenState {
    const float* noise;      // [max_new][V] Exp(1) draws, row t for token t; null = draw them from `seed` (ar_exp_draw4)
    unsigned long long seed;
    int* toks;               // [max_new] generated tokens
    int cnt;                 // index of the token being generated (>= 1 inside the loop)
    int min_before_eos, eos;
    float temperature, top_p, rep_pen;
};

constexpr int MAXB = 64;             // slots (sequences) of one batched decode step

// GenState of one slot + its loop flags.  A finished slot (EOS drawn, max_new reached, or the next position would leave the
// cache) stays in the batch: it re-runs its last step in place (same positions, same cache row) and records nothing.
struct GenSlot : GenState {
    int done;
    int max_new;
};

constexpr int SORT_N = 4096;         // the sampler runs one block over a vocabulary of at most SORT_N entries

// Cross-lane sums on the DPP path (one VALU instruction per step, no LDS crossbar round trip: `__shfl_xor` compiles to
// ds_bpermute_b32, ~100+ cycles each, and the one-token kernels are chains of such latencies).  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
__device__ __forceinline__ float row8_sum_f(float v) {      // every lane of an aligned 8-lane group gets the group's sum
    v += dpp_f<DPP_XOR1>(v); v += dpp_f<DPP_XOR2>(v); v += dpp_f<DPP_HALF_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float row16_sum_f(float v) {     // ... of an aligned 16-lane group (a DPP row)
    v = row8_sum_f(v); v += dpp_f<DPP_ROW_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {      // every lane gets the wave's sum
    v = row16_sum_f(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
}

// The ar_base sizes (dim 768, intermediate 2304) are known at compile time: the decode-step and batched kernels are
// instantiated for them (KD = 768, KI = 2304: reduction loops unrolled, dead chunks pruned) and for runtime sizes
// (KD = KI = 0).  Calls f(KD, KI) with the instance for this shape, as compile-time constants.
template <int N> using IntC = std::integral_constant<int, N>;
template <class F>
int with_ar_sizes(int D, int I, F&& f) {
    return D == 768 && I == 2304 ? f(IntC<768>(), IntC<2304>()) : f(IntC<0>(), IntC<0>());
}

}  // namespace
