// Real-time sessions, pitch: the drivers' voiced-median shift and semitone shift (svc_f0_adjust) restated for
// a stream.  Offline the shift is median(reference) - median(whole source); a stream has no whole source, so every slot keeps
// running voiced-pitch statistics on the device: a histogram of 256 bins per octave over [32, 2048) Hz in which every 10 ms frame
// of the stream is counted exactly once, the total, and the shift that was applied last (the shift glides towards its target by
// at most max_step per call).  ONE launch per call, one workgroup of 256 threads (four wave64) per listed stream:
//
//   1. the n_new counted frames of the row are binned into a zeroed LDS histogram with integer LDS atomics (the bin is a shift
//      of the float's own bit pattern: no transcendental, nothing a host statement cannot restate in exact integers);
//   2. thread t owns bins 6 t .. 6 t + 5: it adds the slot's global row to its LDS counts, stores back the bins that changed, and
//      the block prefix sum of the per-thread totals (wave scan by shuffles, four wave totals through LDS) tells the one thread
//      whose bins straddle the lower-middle rank to name the median bin;
//   3. thread 0 turns the bin centre into the running log median, glides the applied shift and writes the slot's three scalar
//      words (and shift_out);
//   4. all threads write the Tf outputs with the per-frame expressions of f0_adjust_kernel (rmvpe.hip).
//
// Only this workgroup reads or writes the slot's row during the launch, every count is an integer and the float path of a frame
// is a function of that frame, the slot's shift and its semitones alone: nothing depends on N, k, the slot number, the other
// streams or an order of arrival.  Slots, flags and semitones travel as kernel arguments (at most 64 streams per call), so the
// call copies nothing and synchronises nothing.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "model_util.h"

using namespace svc;

namespace {

constexpr int RP_MAXN = 64;
constexpr int RP_BINS = SVC_RT_PITCH_BINS, RP_WORDS = SVC_RT_PITCH_STATE_WORDS;
constexpr int RP_THREADS = 256, RP_PER = RP_BINS / RP_THREADS;                     // 6 bins per thread
constexpr int RP_W_N = RP_BINS, RP_W_SHIFT = RP_BINS + 1, RP_W_BIN = RP_BINS + 2;   // the scalar words of a slot's row
constexpr int RP_BIN0 = 33792;                                                     // float_bits(32.f) >> 15
static_assert(RP_PER * RP_THREADS == RP_BINS, "the scan gives every thread the same number of bins");

struct RpRows { int slot[RP_MAXN]; int aut[RP_MAXN]; float semis[RP_MAXN]; };

struct RpArgs {
    const float* f0; long stride; int Tf, lo, hi;          // counted frames: [lo, hi) of every row
    int32_t* state; const float* ref_median;
    int warmup; float max_step;                             // max_step <= 0 or +inf: no limit
    float* out; long out_stride; float* shift_out;
};

__device__ __forceinline__ int rp_bin(float v) {
    const int b = (int)(__float_as_uint(v) >> 15) - RP_BIN0;   // v > 1: a positive float, bits below 2^31
    return min(max(b, 0), RP_BINS - 1);
}

__global__ __launch_bounds__(RP_THREADS) void rt_pitch_kernel(RpArgs a, RpRows rows) {
    __shared__ int hist[RP_BINS];
    __shared__ int wave_tot[RP_THREADS / 64];
    __shared__ int sh_added, sh_bin;
    __shared__ float sh_shift;
    const int k = blockIdx.x, tid = threadIdx.x, slot = rows.slot[k];
    const float* f = a.f0 + (long)k * a.stride;
    int32_t* st = a.state + (long)slot * RP_WORDS;

    for (int i = tid; i < RP_BINS; i += RP_THREADS) hist[i] = 0;
    if (tid == 0) { sh_added = 0; sh_bin = RP_BINS - 1; }
    __syncthreads();
    for (int i = a.lo + tid; i < a.hi; i += RP_THREADS) {
        const float v = f[i];
        if (v > 1.f) {                                         // NaN is unvoiced
            atomicAdd(&hist[rp_bin(v)], 1);
            atomicAdd(&sh_added, 1);
        }
    }
    __syncthreads();
    const int n = st[RP_W_N] + sh_added, rank = (n - 1) / 2;   // the lower-middle element, torch.median's
    int c[RP_PER], tot = 0;
#pragma unroll
    for (int j = 0; j < RP_PER; ++j) {
        const int b = tid * RP_PER + j, add = hist[b];
        c[j] = st[b] + add;
        if (add) st[b] = c[j];
        tot += c[j];
    }
    int incl = tot;                                            // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if ((tid & 63) >= d) incl += up;
    }
    if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
    __syncthreads();
    int excl = incl - tot;
    for (int w = 0; w < (tid >> 6); ++w) excl += wave_tot[w];
    if (n > 0 && excl <= rank && rank < excl + tot) {          // exactly one thread: its bins hold the element of that rank
        int cum = excl, j = 0;
        for (; j < RP_PER - 1; ++j) {
            if (cum + c[j] > rank) break;
            cum += c[j];
        }
        sh_bin = tid * RP_PER + j;
    }
    __syncthreads();
    if (tid == 0) {
        const int bin = n > 0 ? sh_bin : 0;
        const float centre = __uint_as_float(((unsigned)(bin + RP_BIN0) << 15) | 0x4000u);
        const float m_run = logf(centre + 1e-5f);
        // a voiced median is the log of a float above 1: positive.  0 (svc_f0_adjust's median of a track without a voiced
        // frame), a negative value or NaN means the slot has no reference: no shift, as svc_f0_adjust applies none
        const float ref = a.ref_median[slot];
        const float d = rows.aut[k] && ref > 0.f && n >= max(a.warmup, 1) ? ref - m_run : 0.f;
        const float s_old = __int_as_float(st[RP_W_SHIFT]);
        const bool limited = a.max_step > 0.f && a.max_step < INFINITY;
        float s_new = d;                                       // arrival is exact
        if (limited && !(fabsf(d - s_old) <= a.max_step)) s_new = d > s_old ? s_old + a.max_step : s_old - a.max_step;
        st[RP_W_N] = n;
        st[RP_W_SHIFT] = __float_as_int(s_new);
        st[RP_W_BIN] = bin;
        if (a.shift_out) a.shift_out[k] = s_new;
        sh_shift = s_new;
    }
    __syncthreads();
    const float s_new = sh_shift, factor = exp2f(rows.semis[k] * (1.f / 12.f));
    float* o = a.out + (long)k * a.out_stride;
    for (int i = tid; i < a.Tf; i += RP_THREADS) {             // the expressions of f0_adjust_kernel
        const float v = f[i], lg = logf(v + 1e-5f);
        o[i] = v > 1.f ? expf(s_new == 0.f ? lg : lg + s_new) * factor : expf(lg);
    }
}

inline bool disjoint(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a1 <= b0 || b1 <= a0; }

}  // namespace

extern "C" {

long long svc_rt_pitch_state_words(int max_slots) { return max_slots >= 1 ? (long long)max_slots * RP_WORDS : 0; }

int svc_rt_pitch(const float* f0, long long stride, int Tf, int n_new, int lag, int N, const int32_t* slots, int max_slots,
                 int32_t* state, const float* ref_median, const int32_t* auto_adjust, const float* semitones, int warmup,
                 float max_step, float* out, long long out_stride, float* shift_out, void* stream) {
    SVC_REQUIRE(f0 && slots && state && ref_median && auto_adjust && out,
                "rt_pitch: null argument (f0, slots, state, ref_median, auto_adjust, out)");
    SVC_REQUIRE(N >= 1 && N <= RP_MAXN, "rt_pitch: N outside [1, 64]");
    SVC_REQUIRE(max_slots >= 1 && Tf >= 1, "rt_pitch: max_slots and Tf must be at least 1");
    SVC_REQUIRE(n_new >= 1 && lag >= 0, "rt_pitch: n_new must be at least 1 and lag at least 0");
    const long long lo = (long long)Tf - lag - n_new;
    SVC_REQUIRE(lo >= 0, "rt_pitch: Tf - lag - n_new is negative: the row does not hold the counted frames");
    SVC_REQUIRE(stride >= Tf && out_stride >= Tf, "rt_pitch: stride or out_stride below Tf");
    SVC_REQUIRE(warmup >= 0, "rt_pitch: warmup is negative");
    SVC_REQUIRE(max_step == max_step, "rt_pitch: max_step is NaN");
    std::vector<int32_t> sorted(slots, slots + N);
    std::sort(sorted.begin(), sorted.end());
    SVC_REQUIRE(sorted.front() >= 0 && sorted.back() < max_slots, "rt_pitch: a slot outside 0 .. max_slots - 1");
    SVC_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "rt_pitch: a slot appears twice in one call");
    RpRows rows;
    memset(&rows, 0, sizeof(rows));
    for (int k = 0; k < N; ++k) {
        const float s = semitones ? semitones[k] : 0.f;
        SVC_REQUIRE(std::isfinite(s), "rt_pitch: a semitones entry is not finite");
        rows.slot[k] = slots[k]; rows.aut[k] = auto_adjust[k] != 0; rows.semis[k] = s;
    }
    SVC_REQUIRE((((uintptr_t)f0 | (uintptr_t)state | (uintptr_t)ref_median | (uintptr_t)out | (uintptr_t)shift_out) & 3) == 0,
                "rt_pitch: a buffer is not aligned to 4 bytes");
    const uintptr_t f0a = (uintptr_t)f0, f1 = f0a + (uintptr_t)(((long long)(N - 1) * stride + Tf) * 4);
    const uintptr_t s0 = (uintptr_t)state, s1 = s0 + (uintptr_t)(svc_rt_pitch_state_words(max_slots) * 4);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(((long long)(N - 1) * out_stride + Tf) * 4);
    SVC_REQUIRE(disjoint(o0, o1, f0a, f1) && disjoint(o0, o1, s0, s1), "rt_pitch: out overlaps f0 or state");

    RpArgs a;
    a.f0 = f0; a.stride = (long)stride; a.Tf = Tf; a.lo = (int)lo; a.hi = Tf - lag;
    a.state = state; a.ref_median = ref_median; a.warmup = warmup; a.max_step = max_step;
    a.out = out; a.out_stride = (long)out_stride; a.shift_out = shift_out;
    hipLaunchKernelGGL(rt_pitch_kernel, dim3((unsigned)N), dim3(RP_THREADS), 0, (hipStream_t)stream, a, rows);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
