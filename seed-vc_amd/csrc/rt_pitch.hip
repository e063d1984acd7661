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
//
// svc_rt_pitch_win is the same step for a stream whose RMVPE track covers only the last W frames of its context:
// the slot's cache row of raw Hz moves n_new frames to the left and takes the window's trusted frames, the counted frames come
// from that row, and an optional ring of the last `memory` counted bins takes the oldest ones out of the histogram again.
// Steps 2 - 4 are one __device__ function (rp_finish) that both kernels inline.
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

// svc_rt_pitch_win: the window, the slot's cache row and its ring of counted bins
struct RpWin {
    int W, guard, n_new, memory;
    float* cache; int32_t* ring;                            // [max_slots][Tf]; [max_slots][memory + 2] or null
    float* raw_out; long raw_stride;
};

struct RpShared {
    int hist[RP_BINS];                                      // this call's change of every bin (signed once a ring forgets)
    int wave_tot[RP_THREADS / 64];
    int dn, bin;                                            // this call's change of n; the median bin
    float shift;
};

__device__ __forceinline__ int rp_bin(float v) {
    const int b = (int)(__float_as_uint(v) >> 15) - RP_BIN0;   // v > 1: a positive float, bits below 2^31
    return min(max(b, 0), RP_BINS - 1);
}

// What the two kernels share, after sh.hist and sh.dn hold the call's changes (and a barrier): the merge into the slot's row,
// the median bin, the glide, the three scalar words and the Tf outputs over the row f (global for rt_pitch_kernel, LDS for
// rt_pitch_win_kernel).
__device__ __forceinline__ void rp_finish(const RpArgs& a, const RpRows& rows, RpShared& sh, int32_t* st, const float* f) {
    const int k = blockIdx.x, tid = threadIdx.x, slot = rows.slot[k];
    const int n = st[RP_W_N] + sh.dn, rank = (n - 1) / 2;      // the lower-middle element, torch.median's
    int c[RP_PER], tot = 0;
#pragma unroll
    for (int j = 0; j < RP_PER; ++j) {
        const int b = tid * RP_PER + j, add = sh.hist[b];
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
    if ((tid & 63) == 63) sh.wave_tot[tid >> 6] = incl;
    __syncthreads();
    int excl = incl - tot;
    for (int w = 0; w < (tid >> 6); ++w) excl += sh.wave_tot[w];
    if (n > 0 && excl <= rank && rank < excl + tot) {          // exactly one thread: its bins hold the element of that rank
        int cum = excl, j = 0;
        for (; j < RP_PER - 1; ++j) {
            if (cum + c[j] > rank) break;
            cum += c[j];
        }
        sh.bin = tid * RP_PER + j;
    }
    __syncthreads();
    if (tid == 0) {
        const int bin = n > 0 ? sh.bin : 0;
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
        sh.shift = s_new;
    }
    __syncthreads();
    const float s_new = sh.shift, factor = exp2f(rows.semis[k] * (1.f / 12.f));
    float* o = a.out + (long)k * a.out_stride;
    for (int i = tid; i < a.Tf; i += RP_THREADS) {             // the expressions of f0_adjust_kernel
        const float v = f[i], lg = logf(v + 1e-5f);
        o[i] = v > 1.f ? expf(s_new == 0.f ? lg : lg + s_new) * factor : expf(lg);
    }
}

__global__ __launch_bounds__(RP_THREADS) void rt_pitch_kernel(RpArgs a, RpRows rows) {
    __shared__ RpShared sh;
    const int k = blockIdx.x, tid = threadIdx.x;
    const float* f = a.f0 + (long)k * a.stride;

    for (int i = tid; i < RP_BINS; i += RP_THREADS) sh.hist[i] = 0;
    if (tid == 0) { sh.dn = 0; sh.bin = RP_BINS - 1; }
    __syncthreads();
    for (int i = a.lo + tid; i < a.hi; i += RP_THREADS) {
        const float v = f[i];
        if (v > 1.f) {                                         // NaN is unvoiced
            atomicAdd(&sh.hist[rp_bin(v)], 1);
            atomicAdd(&sh.dn, 1);
        }
    }
    __syncthreads();
    rp_finish(a, rows, sh, a.state + (long)rows.slot[k] * RP_WORDS, f);
}

// The in-place shift of the cache row: new[i] = old[i + n_new] must not be stored before every thread has loaded its old
// frames, whatever n_new and Tf are against the 256 threads.  The workgroup builds the whole new row in LDS (window frames
// and shifted old frames), passes a barrier, and only then stores; the counted frames and the outputs read the LDS row.
__global__ __launch_bounds__(RP_THREADS) void rt_pitch_win_kernel(RpArgs a, RpWin w, RpRows rows) {
    __shared__ RpShared sh;
    __shared__ float row[SVC_RT_PITCH_WIN_MAX_TF];
    const int k = blockIdx.x, tid = threadIdx.x, slot = rows.slot[k];
    const float* f = a.f0 + (long)k * a.stride;
    float* cache = w.cache + (long)slot * a.Tf;
    const int w0 = a.Tf - w.W, keep = w0 + w.guard;            // context frame of window frame 0; frames below `keep` come from old

    for (int i = tid; i < RP_BINS; i += RP_THREADS) sh.hist[i] = 0;
    if (tid == 0) { sh.dn = 0; sh.bin = RP_BINS - 1; }
    for (int i = tid; i < a.Tf; i += RP_THREADS) row[i] = i >= keep ? f[i - w0] : cache[i + w.n_new];   // W - guard >= n_new: inside the row
    __syncthreads();                                           // every old frame is loaded
    for (int i = tid; i < a.Tf; i += RP_THREADS) cache[i] = row[i];
    if (w.raw_out) {
        float* r = w.raw_out + (long)k * w.raw_stride;
        for (int i = tid; i < a.Tf; i += RP_THREADS) r[i] = row[i];
    }
    int32_t* ring = w.memory ? w.ring + (long)slot * (w.memory + 2) : nullptr;
    int head = 0, fill = 0, gone = 0;
    if (ring) {                                                // the oldest entries leave before a counted frame takes their place
        head = min(max(ring[w.memory], 0), w.memory - 1);     // the clamps change nothing in a ring this kernel wrote: they keep
        fill = min(max(ring[w.memory + 1], 0), w.memory);      // a row that something else wrote from sending an index outside
        gone = max(fill + w.n_new - w.memory, 0);
        for (int j = tid; j < gone; j += RP_THREADS) {
            const int b = ring[(head + j) % w.memory];
            if (b >= 0 && b < RP_BINS) {
                atomicSub(&sh.hist[b], 1);
                atomicSub(&sh.dn, 1);
            }
        }
        __syncthreads();
    }
    for (int j = tid; j < w.n_new; j += RP_THREADS) {
        const float v = row[a.lo + j];
        const bool voiced = v > 1.f;                           // NaN is unvoiced
        const int b = rp_bin(v);
        if (voiced) {
            atomicAdd(&sh.hist[b], 1);
            atomicAdd(&sh.dn, 1);
        }
        if (ring) ring[(head + fill + j) % w.memory] = voiced ? b : -1;
    }
    if (ring && tid == 0) {
        ring[w.memory] = (head + gone) % w.memory;
        ring[w.memory + 1] = fill + w.n_new - gone;
    }
    __syncthreads();
    rp_finish(a, rows, sh, a.state + (long)slot * RP_WORDS, row);
}

inline bool disjoint(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a1 <= b0 || b1 <= a0; }

// The checks the two entries share (`who` names the entry in the message; `row` is the width of an f0 row: Tf, or W); fills rows.
int rp_check(const std::string& who, const void* f0, long long stride, int row, int Tf, int n_new, int lag, int N, const int32_t* slots,
             int max_slots, const void* state, const void* ref_median, const int32_t* auto_adjust, const float* semitones, int warmup,
             float max_step, const void* out, long long out_stride, RpRows& rows) {
    SVC_REQUIRE(f0 && slots && state && ref_median && auto_adjust && out,
                who + ": null argument (f0, slots, state, ref_median, auto_adjust, out)");
    SVC_REQUIRE(N >= 1 && N <= RP_MAXN, who + ": N outside [1, 64]");
    SVC_REQUIRE(max_slots >= 1 && Tf >= 1, who + ": max_slots and Tf must be at least 1");
    SVC_REQUIRE(n_new >= 1 && lag >= 0, who + ": n_new must be at least 1 and lag at least 0");
    SVC_REQUIRE((long long)Tf - lag - n_new >= 0, who + ": Tf - lag - n_new is negative: the row does not hold the counted frames");
    SVC_REQUIRE(stride >= row && out_stride >= Tf, who + ": stride or out_stride below the row");
    SVC_REQUIRE(warmup >= 0, who + ": warmup is negative");
    SVC_REQUIRE(max_step == max_step, who + ": max_step is NaN");
    std::vector<int32_t> sorted(slots, slots + N);
    std::sort(sorted.begin(), sorted.end());
    SVC_REQUIRE(sorted.front() >= 0 && sorted.back() < max_slots, who + ": a slot outside 0 .. max_slots - 1");
    SVC_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), who + ": a slot appears twice in one call");
    memset(&rows, 0, sizeof(rows));
    for (int k = 0; k < N; ++k) {
        const float s = semitones ? semitones[k] : 0.f;
        SVC_REQUIRE(std::isfinite(s), who + ": a semitones entry is not finite");
        rows.slot[k] = slots[k]; rows.aut[k] = auto_adjust[k] != 0; rows.semis[k] = s;
    }
    return 0;
}

struct Span { uintptr_t lo, hi; };
inline Span span(const void* p, long long words) { return {(uintptr_t)p, (uintptr_t)p + (uintptr_t)(words * 4)}; }
inline bool disjoint(Span a, Span b) { return !a.lo || !b.lo || disjoint(a.lo, a.hi, b.lo, b.hi); }      // a NULL buffer overlaps nothing

}  // namespace

extern "C" {

long long svc_rt_pitch_state_words(int max_slots) { return max_slots >= 1 ? (long long)max_slots * RP_WORDS : 0; }

int svc_rt_pitch(const float* f0, long long stride, int Tf, int n_new, int lag, int N, const int32_t* slots, int max_slots,
                 int32_t* state, const float* ref_median, const int32_t* auto_adjust, const float* semitones, int warmup,
                 float max_step, float* out, long long out_stride, float* shift_out, void* stream) {
    RpRows rows;
    if (rp_check("rt_pitch", f0, stride, Tf, Tf, n_new, lag, N, slots, max_slots, state, ref_median, auto_adjust, semitones, warmup,
                 max_step, out, out_stride, rows)) return 1;
    SVC_REQUIRE((((uintptr_t)f0 | (uintptr_t)state | (uintptr_t)ref_median | (uintptr_t)out | (uintptr_t)shift_out) & 3) == 0,
                "rt_pitch: a buffer is not aligned to 4 bytes");
    const Span sf = span(f0, (long long)(N - 1) * stride + Tf), ss = span(state, svc_rt_pitch_state_words(max_slots));
    const Span so = span(out, (long long)(N - 1) * out_stride + Tf);
    SVC_REQUIRE(disjoint(so, sf) && disjoint(so, ss), "rt_pitch: out overlaps f0 or state");

    RpArgs a;
    a.f0 = f0; a.stride = (long)stride; a.Tf = Tf; a.lo = Tf - lag - n_new; a.hi = Tf - lag;
    a.state = state; a.ref_median = ref_median; a.warmup = warmup; a.max_step = max_step;
    a.out = out; a.out_stride = (long)out_stride; a.shift_out = shift_out;
    hipLaunchKernelGGL(rt_pitch_kernel, dim3((unsigned)N), dim3(RP_THREADS), 0, (hipStream_t)stream, a, rows);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

long long svc_rt_pitch_cache_words(int max_slots, int Tf) {
    return max_slots >= 1 && Tf >= 1 && Tf <= SVC_RT_PITCH_WIN_MAX_TF ? (long long)max_slots * Tf : 0;
}

long long svc_rt_pitch_ring_words(int max_slots, int memory) { return max_slots >= 1 && memory >= 1 ? (long long)max_slots * (memory + 2LL) : 0; }

int svc_rt_pitch_win(const float* f0_win, long long stride, int W, int guard, int Tf, int n_new, int lag, int N, const int32_t* slots,
                     int max_slots, float* cache, int32_t* ring, int memory, int32_t* state, const float* ref_median,
                     const int32_t* auto_adjust, const float* semitones, int warmup, float max_step, float* out, long long out_stride,
                     float* raw_out, long long raw_stride, float* shift_out, void* stream) {
    RpRows rows;
    if (rp_check("rt_pitch_win", f0_win, stride, W, Tf, n_new, lag, N, slots, max_slots, state, ref_median, auto_adjust, semitones,
                 warmup, max_step, out, out_stride, rows)) return 1;
    SVC_REQUIRE(Tf <= SVC_RT_PITCH_WIN_MAX_TF, "rt_pitch_win: Tf above SVC_RT_PITCH_WIN_MAX_TF = 4096 (the row is staged in LDS)");
    SVC_REQUIRE(W >= 1 && W <= Tf, "rt_pitch_win: W outside [1, Tf]");
    SVC_REQUIRE(guard >= 0, "rt_pitch_win: guard is negative");
    SVC_REQUIRE((long long)W - guard >= n_new, "rt_pitch_win: W - guard is below n_new: frames of the cache would be left unwritten");
    SVC_REQUIRE(cache, "rt_pitch_win: cache is null");
    SVC_REQUIRE(memory >= 0 && (memory == 0 || memory >= n_new), "rt_pitch_win: memory is negative or below n_new");
    SVC_REQUIRE((memory > 0) == (ring != nullptr), "rt_pitch_win: ring and memory disagree (a ring needs memory > 0, memory > 0 a ring)");
    SVC_REQUIRE(!raw_out || raw_stride >= Tf, "rt_pitch_win: raw_stride below Tf");
    SVC_REQUIRE((((uintptr_t)f0_win | (uintptr_t)cache | (uintptr_t)ring | (uintptr_t)state | (uintptr_t)ref_median | (uintptr_t)out |
                  (uintptr_t)raw_out | (uintptr_t)shift_out) & 3) == 0, "rt_pitch_win: a buffer is not aligned to 4 bytes");
    const Span sf = span(f0_win, (long long)(N - 1) * stride + W), ss = span(state, svc_rt_pitch_state_words(max_slots));
    const Span sc = span(cache, (long long)max_slots * Tf), sr = span(ring, svc_rt_pitch_ring_words(max_slots, memory));
    const Span so = span(out, (long long)(N - 1) * out_stride + Tf), sw = span(raw_out, (long long)(N - 1) * raw_stride + Tf);
    for (const Span& o : {so, sw})
        SVC_REQUIRE(disjoint(o, sf) && disjoint(o, sc) && disjoint(o, ss) && disjoint(o, sr),
                    "rt_pitch_win: out or raw_out overlaps f0_win, cache, state or ring");
    SVC_REQUIRE(disjoint(so, sw), "rt_pitch_win: out overlaps raw_out");
    SVC_REQUIRE(disjoint(sf, sc) && disjoint(sf, ss) && disjoint(sf, sr) && disjoint(sc, ss) && disjoint(sc, sr) && disjoint(ss, sr),
                "rt_pitch_win: f0_win, cache, state and ring overlap one another");

    RpArgs a;
    a.f0 = f0_win; a.stride = (long)stride; a.Tf = Tf; a.lo = Tf - lag - n_new; a.hi = Tf - lag;
    a.state = state; a.ref_median = ref_median; a.warmup = warmup; a.max_step = max_step;
    a.out = out; a.out_stride = (long)out_stride; a.shift_out = shift_out;
    RpWin w;
    w.W = W; w.guard = guard; w.n_new = n_new; w.memory = memory; w.cache = cache; w.ring = ring;
    w.raw_out = raw_out; w.raw_stride = (long)raw_stride;
    hipLaunchKernelGGL(rt_pitch_win_kernel, dim3((unsigned)N), dim3(RP_THREADS), 0, (hipStream_t)stream, a, w, rows);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
