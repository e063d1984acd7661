// Real-time sessions: the SOLA splice of the reference GUI's audio callback (real-time-gui.py, `audio_callback`, restated
// from memory) as ONE launch per 64 streams: offset search, cross-fade, state update and block copy.  The offset is
// data-dependent, so doing all four on the device lets a block step be enqueued from host integers alone.
//
// `svc_rt_out` is the same kernel behind a prologue: the stream's workgroup first resamples its segment of the
// vocoder output to the output rate (resample_core.h: `rs_dot4`, tile by tile as `svc_resample` cuts them) or writes zeros where
// the caller's VAD reports no speech, into the stream's row of `infer`, and after a barrier splices that row.  The prologue is a
// template flag: `svc_sola_step` launches the form without it.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "resample_core.h"

namespace svc {
namespace {
constexpr int SOLA_MAXN = 64;                 // streams per launch: their slots travel as kernel arguments
constexpr int SOLA_THREADS = 256;
constexpr int SOLA_LDS_FLOATS = 16128;        // 63 KiB of samples beside the argmax scratch: 2 * Lb + Ls must fit
struct SolaSlots { int slot[SOLA_MAXN]; };

// the prologue of svc_rt_out: infer[k] = resample(wave[k][start : start + n_in]), the segment itself where !resample, +0.0 where
// bit k of `muted` is set
struct SolaPro {
    float* infer; int n_in, n_inf, resample; unsigned long long muted;
    const int* speech_dev;                   // svc_rt_out_dev: device flags [max_slots], 0 mutes (the DEV forms only read it)
    RsGeom q; const float* taps_kn; const int* first;
};

// fl(fl(y * fi) + fl(b * fo)): the GUI's `y *= fade_in; y += buffer * fade_out` on fp32 tensors.  Contraction is switched off
// for these statements: __fmul_rn / __fadd_rn are plain operators here and the compiler fused them into an fma.
__device__ __forceinline__ float fade_mix(float y, float fi, float b, float fo) {
#pragma clang fp contract(off)
    const float p = y * fi;
    const float q = b * fo;
    return p + q;
}

// One workgroup per stream.  x = wave[k][start ..], b = state[slot]:
//   score[o] = sum_i x[o+i] b[i] / sqrt(sum_i x[o+i]^2 + 1e-8),  o = 0 .. Ls     (every sum from its own Lb terms)
//   o* = lowest o with the highest score;  y = x[o* ..]
//   y[i] = fl(fl(y[i] fade_in[i]) + fl(b[i] fade_out[i]))  (i < Lb);  out = y[:block];  state[slot] = y[block : block + Lb]
// The Lb + Ls samples the search reads and the old buffer are staged in LDS: a lane owns offsets tid, tid + 256, ..., so the
// input reads of a wave are consecutive words and the buffer read is a broadcast.  The epilogue reads the old buffer from
// LDS only, so writing the new state over the same row (block < Lb included) needs no ordering beyond the barrier.
// No sample at or above start + block + Lb + Ls is read.  VEC: block and Lb are multiples of 4 and out / state / fades
// are 16-byte aligned, so a group of 4 samples lies on one side of the fade and of the out / state boundary.
// PRO: x is the stream's row of pro.infer, which this workgroup writes first (and reads back behind the barrier: a workgroup's
// own global writes are visible to it there); `start` then counts in `wave` only.  DEV (with PRO): the stream is also muted
// where pro.speech_dev[slot] is 0, one workgroup-uniform read; the other forms are compiled without it.
template <bool VEC, bool PRO, bool DEV>
__global__ __launch_bounds__(SOLA_THREADS) void sola_step_kernel(const float* __restrict__ wave, long stride, int start,
                                                                 float* __restrict__ state, const SolaSlots slots,
                                                                 const float* __restrict__ fade_in, const float* __restrict__ fade_out,
                                                                 int block, int Lb, int Ls, float* __restrict__ out,
                                                                 int* __restrict__ offsets, const SolaPro pro) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* red_s = lds;                                   // [4] best score of each wave
    int* red_o = reinterpret_cast<int*>(lds + 4);         // [4] its offset, [4]: the winner
    float* bs = lds + 16;                                 // [Lb rounded up to 4] old buffer
    float* xs = bs + ((Lb + 3) & ~3);                     // [Lb + Ls] input the search reads
    const int k = blockIdx.x, tid = threadIdx.x;
    const float* x = wave + (long)k * stride + start;
    if constexpr (PRO) {
        float* y = pro.infer + (long)k * pro.n_inf;
        const float* seg = x;
        bool muted = (pro.muted >> k) & 1ULL;
        if constexpr (DEV) muted = muted || pro.speech_dev[slots.slot[k]] == 0;
        if (muted) {
            for (int i = tid; i < pro.n_inf; i += SOLA_THREADS) y[i] = 0.f;
        } else if (!pro.resample) {
            for (int i = tid; i < pro.n_inf; i += SOLA_THREADS) y[i] = seg[i];
        } else {
            const RsGeom& q = pro.q;
            const int S = q.G * q.n;
            const long len = pro.n_in;
            for (long m0 = 0; m0 < pro.n_inf; m0 += (long)RS_ROWS * S) {      // tiles as svc_resample cuts them
                const long lo = (m0 / q.n) * q.o + q.fmin - q.width;
                const int sh = (int)((((long)(reinterpret_cast<uintptr_t>(seg) >> 2) + lo) % 4 + 4) % 4);
                const long p0 = lo - sh;
                if (m0 != 0) __syncthreads();                     // the previous tile's readers are done with lds
                for (int v = tid * 4; v < q.span; v += SOLA_THREADS * 4) {
                    const long p = p0 + v;
                    float4v t;
                    if (p >= 0 && p + 3 < len) {
                        t = *reinterpret_cast<const float4v*>(seg + p);
                    } else {                                      // the segment's ends: zeros outside, element by element
#pragma unroll
                        for (int e = 0; e < 4; ++e) t[e] = (p + e >= 0 && p + e < len) ? seg[p + e] : 0.f;
                    }
                    *reinterpret_cast<float4v*>(lds + v) = t;
                }
                __syncthreads();
                for (int w = tid; w < S && m0 + w < pro.n_inf; w += SOLA_THREADS) {      // the last tile: no item without an output
                    float acc[RS_ROWS];
                    rs_dot4(lds, sh, q, pro.taps_kn, pro.first, w, acc[0], acc[1], acc[2], acc[3]);
#pragma unroll
                    for (int r = 0; r < RS_ROWS; ++r) {
                        const long m = m0 + w + (long)r * S;
                        if (m < pro.n_inf) y[m] = acc[r];
                    }
                }
            }
        }
        __syncthreads();                                          // infer[k] is written, and nobody reads the staged span any more
        x = y;
    }
    float* st = state + (long)slots.slot[k] * Lb;
    for (int i = tid; i < Lb; i += SOLA_THREADS) bs[i] = st[i];
    for (int i = tid; i < Lb + Ls; i += SOLA_THREADS) xs[i] = x[i];
    __syncthreads();

    float best = -INFINITY;
    int best_o = 0;                                       // a NaN score never wins: the offset stays inside 0 .. Ls
    for (int o = tid; o <= Ls; o += SOLA_THREADS) {
        const float* xo = xs + o;
        float n0 = 0.f, n1 = 0.f, n2 = 0.f, n3 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
        int i = 0;
        for (; i + 4 <= Lb; i += 4) {
            const float4v b4 = *reinterpret_cast<const float4v*>(bs + i);
            const float x0 = xo[i], x1 = xo[i + 1], x2 = xo[i + 2], x3 = xo[i + 3];
            n0 = fmaf(x0, b4[0], n0); e0 = fmaf(x0, x0, e0);
            n1 = fmaf(x1, b4[1], n1); e1 = fmaf(x1, x1, e1);
            n2 = fmaf(x2, b4[2], n2); e2 = fmaf(x2, x2, e2);
            n3 = fmaf(x3, b4[3], n3); e3 = fmaf(x3, x3, e3);
        }
        for (; i < Lb; ++i) {
            const float x0 = xo[i];
            n0 = fmaf(x0, bs[i], n0); e0 = fmaf(x0, x0, e0);
        }
        const float s = ((n0 + n1) + (n2 + n3)) / sqrtf(((e0 + e1) + (e2 + e3)) + 1e-8f);
        if (s > best) { best = s; best_o = o; }           // offsets ascend per lane: a tie keeps the lower one
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float s2 = __shfl_xor(best, d, 64);
        const int o2 = __shfl_xor(best_o, d, 64);
        if (s2 > best || (s2 == best && o2 < best_o)) { best = s2; best_o = o2; }
    }
    if ((tid & 63) == 0) { red_s[tid >> 6] = best; red_o[tid >> 6] = best_o; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SOLA_THREADS / 64; ++w)
            if (red_s[w] > best || (red_s[w] == best && red_o[w] < best_o)) { best = red_s[w]; best_o = red_o[w]; }
        red_o[4] = best_o;
        if (offsets) offsets[k] = best_o;
    }
    __syncthreads();
    const int os = red_o[4];

    const float* y = x + os;
    float* o_row = out + (long)k * block;
    constexpr int W = VEC ? 4 : 1;
    const bool src16 = VEC && ((reinterpret_cast<uintptr_t>(y) & 15) == 0);       // uniform: depends on o*
    for (int i0 = tid * W; i0 < block + Lb; i0 += SOLA_THREADS * W) {
        float v[W];
        if constexpr (VEC) {
            if (src16) {
                const float4v t = *reinterpret_cast<const float4v*>(y + i0);
                v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j) v[j] = y[i0 + j];
            }
        } else {
            v[0] = y[i0];
        }
        if (i0 < Lb) {
            float fi[W], fo[W];
            if constexpr (VEC) {
                const float4v a = *reinterpret_cast<const float4v*>(fade_in + i0), b = *reinterpret_cast<const float4v*>(fade_out + i0);
                fi[0] = a[0]; fi[1] = a[1]; fi[2] = a[2]; fi[3] = a[3];
                fo[0] = b[0]; fo[1] = b[1]; fo[2] = b[2]; fo[3] = b[3];
            } else {
                fi[0] = fade_in[i0]; fo[0] = fade_out[i0];
            }
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = fade_mix(v[j], fi[j], bs[i0 + j], fo[j]);
        }
        float* dst = i0 < block ? o_row + i0 : st + (i0 - block);
        if constexpr (VEC) *reinterpret_cast<float4v*>(dst) = (float4v){v[0], v[1], v[2], v[3]};
        else dst[0] = v[0];
    }
}
}  // namespace
}  // namespace svc

using namespace svc;

static_assert(SOLA_THREADS == RS_THREADS, "the prologue runs rs_dot4 with the resampler's work-item layout");

namespace {
inline bool apart(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a1 <= b0 || b1 <= a0; }

// The checks and launches of both entries.  !pro: svc_sola_step, the kernel without the prologue.
int sola_launch(const char* who, const float* wave, long long stride, int start, int N, float* sola_state, int max_slots,
                const int32_t* slots, const float* fade_in, const float* fade_out, int block, int Lb, int Ls, float* out,
                int32_t* offsets, const svc_resampler_t* r, int n_in, const int32_t* speech, const int32_t* speech_dev, float* infer, bool pro,
                void* stream) {
#define SOLA_REQUIRE(cond, msg) \
    do { if (!(cond)) { set_error(std::string(who) + msg); return 1; } } while (0)
    SOLA_REQUIRE(N >= 0 && stride >= 0 && start >= 0 && max_slots >= 0, ": negative argument");
    SOLA_REQUIRE(block >= 1 && Lb >= 1 && Ls >= 0, ": block and Lb must be at least 1, Ls at least 0");
    const long long n_inf = (long long)block + Lb + Ls;
    if (!pro) SOLA_REQUIRE((long long)start + n_inf <= stride, ": start + block + Lb + Ls lies past the row (stride)");
    SOLA_REQUIRE(2LL * Lb + Ls <= SOLA_LDS_FLOATS, ": 2 * Lb + Ls above 16128 samples (the search is staged in LDS)");
    if (pro) {
        SOLA_REQUIRE(n_in >= 1 && (long long)start + n_in <= stride, ": start + n_in lies past the row (stride)");
        SOLA_REQUIRE(n_inf == (r ? (long long)svc_resample_len(r->q.o, r->q.n, n_in) : (long long)n_in),
                     ": block + Lb + Ls is not svc_resample_len(o, n, n_in)");
        SOLA_REQUIRE(!r || r->q.span <= 16000, ": the resampler's span does not fit the LDS");
        SOLA_REQUIRE(infer != nullptr, ": infer is NULL");
        for (int k = 0; speech && k < N; ++k) SOLA_REQUIRE(speech[k] == 0 || speech[k] == 1, ": a speech entry is neither 0 nor 1");
    }
    if (N == 0) return 0;
    SOLA_REQUIRE(wave && sola_state && slots && fade_in && fade_out && out, ": null argument");
    std::vector<int32_t> sorted(slots, slots + N);
    std::sort(sorted.begin(), sorted.end());
    SOLA_REQUIRE(sorted.front() >= 0 && sorted.back() < max_slots, ": a slot outside 0 .. max_slots - 1");
    SOLA_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), ": a slot appears twice in one call");
    if (pro) {
        SOLA_REQUIRE((((uintptr_t)wave | (uintptr_t)infer) & 3) == 0, ": wave or infer is not aligned to 4 bytes");
        const uintptr_t i0 = (uintptr_t)infer, i1 = i0 + (uintptr_t)((long long)N * n_inf * 4);
        const uintptr_t w0 = (uintptr_t)wave, w1 = w0 + (uintptr_t)(((long long)(N - 1) * stride + start + n_in) * 4);
        const uintptr_t s0 = (uintptr_t)sola_state, s1 = s0 + (uintptr_t)((long long)max_slots * Lb * 4);
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((long long)N * block * 4);
        const uintptr_t f0 = (uintptr_t)fade_in, f1 = f0 + (uintptr_t)Lb * 4, g0 = (uintptr_t)fade_out, g1 = g0 + (uintptr_t)Lb * 4;
        const uintptr_t d0 = (uintptr_t)offsets, d1 = d0 + (uintptr_t)N * 4;
        SOLA_REQUIRE(apart(i0, i1, w0, w1) && apart(i0, i1, s0, s1) && apart(i0, i1, o0, o1) && apart(i0, i1, f0, f1) &&
                     apart(i0, i1, g0, g1) && (!offsets || apart(i0, i1, d0, d1)),
                     ": infer overlaps wave, sola_state, out, the windows or offsets");
        if (speech_dev) {
            SOLA_REQUIRE(((uintptr_t)speech_dev & 3) == 0, ": speech_dev is not aligned to 4 bytes");
            const uintptr_t v0 = (uintptr_t)speech_dev, v1 = v0 + (uintptr_t)max_slots * 4;
            SOLA_REQUIRE(apart(v0, v1, i0, i1) && apart(v0, v1, w0, w1) && apart(v0, v1, s0, s1) && apart(v0, v1, o0, o1) &&
                         apart(v0, v1, f0, f1) && apart(v0, v1, g0, g1) && (!offsets || apart(v0, v1, d0, d1)),
                         ": speech_dev overlaps wave, infer, sola_state, out, the windows or offsets");
        }
    }
#undef SOLA_REQUIRE
    const bool vec = block % 4 == 0 && Lb % 4 == 0 &&
                     (((uintptr_t)sola_state | (uintptr_t)out | (uintptr_t)fade_in | (uintptr_t)fade_out) & 15) == 0;
    size_t lds = (size_t)(16 + ((Lb + 3) & ~3) + Lb + Ls) * sizeof(float);
    if (pro && r) lds = std::max(lds, (size_t)r->q.span * sizeof(float));        // the larger of the two phases
    for (int k0 = 0; k0 < N; k0 += SOLA_MAXN) {
        const int nk = std::min(N - k0, SOLA_MAXN);
        SolaSlots s;
        memset(&s, 0, sizeof(s));
        for (int k = 0; k < nk; ++k) s.slot[k] = slots[k0 + k];
        SolaPro p;
        memset(&p, 0, sizeof(p));
        if (pro) {
            p.infer = infer + (long long)k0 * n_inf; p.n_in = n_in; p.n_inf = (int)n_inf; p.resample = r ? 1 : 0;
            for (int k = 0; speech && k < nk; ++k)
                if (!speech[k0 + k]) p.muted |= 1ULL << k;
            p.speech_dev = speech_dev;
            if (r) { p.q = r->q; p.taps_kn = r->taps_kn; p.first = r->first; }
        }
        const float* w = wave + (long long)k0 * stride;
        float* o = out + (long long)k0 * block;
        int32_t* off = offsets ? offsets + k0 : nullptr;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(nk), dim3(SOLA_THREADS), lds, (hipStream_t)stream, w, (long)stride, start, sola_state, s,
                               fade_in, fade_out, block, Lb, Ls, o, off, p);
        };
        if (pro && speech_dev) { if (vec) launch(sola_step_kernel<true, true, true>); else launch(sola_step_kernel<false, true, true>); }
        else if (pro) { if (vec) launch(sola_step_kernel<true, true, false>); else launch(sola_step_kernel<false, true, false>); }
        else { if (vec) launch(sola_step_kernel<true, false, false>); else launch(sola_step_kernel<false, false, false>); }
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
}  // namespace

extern "C" int svc_sola_step(const float* wave, long long stride, int start, int N, float* sola_state, int max_slots,
                             const int32_t* slots, const float* fade_in, const float* fade_out, int block, int Lb, int Ls,
                             float* out, int32_t* offsets, void* stream) {
    return sola_launch("sola_step", wave, stride, start, N, sola_state, max_slots, slots, fade_in, fade_out, block, Lb, Ls, out, offsets,
                       nullptr, 0, nullptr, nullptr, nullptr, false, stream);
}

extern "C" int svc_rt_out(const svc_resampler_t* r, const float* wave, long long stride, int start, int n_in, int N, float* sola_state,
                          int max_slots, const int32_t* slots, const int32_t* speech, const float* fade_in, const float* fade_out,
                          int block, int Lb, int Ls, float* infer, float* out, int32_t* offsets, void* stream) {
    return sola_launch("rt_out", wave, stride, start, N, sola_state, max_slots, slots, fade_in, fade_out, block, Lb, Ls, out, offsets,
                       r, n_in, speech, nullptr, infer, true, stream);
}

extern "C" int svc_rt_out_dev(const svc_resampler_t* r, const float* wave, long long stride, int start, int n_in, int N, float* sola_state,
                              int max_slots, const int32_t* slots, const int32_t* speech, const int32_t* speech_dev, const float* fade_in,
                              const float* fade_out, int block, int Lb, int Ls, float* infer, float* out, int32_t* offsets, void* stream) {
    return sola_launch("rt_out_dev", wave, stride, start, N, sola_state, max_slots, slots, fade_in, fade_out, block, Lb, Ls, out, offsets,
                       r, n_in, speech, speech_dev, infer, true, stream);
}
