// Real-time sessions: the SOLA splice of the reference GUI's audio callback (real-time-gui.py, `audio_callback`, restated
// from memory) as ONE launch per 64 streams: offset search, cross-fade, state update and block copy.  The offset is
// data-dependent, so doing all four on the device lets a block step be enqueued from host integers alone.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.h"

namespace svc {
namespace {
constexpr int SOLA_MAXN = 64;                 // streams per launch: their slots travel as kernel arguments
constexpr int SOLA_THREADS = 256;
constexpr int SOLA_LDS_FLOATS = 16128;        // 63 KiB of samples beside the argmax scratch: 2 * Lb + Ls must fit
struct SolaSlots { int slot[SOLA_MAXN]; };

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
template <bool VEC>
__global__ __launch_bounds__(SOLA_THREADS) void sola_step_kernel(const float* __restrict__ wave, long stride, int start,
                                                                 float* __restrict__ state, const SolaSlots slots,
                                                                 const float* __restrict__ fade_in, const float* __restrict__ fade_out,
                                                                 int block, int Lb, int Ls, float* __restrict__ out,
                                                                 int* __restrict__ offsets) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* red_s = lds;                                   // [4] best score of each wave
    int* red_o = reinterpret_cast<int*>(lds + 4);         // [4] its offset, [4]: the winner
    float* bs = lds + 16;                                 // [Lb rounded up to 4] old buffer
    float* xs = bs + ((Lb + 3) & ~3);                     // [Lb + Ls] input the search reads
    const int k = blockIdx.x, tid = threadIdx.x;
    const float* x = wave + (long)k * stride + start;
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

extern "C" int svc_sola_step(const float* wave, long long stride, int start, int N, float* sola_state, int max_slots,
                             const int32_t* slots, const float* fade_in, const float* fade_out, int block, int Lb, int Ls,
                             float* out, int32_t* offsets, void* stream) {
    SVC_REQUIRE(N >= 0 && stride >= 0 && start >= 0 && max_slots >= 0, "sola_step: negative argument");
    SVC_REQUIRE(block >= 1 && Lb >= 1 && Ls >= 0, "sola_step: block and Lb must be at least 1, Ls at least 0");
    SVC_REQUIRE((long long)start + block + Lb + Ls <= stride, "sola_step: start + block + Lb + Ls lies past the row (stride)");
    SVC_REQUIRE(2LL * Lb + Ls <= SOLA_LDS_FLOATS, "sola_step: 2 * Lb + Ls above 16128 samples (the search is staged in LDS)");
    if (N == 0) return 0;
    SVC_REQUIRE(wave && sola_state && slots && fade_in && fade_out && out, "sola_step: null argument");
    std::vector<int32_t> sorted(slots, slots + N);
    std::sort(sorted.begin(), sorted.end());
    SVC_REQUIRE(sorted.front() >= 0 && sorted.back() < max_slots, "sola_step: a slot outside 0 .. max_slots - 1");
    SVC_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "sola_step: a slot appears twice in one call");
    const bool vec = block % 4 == 0 && Lb % 4 == 0 &&
                     (((uintptr_t)sola_state | (uintptr_t)out | (uintptr_t)fade_in | (uintptr_t)fade_out) & 15) == 0;
    const size_t lds = (size_t)(16 + ((Lb + 3) & ~3) + Lb + Ls) * sizeof(float);
    for (int k0 = 0; k0 < N; k0 += SOLA_MAXN) {
        const int nk = std::min(N - k0, SOLA_MAXN);
        SolaSlots s;
        memset(&s, 0, sizeof(s));
        for (int k = 0; k < nk; ++k) s.slot[k] = slots[k0 + k];
        const float* w = wave + (long long)k0 * stride;
        float* o = out + (long long)k0 * block;
        int32_t* off = offsets ? offsets + k0 : nullptr;
        if (vec)
            hipLaunchKernelGGL(sola_step_kernel<true>, dim3(nk), dim3(SOLA_THREADS), lds, (hipStream_t)stream, w, (long)stride, start,
                               sola_state, s, fade_in, fade_out, block, Lb, Ls, o, off);
        else
            hipLaunchKernelGGL(sola_step_kernel<false>, dim3(nk), dim3(SOLA_THREADS), lds, (hipStream_t)stream, w, (long)stride, start,
                               sola_state, s, fade_in, fade_out, block, Lb, Ls, o, off);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
