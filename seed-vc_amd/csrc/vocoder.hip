// BigVGAN-v2 and HiFT mel -> waveform vocoders on the tap-GEMM (channels-last activations).
//
// Layout: every activation is [B][L][Cpad] (channels contiguous, Cpad = C rounded up to the k-tile: 32
// fp32 / 64 fp16, pad channels are kept at zero).  Conv1d = k-tap GEMM over shifted rows (zero pad),
// ConvTranspose1d(k = 2s, p = s/2) = 3-tap GEMM with N = s * Cpad_out whose output row q holds output
// samples s*q .. s*q+s-1, i.e. it IS the channels-last up-sampled tensor.  precision 0 runs the
// contractions on the fp32 MFMA (exact fp32 products, needed for the 1e-4 waveform RMS parity bar);
// precision 1 feeds fp16 operands (fp32 accumulate); precision 2 ("fp16x3") splits every operand into fp16
// hi + lo planes and issues the three significant products hi*hi + hi*lo + lo*hi on the fp16 MFMA (fp32
// accumulate): ~2^-22 relative product error (fp32-class results) at 3/16 of the fp32-MFMA cycles.
//
// Ragged batches (svc_bigvgan_forward_ragged, svc_hift_forward_ragged): utterances of different lengths in one call, longest
// first in micro-batches padded to their own longest member, each row being that of the utterance run alone.  BigVGAN masks the
// producers of conv operands (its activations are kernels of their own); HiFT, whose Snake is fused into the conv epilogues,
// bounds every conv's operand LOAD instead (tap-GEMM seq_len, resident-tile conv's ragged form) and ends the source, the STFT
// and the overlap-add at each utterance's own last sample.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <vector>

#include "conv_util.h"
#include "noise.h"
#include "range_census.h"

using namespace svc;

namespace {


// ---- small kernels -------------------------------------------------------------------------------
// snake parameter preparation: mode 0 BigVGAN log-scale snakebeta (alpha, beta), 1 log-scale snake (alpha only),
// 2 HiFT linear snake.  out a[c], inv_b[c]
__global__ void snake_params_kernel(const float* alpha, const float* beta, float* a, float* inv_b, int C, int mode) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float al = alpha[c], be = beta ? beta[c] : alpha[c];
    if (mode != 2) { al = expf(al); be = expf(be); }
    a[c] = al;
    inv_b[c] = 1.0f / (be + 1e-9f);
}

// How the rows of a micro-batch map onto the caller's batch, for the pointwise stages that serve the plain and the ragged call
// alike.  Plain call (the default): row j is utterance j of the pointers handed in and all S frames are valid.  Ragged call: row
// j is utterance src[j] of the caller's whole tensors and ends after len[j] frames.
struct RowMap {
    const int* src = nullptr;   // device [B], or null: row j is utterance j
    const int* len = nullptr;   // device [B] valid frames, or null: all S
    int S_in = 0;               // frames per utterance of the caller's tensors (their row stride); S in a plain call
    __device__ __forceinline__ int utt(int b) const { return src ? src[b] : b; }
    __device__ __forceinline__ int frames(int b, int S) const { return len ? len[b] : S; }
};

// (.., C, S_in) fp32 -> channels-last [B][S][ld] in fp32 or fp16, pad channels zero.  Frames at and above the row's end become zero
// rows by selection (they may hold NaN, and 0 * NaN is NaN) and are never loaded
template <typename OutT>
__global__ void mel_to_cl_kernel(const float* __restrict__ mel, OutT* __restrict__ dst, OutT* __restrict__ dst_lo, RowMap rm, int B,
                                 int C, int S, int ld) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * S * ld) return;
    const int c = (int)(i % ld);
    const long bs = i / ld;
    const int s = (int)(bs % S), b = (int)(bs / S);
    float v = 0.f;
    if (c < C && s < rm.frames(b, S)) v = mel[((long)rm.utt(b) * C + c) * rm.S_in + s];
    const OutT h = (OutT)v;
    dst[i] = h;
    if (dst_lo) dst_lo[i] = (OutT)(v - (float)h);
}

// Ragged batch, last step: waveform row j of the micro-batch ([B][L], L <= Lw) -> row src[j] of the caller's [..][Lw] output,
// samples at and above lens[j] written as zero (w is not read there)
__global__ void wave_scatter_kernel(const float* __restrict__ w, float* __restrict__ out, const int* __restrict__ src,
                                    const int* __restrict__ lens, int B, long L, long Lw) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * Lw) return;
    const int b = (int)(i / Lw);
    const long n = i - (long)b * Lw;
    out[(long)src[b] * Lw + n] = n < lens[b] ? w[(long)b * L + n] : 0.f;
}

// elementwise channels-last: y = f(x) with pad channels zeroed. mode 2 leaky relu, 3 identity (cast)
template <typename OutT>
__global__ void ew_cl_kernel(const float* __restrict__ x, OutT* __restrict__ y, OutT* __restrict__ y_lo, long rows, int C, int ld,
                             int mode, float slope) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ld) return;
    const int c = (int)(i % ld);
    float v = c < C ? x[i] : 0.f;
    if (mode == 2) v = v > 0.f ? v : v * slope;
    const OutT h = (OutT)v;
    y[i] = h;
    if (y_lo) y_lo[i] = (OutT)(v - (float)h);
}

__global__ void copy_row_kernel(float* x, int B, int rows, int ld, int src_row, int dst_row) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * ld) return;
    const int b = i / ld, c = i - b * ld;
    x[((long)b * rows + dst_row) * ld + c] = x[((long)b * rows + src_row) * ld + c];
}

// ---- HiFT source / STFT / iSTFT ---------------------------------------------------------------------
// per (b, harmonic): exclusive prefix over frames of up * (double) v_f, v_f = fp32((f0 * (h+1)) / sr)
__global__ void hift_phase_prefix_kernel(const float* __restrict__ f0, double* __restrict__ prefix, int B, int S, int NH, int up,
                                         float sr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * NH) return;
    const int b = i / NH, h = i - b * NH;
    double acc = 0.0;
    for (int f = 0; f < S; ++f) {
        prefix[((long)b * NH + h) * S + f] = acc;
        const float v = (f0[(long)b * S + f] * (float)(h + 1)) / sr;
        // the reference adds the value `up` times in a double accumulator (torch.cumsum on CPU floats);
        // up * v is exact in double, so this differs from the sequential sum by < 1e-13 relative
        acc += (double)up * (double)v;
    }
}

// The randn_like draw of one sample (generator.py:222), harmonic by harmonic in ascending order: loaded from the caller's
// tensor ...
struct HiftNoiseLoad {
    typedef const float* Src;       // the caller's [..][NH][ld] draws
    const float* __restrict__ p;    // the utterance's [NH][ld] rows, already at sample n
    long ld;
    __device__ __forceinline__ HiftNoiseLoad(Src noise, int u, int NH, long n, long ld_) : p(noise + (long)u * NH * ld_ + n), ld(ld_) {}
    __device__ __forceinline__ float operator()(int h) { return p[(long)h * ld]; }
};
// ... or drawn here from the utterance's seed (noise.h, domain NOISE_HIFT_SOURCE: row = harmonic, pos = sample; one Philox call
// per four harmonics, three for NH = 9).  No [NH][S * up] tensor exists on this path.
struct HiftNoiseDraw {
    typedef const unsigned long long* Src;      // the caller's [..] seeds
    unsigned long long seed;
    unsigned pos;
    float n[4];
    __device__ __forceinline__ HiftNoiseDraw(Src seeds, int u, int, long n_, long) : seed(seeds[u]), pos((unsigned)n_), n{} {}
    __device__ __forceinline__ float operator()(int h) {
        if ((h & 3) == 0) noise_normal4(seed, NOISE_HIFT_SOURCE, (unsigned)h >> 2, pos, n);
        return (h & 3) == 0 ? n[0] : (h & 3) == 1 ? n[1] : (h & 3) == 2 ? n[2] : n[3];
    }
};

// merged source sample: tanh(sum_h lin_w[h] * (sine_h * uv + noise_amp * noise_h) + lin_b) at sample r of frame f.
// prefix: this utterance's [NH][S] rows; phase0: its [NH]; noise(h): its draw for harmonic h at this sample
template <typename Noise>
__device__ __forceinline__ float hift_source_sample(float f0v, const double* __restrict__ prefix, const float* __restrict__ phase0,
                                                    Noise noise, const float* __restrict__ lin_w,
                                                    const float* __restrict__ lin_b, int S, int NH, int f, int r, float sr,
                                                    float sine_amp, float noise_std, float voiced_thr) {
    const float uv = f0v > voiced_thr ? 1.f : 0.f;
    const float namp = uv * noise_std + (1.f - uv) * sine_amp / 3.f;
    const float two_pi = 6.283185307179586f;
    float acc = lin_b[0];
    for (int h = 0; h < NH; ++h) {
        const float v = (f0v * (float)(h + 1)) / sr;
        const double cum = prefix[(long)h * S + f] + (double)(r + 1) * (double)v;
        const float cf = (float)cum;
        const float frac = fmodf(cf, 1.0f);
        const float theta = two_pi * frac;
        const float ph = h == 0 ? 0.f : phase0[h];
        const float sine = sine_amp * sinf(theta + ph);
        const float val = sine * uv + namp * noise(h);
        acc += lin_w[h] * val;
    }
    return tanhf(acc);
}

// Row j of the micro-batch ([B][S] frames) is utterance u = rm.utt(j) of phase0 [..][NH] and of the noise source: draws
// [..][NH][S_in * up], of which it uses the first frames * up samples of its rows (the draws of the run alone), or seeds [..], from
// which it draws at its own sample index -- the draws of the run alone whatever the row, the padding and the micro-batch.  f0 and
// prefix are the micro-batch's own [B][S] / [B][NH][S].  Samples past the row's end are written as zero and nothing is read for them.
template <typename Noise>
__global__ void hift_source_kernel(const float* __restrict__ f0, const double* __restrict__ prefix, const float* __restrict__ phase0,
                                   typename Noise::Src noise, const float* __restrict__ lin_w, const float* __restrict__ lin_b,
                                   float* __restrict__ s_out, RowMap rm, int B, int S, int NH, int up, float sr, float sine_amp,
                                   float noise_std, float voiced_thr) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long Lw = (long)S * up;
    if (i >= B * Lw) return;
    const int b = (int)(i / Lw);
    const long n = i - (long)b * Lw;
    const int f = (int)(n / up), r = (int)(n - (long)f * up);
    float v = 0.f;
    if (f < rm.frames(b, S)) {
        const int u = rm.utt(b);
        v = hift_source_sample(f0[(long)b * S + f], prefix + (long)b * NH * S, phase0 + (long)u * NH,
                               Noise(noise, u, NH, n, (long)rm.S_in * up), lin_w, lin_b, S, NH, f, r, sr, sine_amp, noise_std, voiced_thr);
    }
    s_out[i] = v;
}

// Ragged batch: the caller's f0 [..][S_in] -> the micro-batch's [B][S], values at and above lens[j] zero by selection (never loaded)
__global__ void f0_gather_kernel(const float* __restrict__ f0, float* __restrict__ dst, const int* __restrict__ src,
                                 const int* __restrict__ lens, int B, int S, int S_in) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * S) return;
    const int b = (int)(i / S), f = (int)(i - (long)b * S);
    dst[i] = f < lens[b] ? f0[(long)src[b] * S_in + f] : 0.f;
}

// centred, reflect-padded STFT (n_fft 16, hop 4, periodic Hann): out [B][F][ld]: channels 0..8 real, 9..17 imag
// one frame: s = the utterance's Lw samples, o = its output row
__device__ __forceinline__ void hift_stft_frame(const float* __restrict__ s, float* __restrict__ o, long Lw, int fr, int ld) {
    float x[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) {
        long q = 4L * fr - 8 + n;
        if (q < 0) q = -q;
        if (q >= Lw) q = 2 * (Lw - 1) - q;
        const float w = 0.5f - 0.5f * cosf(6.283185307179586f * (float)n / 16.0f);
        x[n] = s[q] * w;
    }
    for (int k = 0; k < 9; ++k) {
        float re = 0.f, im = 0.f;
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const int kn = (k * n) & 15;
            const float ang = 6.283185307179586f * (float)kn / 16.0f;
            re += x[n] * cosf(ang);
            im -= x[n] * sinf(ang);
        }
        o[k] = re;
        o[9 + k] = im;
    }
    for (int c = 18; c < ld; ++c) o[c] = 0.f;
}

// lw, nf (device [B], ragged batch; null: Lw samples and F frames each): utterance b holds lw[b] samples of its Lw-sample row and
// gets nf[b] = lw[b] / 4 + 1 frames, reflected at ITS last sample; frame rows at and above nf[b] are written as zero (the
// source_downs convs read them as their zero padding)
__global__ void hift_stft_kernel(const float* __restrict__ s, float* __restrict__ out, const int* __restrict__ lw,
                                 const int* __restrict__ nf, int B, long Lw, int F, int ld) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * F) return;
    const int b = (int)(i / F), fr = (int)(i - (long)b * F);
    float* o = out + i * ld;
    if (fr < (nf ? nf[b] : F)) hift_stft_frame(s + (long)b * Lw, o, lw ? lw[b] : Lw, fr, ld);
    else for (int c = 0; c < ld; ++c) o[c] = 0.f;
}

// conv_post output [B][F][ld] (9 log-magnitudes | 9 phase pre-activations) -> windowed time frames [B][F][16]
__global__ void hift_frames_kernel(const float* __restrict__ x, float* __restrict__ frames, long BF, int ld) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BF) return;
    const float* v = x + i * ld;
    float re[9], im[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float mag = fminf(expf(v[k]), 1e2f);
        const float ph = sinf(v[9 + k]);
        re[k] = mag * cosf(ph);
        im[k] = mag * sinf(ph);
    }
    for (int n = 0; n < 16; ++n) {
        float acc = re[0] + ((n & 1) ? -re[8] : re[8]);
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            const int kn = (k * n) & 15;
            const float ang = 6.283185307179586f * (float)kn / 16.0f;
            acc += 2.f * (re[k] * cosf(ang) - im[k] * sinf(ang));
        }
        const float w = 0.5f - 0.5f * cosf(6.283185307179586f * (float)n / 16.0f);
        frames[i * 16 + n] = acc * (1.0f / 16.0f) * w;
    }
}

// overlap-add + window-envelope normalisation + trim + clamp: out [B][Lw]
// sample n of an utterance: frames = its [F][16] rows
__device__ __forceinline__ float hift_ola_sample(const float* __restrict__ frames, int F, long n, float limit) {
    const long p = n + 8;                         // index in the untrimmed signal
    float acc = 0.f, env = 0.f;
    const long f_hi = p / 4;
    for (int j = 0; j < 4; ++j) {
        const long f = f_hi - j;
        if (f < 0 || f >= F) continue;
        const int o = (int)(p - 4 * f);
        if (o < 0 || o >= 16) continue;
        const float w = 0.5f - 0.5f * cosf(6.283185307179586f * (float)o / 16.0f);
        acc += frames[f * 16 + o];
        env += w * w;
    }
    const float v = acc / env;
    return fminf(fmaxf(v, -limit), limit);
}

// Last step: row j of the micro-batch overlap-adds its frames (of the F-frame row) into row rm.utt(j) of the [..][Lw_out] output,
// Lw_out = S_in * up.  lw, nf (device [B], ragged batch; null: Lw_out samples from F frames each): samples at and above lw[j] are
// written as zero and no frame is read for them; the others come from the utterance's own nf[j] frames
__global__ void hift_ola_kernel(const float* __restrict__ frames, float* __restrict__ out, RowMap rm, const int* __restrict__ lw,
                                const int* __restrict__ nf, int B, int F, long Lw_out, float limit) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * Lw_out) return;
    const int b = (int)(i / Lw_out);
    const long n = i - (long)b * Lw_out;
    out[(long)rm.utt(b) * Lw_out + n] = !lw || n < lw[b] ? hift_ola_sample(frames + (long)b * F * 16, nf ? nf[b] : F, n, limit) : 0.f;
}

__global__ void abs_copy_kernel(const float* __restrict__ src, long ld, float* __restrict__ dst, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = fabsf(src[i * ld]);
}

// writable operand planes of a model (hi, and lo in split mode)
struct ActOut {
    void* hi = nullptr;
    void* lo = nullptr;
    ActBuf in() const { ActBuf a; a.hi = hi; a.lo = lo; return a; }
};

int ew_cl(const float* x, ActOut y, int vd, long rows, int C, int ld, int mode, float slope, hipStream_t st) {
    const long n = rows * ld;
    if (vd != 1)
        hipLaunchKernelGGL(ew_cl_kernel<half_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, x, (half_t*)y.hi,
                           is_split(vd) ? (half_t*)y.lo : nullptr, rows, C, ld, mode, slope);
    else
        hipLaunchKernelGGL(ew_cl_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, x, (float*)y.hi, (float*)nullptr, rows, C, ld,
                           mode, slope);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int mel_to_cl(const float* mel, ActOut dst, int vd, RowMap rm, int B, int C, int S, int ld, hipStream_t st) {
    const long n = (long)B * S * ld;
    if (vd != 1)
        hipLaunchKernelGGL(mel_to_cl_kernel<half_t>, dim3(cdiv(n, 256)), dim3(256), 0, st, mel, (half_t*)dst.hi,
                           is_split(vd) ? (half_t*)dst.lo : nullptr, rm, B, C, S, ld);
    else
        hipLaunchKernelGGL(mel_to_cl_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, mel, (float*)dst.hi, (float*)nullptr, rm, B, C, S,
                           ld);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// The HiFT signal stages' launches, one function each: svc_hift::run and the parity tests' svc_op_hift_signal call the same
// launch geometry.
// phase prefix + merged source: draws from `seeds` ([..] per utterance) when given, else loaded from `noise`
int hift_source_launch(const float* f0, double* prefix, const float* phase0, const float* noise, const unsigned long long* seeds,
                       const float* lin_w, const float* lin_b, float* s_out, RowMap rm, int B, int S, int NH, int up, float sr,
                       float sine_amp, float noise_std, float voiced_thr, hipStream_t st) {
    hipLaunchKernelGGL(hift_phase_prefix_kernel, dim3(cdiv(B * NH, 64)), dim3(64), 0, st, f0, prefix, B, S, NH, up, sr);
    SVC_CHECK_HIP(hipGetLastError());
    const long Lw = (long)S * up;
    auto source = [&](auto kernel, auto draws) {
        hipLaunchKernelGGL(kernel, dim3(cdiv((long)B * Lw, 256)), dim3(256), 0, st, f0, prefix, phase0, draws, lin_w, lin_b, s_out,
                           rm, B, S, NH, up, sr, sine_amp, noise_std, voiced_thr);
    };
    if (seeds) source(hift_source_kernel<HiftNoiseDraw>, seeds);
    else source(hift_source_kernel<HiftNoiseLoad>, noise);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int hift_stft_launch(const float* s, float* out, const int* lw, const int* nf, int B, long Lw, int F, int ld, hipStream_t st) {
    hipLaunchKernelGGL(hift_stft_kernel, dim3(cdiv((long)B * F, 256)), dim3(256), 0, st, s, out, lw, nf, B, Lw, F, ld);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int hift_frames_launch(const float* post, float* frames, long BF, int ld, hipStream_t st) {
    hipLaunchKernelGGL(hift_frames_kernel, dim3(cdiv(BF, 256)), dim3(256), 0, st, post, frames, BF, ld);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int hift_ola_launch(const float* frames, float* out, RowMap rm, const int* lw, const int* nf, int B, int F, long Lw_out, float limit,
                    hipStream_t st) {
    hipLaunchKernelGGL(hift_ola_kernel, dim3(cdiv((long)B * Lw_out, 256)), dim3(256), 0, st, frames, out, rm, lw, nf, B, F, Lw_out,
                       limit);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

struct SnakeP {
    float* a = nullptr;
    float* inv_b = nullptr;
};

int make_snake(const StateDict& sd, const std::string& alpha_key, const std::string& beta_key, int C, int mode, Arena& ar,
               hipStream_t st, SnakeP* out) {
    const auto* al = sd.get(alpha_key);
    if (require_shape(al, alpha_key, {C})) return 1;
    const float* be = nullptr;
    if (!beta_key.empty()) {
        const auto* b = sd.get(beta_key);
        if (require_shape(b, beta_key, {C})) return 1;
        be = b->data;
    }
    out->a = ar.alloc_n<float>(C, st);
    out->inv_b = ar.alloc_n<float>(C, st);
    if (!out->a || !out->inv_b) return 1;
    hipLaunchKernelGGL(snake_params_kernel, dim3(cdiv(C, 256)), dim3(256), 0, st, al->data, be, out->a, out->inv_b, C, mode);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// One residual pair-stack "AMPBlock1 / ResBlock": for d in dils: xt = act(y); xt = c1(xt); xt = act(xt); xt = c2(xt); y = xt + y
struct ResBlockW {
    int k = 0, ch = 0, ndil = 0;
    int dil[3] = {1, 1, 1};
    ConvW c1[3], c2[3];
    SnakeP a1[3], a2[3];
    int cand1[3] = {-1, -1, -1}, cand2[3] = {-1, -1, -1};   // index of c1[d] / c2[d] in the handle's precision plan, -1: no candidate
};

// The precision plan of an fp16p8 handle: its p8 candidates -- the ResBlock convs that own the fp8 packing -- in model order,
// each with its state-dict prefix.  The veto itself lives in the conv (ConvW::p8_veto), where conv_p8_ok reads it.
struct P8Plan {
    std::vector<ConvW*> conv;
    std::vector<std::string> name;
    int size() const { return (int)conv.size(); }
    void add(ResBlockW& rb, const std::string& prefix) {
        for (int d = 0; d < rb.ndil; ++d) {
            ConvW* c[2] = {&rb.c1[d], &rb.c2[d]};
            int* idx[2] = {&rb.cand1[d], &rb.cand2[d]};
            for (int i = 0; i < 2; ++i) {
                if (!c[i]->w8) continue;
                *idx[i] = size();
                conv.push_back(c[i]);
                name.push_back(prefix + (i == 0 ? ".convs1." : ".convs2.") + std::to_string(d));
            }
        }
    }
};

// Where a calibration forward leaves the census of each candidate's operand planes (resblock_run): rec[i] (device)
// accumulates candidate i's records over the micro-batches in stream order; L[i] (host) keeps its rows per utterance
struct CensusSink {
    svc_census_t* rec = nullptr;
    svc_census_t* part = nullptr;
    long part_cap = 0;
    int* L = nullptr;
    int take(int cand, const ActBuf& a, int B, int L_, int C, int ld, const int* lens, hipStream_t st) const {
        if (cand < 0) return 0;
        L[cand] = std::max(L[cand], L_);
        return census_launch(a.hi, a.lo, B, L_, C, ld, lens, rec + cand, part, part_cap, st);
    }
};

// One micro-batch of a ragged call (device pointers into the call's length table): row j is utterance src[j] of the caller's
// batch and holds len[i][j] valid rows after i up-sampling stages
struct RaggedMB {
    int nb = 0, S = 0;      // its rows, and the frames of the longest of them (row 0)
    const int* src = nullptr;
    const int* len[9] = {};
    int S_in = 0;           // frames per utterance of the caller's mel (its row stride)
    const int* lw = nullptr;        // HiFT only: waveform samples per row (device)
    const int* h_len0 = nullptr;    // the rows' frame counts on the host (len[0] again)
    RowMap rows() const { return RowMap{src, len[0], S_in}; }
};

// The batch plan of a ragged call, one for both vocoders.  Longest first, micro-batch by micro-batch, each padded to its own
// longest member only: a batch padded to the longest utterance of all would compute B * Smax rows.  The stable sort keeps the
// order of equal lengths, so a batch of equal lengths runs exactly as the plain call runs it.
struct RaggedPlan {
    PinnedRing staging;     // pinned slots for what the host builds per call: the length table (and a seeded call's seeds)
    Arena tab;              // the table's device copy
    int* d_tab = nullptr;
    size_t tab_cap = 0;
    std::vector<int> first;             // the first row of each micro-batch, then B
    const int* h_tab = nullptr;         // this call's table in its pinned slot
    int nu = 0, n_arr = 0, S_in = 0;
    bool has_lw = false;
    int nb_max = 0, S_max = 0;          // the largest micro-batch and the longest utterance: one workspace reservation per call

    // lens: HOST [B].  Comes first in a ragged call: before the handle is touched or anything is launched
    static int check(const char* who, const int32_t* lens, int B, int S) {
        for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 0 && lens[b] <= S, std::string(who) + ": lens out of range");
        return 0;
    }
    // A micro-batch ends after `microbatch` members (0: 32) or where cls(length) changes (cls empty: nowhere else).
    // rows_after(i, l): valid rows of an utterance of l frames after i of the nu up-sampling stages.  lw_up > 0: a row's
    // lw = l * lw_up waveform samples as well.
    // Length table, per micro-batch of nb rows: src[nb], the valid rows after 0 .. nu stages ([nb] each), lw[nb].  Built in a
    // pinned slot and copied once: the caller's array is consumed here and nothing waits for the stream.
    int build(const int32_t* lens, int B, int S, int microbatch, int nu_, const std::function<long(int, long)>& rows_after,
              const std::function<int(long)>& cls, int lw_up, hipStream_t st) {
        std::vector<int> order(B);
        for (int b = 0; b < B; ++b) order[b] = b;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lens[a] > lens[b]; });
        const int mb = microbatch > 0 ? microbatch : 32;
        first.clear();
        for (int b = 0; b < B; ++b)
            if (b == 0 || b - first.back() == mb || (cls && cls(lens[order[b]]) != cls(lens[order[first.back()]]))) first.push_back(b);
        first.push_back(B);
        nu = nu_; S_in = S; has_lw = lw_up > 0;
        n_arr = nu + 2 + (has_lw ? 1 : 0);
        const size_t n_tab = (size_t)B * n_arr;
        if (n_tab > tab_cap) {
            SVC_CHECK_HIP(hipStreamSynchronize(st));
            tab.release();
            d_tab = tab.alloc_n<int>(n_tab, st);
            if (!d_tab) { tab_cap = 0; return 1; }
            tab_cap = n_tab;
        }
        int* h = reinterpret_cast<int*>(staging.acquire(n_tab * sizeof(int)));
        if (!h) return 1;
        h_tab = h;
        nb_max = 0;
        S_max = lens[order[0]];
        for (int k = 0; k < count(); ++k) {
            const int b0 = first[k], nb = first[k + 1] - b0;
            nb_max = std::max(nb_max, nb);
            int* row = h + (size_t)b0 * n_arr;
            for (int j = 0; j < nb; ++j) {
                const long l = lens[order[b0 + j]];
                row[j] = order[b0 + j];
                for (int i = 0; i <= nu; ++i) row[(size_t)(i + 1) * nb + j] = (int)rows_after(i, l);
                if (has_lw) row[(size_t)(nu + 2) * nb + j] = (int)(l * lw_up);
            }
        }
        SVC_CHECK_HIP(hipMemcpyAsync(d_tab, h, n_tab * sizeof(int), hipMemcpyHostToDevice, st));
        return staging.commit(st);
    }
    int count() const { return (int)first.size() - 1; }
    RaggedMB mb(int k) const {
        const int b0 = first[k];
        RaggedMB rg;
        rg.nb = first[k + 1] - b0;
        const int* row = d_tab + (size_t)b0 * n_arr;
        rg.src = row;
        for (int i = 0; i <= nu; ++i) rg.len[i] = row + (size_t)(i + 1) * rg.nb;
        if (has_lw) rg.lw = row + (size_t)(nu + 2) * rg.nb;
        rg.h_len0 = h_tab + (size_t)b0 * n_arr + rg.nb;
        rg.S = rg.h_len0[0];
        rg.S_in = S_in;
        return rg;
    }
};

// A micro-batch of nothing but empty utterances (they sort last): rows src[j] of the caller's [..][row_len] output are all tail
int zero_rows(const RaggedMB& rg, float* out, long row_len, hipStream_t st) {
    hipLaunchKernelGGL(wave_scatter_kernel, dim3(cdiv((long)rg.nb * row_len, 256)), dim3(256), 0, st, (const float*)nullptr, out, rg.src,
                       rg.len[0], rg.nb, 0L, row_len);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

// ================================================================================================ BigVGAN
struct svc_bigvgan {
    svc_bigvgan_config_t cfg;
    int dtype;          // kgemm dtype: 1 = f32 (precision 0), 0 = f16 (precision 1)
    Arena wts, ws;
    ConvW conv_pre, conv_post;
    std::vector<ConvW> ups;
    std::vector<ResBlockW> blocks;
    SnakeP act_post;
    float taps[12];
    int cap_B = 0, cap_S = 0;
    ActOut mel_a, act_a;
    float *x, *y, *t, *xsum;
    int microbatch = 0;
    RaggedPlan plan;    // ragged calls
    P8Plan p8;          // precision plan (dtype == 3)
    const CensusSink* sink = nullptr;   // set for the forward of svc_bigvgan_calibrate only

    int reserve(int B, int S, hipStream_t st);
    // rg == null: B utterances of S frames each.  rg != null: micro-batch of a ragged call, `mel` / `out` are the caller's
    // whole tensors and S the micro-batch's longest member
    int run(const float* mel, int B, int S, float* out, hipStream_t st, const RaggedMB* rg = nullptr);
};

namespace {
int act_cl_any(const float* x, int ld, ActOut y, int vd, const float* taps, const SnakeP& sp, int B, int C, int L, int mode,
               float slope, hipStream_t st, int lo_fmt = 0, const int* lens = nullptr) {
    return act_cl_launch(x, ld, y.hi, is_split(vd) ? y.lo : nullptr, ld, vd != 1, taps, sp.a, sp.inv_b, B, C, L, mode, slope, st,
                         is_split(vd) ? lo_fmt : 0, lens);
}

// runs one residual stack on stream buffer `x_in` (read only) producing the block output either into `y`
// (intermediate pairs) and, for the last pair, (y_last) * out_scale + res2 -> final_dst.
// lens (device [B], anti-aliased mode without fusion only): valid rows per sequence.  The activations are the only producers of
// conv operands here, so masking them is enough; the raw conv outputs past lens[b] are garbage that only pointwise ops touch.
// conv_lens (device [B], HiFT's ragged call): the convs themselves treat rows at and above conv_lens[b] as padding.  With the
// pointwise Snake fused into the producing conv's epilogue there is no activation kernel to mask, so the bound sits on each
// conv's operand load (tap-GEMM: seq_len; resident-tile conv: its ragged form) and the operand planes past the end hold anything.
int resblock_run(const ResBlockW& rb, int dtype, const float* taps, int act_mode, const float* x_in, float* y, float* t, ActOut act_a,
                 int B, int L, float out_scale, const float* res2, float* final_dst, hipStream_t st, ActOut act_b = ActOut(),
                 const int* lens = nullptr, const int* conv_lens = nullptr, const CensusSink* sink = nullptr) {
    const int f16 = dtype;      // operand mode handed to the activation writers
    const int ld = cpad(rb.ch, dtype);
    const float* cur = x_in;
    // Pointwise Snake (HiFT) with fp16 operand planes: only the first activation is a kernel of its own; every later
    // one is the epilogue of the conv that produces its input (conv1 -> a2, conv2 -> next pair's a1), writing the hi / lo
    // planes straight into the other operand buffer.  The fp32 intermediate `t` disappears.
    const bool fuse = act_mode == 1 && dtype != 1 && act_b.hi != nullptr;
    // vd == 3: whoever writes a conv's operand planes (an activation kernel or the previous conv's epilogue) writes the lo
    // plane in the format that conv will read: fp8 byte pairs when it runs as fp16 + fp8 corrections (conv_p8_ok).  The
    // decision is per producer / consumer pair: a consumer runs p8 only if its producer can write byte pairs -- an activation
    // kernel always can, a conv only from the resident-tile kernel's epilogue (conv_takes_kconv; an 11-tap conv of dilation 7
    // spans 70 rows and runs on the tap-GEMM).  Otherwise the consumer runs the fp16x3 form on fp16 planes.
    // Returns whether `next` (null: none) runs p8 on the planes r's epilogue writes.
    auto fuse_into = [&](const ConvW& w, ConvRun& r, const SnakeP& sp, const ActOut& dst, const ConvW* next, int next_dil) {
        r.post_a = sp.a; r.post_ib = sp.inv_b; r.post_n = rb.ch;
        r.c16 = reinterpret_cast<half_t*>(dst.hi); r.ldc16 = ld;
        r.c16_lo = is_split(dtype) ? reinterpret_cast<half_t*>(dst.lo) : nullptr;
        const bool next_p8 = dtype == 3 && next && conv_p8_ok(*next, L, next_dil) && conv_takes_kconv(w, r);
        r.c16_lo_fmt = next_p8 ? 1 : 0;
        return next_p8;
    };
    const int* live = lens ? lens : conv_lens;     // the census of a calibration forward stops at each utterance's end
    bool p8_next = false;       // fused path: c1[d + 1] runs p8 (decided when c2[d]'s epilogue was set up)
    for (int d = 0; d < rb.ndil; ++d) {
        const bool p8_1 = fuse && d > 0 ? p8_next : dtype == 3 && conv_p8_ok(rb.c1[d], L, rb.dil[d]);
        bool p8_2 = dtype == 3 && conv_p8_ok(rb.c2[d], L, 1);
        if (!fuse || d == 0) {
            if (act_cl_any(cur, ld, act_a, f16, taps, rb.a1[d], B, rb.ch, L, act_mode, 0.f, st, p8_1, lens)) return 1;
        }
        ConvRun r1;
        r1.a = act_a.in(); r1.B = B; r1.Lin = L; r1.Lout = L; r1.dilation = rb.dil[d];
        r1.pad_left = (rb.k * rb.dil[d] - rb.dil[d]) / 2;
        r1.p8 = p8_1;
        r1.seq_len = conv_lens; r1.seq_kconv = true;
        if (fuse) p8_2 = fuse_into(rb.c1[d], r1, rb.a2[d], act_b, &rb.c2[d], 1);
        else { r1.c32 = t; r1.ldc32 = ld; }
        if (sink && sink->take(rb.cand1[d], r1.a, B, L, rb.ch, ld, live, st)) return 1;
        if (conv1d_run(rb.c1[d], r1, st)) return 1;
        if (!fuse) {
            if (act_cl_any(t, ld, act_a, f16, taps, rb.a2[d], B, rb.ch, L, act_mode, 0.f, st, p8_2, lens)) return 1;
        }
        ConvRun r2;
        r2.a = fuse ? act_b.in() : act_a.in(); r2.B = B; r2.Lin = L; r2.Lout = L; r2.dilation = 1;
        r2.pad_left = (rb.k - 1) / 2;
        r2.p8 = p8_2;
        r2.seq_len = conv_lens; r2.seq_kconv = true;
        r2.res = cur; r2.ldres = ld;
        const bool last = d == rb.ndil - 1;
        if (last) {
            r2.out_scale = out_scale;
            r2.res2 = res2; r2.ldres2 = ld;
            r2.c32 = final_dst; r2.ldc32 = ld;
        } else {
            r2.c32 = y; r2.ldc32 = ld;
            if (fuse) p8_next = fuse_into(rb.c2[d], r2, rb.a1[d + 1], act_a, &rb.c1[d + 1], rb.dil[d + 1]);
        }
        if (sink && sink->take(rb.cand2[d], r2.a, B, L, rb.ch, ld, live, st)) return 1;
        if (conv1d_run(rb.c2[d], r2, st)) return 1;
        cur = y;
    }
    return 0;
}
}  // namespace

int svc_bigvgan::reserve(int B, int S, hipStream_t st) {
    if (B <= cap_B && S <= cap_S) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws.release();
    cap_B = std::max(B, cap_B);
    cap_S = std::max(S, cap_S);
    long L = cap_S;
    long max_el = L * cpad(cfg.upsample_initial_channel, dtype);
    int ch = cfg.upsample_initial_channel;
    for (int i = 0; i < cfg.num_upsamples; ++i) {
        L *= cfg.upsample_rates[i];
        ch /= 2;
        max_el = std::max(max_el, L * cpad(ch, dtype));
    }
    max_el *= cap_B;
    mel_a.hi = ws.alloc((size_t)cap_B * cap_S * cpad(cfg.num_mels, dtype) * vesize(dtype), st);
    mel_a.lo = ws.alloc((size_t)cap_B * cap_S * cpad(cfg.num_mels, dtype) * vesize(dtype), st);
    act_a.hi = ws.alloc((size_t)max_el * vesize(dtype), st);
    act_a.lo = ws.alloc((size_t)max_el * vesize(dtype), st);
    x = ws.alloc_n<float>(max_el, st);
    y = ws.alloc_n<float>(max_el, st);
    t = ws.alloc_n<float>(max_el, st);
    xsum = ws.alloc_n<float>(max_el, st);
    if (!mel_a.hi || !mel_a.lo || !act_a.hi || !act_a.lo || !x || !y || !t || !xsum) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// Ragged micro-batches (rg): every PRODUCER OF A CONV OPERAND respects the lengths -- the mel copy, the transposed convs (which
// read the previous stage's raw output, through the tap-GEMM's per-sequence valid-row array) and the anti-aliased activations
// -- so each conv sees zero rows past an utterance's end exactly as its zero padding would supply them.  The convs themselves
// are unchanged; what they write past lens[b] (x, y, t, xsum) is read only by pointwise ops and by the masked producers.
int svc_bigvgan::run(const float* mel, int B, int S, float* out, hipStream_t st, const RaggedMB* rg) {
    const int vd = dtype;
    const RowMap rm = rg ? rg->rows() : RowMap{nullptr, nullptr, S};
    if (mel_to_cl(mel, mel_a, vd, rm, B, cfg.num_mels, S, cpad(cfg.num_mels, vd), st)) return 1;
    int ch = cfg.upsample_initial_channel;
    long L = S;
    {
        ConvRun r;
        r.a = mel_a.in(); r.B = B; r.Lin = S; r.Lout = S; r.pad_left = 3;
        r.c32 = xsum; r.ldc32 = cpad(ch, vd);
        if (conv1d_run(conv_pre, r, st)) return 1;
    }
    const int nk = cfg.num_kernels;
    for (int i = 0; i < cfg.num_upsamples; ++i) {
        // transposed conv reads the previous stage output (xsum); fp16 / split modes go through a cast copy
        ActBuf a;
        a.hi = xsum;
        if (vd != 1) {
            if (ew_cl(xsum, act_a, vd, (long)B * L, ch, cpad(ch, vd), 3, 0.f, st)) return 1;
            a = act_a.in();
        }
        if (convT_run(ups[i], a, B, (int)L, x, 0, 0, st, rg ? rg->len[i] : nullptr)) return 1;
        L *= cfg.upsample_rates[i];
        ch /= 2;
        for (int j = 0; j < nk; ++j) {
            // x = mean_j block_j(x): block j's last conv writes (y_j) / nk + (j > 0 ? xsum : 0) into xsum
            if (resblock_run(blocks[i * nk + j], vd, taps, 0, x, y, t, act_a, B, (int)L, 1.0f / (float)nk,
                             j > 0 ? xsum : nullptr, xsum, st, ActOut(), rg ? rg->len[i + 1] : nullptr, nullptr, sink)) return 1;
        }
    }
    const int* len_w = rg ? rg->len[cfg.num_upsamples] : nullptr;
    if (act_cl_any(xsum, cpad(ch, vd), act_a, vd, taps, act_post, B, ch, (int)L, 0, 0.f, st, 0, len_w)) return 1;
    {
        ConvRun r;
        r.a = act_a.in(); r.B = B; r.Lin = (int)L; r.Lout = (int)L; r.pad_left = 3;
        r.c32 = rg ? x : out; r.ldc32 = 1; r.n_override = 1;     // x is free after the last stage (B * L <= its B * L * Cpad)
        r.act = cfg.use_tanh_at_final ? KG_ACT_TANH : KG_ACT_CLAMP;
        r.act_slope = 1.0f;
        if (conv1d_run(conv_post, r, st)) return 1;
    }
    if (rg) {   // back to the caller's order and row length, tails zeroed
        const long Lw = (long)rg->S_in * (L / S);
        hipLaunchKernelGGL(wave_scatter_kernel, dim3(cdiv((long)B * Lw, 256)), dim3(256), 0, st, x, out, rg->src, len_w, B, L, Lw);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

namespace {
int pack_resblock(const StateDict& sd, const std::string& p, int ch, int k, const int* dils, int ndil, int dtype, int snake_mode,
                  bool bigvgan_names, bool has_beta, Arena& ar, hipStream_t st, ResBlockW* rb) {
    rb->k = k;
    rb->ch = ch;
    rb->ndil = ndil;
    for (int d = 0; d < ndil; ++d) {
        rb->dil[d] = dils[d];
        const std::string ds = std::to_string(d);
        if (pack_conv1d(sd, p + ".convs1." + ds, ch, ch, k, true, dtype, ar, st, &rb->c1[d])) return 1;
        if (pack_conv1d(sd, p + ".convs2." + ds, ch, ch, k, true, dtype, ar, st, &rb->c2[d])) return 1;
        if (bigvgan_names) {
            const std::string a1 = p + ".activations." + std::to_string(2 * d) + ".act";
            const std::string a2 = p + ".activations." + std::to_string(2 * d + 1) + ".act";
            if (make_snake(sd, a1 + ".alpha", has_beta ? a1 + ".beta" : "", ch, snake_mode, ar, st, &rb->a1[d])) return 1;
            if (make_snake(sd, a2 + ".alpha", has_beta ? a2 + ".beta" : "", ch, snake_mode, ar, st, &rb->a2[d])) return 1;
        } else {
            if (make_snake(sd, p + ".activations1." + ds + ".alpha", "", ch, 2, ar, st, &rb->a1[d])) return 1;
            if (make_snake(sd, p + ".activations2." + ds + ".alpha", "", ch, 2, ar, st, &rb->a2[d])) return 1;
        }
    }
    return 0;
}
}  // namespace

// ================================================================================================ HiFT
struct svc_hift {
    svc_hift_config_t cfg;
    int dtype;
    int microbatch = 0;
    Arena wts, ws;
    ConvW f0_convs[5];
    float *f0_lin_w, *f0_lin_b, *src_lin_w, *src_lin_b;
    ConvW conv_pre, conv_post, ups[2], src_down[2];
    ResBlockW src_rb[2];
    std::vector<ResBlockW> blocks;
    int up_total;
    int cap_B = 0, cap_S = 0;
    ActOut mel_a, act_a, act_b, stft_a;
    void *f0_a, *f0_b;
    float *f0_buf, *s_buf, *stft32, *x, *y, *t, *xsum, *si, *post, *frames;
    double* prefix;
    RaggedPlan plan;    // ragged calls
    P8Plan p8;          // precision plan (dtype == 3)
    const CensusSink* sink = nullptr;   // set for the forward of svc_hift_calibrate only
    // seeded calls: the call's seeds [B] and the phase0 [B][NH] drawn from them (the only draws that are ever stored)
    int device = -1;
    Arena seed_ar;
    unsigned long long* d_seeds = nullptr;
    float* d_phase0 = nullptr;
    int seed_cap = 0;

    int reserve(int B, int S, hipStream_t st);
    // rg == null: B utterances of S frames each.  rg != null: micro-batch of a ragged call; mel / f0 / phase0 / noise / out / f0_out
    // are the caller's whole tensors and S the micro-batch's longest member
    // seeds (device, indexed like phase0) set: the source noise is drawn from them and `noise` is not read
    int run(const float* mel, const float* f0, const float* phase0, const float* noise, int B, int S, float* out, float* f0_out,
            hipStream_t st, const RaggedMB* rg = nullptr, const unsigned long long* seeds = nullptr);
    int forward(const float* mel, const float* f0, const float* phase0, const float* noise, const unsigned long long* seeds, int B,
                int S, float* out, float* f0_out, hipStream_t st);
    int forward_ragged(const float* mel, const int32_t* lens, const float* f0, const float* phase0, const float* noise,
                       const unsigned long long* seeds, int B, int S, float* out, float* f0_out, hipStream_t st);
    // valid rows of an utterance of S frames after `stage` up-sampling stages (the last stage's reflection pad adds one row)
    long rows_after(int stage, long S) const {
        long L = S;
        for (int i = 0; i < stage; ++i) L = L * cfg.upsample_rates[i] + (i == cfg.num_upsamples - 1 && S > 0 ? 1 : 0);
        return L;
    }
    // Which convs of an utterance take the resident-tile kernel depends on its stage lengths alone (KCONV_MIN_ROWS): the number
    // of stages that reach it.  A ragged micro-batch holds utterances of ONE class, so every utterance runs the kernels it
    // would run alone whatever its neighbours are.
    int kernel_class(long S) const {
        int c = 0;
        for (int i = 0; i <= cfg.num_upsamples; ++i) c += rows_after(i, S) >= KCONV_MIN_ROWS;
        return c;
    }
};

int svc_hift::reserve(int B, int S, hipStream_t st) {
    if (B <= cap_B && S <= cap_S) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws.release();
    cap_B = std::max(B, cap_B);
    cap_S = std::max(S, cap_S);
    const long Bc = cap_B, Sc = cap_S;
    const int bc = cfg.base_channels;
    const long F = Sc * (up_total / cfg.istft_hop) + 1;       // frames of the source STFT / output iSTFT
    long max_el = Sc * cpad(bc, dtype);
    {
        long L = Sc;
        int ch = bc;
        for (int i = 0; i < cfg.num_upsamples; ++i) {
            L = L * cfg.upsample_rates[i] + (i == cfg.num_upsamples - 1 ? 1 : 0);
            ch /= 2;
            max_el = std::max(max_el, L * cpad(ch, dtype));
        }
    }
    max_el *= Bc;
    const int fc = cfg.f0_cond_channels;
    mel_a.hi = ws.alloc((size_t)Bc * Sc * cpad(cfg.in_channels, dtype) * vesize(dtype), st);
    mel_a.lo = ws.alloc((size_t)Bc * Sc * cpad(cfg.in_channels, dtype) * vesize(dtype), st);
    // the predictor's ping-pong buffers: f0_a first holds the fp32 channels-last mel (in_channels wide), then both hold fc-wide rows
    const size_t f0_ld = std::max(cpad(fc, 1), cpad(cfg.in_channels, 1));
    f0_a = ws.alloc((size_t)Bc * Sc * f0_ld * 4, st);
    f0_b = ws.alloc((size_t)Bc * Sc * f0_ld * 4, st);
    act_a.hi = ws.alloc((size_t)max_el * vesize(dtype), st);
    act_a.lo = ws.alloc((size_t)max_el * vesize(dtype), st);
    act_b.hi = ws.alloc((size_t)max_el * vesize(dtype), st);
    act_b.lo = ws.alloc((size_t)max_el * vesize(dtype), st);
    stft_a.hi = ws.alloc((size_t)Bc * F * 64 * vesize(dtype), st);
    stft_a.lo = ws.alloc((size_t)Bc * F * 64 * vesize(dtype), st);
    f0_buf = ws.alloc_n<float>(Bc * Sc, st);
    s_buf = ws.alloc_n<float>(Bc * Sc * up_total, st);
    stft32 = ws.alloc_n<float>(Bc * F * 64, st);
    x = ws.alloc_n<float>(max_el, st);
    y = ws.alloc_n<float>(max_el, st);
    t = ws.alloc_n<float>(max_el, st);
    xsum = ws.alloc_n<float>(max_el, st);
    si = ws.alloc_n<float>(max_el, st);
    post = ws.alloc_n<float>(Bc * F * 64, st);
    frames = ws.alloc_n<float>(Bc * F * 16, st);
    prefix = ws.alloc_n<double>(Bc * (cfg.nb_harmonics + 1) * Sc, st);
    if (!mel_a.hi || !mel_a.lo || !f0_a || !f0_b || !act_a.hi || !act_a.lo || !act_b.hi || !act_b.lo || !stft_a.hi || !stft_a.lo || !f0_buf || !s_buf || !stft32 || !x || !y || !t || !xsum || !si ||
        !post || !frames || !prefix)
        return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// Ragged micro-batches (rg): nothing past an utterance's end reaches its rows.  The inputs are gathered by selection (mel, f0)
// or read up to the end only (noise); every conv, the f0 predictor's included, bounds its operand load by the utterance's
// rows at that stage; the source stops at the last sample, the STFT reflects there and gives F_b frames, and the overlap-add
// runs over those F_b frames.  What the convs write past the end (x, y, xsum, si, post and the operand planes) is touched by
// pointwise ops only.
int svc_hift::run(const float* mel, const float* f0_in, const float* phase0, const float* noise, int B, int S, float* out,
                  float* f0_out, hipStream_t st, const RaggedMB* rg, const unsigned long long* seeds) {
    const int vd = dtype;
    const RowMap rm = rg ? rg->rows() : RowMap{nullptr, nullptr, S};
    const int* len0 = rm.len;
    const int NH = cfg.nb_harmonics + 1;
    const long Lw = (long)S * up_total;
    const int F = (int)(Lw / cfg.istft_hop) + 1;
    const int bc = cfg.base_channels;
    // ---- f0 (predictor runs in fp32 MFMA regardless of `precision`: the phase integrates f0 over seconds)
    const float* f0 = f0_in;
    if (!f0) {
        const int fc = cfg.f0_cond_channels, fld = cpad(fc, 1);
        ActOut f0in;
        f0in.hi = f0_a;
        if (mel_to_cl(mel, f0in, 1, rm, B, cfg.in_channels, S, cpad(cfg.in_channels, 1), st)) return 1;
        void* src = f0_a;
        void* dst = f0_b;
        for (int i = 0; i < 5; ++i) {
            ConvRun r;
            r.a.hi = src; r.B = B; r.Lin = S; r.Lout = S; r.pad_left = 1;
            r.c32 = (float*)dst; r.ldc32 = fld; r.act = KG_ACT_ELU;
            r.seq_len = len0;
            if (conv1d_run(f0_convs[i], r, st)) return 1;
            std::swap(src, dst);
        }
        // classifier: Linear(fc -> 1) then abs
        if (small_linear_launch((const float*)src, fld, f0_lin_w, fc, f0_lin_b, f0_buf, 1, B * S, 1, fc, KG_ACT_NONE, st)) return 1;
        hipLaunchKernelGGL(abs_copy_kernel, dim3(cdiv((long)B * S, 256)), dim3(256), 0, st, f0_buf, 1L, f0_buf, (long)B * S);
        SVC_CHECK_HIP(hipGetLastError());
        f0 = f0_buf;
    } else if (rg) {    // the caller's rows, cut to the micro-batch: the prefix below is causal, so the zeros past the end are inert
        hipLaunchKernelGGL(f0_gather_kernel, dim3(cdiv((long)B * S, 256)), dim3(256), 0, st, f0_in, f0_buf, rg->src, len0, B, S, rg->S_in);
        SVC_CHECK_HIP(hipGetLastError());
        f0 = f0_buf;
    }
    if (f0_out) {
        if (rg) {
            hipLaunchKernelGGL(wave_scatter_kernel, dim3(cdiv((long)B * rg->S_in, 256)), dim3(256), 0, st, f0, f0_out, rg->src, len0, B,
                               (long)S, (long)rg->S_in);
            SVC_CHECK_HIP(hipGetLastError());
        } else SVC_CHECK_HIP(hipMemcpyAsync(f0_out, f0, (size_t)B * S * 4, hipMemcpyDeviceToDevice, st));
    }
    // ---- harmonic source + its STFT
    const int ld18 = cpad(cfg.istft_n_fft + 2, dtype);
    const int* len_f = rg ? rg->len[cfg.num_upsamples] : nullptr;      // frames of the STFT / iSTFT = rows of the last stage
    const int* lw = rg ? rg->lw : nullptr;                             // its waveform samples
    if (hift_source_launch(f0, prefix, phase0, noise, seeds, src_lin_w, src_lin_b, s_buf, rm, B, S, NH, up_total,
                           (float)cfg.sampling_rate, cfg.nsf_alpha, cfg.nsf_sigma, cfg.nsf_voiced_threshold, st)) return 1;
    if (hift_stft_launch(s_buf, stft32, lw, len_f, B, Lw, F, ld18, st)) return 1;
    ActBuf stft_in;
    stft_in.hi = stft32;
    if (vd != 1) {
        if (ew_cl(stft32, stft_a, vd, (long)B * F, ld18, ld18, 3, 0.f, st)) return 1;
        stft_in = stft_a.in();
    }
    // ---- main path
    if (mel_to_cl(mel, mel_a, vd, rm, B, cfg.in_channels, S, cpad(cfg.in_channels, dtype), st)) return 1;
    {
        ConvRun r;
        r.a = mel_a.in(); r.B = B; r.Lin = S; r.Lout = S; r.pad_left = 3;
        r.c32 = xsum; r.ldc32 = cpad(bc, dtype);
        r.seq_len = len0; r.seq_kconv = true;
        if (conv1d_run(conv_pre, r, st)) return 1;
    }
    int ch = bc;
    long L = S;
    const int nk = cfg.num_kernels;
    for (int i = 0; i < cfg.num_upsamples; ++i) {
        const bool last_up = i == cfg.num_upsamples - 1;
        if (ew_cl(xsum, act_a, vd, (long)B * L, ch, cpad(ch, dtype), 2, cfg.lrelu_slope, st)) return 1;
        const int u = cfg.upsample_rates[i];
        const long Lnew = L * u + (last_up ? 1 : 0);
        ch /= 2;
        const int ld = cpad(ch, dtype);
        if (last_up) {
            // ReflectionPad1d((1, 0)) (generator.py:413-414): each utterance's up-sampled rows land at row offset 1
            // of its (L*u + 1)-row sequence, then row 0 = row 2 (reflect).  One launch per utterance because the
            // one-row shift is not a whole number of GEMM output rows (each holds u samples).
            const size_t a_step = (size_t)L * ups[i].cin_pad * vesize(dtype);
            // (ragged: each launch covers the utterance's own rows, known on the host, so it needs no length array)
            for (int b = 0; b < B; ++b) {
                ActBuf ab;
                ab.hi = (const char*)act_a.hi + b * a_step;
                ab.lo = (const char*)act_a.lo + b * a_step;
                const int Lb = rg ? (int)((long)rg->h_len0[b] * (L / S)) : (int)L;
                if (Lb == 0) continue;
                if (convT_run(ups[i], ab, 1, Lb, x + ((long)b * Lnew + 1) * ld, 0, 0, st)) return 1;
            }
            hipLaunchKernelGGL(copy_row_kernel, dim3(cdiv((long)B * ld, 256)), dim3(256), 0, st, x, B, (int)Lnew, ld, 2, 0);
            SVC_CHECK_HIP(hipGetLastError());
        } else {
            if (convT_run(ups[i], act_a.in(), B, (int)L, x, 0, 0, st, rg ? rg->len[i] : nullptr)) return 1;
        }
        L = Lnew;
        const int* len_i = rg ? rg->len[i + 1] : nullptr;
        // source fusion: si = source_resblock(source_down(s_stft)); x = x + si  (generator.py:416-419)
        {
            ConvRun r;
            r.a = stft_in; r.B = B; r.Lin = F; r.Lout = (int)L;
            const int dk = src_down[i].k;
            if (dk == 1) { r.stride = 1; r.pad_left = 0; }
            else { r.stride = dk / 2; r.pad_left = dk / 4; }
            r.c32 = si; r.ldc32 = ld;
            r.seq_len = len_f;
            if (conv1d_run(src_down[i], r, st)) return 1;
        }
        // x <- x + source_resblock(si): last conv of the stack adds res2 = x and writes x
        if (resblock_run(src_rb[i], dtype, nullptr, 1, si, y, t, act_a, B, (int)L, 1.0f, x, x, st, act_b, nullptr, len_i, sink)) return 1;
        for (int j = 0; j < nk; ++j) {
            if (resblock_run(blocks[i * nk + j], dtype, nullptr, 1, x, y, t, act_a, B, (int)L, 1.0f / (float)nk,
                             j > 0 ? xsum : nullptr, xsum, st, act_b, nullptr, len_i, sink)) return 1;
        }
    }
    if (ew_cl(xsum, act_a, vd, (long)B * L, ch, cpad(ch, dtype), 2, 0.01f, st)) return 1;     // F.leaky_relu default slope
    {
        ConvRun r;
        r.a = act_a.in(); r.B = B; r.Lin = (int)L; r.Lout = (int)L; r.pad_left = 3;
        r.c32 = post; r.ldc32 = ld18;
        r.seq_len = len_f; r.seq_kconv = true;
        if (conv1d_run(conv_post, r, st)) return 1;
    }
    if (hift_frames_launch(post, frames, (long)B * F, ld18, st)) return 1;
    const long Lw_out = (long)rm.S_in * up_total;      // ragged: straight into the caller's rows, tails zeroed
    return hift_ola_launch(frames, out, rm, lw, len_f, B, F, Lw_out, cfg.audio_limit, st);
}

// ================================================================================================ C ABI
extern "C" {

int svc_bigvgan_create(const svc_bigvgan_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream,
                       svc_bigvgan_t** out) {
    SVC_REQUIRE(cfg && weights && out, "null argument");
    SVC_REQUIRE(cfg->num_upsamples >= 1 && cfg->num_upsamples <= 8 && cfg->num_kernels >= 1 && cfg->num_kernels <= 4, "config");
    hipStream_t st = (hipStream_t)stream;
    svc_bigvgan* m = new svc_bigvgan();
    m->cfg = *cfg;
    m->dtype = cfg->precision == 1 ? 0 : (cfg->precision == 2 ? 2 : (cfg->precision == 3 ? 3 : 1));   // operand mode: fp32 | fp16 | fp16x3 | fp16 + fp8 corrections
    StateDict sd(weights, n_weights);
    auto fail = [&]() { delete m; return 1; };
    const int c0 = cfg->upsample_initial_channel;
    if (pack_conv1d(sd, "conv_pre", c0, cfg->num_mels, 7, true, m->dtype, m->wts, st, &m->conv_pre)) return fail();
    m->ups.resize(cfg->num_upsamples);
    int ch = c0;
    const int snake_mode = cfg->snake_logscale ? (cfg->snakebeta ? 0 : 1) : 2;
    for (int i = 0; i < cfg->num_upsamples; ++i) {
        if (pack_convT(sd, "ups." + std::to_string(i) + ".0", ch, ch / 2, cfg->upsample_kernel_sizes[i], cfg->upsample_rates[i],
                       m->dtype, m->wts, st, &m->ups[i])) return fail();
        ch /= 2;
        for (int j = 0; j < cfg->num_kernels; ++j) {
            ResBlockW rb;
            if (pack_resblock(sd, "resblocks." + std::to_string(i * cfg->num_kernels + j), ch, cfg->resblock_kernel_sizes[j],
                              cfg->resblock_dilation_sizes[j], 3, m->dtype, snake_mode, true, cfg->snakebeta != 0, m->wts, st, &rb))
                return fail();
            m->blocks.push_back(rb);
        }
    }
    if (make_snake(sd, "activation_post.act.alpha", cfg->snakebeta ? "activation_post.act.beta" : "", ch, snake_mode, m->wts, st,
                   &m->act_post)) return fail();
    if (pack_conv1d(sd, "conv_post", 1, ch, 7, cfg->use_bias_at_final != 0, m->dtype, m->wts, st, &m->conv_post)) return fail();
    {
        const auto* f = sd.get("activation_post.upsample.filter");
        if (!f || StateDict::numel(f) != 12) { set_error("missing activation_post.upsample.filter (12 taps)"); return fail(); }
        if (hipMemcpy(m->taps, f->data, 48, hipMemcpyDeviceToHost) != hipSuccess) { set_error("filter copy failed"); return fail(); }
    }
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("sync failed"); return fail(); }
    if (m->dtype == 3)
        for (size_t i = 0; i < m->blocks.size(); ++i) m->p8.add(m->blocks[i], "resblocks." + std::to_string(i));
    *out = m;
    return 0;
}

void svc_bigvgan_destroy(svc_bigvgan_t* m) { delete m; }

int svc_bigvgan_set_microbatch(svc_bigvgan_t* m, int utterances) {
    SVC_REQUIRE(m && utterances >= 0, "bad argument");
    m->microbatch = utterances;
    return 0;
}

int svc_bigvgan_forward(svc_bigvgan_t* m, const float* mel, int B, int S, float* out, void* stream) {
    SVC_REQUIRE(m && mel && out && B >= 1 && S >= 1, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    long total = 1;
    for (int i = 0; i < m->cfg.num_upsamples; ++i) total *= m->cfg.upsample_rates[i];
    // measured, vocoder alone, B = 32 x S = 430 (round 3, fp16p8): 4: 132.6, 8: 119.1, 16: 112.9, 32: 108.8 ms (round 1, small B = 64
    // end to end: 4: 27.3k, 8: 28.2k, 16: 28.5k frames/s)
    const int mb = m->microbatch > 0 ? m->microbatch : 32;
    for (int b0 = 0; b0 < B; b0 += mb) {
        const int nb = std::min(mb, B - b0);
        if (m->reserve(nb, S, st)) return 1;
        if (m->run(mel + (long)b0 * m->cfg.num_mels * S, nb, S, out + (long)b0 * S * total, st)) return 1;
    }
    return 0;
}

int svc_bigvgan_forward_ragged(svc_bigvgan_t* m, const float* mel, const int32_t* lens, int B, int S, float* out, void* stream) {
    SVC_REQUIRE(m && mel && lens && out && B >= 1 && S >= 1, "bad argument");
    if (RaggedPlan::check("svc_bigvgan_forward_ragged", lens, B, S)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int nu = m->cfg.num_upsamples;
    long total = 1;
    for (int i = 0; i < nu; ++i) total *= m->cfg.upsample_rates[i];
    // No class cut: a short utterance may share a padded micro-batch with a long one
    auto rows_after = [&](int stage, long l) {
        for (int i = 0; i < stage; ++i) l *= m->cfg.upsample_rates[i];
        return l;
    };
    RaggedPlan& plan = m->plan;
    if (plan.build(lens, B, S, m->microbatch, nu, rows_after, nullptr, 0, st)) return 1;
    if (plan.S_max > 0 && m->reserve(plan.nb_max, plan.S_max, st)) return 1;
    for (int k = 0; k < plan.count(); ++k) {
        const RaggedMB rg = plan.mb(k);
        if (rg.S == 0) {
            if (zero_rows(rg, out, (long)S * total, st)) return 1;
        } else if (m->run(mel, rg.nb, rg.S, out, st, &rg)) return 1;
    }
    return 0;
}

int svc_hift_create(const svc_hift_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream,
                    svc_hift_t** out) {
    SVC_REQUIRE(cfg && weights && out, "null argument");
    SVC_REQUIRE(cfg->num_upsamples == 2 && cfg->istft_n_fft == 16 && cfg->istft_hop == 4 && cfg->nb_harmonics + 1 <= 16,
                "HiFT: only the 2-stage, n_fft 16 / hop 4 generator of configs/hifigan.yml is supported");
    hipStream_t st = (hipStream_t)stream;
    svc_hift* m = new svc_hift();
    m->cfg = *cfg;
    m->device = current_device();
    m->dtype = cfg->precision == 1 ? 0 : (cfg->precision == 2 ? 2 : (cfg->precision == 3 ? 3 : 1));   // operand mode: fp32 | fp16 | fp16x3 | fp16 + fp8 corrections
    m->up_total = cfg->istft_hop;
    for (int i = 0; i < cfg->num_upsamples; ++i) m->up_total *= cfg->upsample_rates[i];
    StateDict sd(weights, n_weights);
    auto fail = [&]() { delete m; return 1; };
    const int bc = cfg->base_channels, fc = cfg->f0_cond_channels;
    for (int i = 0; i < 5; ++i) {
        if (pack_conv1d(sd, "f0_predictor.condnet." + std::to_string(2 * i), fc, i == 0 ? cfg->in_channels : fc, 3, true, 1,
                        m->wts, st, &m->f0_convs[i])) return fail();
    }
    {
        const auto* w = sd.get("f0_predictor.classifier.weight");
        const auto* b = sd.get("f0_predictor.classifier.bias");
        const auto* lw = sd.get("m_source.l_linear.weight");
        const auto* lb = sd.get("m_source.l_linear.bias");
        if (require_shape(w, "f0_predictor.classifier.weight", {1, fc}) || require_shape(b, "f0_predictor.classifier.bias", {1}) ||
            require_shape(lw, "m_source.l_linear.weight", {1, cfg->nb_harmonics + 1}) || require_shape(lb, "m_source.l_linear.bias", {1}))
            return fail();
        m->f0_lin_w = m->wts.alloc_n<float>(fc, st);
        m->f0_lin_b = m->wts.alloc_n<float>(1, st);
        m->src_lin_w = m->wts.alloc_n<float>(16, st);
        m->src_lin_b = m->wts.alloc_n<float>(1, st);
        if (!m->f0_lin_w || !m->f0_lin_b || !m->src_lin_w || !m->src_lin_b) return fail();
        (void)hipMemcpyAsync(m->f0_lin_w, w->data, fc * 4, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(m->f0_lin_b, b->data, 4, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(m->src_lin_w, lw->data, (cfg->nb_harmonics + 1) * 4, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(m->src_lin_b, lb->data, 4, hipMemcpyDeviceToDevice, st);
    }
    if (pack_conv1d(sd, "conv_pre", bc, cfg->in_channels, 7, true, m->dtype, m->wts, st, &m->conv_pre)) return fail();
    int ch = bc;
    // downsample rates of the source branch: cumulative products of [1] + reversed(ups)[:-1], reversed (generator.py:349-351)
    int down_rate[2] = {cfg->upsample_rates[1], 1};
    for (int i = 0; i < 2; ++i) {
        if (pack_convT(sd, "ups." + std::to_string(i), ch, ch / 2, cfg->upsample_kernel_sizes[i], cfg->upsample_rates[i], m->dtype,
                       m->wts, st, &m->ups[i])) return fail();
        ch /= 2;
        const int u = down_rate[i];
        const int dk = u == 1 ? 1 : 2 * u;
        if (pack_conv1d(sd, "source_downs." + std::to_string(i), ch, cfg->istft_n_fft + 2, dk, true, m->dtype, m->wts, st,
                        &m->src_down[i])) return fail();
        if (pack_resblock(sd, "source_resblocks." + std::to_string(i), ch, cfg->source_resblock_kernel_sizes[i],
                          cfg->source_resblock_dilation_sizes[i], 3, m->dtype, 2, false, false, m->wts, st, &m->src_rb[i]))
            return fail();
        for (int j = 0; j < cfg->num_kernels; ++j) {
            ResBlockW rb;
            if (pack_resblock(sd, "resblocks." + std::to_string(i * cfg->num_kernels + j), ch, cfg->resblock_kernel_sizes[j],
                              cfg->resblock_dilation_sizes[j], 3, m->dtype, 2, false, false, m->wts, st, &rb)) return fail();
            m->blocks.push_back(rb);
        }
    }
    if (pack_conv1d(sd, "conv_post", cfg->istft_n_fft + 2, ch, 7, true, m->dtype, m->wts, st, &m->conv_post)) return fail();
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("sync failed"); return fail(); }
    if (m->dtype == 3)
        for (int i = 0; i < 2; ++i) {
            m->p8.add(m->src_rb[i], "source_resblocks." + std::to_string(i));
            for (int j = 0; j < cfg->num_kernels; ++j)
                m->p8.add(m->blocks[i * cfg->num_kernels + j], "resblocks." + std::to_string(i * cfg->num_kernels + j));
        }
    *out = m;
    return 0;
}

void svc_hift_destroy(svc_hift_t* m) { delete m; }

int svc_hift_set_microbatch(svc_hift_t* m, int utterances) {
    SVC_REQUIRE(m && utterances >= 0, "bad argument");
    m->microbatch = utterances;
    return 0;
}

int svc_hift_forward(svc_hift_t* m, const float* mel, const float* f0, const float* phase0, const float* noise, int B, int S,
                     float* out, float* f0_out, void* stream) {
    SVC_REQUIRE(m && mel && phase0 && noise && out && B >= 1 && S >= 1, "bad argument");
    return m->forward(mel, f0, phase0, noise, nullptr, B, S, out, f0_out, (hipStream_t)stream);
}

int svc_hift_forward_ragged(svc_hift_t* m, const float* mel, const int32_t* lens, const float* f0, const float* phase0,
                            const float* noise, int B, int S, float* out, float* f0_out, void* stream) {
    SVC_REQUIRE(m && mel && lens && phase0 && noise && out && B >= 1 && S >= 1, "bad argument");
    return m->forward_ragged(mel, lens, f0, phase0, noise, nullptr, B, S, out, f0_out, (hipStream_t)stream);
}

int svc_hift_forward_seeded(svc_hift_t* m, const float* mel, const int32_t* lens, const float* f0, const uint64_t* seeds, int B,
                            int S, float* out, float* f0_out, void* stream) {
    SVC_REQUIRE(m && mel && out, "null argument");
    SVC_REQUIRE(seeds, "svc_hift_forward_seeded: seeds is NULL (HOST [B], one per utterance)");
    SVC_REQUIRE(B >= 1 && S >= 1, "svc_hift_forward_seeded: B and S must be at least 1");
    SVC_REQUIRE((long)S * m->up_total <= 0x7fffffffL, "svc_hift_forward_seeded: the sample index is a 32-bit counter word");
    SVC_REQUIRE(current_device() == m->device, "this handle was created on another device (make it current before the call)");
    if (lens)
        for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 0 && lens[b] <= S, "svc_hift_forward_seeded: lens out of range");
    hipStream_t st = (hipStream_t)stream;
    const int NH = m->cfg.nb_harmonics + 1;
    if (B > m->seed_cap) {
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        m->seed_ar.release();
        m->seed_cap = 0;
        m->d_seeds = m->seed_ar.alloc_n<unsigned long long>(B, st);
        m->d_phase0 = m->seed_ar.alloc_n<float>((size_t)B * NH, st);
        if (!m->d_seeds || !m->d_phase0) return 1;
        m->seed_cap = B;
    }
    void* h = m->plan.staging.acquire((size_t)B * 8);
    if (!h) return 1;
    memcpy(h, seeds, (size_t)B * 8);
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_seeds, h, (size_t)B * 8, hipMemcpyHostToDevice, st));
    if (m->plan.staging.commit(st)) return 1;
    hipLaunchKernelGGL(noise_phase0_kernel, dim3(cdiv(B * NH, 256)), dim3(256), 0, st, m->d_seeds, 0ull, B, NH, m->d_phase0);
    SVC_CHECK_HIP(hipGetLastError());
    if (lens) return m->forward_ragged(mel, lens, f0, m->d_phase0, nullptr, m->d_seeds, B, S, out, f0_out, st);
    return m->forward(mel, f0, m->d_phase0, nullptr, m->d_seeds, B, S, out, f0_out, st);
}

}  // extern "C"

int svc_hift::forward(const float* mel, const float* f0, const float* phase0, const float* noise, const unsigned long long* seeds,
                      int B, int S, float* out, float* f0_out, hipStream_t st) {
    svc_hift* m = this;
    const int NH = m->cfg.nb_harmonics + 1;
    const long Lw = (long)S * m->up_total;
    // measured, vocoder alone, B = 32 x S = 430 (round 3, fp16p8): 4: 37.4, 8: 29.5, 16: 28.2, 32: 26.9 ms
    const int mb = m->microbatch > 0 ? m->microbatch : 32;
    for (int b0 = 0; b0 < B; b0 += mb) {
        const int nb = std::min(mb, B - b0);
        if (m->reserve(nb, S, st)) return 1;
        if (m->run(mel + (long)b0 * m->cfg.in_channels * S, f0 ? f0 + (long)b0 * S : nullptr, phase0 + (long)b0 * NH,
                   noise ? noise + (long)b0 * NH * Lw : nullptr, nb, S, out + (long)b0 * Lw, f0_out ? f0_out + (long)b0 * S : nullptr, st,
                   nullptr, seeds ? seeds + b0 : nullptr))
            return 1;
    }
    return 0;
}

int svc_hift::forward_ragged(const float* mel, const int32_t* lens, const float* f0, const float* phase0, const float* noise,
                             const unsigned long long* seeds, int B, int S, float* out, float* f0_out, hipStream_t st) {
    if (RaggedPlan::check("svc_hift_forward_ragged", lens, B, S)) return 1;
    // Micro-batches of one kernel class (svc_hift::kernel_class); one reservation for the whole call: the first micro-batch is the
    // longest, not necessarily the largest
    if (plan.build(lens, B, S, microbatch, cfg.num_upsamples, [&](int i, long l) { return rows_after(i, l); },
                   [&](long l) { return kernel_class(l); }, up_total, st))
        return 1;
    if (plan.S_max > 0 && reserve(plan.nb_max, plan.S_max, st)) return 1;
    for (int k = 0; k < plan.count(); ++k) {
        const RaggedMB rg = plan.mb(k);
        if (rg.S == 0) {
            if (zero_rows(rg, out, (long)S * up_total, st)) return 1;
            if (f0_out && zero_rows(rg, f0_out, (long)S, st)) return 1;
        } else if (run(mel, f0, phase0, noise, rg.nb, rg.S, out, f0_out, st, &rg, seeds)) return 1;
    }
    return 0;
}

// ================================================================================================ precision plan
namespace {
int plan_handle_ok(const void* m, int dtype, const std::string& who) {
    SVC_REQUIRE(m != nullptr, who + ": null handle");
    SVC_REQUIRE(dtype == 3, who + ": the precision plan belongs to an fp16p8 handle (precision 3)");
    return 0;
}

int plan_get(const P8Plan& p8, uint8_t* veto, int n, const std::string& who) {
    SVC_REQUIRE(veto != nullptr, who + ": veto is NULL");
    SVC_REQUIRE(n == p8.size(), who + ": n differs from the plan size");
    for (int i = 0; i < n; ++i) veto[i] = p8.conv[i]->p8_veto ? 1 : 0;
    return 0;
}

int plan_set(P8Plan& p8, const uint8_t* veto, int n, const std::string& who) {
    SVC_REQUIRE(veto != nullptr, who + ": veto is NULL");
    SVC_REQUIRE(n == p8.size(), who + ": n differs from the plan size");
    for (int i = 0; i < n; ++i) p8.conv[i]->p8_veto = veto[i] != 0;
    return 0;
}

// The decision of calibrate, row by row: a conv is vetoed when a loss ratio of its activations or weights exceeds tau, and the
// vetoes are ORed into the plan (calls on different material accumulate)
void plan_apply(P8Plan& p8, svc_plan_row_t* rows, float tau) {
    for (int i = 0; i < p8.size(); ++i) {
        svc_plan_row_t& r = rows[i];
        r.veto = r.rho > tau || r.eta > tau || r.omega_hi > tau || r.omega_lo > tau;
        if (r.veto) p8.conv[i]->p8_veto = true;
    }
}

// the argument checks of both calibrate calls: before the handle is touched or anything is launched.  up: waveform samples per frame
int calibrate_check(const std::string& who, const void* mel, const int32_t* lens, int B, int S, long up, float tau, const void* rows,
                    int n_rows, int n_plan) {
    SVC_REQUIRE(mel != nullptr && rows != nullptr, who + ": mel and rows are required");
    SVC_REQUIRE(n_rows == n_plan, who + ": n_rows differs from the plan size");
    SVC_REQUIRE(tau > 0.f && tau <= 1.f, who + ": tau lies in (0, 1]");      // false for NaN
    SVC_REQUIRE(B >= 1 && S >= 1, who + ": B and S must be at least 1");
    SVC_REQUIRE((double)B * ((double)S * (double)up + 1.0) < 2147483648.0, who + ": B * S * up must stay below 2^31");
    if (lens)
        for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 1 && lens[b] <= S, who + ": lens outside [1, S]");
    return 0;
}

// The body of both calibrate calls.  fwd(out) runs the handle's forward (plain or ragged) into the scratch waveform `out`
// ([B][S * up]); while it runs every candidate is vetoed and *slot points at the sink resblock_run feeds.
int calibrate_run(P8Plan& p8, const CensusSink** slot, int B, int S, long up, float tau, svc_plan_row_t* rows, hipStream_t st,
                  const std::function<int(float*)>& fwd) {
    const int n = p8.size();
    if (n == 0) return 0;
    Arena ar;
    std::vector<int> L(n, 0);
    std::vector<long> wc_off(n + 1, 0);
    for (int i = 0; i < n; ++i) wc_off[i + 1] = wc_off[i] + 4L * p8.conv[i]->cout;
    CensusSink sink;
    sink.part_cap = census_parts(B, (int)(S * up + 1));      // no conv of either vocoder has more rows per utterance
    sink.rec = ar.alloc_n<svc_census_t>(n, st);
    sink.part = ar.alloc_n<svc_census_t>((size_t)sink.part_cap, st);
    sink.L = L.data();
    double* d_wc = ar.alloc_n<double>((size_t)wc_off[n], st);
    float* out = ar.alloc_n<float>((size_t)B * S * up, st);
    if (!sink.rec || !sink.part || !d_wc || !out) return 1;
    std::vector<uint8_t> saved(n);
    for (int i = 0; i < n; ++i) { saved[i] = p8.conv[i]->p8_veto; p8.conv[i]->p8_veto = true; }
    *slot = &sink;
    int rc = fwd(out);
    *slot = nullptr;
    for (int i = 0; i < n; ++i) p8.conv[i]->p8_veto = saved[i] != 0;
    for (int i = 0; i < n && !rc; ++i) rc = weight_census_launch(*p8.conv[i], d_wc + wc_off[i], st);
    if (rc) { (void)hipStreamSynchronize(st); return 1; }       // the arena's buffers may still be in use
    std::vector<svc_census_t> rec(n);
    std::vector<double> wc((size_t)wc_off[n]);
    hipError_t e = hipMemcpyAsync(rec.data(), sink.rec, n * sizeof(svc_census_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(wc.data(), d_wc, wc.size() * sizeof(double), hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    SVC_CHECK_HIP(e);
    SVC_CHECK_HIP(e2);
    auto ratio = [](double err, double s) { return s > 0.0 ? err / s : 0.0; };
    for (int i = 0; i < n; ++i) {
        svc_plan_row_t& r = rows[i];
        memset(&r, 0, sizeof(r));
        r.index = i;
        r.L = L[i];
        r.census = rec[i];
        r.rho = ratio(rec[i].s_lo_err2, rec[i].s_lo2);
        r.eta = ratio(rec[i].s_hi_err2, rec[i].s_hi2);
        for (int c = 0; c < p8.conv[i]->cout; ++c) {       // all-zero channels are exempt: their ratio is 0
            const double* w = &wc[(size_t)wc_off[i] + 4 * c];
            r.omega_hi = std::max(r.omega_hi, ratio(w[1], w[0]));
            r.omega_lo = std::max(r.omega_lo, ratio(w[3], w[2]));
        }
    }
    plan_apply(p8, rows, tau);
    return 0;
}
}  // namespace

extern "C" {

int svc_bigvgan_plan_size(svc_bigvgan_t* m) { return m && m->dtype == 3 ? m->p8.size() : -1; }
const char* svc_bigvgan_plan_name(svc_bigvgan_t* m, int i) {
    return m && m->dtype == 3 && i >= 0 && i < m->p8.size() ? m->p8.name[i].c_str() : nullptr;
}
int svc_bigvgan_plan_get(svc_bigvgan_t* m, uint8_t* veto, int n) {
    if (plan_handle_ok(m, m ? m->dtype : 0, "svc_bigvgan_plan_get")) return 1;
    return plan_get(m->p8, veto, n, "svc_bigvgan_plan_get");
}
int svc_bigvgan_plan_set(svc_bigvgan_t* m, const uint8_t* veto, int n) {
    if (plan_handle_ok(m, m ? m->dtype : 0, "svc_bigvgan_plan_set")) return 1;
    return plan_set(m->p8, veto, n, "svc_bigvgan_plan_set");
}
int svc_bigvgan_plan_reset(svc_bigvgan_t* m) {
    if (plan_handle_ok(m, m ? m->dtype : 0, "svc_bigvgan_plan_reset")) return 1;
    for (ConvW* c : m->p8.conv) c->p8_veto = false;
    return 0;
}
int svc_bigvgan_calibrate(svc_bigvgan_t* m, const float* mel, const int32_t* lens, int B, int S, float tau, svc_plan_row_t* rows,
                          int n_rows, void* stream) {
    const char* who = "svc_bigvgan_calibrate";
    if (plan_handle_ok(m, m ? m->dtype : 0, who)) return 1;
    long up = 1;
    for (int i = 0; i < m->cfg.num_upsamples; ++i) up *= m->cfg.upsample_rates[i];
    if (calibrate_check(who, mel, lens, B, S, up, tau, rows, n_rows, m->p8.size())) return 1;
    return calibrate_run(m->p8, &m->sink, B, S, up, tau, rows, (hipStream_t)stream, [&](float* out) {
        return lens ? svc_bigvgan_forward_ragged(m, mel, lens, B, S, out, stream) : svc_bigvgan_forward(m, mel, B, S, out, stream);
    });
}

int svc_hift_plan_size(svc_hift_t* m) { return m && m->dtype == 3 ? m->p8.size() : -1; }
const char* svc_hift_plan_name(svc_hift_t* m, int i) {
    return m && m->dtype == 3 && i >= 0 && i < m->p8.size() ? m->p8.name[i].c_str() : nullptr;
}
int svc_hift_plan_get(svc_hift_t* m, uint8_t* veto, int n) {
    if (plan_handle_ok(m, m ? m->dtype : 0, "svc_hift_plan_get")) return 1;
    return plan_get(m->p8, veto, n, "svc_hift_plan_get");
}
int svc_hift_plan_set(svc_hift_t* m, const uint8_t* veto, int n) {
    if (plan_handle_ok(m, m ? m->dtype : 0, "svc_hift_plan_set")) return 1;
    return plan_set(m->p8, veto, n, "svc_hift_plan_set");
}
int svc_hift_plan_reset(svc_hift_t* m) {
    if (plan_handle_ok(m, m ? m->dtype : 0, "svc_hift_plan_reset")) return 1;
    for (ConvW* c : m->p8.conv) c->p8_veto = false;
    return 0;
}
int svc_hift_calibrate(svc_hift_t* m, const float* mel, const int32_t* lens, const float* f0, const float* phase0, const float* noise,
                       int B, int S, float tau, svc_plan_row_t* rows, int n_rows, void* stream) {
    const char* who = "svc_hift_calibrate";
    if (plan_handle_ok(m, m ? m->dtype : 0, who)) return 1;
    SVC_REQUIRE(phase0 && noise, std::string(who) + ": phase0 and noise are required");
    if (calibrate_check(who, mel, lens, B, S, m->up_total, tau, rows, n_rows, m->p8.size())) return 1;
    hipStream_t st = (hipStream_t)stream;
    return calibrate_run(m->p8, &m->sink, B, S, m->up_total, tau, rows, st, [&](float* out) {
        return lens ? m->forward_ragged(mel, lens, f0, phase0, noise, nullptr, B, S, out, nullptr, st)
                    : m->forward(mel, f0, phase0, noise, nullptr, B, S, out, nullptr, st);
    });
}

// ---- op-level entry points for the parity tests -------------------------------------------------------
// A BigVGAN handle that holds nothing but a precision plan of n candidates (one 3-pair ResBlock per six of them): no device is
// touched, no weight exists, and the only calls it supports are the svc_bigvgan_plan_* family, the refusals of
// svc_bigvgan_calibrate, svc_op_plan_apply and svc_bigvgan_destroy.
int svc_op_plan_fake(int precision, int n_candidates, svc_bigvgan_t** out) {
    SVC_REQUIRE(out && precision >= 0 && precision <= 3 && n_candidates >= 0 && n_candidates <= 96, "svc_op_plan_fake: bad argument");
    static char never_read;
    svc_bigvgan* m = new svc_bigvgan();
    memset(&m->cfg, 0, sizeof(m->cfg));
    m->cfg.precision = precision;
    m->cfg.num_upsamples = 1;
    m->cfg.upsample_rates[0] = 4;
    m->dtype = precision == 1 ? 0 : (precision == 2 ? 2 : (precision == 3 ? 3 : 1));
    m->x = m->y = m->t = m->xsum = nullptr;
    m->blocks.resize((n_candidates + 5) / 6);
    int left = n_candidates;
    for (ResBlockW& rb : m->blocks) {
        rb.ndil = 3;
        for (int d = 0; d < 3; ++d) {
            if (left-- > 0) rb.c1[d].w8 = &never_read;
            if (left-- > 0) rb.c2[d].w8 = &never_read;
        }
    }
    if (m->dtype == 3)
        for (size_t i = 0; i < m->blocks.size(); ++i) m->p8.add(m->blocks[i], "resblocks." + std::to_string(i));
    *out = m;
    return 0;
}

// calibrate's decision step alone on the caller's rows (rho, eta, omega_hi, omega_lo in; veto out; the plan takes the OR)
int svc_op_plan_apply(svc_bigvgan_t* m, svc_plan_row_t* rows, int n_rows, float tau) {
    if (plan_handle_ok(m, m ? m->dtype : 0, "svc_op_plan_apply")) return 1;
    SVC_REQUIRE(rows && n_rows == m->p8.size() && tau > 0.f && tau <= 1.f, "svc_op_plan_apply: bad argument");
    plan_apply(m->p8, rows, tau);
    return 0;
}

namespace {
thread_local int g_conv1d_took = 0;      // svc_op_conv1d_last_took

// One body for both Conv1d seams.  `e` carries what svc_op_conv1d has no argument for; stride / pad_mode are its own.
int op_conv1d_body(svc_conv1d_ex_t& e, int stride, int pad_mode, bool ex, hipStream_t st) {
    const int B = e.B, L = e.L, Cin = e.Cin, Cout = e.Cout, Lout = e.Lout;
    const int dtype = e.dtype;     // 0 f16, 1 f32, 2 f16x3, 3 fp16 + fp8 corrections
    const int c_rows = e.c_rows ? e.c_rows : Lout;
    Arena ar;
    svc_tensor_desc_t d[2];
    d[0].name = "c.weight"; d[0].data = e.w; d[0].ndim = 3; d[0].shape[0] = Cout; d[0].shape[1] = Cin; d[0].shape[2] = e.k; d[0].shape[3] = 1;
    d[1].name = "c.bias"; d[1].data = e.bias; d[1].ndim = 1; d[1].shape[0] = Cout; d[1].shape[1] = d[1].shape[2] = d[1].shape[3] = 1;
    StateDict sd(d, e.bias ? 2 : 1);
    ConvW cw;
    if (pack_conv1d(sd, "c", Cout, Cin, e.k, e.bias != nullptr, dtype, ar, st, &cw)) return 1;
    const size_t n_c = (size_t)B * c_rows * cw.cout_pad;
    float* c = ar.alloc_n<float>(n_c, st);
    if (!c) return 1;
    ConvRun r;
    if (e.a_hi) {      // the caller's operand planes (a fused Snake's output fed to the next conv)
        r.a.hi = e.a_hi; r.a.lo = e.a_lo;
    } else {
        void* a = ar.alloc((size_t)B * L * cw.cin_pad * vesize(dtype), st);
        void* a_lo = ar.alloc((size_t)B * L * cw.cin_pad * vesize(dtype), st);
        if (!a || !a_lo) return 1;
        if (dtype == 3) {
            // the planes as the model's activation kernels write them: leaky ReLU of slope 1 is the identity (v * 1.0f is exact)
            if (act_cl_launch(e.x, Cin, a, a_lo, cw.cin_pad, 1, nullptr, nullptr, nullptr, B, Cin, L, 2, 1.0f, st, 1)) return 1;
        } else {
            if (pack_any(gdt(dtype), e.x, a, 0, B * L, 1, Cin, Cin, 0, 1, cw.cin_pad, 0, 1, nullptr, st)) return 1;
            if (is_split(dtype))
                if (pack_f16_lo_launch(e.x, (half_t*)a_lo, B * L, 1, Cin, Cin, 0, 1, cw.cin_pad, 0, 1, nullptr, st)) return 1;
        }
        r.a.hi = a; r.a.lo = a_lo;
    }
    r.B = B; r.Lin = L; r.Lout = Lout; r.dilation = e.dilation; r.stride = stride; r.pad_left = e.pad_left; r.pad_mode = pad_mode;
    r.c32 = c; r.ldc32 = cw.cout_pad;
    if (ex) {
        // rows outside [c_off, c_off + Lout) of y come back as they went in: the conv must not write them
        if (pack_f32_launch(e.y, c, B * c_rows, 1, Cout, Cout, 0, 1, cw.cout_pad, 0, 1, nullptr, st)) return 1;
        r.c_rows = e.c_rows; r.c_off = e.c_off;
        r.out_scale = e.out_scale; r.act = e.act; r.act_slope = e.act_slope;
        const float* src[2] = {e.res, e.res2};
        for (int i = 0; i < 2; ++i) {
            if (!src[i]) continue;
            float* q = c;      // res / res2 == y: in place, the conv reads the addend from the buffer it writes
            if (src[i] != e.y) {
                q = ar.alloc_n<float>(n_c, st);
                if (!q) return 1;
                if (pack_f32_launch(src[i], q, B * c_rows, 1, Cout, Cout, 0, 1, cw.cout_pad, 0, 1, nullptr, st)) return 1;
            }
            if (i == 0) { r.res = q; r.ldres = cw.cout_pad; } else { r.res2 = q; r.ldres2 = cw.cout_pad; }
        }
        if (e.seq_len) {
            int* d_len = ar.alloc_n<int>(B, st);
            if (!d_len) return 1;
            SVC_CHECK_HIP(hipMemcpyAsync(d_len, e.seq_len, B * sizeof(int), hipMemcpyHostToDevice, st));
            SVC_CHECK_HIP(hipStreamSynchronize(st));      // the caller's array is pageable
            r.seq_len = d_len; r.seq_kconv = true;
        }
        if (e.post_a) {
            r.post_a = e.post_a; r.post_ib = e.post_ib; r.post_n = Cout;
            r.c16 = reinterpret_cast<half_t*>(e.plane_hi); r.c16_lo = reinterpret_cast<half_t*>(e.plane_lo); r.ldc16 = cw.cout_pad;
            r.c16_lo_fmt = e.next_p8 ? 1 : 0;
        }
        r.p8 = dtype == 3;
        r.bm = e.bm; r.force_gemm = e.force_gemm != 0;
    }
    r.took = &e.took;
    if (conv1d_run(cw, r, st)) return 1;
    g_conv1d_took = e.took;
    if (pack_f32_launch(c, e.y, B * c_rows, 1, Cout, cw.cout_pad, 0, 1, Cout, 0, 1, nullptr, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}
}  // namespace

int svc_op_conv1d(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin, int Cout, int k,
                  int dilation, int stride, int pad_left, int Lout, int pad_mode, int dtype_in, void* stream) {
    svc_conv1d_ex_t e;
    memset(&e, 0, sizeof(e));
    e.x = x; e.w = w; e.bias = bias; e.y = y;
    e.B = B; e.L = L; e.Cin = Cin; e.Cout = Cout; e.k = k; e.dilation = dilation; e.pad_left = pad_left; e.Lout = Lout;
    e.dtype = dtype_in;    // 0 f16, 1 f32, 2 f16x3
    return op_conv1d_body(e, stride, pad_mode, false, (hipStream_t)stream);
}

int svc_op_conv1d_last_took(void) { return g_conv1d_took; }

int svc_op_conv1d_ex(svc_conv1d_ex_t* e, void* stream) {
    SVC_REQUIRE(e && e->w && e->y && (e->x || e->a_hi), "bad argument");
    SVC_REQUIRE(e->B >= 1 && e->L >= 1 && e->Cin >= 1 && e->Cout >= 1 && e->k >= 1 && e->dilation >= 1 && e->Lout >= 1 && e->pad_left >= 0,
                "svc_op_conv1d_ex: bad shape");
    SVC_REQUIRE(e->dtype == 0 || e->dtype == 2 || e->dtype == 3, "svc_op_conv1d_ex: dtype is 0 (f16), 2 (f16x3) or 3 (fp16 + fp8 corrections)");
    SVC_REQUIRE(e->c_off >= 0 && e->c_off + e->Lout <= (e->c_rows ? e->c_rows : e->Lout), "svc_op_conv1d_ex: the output rows do not fit c_rows");
    SVC_REQUIRE(!e->a_hi || e->dtype == 0 || e->a_lo, "svc_op_conv1d_ex: split operand planes come in pairs");
    SVC_REQUIRE(!e->post_a == !e->post_ib && (!e->post_a || (e->plane_hi && e->plane_lo)), "svc_op_conv1d_ex: the fused Snake needs a, 1/b and both planes");
    SVC_REQUIRE(!e->next_p8 || e->post_a, "svc_op_conv1d_ex: next_p8 selects the format of a fused Snake's lo plane");
    SVC_REQUIRE(!e->force_gemm || (e->dtype != 3 && !e->next_p8), "svc_op_conv1d_ex: the tap-GEMM neither reads nor writes byte-pair planes");
    SVC_REQUIRE(e->bm == 0 || e->bm == 64 || e->bm == 128 || e->bm == 256, "svc_op_conv1d_ex: bm is 0, 64, 128 or 256");
    if (e->seq_len)
        for (int b = 0; b < e->B; ++b) SVC_REQUIRE(e->seq_len[b] >= 0 && e->seq_len[b] <= e->L, "svc_op_conv1d_ex: seq_len out of range");
    e->took = 0;
    return op_conv1d_body(*e, 1, KG_PAD_ZERO, true, (hipStream_t)stream);
}

int svc_op_conv_transpose1d(const float* x, const float* w, const float* bias, float* y, int B, int L, int Cin, int Cout, int k,
                            int stride, int dtype_in, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int dtype = dtype_in;
    SVC_REQUIRE(bias != nullptr, "bias required");
    Arena ar;
    svc_tensor_desc_t d[2];
    d[0].name = "c.weight"; d[0].data = w; d[0].ndim = 3; d[0].shape[0] = Cin; d[0].shape[1] = Cout; d[0].shape[2] = k; d[0].shape[3] = 1;
    d[1].name = "c.bias"; d[1].data = bias; d[1].ndim = 1; d[1].shape[0] = Cout; d[1].shape[1] = d[1].shape[2] = d[1].shape[3] = 1;
    StateDict sd(d, 2);
    ConvW cw;
    if (pack_convT(sd, "c", Cin, Cout, k, stride, dtype, ar, st, &cw)) return 1;
    void* a = ar.alloc((size_t)B * L * cw.cin_pad * vesize(dtype), st);
    void* a_lo = ar.alloc((size_t)B * L * cw.cin_pad * vesize(dtype), st);
    float* c = ar.alloc_n<float>((size_t)B * L * stride * cw.cout_pad, st);
    if (!a || !a_lo || !c) return 1;
    if (pack_any(gdt(dtype), x, a, 0, B * L, 1, Cin, Cin, 0, 1, cw.cin_pad, 0, 1, nullptr, st)) return 1;
    if (is_split(dtype))
        if (pack_f16_lo_launch(x, (half_t*)a_lo, B * L, 1, Cin, Cin, 0, 1, cw.cin_pad, 0, 1, nullptr, st)) return 1;
    ActBuf ab;
    ab.hi = a; ab.lo = a_lo;
    if (convT_run(cw, ab, B, L, c, 0, 0, st)) return 1;
    if (pack_f32_launch(c, y, B * L * stride, 1, Cout, cw.cout_pad, 0, 1, Cout, 0, 1, nullptr, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

namespace {
// a HOST int32 array of a test aid -> the device (null stays null)
int op_host_ints(const int32_t* h, int n, Arena& ar, hipStream_t st, const int** out) {
    *out = nullptr;
    if (!h) return 0;
    int* d = ar.alloc_n<int>(n, st);
    if (!d) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(d, h, n * sizeof(int), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));      // the caller's array is pageable
    *out = d;
    return 0;
}
}  // namespace

int svc_op_act_cl(const svc_act_cl_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(e, "svc_op_act_cl: null argument");
    SVC_REQUIRE(e->x && e->y_hi, "svc_op_act_cl: x and y_hi are required");
    SVC_REQUIRE(e->B >= 1 && e->C >= 1 && e->L >= 1, "svc_op_act_cl: B, C and L are positive");
    SVC_REQUIRE(e->ldx >= e->C && e->ldy >= e->C, "svc_op_act_cl: ldx and ldy cover C channels");
    SVC_REQUIRE(e->mode >= 0 && e->mode <= 2, "svc_op_act_cl: mode is 0 .. 2");
    SVC_REQUIRE(e->mode == 2 || (e->a && e->inv_b), "svc_op_act_cl: the Snake modes need a and inv_b");
    SVC_REQUIRE(e->lo_fmt == 0 || e->lo_fmt == 1, "svc_op_act_cl: lo_fmt is 0 (fp16 residual) or 1 (fp8 byte pair)");
    SVC_REQUIRE(e->out_f16 || (!e->y_lo && !e->lo_fmt), "svc_op_act_cl: the lo plane belongs to the fp16 output");
    SVC_REQUIRE(!e->lo_fmt || e->y_lo, "svc_op_act_cl: lo_fmt 1 needs y_lo");
    SVC_REQUIRE(!e->lens || e->mode == 0, "svc_op_act_cl: lens is for mode 0 only");
    SVC_REQUIRE((uintptr_t)e->x % 8 == 0 && (uintptr_t)e->y_hi % 4 == 0 && (uintptr_t)e->y_lo % 4 == 0,
                "svc_op_act_cl: alignment: x to 8 bytes, the planes to 4");
    if (e->lens)
        for (int b = 0; b < e->B; ++b) SVC_REQUIRE(e->lens[b] >= 0 && e->lens[b] <= e->L, "svc_op_act_cl: lens out of range");
    Arena ar;
    const int* d_lens = nullptr;
    if (op_host_ints(e->lens, e->B, ar, st, &d_lens)) return 1;
    if (act_cl_launch(e->x, (long)e->ldx, e->y_hi, e->y_lo, (long)e->ldy, e->out_f16, e->taps, e->a, e->inv_b, e->B, e->C, e->L, e->mode,
                      e->slope, st, e->lo_fmt, d_lens)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_op_hift_signal(const svc_hift_signal_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(e, "svc_op_hift_signal: null argument");
    SVC_REQUIRE(e->stage >= 1 && e->stage <= 6, "svc_op_hift_signal: stage is 1 .. 6");
    SVC_REQUIRE(e->in && e->out, "svc_op_hift_signal: in and out are required");
    const int B = e->B;
    SVC_REQUIRE(B >= 1 && e->n_utt >= 1, "svc_op_hift_signal: B and n_utt are positive");
    SVC_REQUIRE(e->src || B <= e->n_utt, "svc_op_hift_signal: without src, row j is utterance j < n_utt");
    if (e->src)
        for (int b = 0; b < B; ++b) SVC_REQUIRE(e->src[b] >= 0 && e->src[b] < e->n_utt, "svc_op_hift_signal: src out of range");
    const int stage = e->stage;
    if (stage == 1 || stage == 5) {
        SVC_REQUIRE(e->S >= 1 && e->S_in >= e->S, "svc_op_hift_signal: 1 <= S <= S_in");
        if (e->len)
            for (int b = 0; b < B; ++b) SVC_REQUIRE(e->len[b] >= 0 && e->len[b] <= e->S, "svc_op_hift_signal: len out of range");
    }
    if (stage == 2 || stage == 4) {
        SVC_REQUIRE(e->F >= 1 && e->Lw >= 1 && !e->lw == !e->nf, "svc_op_hift_signal: F and Lw are positive; lw and nf come together");
        if (e->lw)
            for (int b = 0; b < B; ++b)
                SVC_REQUIRE(e->lw[b] >= 0 && e->lw[b] <= e->Lw && e->nf[b] >= 0 && e->nf[b] <= e->F, "svc_op_hift_signal: lw or nf out of range");
    }
    if (stage == 1) {
        SVC_REQUIRE(e->phase0 && e->noise && e->lin_w && e->lin_b, "svc_op_hift_signal: the source needs phase0, noise, lin_w and lin_b");
        SVC_REQUIRE(e->NH >= 1 && e->up >= 1, "svc_op_hift_signal: NH and up are positive");
    } else if (stage == 2) {
        // every sample index a frame reflects to lies inside the row: 4 fr + 7 <= lw + 7 reflects to >= lw - 9, and 8 to 8
        SVC_REQUIRE(e->ld >= 18, "svc_op_hift_signal: the STFT writes 18 columns");
        for (int b = 0; b < B; ++b) {
            const long lwb = e->lw ? e->lw[b] : e->Lw, nfb = e->nf ? e->nf[b] : e->F;
            SVC_REQUIRE(nfb == 0 || (lwb >= 9 && nfb <= lwb / 4 + 1), "svc_op_hift_signal: frames need lw >= 9 and nf <= lw / 4 + 1");
        }
    } else if (stage == 3) {
        SVC_REQUIRE(e->F >= 1 && e->ld >= 18, "svc_op_hift_signal: F is positive, ld >= 18");
    } else if (stage >= 5) {
        SVC_REQUIRE(e->vd >= 0 && e->vd <= 3 && e->C >= 1 && e->ld >= e->C, "svc_op_hift_signal: vd is 0 .. 3, 1 <= C <= ld");
        SVC_REQUIRE(!is_split(e->vd) || e->out_lo, "svc_op_hift_signal: a split mode needs out_lo");
        SVC_REQUIRE(stage == 5 || (e->S >= 1 && (e->mode == 2 || e->mode == 3)), "svc_op_hift_signal: S is positive; ew_cl mode is 2 or 3");
    }
    Arena ar;
    const int *d_src, *d_len, *d_lw, *d_nf;
    if (op_host_ints(e->src, B, ar, st, &d_src) || op_host_ints(e->len, B, ar, st, &d_len) || op_host_ints(e->lw, B, ar, st, &d_lw) ||
        op_host_ints(e->nf, B, ar, st, &d_nf)) return 1;
    const RowMap rm{d_src, d_len, e->S_in};
    ActOut y;
    y.hi = e->out; y.lo = e->out_lo;
    if (stage == 1) {
        double* prefix = ar.alloc_n<double>((size_t)B * e->NH * e->S, st);
        if (!prefix) return 1;
        if (hift_source_launch(e->in, prefix, e->phase0, e->noise, nullptr, e->lin_w, e->lin_b, (float*)e->out, rm, B, e->S, e->NH, e->up,
                               e->sr, e->sine_amp, e->noise_std, e->voiced_thr, st)) return 1;
    } else if (stage == 2) {
        if (hift_stft_launch(e->in, (float*)e->out, d_lw, d_nf, B, (long)e->Lw, e->F, e->ld, st)) return 1;
    } else if (stage == 3) {
        if (hift_frames_launch(e->in, (float*)e->out, (long)B * e->F, e->ld, st)) return 1;
    } else if (stage == 4) {
        if (hift_ola_launch(e->in, (float*)e->out, rm, d_lw, d_nf, B, e->F, (long)e->Lw, e->limit, st)) return 1;
    } else if (stage == 5) {
        if (mel_to_cl(e->in, y, e->vd, rm, B, e->C, e->S, e->ld, st)) return 1;
    } else {
        if (ew_cl(e->in, y, e->vd, (long)B * e->S, e->C, e->ld, e->mode, e->slope, st)) return 1;
    }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
