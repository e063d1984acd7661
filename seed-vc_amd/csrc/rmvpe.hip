// RMVPE pitch extractor for gfx950: 16 kHz audio -> F0 at 100 frames/s (`rmvpe.infer_from_audio(wave_16k, thred)` of the
// reference drivers; architecture of RVC's rmvpe.py): its own log-mel front-end, a 5-level residual U-Net
// over the (time, mel bin) image, a bidirectional GRU, a 360-bin salience head and the local-average cents decode; plus the
// drivers' pitch step between the two tracks (voiced-median shift in the log domain and a semitone shift, svc_f0_adjust).
//
// Everything is fp32 on the MFMA (v_mfma_f32_16x16x4_f32 through the tap-GEMM).  Layout: a level-l plane is channels-last
// [B][H_l + 2][W_l][C], H_l = Tpad / 2^l time steps, W_l = n_mels / 2^l bins; whole time steps are the tap-GEMM's
// "sequences" and bins its "positions", so a 3 x 3 conv is 9 taps = 3 sequence offsets x 3 position shifts (the bin edges are
// the GEMM's zero padding, the time edges the two zero border sequences of every clip).  Eval-mode BatchNorms that follow a
// bias-free conv are folded into its weights + bias at pack time; the input BatchNorm is applied while the input plane is
// written (the conv's zero padding comes after it).  Every clip of a batch is computed as if alone: clip b has its own
// Tpad_b = 32 ceil(T_b / 32); after every conv the sequences at and above Tpad_b / 2^l are zeroed, the reverse GRU direction
// starts at Tpad_b - 1, and nothing at or above a clip's end is read as a value.  Per-row lengths travel as kernel arguments
// (at most 64 clips per call), so no call copies or synchronises.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "content_encoder.h"       // StageTimer, copy_f32

using namespace svc;

namespace {

constexpr float BN_EPS = 1e-5f;
constexpr int RV_NFFT = 1024, RV_HOP = 160, RV_PAD = RV_NFFT / 2, RV_NB = RV_NFFT / 2 + 1;
constexpr int RV_MAX_B = 64, RV_TMULT = 32, RV_MAX_LEVELS = 5;

struct Rows { int n[RV_MAX_B]; };                 // per-clip lengths (samples or frames) as a kernel argument
struct RowsF { float v[RV_MAX_B]; };

__device__ __forceinline__ int rv_tpad(int t) { return (t + RV_TMULT - 1) / RV_TMULT * RV_TMULT; }

__global__ void rv_bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                                  const float* __restrict__ var, float* __restrict__ scale, float* __restrict__ shift, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = gamma[i] / sqrtf(var[i] + BN_EPS);
    scale[i] = s;
    shift[i] = beta[i] - mean[i] * s;
}

// ---- mel front-end: center=True reflect padding of n_fft / 2 at the clip's own ends; dst [B][stride], zero above
__global__ void rv_pad_kernel(const float* __restrict__ y, Rows lens, int Lrow, float* __restrict__ dst, long stride) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stride) return;
    const int L = lens.n[b];
    float v = 0.f;
    if (i < L + 2 * RV_PAD) {
        long q = i - RV_PAD;
        q = q < 0 ? -q : (q >= L ? 2L * (L - 1) - q : q);
        v = y[(long)b * Lrow + q];
    }
    dst[(long)b * stride + i] = v;
}

// spec [M][ld_s] = (re | im) -> mag [M][ld_m] = sqrt(re^2 + im^2) (no epsilon), pad columns zero
__global__ void rv_mag_kernel(const float* __restrict__ spec, long ld_s, float* __restrict__ mag, long ld_m, int nb) {
    const long m = blockIdx.x;
    const int k = blockIdx.y * blockDim.x + threadIdx.x;
    if (k >= ld_m) return;
    float v = 0.f;
    if (k < nb) {
        const float re = spec[m * ld_s + k], im = spec[m * ld_s + nb + k];
        v = sqrtf(re * re + im * im);
    }
    mag[m * ld_m + k] = v;
}

// out[b][mel][f] = log(max(c[b * frames + f][mel], 1e-5)) for f < 1 + lens[b] / hop, 0 above
__global__ void rv_mellog_kernel(const float* __restrict__ c, long ldc, float* __restrict__ out, Rows lens, int n_mels, int frames) {
    const int b = blockIdx.z, f = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (f >= frames) return;
    const bool live = f < 1 + lens.n[b] / RV_HOP;
    out[((long)b * n_mels + j) * frames + f] = live ? logf(fmaxf(c[((long)b * frames + f) * ldc + j], 1e-5f)) : 0.f;
}

// ---- network input: mel [B][W][Tm] -> channel 0 of plane [B][H + 2][W][32] through the input BatchNorm.  Frames
// [T_b, Tpad_b) hold zero mel BEFORE the BatchNorm (they carry its shift); the border sequences and everything at and above
// Tpad_b are the convs' zero padding.  mel frames at and above T_b are never read
__global__ void rv_input_kernel(const float* __restrict__ mel, int Tm, float* __restrict__ plane, Rows fr, int B, int H, int W,
                                const float* __restrict__ s, const float* __restrict__ h) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * (H + 2) * W) return;
    const int w = (int)(i % W);
    const long bt = i / W;
    const int tp = (int)(bt % (H + 2)), b = (int)(bt / (H + 2)), t = tp - 1;
    const int Tb = fr.n[b];
    float v = 0.f;
    if (tp >= 1 && t < rv_tpad(Tb)) v = (t < Tb ? mel[((long)b * W + w) * Tm + t] : 0.f) * s[0] + h[0];
    plane[i * 32] = v;
}

// zero sequence 0 and every sequence above Tpad_b >> lvl of clip b in columns [0, ncol) of buf [B][Hp][W][ld] (ncol % 4 == 0):
// what a conv wrote there is the zero padding of the next one
__global__ void rv_zero_tail_kernel(float* __restrict__ buf, long ld, int ncol4, Rows fr, int lvl, int B, int Hp, int W) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * Hp * W * ncol4) return;
    const int c4 = (int)(i % ncol4);
    const long row = i / ncol4;
    const long bt = row / W;
    const int tp = (int)(bt % Hp), b = (int)(bt / Hp);
    if (tp == 0 || tp > (rv_tpad(fr.n[b]) >> lvl)) *reinterpret_cast<float4*>(buf + row * ld + 4 * c4) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// AvgPool2d(2, 2): columns [0, C) of x [B][H + 2][W][ldx] -> y [B][H / 2 + 2][W / 2][ldy]; pad columns and borders zero
__global__ void rv_pool_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y, int ldy, int C, int B, int H, int W) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int Ho = H / 2, Wo = W / 2;
    if (i >= (long)B * (Ho + 2) * Wo * ldy) return;
    const int c = (int)(i % ldy);
    const long row = i / ldy;
    const int wo = (int)(row % Wo);
    const long bt = row / Wo;
    const int tpo = (int)(bt % (Ho + 2)), b = (int)(bt / (Ho + 2));
    float v = 0.f;
    if (c < C && tpo >= 1 && tpo <= Ho) {
        const float* p = x + (((long)b * (H + 2) + 2 * (tpo - 1) + 1) * W + 2 * wo) * ldx + c;
        v = ((p[0] + p[ldx]) + (p[(long)W * ldx] + p[(long)W * ldx + ldx])) * 0.25f;
    }
    y[i] = v;
}

// the four output phases of the stride-2 transposed conv, ph [B][Hi + 2][Wi][4 C] (phase = 2 py + px), interleaved into columns
// [0, C) of the concat buffer y [B][2 Hi + 2][2 Wi][ldy]; border sequences and those above the clip's own end are zero
__global__ void rv_interleave_kernel(const float* __restrict__ ph, float* __restrict__ y, long ldy, int C4, Rows fr, int lvl, int B,
                                     int Hi, int Wi) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int H = 2 * Hi, W = 2 * Wi;
    if (i >= (long)B * (H + 2) * W * C4) return;
    const int c4 = (int)(i % C4);
    const long row = i / C4;
    const int w = (int)(row % W);
    const long bt = row / W;
    const int tp = (int)(bt % (H + 2)), b = (int)(bt / (H + 2));
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tp >= 1 && tp <= (rv_tpad(fr.n[b]) >> lvl)) {
        const int py = (tp - 1) & 1, m = (tp - 1) >> 1, px = w & 1, n = w >> 1;
        v = *reinterpret_cast<const float4*>(ph + (((long)b * (Hi + 2) + m + 1) * Wi + n) * (16L * C4) + (py * 2 + px) * 4 * C4 + 4 * c4);
    }
    *reinterpret_cast<float4*>(y + row * ldy + 4 * c4) = v;
}

// ---- bidirectional GRU recurrence (torch gate order r, z, n), one persistent workgroup per (direction, R clips): thread u
// owns hidden unit u of all three gates, the state lives in LDS (double-buffered: one barrier per step), W_hh streams from L2
// as [Hd / 4][3 Hd][4] (16-byte coalesced), every read of it shared by the R clips of the workgroup.  State and sums fp32,
// each sum in k order and every gate rounded the same way whatever R is (a row's bits do not depend on its workgroup's other rows).  xp [B][H][6 Hd] = W_ih x + b_ih (forward | reverse); out [B][H][2 Hd].
// Clip b runs Tpad_b steps: forward t = s, reverse t = Tpad_b - 1 - s.  No workgroup waits for another.
template <int R>
__global__ __launch_bounds__(256) void rv_gru_kernel(const float* __restrict__ xp, const float* __restrict__ w4, const float* __restrict__ bhh,
                                                     float* __restrict__ out, Rows fr, int B, int H, int Hd) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float hs[2][R][256];
    const int u = threadIdx.x, dir = blockIdx.y, b0 = blockIdx.x * R;
    const float4* w = reinterpret_cast<const float4*>(w4) + (long)dir * (Hd / 4) * 3 * Hd;
    const float br = bhh[dir * 3 * Hd + u], bz = bhh[dir * 3 * Hd + Hd + u], bn = bhh[dir * 3 * Hd + 2 * Hd + u];
    int len[R], steps = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        len[r] = b0 + r < B ? rv_tpad(fr.n[b0 + r]) : 0;
        steps = max(steps, len[r]);
        hs[0][r][u] = 0.f;
    }
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const int cur = s & 1;
        float xr[R], xz[R], xn[R], ar[R], az[R], an[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            ar[r] = az[r] = an[r] = 0.f;
            xr[r] = xz[r] = xn[r] = 0.f;
            if (s < len[r]) {
                const int t = dir ? len[r] - 1 - s : s;
                const float* x = xp + ((long)(b0 + r) * H + t) * 6 * Hd + dir * 3 * Hd + u;
                xr[r] = x[0]; xz[r] = x[Hd]; xn[r] = x[2 * Hd];
            }
        }
#pragma unroll 4
        for (int k4 = 0; k4 < Hd / 4; ++k4) {
            const float4 wr = w[(long)k4 * 3 * Hd + u], wz = w[(long)k4 * 3 * Hd + Hd + u], wn = w[(long)k4 * 3 * Hd + 2 * Hd + u];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 h4 = *reinterpret_cast<const float4*>(&hs[cur][r][4 * k4]);
                ar[r] = fmaf(wr.x, h4.x, ar[r]); ar[r] = fmaf(wr.y, h4.y, ar[r]); ar[r] = fmaf(wr.z, h4.z, ar[r]); ar[r] = fmaf(wr.w, h4.w, ar[r]);
                az[r] = fmaf(wz.x, h4.x, az[r]); az[r] = fmaf(wz.y, h4.y, az[r]); az[r] = fmaf(wz.z, h4.z, az[r]); az[r] = fmaf(wz.w, h4.w, az[r]);
                an[r] = fmaf(wn.x, h4.x, an[r]); an[r] = fmaf(wn.y, h4.y, an[r]); an[r] = fmaf(wn.z, h4.z, an[r]); an[r] = fmaf(wn.w, h4.w, an[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float hold = hs[cur][r][u];
            float hnew = hold;
            if (s < len[r]) {                                // every product below is an explicit fmaf (and contraction is off):
                const float rg = 1.f / (1.f + expf(-((xr[r] + ar[r]) + br)));      // the rounding does not depend on R
                const float zg = 1.f / (1.f + expf(-((xz[r] + az[r]) + bz)));
                const float ng = tanhf(fmaf(rg, an[r] + bn, xn[r]));
                hnew = fmaf(zg, hold - ng, ng);              // (1 - z) n + z h
                const int t = dir ? len[r] - 1 - s : s;
                out[((long)(b0 + r) * H + t) * 2 * Hd + dir * Hd + u] = hnew;
            }
            hs[cur ^ 1][r][u] = hnew;
        }
        __syncthreads();
    }
}

// rows t >= T_b of out [B][T][n] become zero
__global__ void rv_zero_rows_kernel(float* __restrict__ out, Rows fr, int B, int T, int n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * T * n) return;
    const long bt = i / n;
    if ((int)(bt % T) >= fr.n[bt / T]) out[i] = 0.f;
}

// ---- decode: one wave per frame.  arg-max bin (first maximum on ties), salience-weighted mean of cents[k] = 20 k + c0 over the 9
// bins around it (bins outside [0, n_bins) contribute zero), 0 when the maximum is <= thred; f0 = 10 * 2^(cents / 1200), unvoiced
// frames and frames at and above the clip's count exactly 0 (those are never read)
__global__ __launch_bounds__(256) void rv_decode_kernel(const float* __restrict__ sal, Rows fr, int B, int T, int n_bins, float thred,
                                                        float* __restrict__ f0) {
    const long f = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= (long)B * T) return;
    const int b = (int)(f / T), t = (int)(f % T);
    if (t >= fr.n[b]) {
        if (lane == 0) f0[f] = 0.f;
        return;
    }
    const float* s = sal + f * n_bins;
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int k = lane; k < n_bins; k += 64) {
        const float v = s[k];
        if (v > best) { best = v; arg = k; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oa = __shfl_xor(arg, o);
        if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
    }
    if (lane == 0) {
        float ps = 0.f, ws = 0.f;
        if (arg < n_bins)                                    // (a row of NaN has no maximum: unvoiced)
            for (int k = arg - 4; k <= arg + 4; ++k)
                if (k >= 0 && k < n_bins) {
                    const float v = s[k];
                    ps = fmaf(v, 20.f * (float)k + 1997.3794084376191f, ps);
                    ws += v;
                }
        const bool voiced = best > thred && ws > 0.f;
        f0[f] = voiced ? 10.f * exp2f(ps / ws * (1.f / 1200.f)) : 0.f;
    }
}

// ---- the drivers' pitch step, one workgroup per row.  key(f) = bits of log(f + 1e-5) for voiced frames (f > 1: the log is
// positive, and positive floats order like unsigned integers).  Lower-middle median (torch.median) by a 4-pass radix select:
// 256-bin histogram of the next byte of the keys that match the prefix found so far, in LDS; no sort
__device__ float f0_median(const float* __restrict__ f, int n, unsigned* hist, unsigned* sh, int* n_voiced) {
    const int tid = threadIdx.x;
    unsigned cnt = 0;
    for (int i = tid; i < n; i += 256) cnt += f[i] > 1.f;
    hist[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned tot = 0;
        for (int i = 0; i < 256; ++i) tot += hist[i];
        sh[0] = tot;
    }
    __syncthreads();
    const unsigned nv = sh[0];
    *n_voiced = (int)nv;
    __syncthreads();
    if (nv == 0) return 0.f;
    unsigned rank = (nv - 1) / 2, prefix = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            const float v = f[i];
            if (v > 1.f) {
                const unsigned key = __float_as_uint(logf(v + 1e-5f));
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            unsigned cum = 0;
            int d = 0;
            for (; d < 255; ++d) {
                if (cum + hist[d] > rank) break;
                cum += hist[d];
            }
            sh[1] = prefix | ((unsigned)d << shift);
            sh[2] = rank - cum;
        }
        __syncthreads();
        prefix = sh[1]; rank = sh[2];
        __syncthreads();
    }
    return __uint_as_float(prefix);
}

__global__ __launch_bounds__(256) void f0_adjust_kernel(const float* __restrict__ f0_alt, Rows alt_lens, const float* __restrict__ f0_ori,
                                                        Rows ori_lens, int Talt, int Tori, int auto_adjust, RowsF semis,
                                                        float* __restrict__ out, float* __restrict__ medians) {
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[4];
    const int b = blockIdx.x, na = alt_lens.n[b], no = ori_lens.n[b];
    const float* fa = f0_alt + (long)b * Talt;
    int va = 0, vo = 0;
    const float m_alt = f0_median(fa, na, hist, sh, &va);
    const float m_ori = f0_median(f0_ori + (long)b * Tori, no, hist, sh, &vo);
    if (medians && threadIdx.x == 0) { medians[2 * b] = m_alt; medians[2 * b + 1] = m_ori; }
    const bool shifted = auto_adjust && va > 0 && vo > 0;                             // a side without voiced frames: no shift
    const float factor = exp2f(semis.v[b] * (1.f / 12.f));
    for (int i = threadIdx.x; i < Talt; i += 256) {
        float o = 0.f;
        if (i < na) {
            const float v = fa[i], lg = logf(v + 1e-5f);
            o = v > 1.f ? expf(shifted ? (lg - m_alt) + m_ori : lg) * factor : expf(lg);
        }
        out[(long)b * Talt + i] = o;
    }
}

struct Gemm {          // one fp32 tap-GEMM launch on channels-last rows
    KGemmParams p;
    Gemm(long M, int N, int Lout) {
        memset(&p, 0, sizeof(p));
        p.M = (int)M; p.N = N; p.Lout = Lout; p.a_seq_rows = Lout; p.c_seq_rows = Lout; p.a_stride = 1; p.a_len = Lout; p.n_taps = 1;
    }
    int run(hipStream_t st) {
        p.vec_ok = (p.N % 8 == 0) && (p.ldc32 % 8 == 0) && (p.ldres % 8 == 0);
        return kgemm_launch(p, 1, KG_EPI_STORE, st);
    }
};

struct Plane {         // device buffer with one guard sequence in front (a conv's t - 1 tap of the first sequence lands there)
    float* base = nullptr;
    float* p = nullptr;
};

}  // namespace

struct svc_rmvpe {
    svc_rmvpe_config_t cfg;
    int L = 0;                      // U-Net depth
    int C[RV_MAX_LEVELS + 1];       // channels of level l
    Arena wts, ws, mws, tmp;
    long plane_budget = 256L << 20; // bytes of ONE level-0 plane [B][Tpad + 2][n_mels][32] a group of clips may take
    struct Conv { float* w = nullptr; float* b = nullptr; long ldw = 0; int N = 0; };
    struct Block { Conv c1, c2, sc; bool has_sc = false; };
    std::vector<Block> enc[RV_MAX_LEVELS], dec[RV_MAX_LEVELS];
    std::vector<Block> inter;
    Conv up[RV_MAX_LEVELS][4];      // transposed conv of decoder layer d, one weight matrix per output phase
    Conv cnn, gru_in, fc;
    float *in_s = nullptr, *in_h = nullptr, *w_hh4 = nullptr, *b_hh = nullptr;
    // mel front-end
    float *dft = nullptr, *fb = nullptr;
    long ld_fb = 0;
    long mel_cap_rows = 0, mel_cap_stride = 0;
    int mel_cap_B = 0;
    float *padded = nullptr, *spec = nullptr, *mag = nullptr, *melc = nullptr;
    // network workspace for cap_B clips of cap_H (padded) frames
    int cap_B = 0, cap_H = 0;
    Plane pin[RV_MAX_LEVELS + 1], pa[RV_MAX_LEVELS + 1], pb[RV_MAX_LEVELS + 1], pt[RV_MAX_LEVELS + 1], pk[RV_MAX_LEVELS];
    float *phases = nullptr, *cnn_out = nullptr, *xp = nullptr, *gru_out = nullptr;
    StageTimer tm;                  // svc_rmvpe_set_timing
    // svc_rmvpe_f0 scratch
    long f0_cap = 0;
    float *f0_mel = nullptr, *f0_sal = nullptr;

    int ldl(int l) const { return std::max(32, C[l]); }
    int pack(const StateDict& sd, const float* mel_basis, hipStream_t st);
    int pack_block(const StateDict& sd, const std::string& p, int cin, int cin_ld, int cout, Block* b, hipStream_t st);
    int reserve(int B, int H, hipStream_t st);
    int conv(const Conv& c, const float* x, long ldx, float* y, long ldy, int lvl, int taps, const float* res, long ldres, int act,
             bool zero_tail, const Rows& fr, int B, int H, hipStream_t st);
    int run_blocks(const std::vector<Block>& blocks, const float* x, long ldx, int lvl, float* last_dst, long last_ld, const Rows& fr, int B,
                   int H, const float** out, hipStream_t st);
    int mel(const float* wave, const Rows& lens, int B, int L, float* out, hipStream_t st);
    int salience_group(const float* mel, int Tm, const Rows& fr, int B, int T, float* out, hipStream_t st);
    int salience(const float* mel, const int32_t* frame_lens, int B, int T, float* out, hipStream_t st);
    int group_size(int B, int H) const {
        const long per_clip = (long)(H + 2) * cfg.n_mels * 32 * 4;
        return (int)std::max(1L, std::min((long)B, plane_budget / per_clip));
    }
};

namespace {

int rv_bn_fold(const StateDict& sd, const std::string& p, int n, Arena& ar, hipStream_t st, float** scale, float** shift) {
    const auto *g = sd.get(p + ".weight"), *b = sd.get(p + ".bias"), *m = sd.get(p + ".running_mean"), *v = sd.get(p + ".running_var");
    if (require_shape(g, p + ".weight", {n}) || require_shape(b, p + ".bias", {n}) || require_shape(m, p + ".running_mean", {n}) ||
        require_shape(v, p + ".running_var", {n})) return 1;
    *scale = ar.alloc_n<float>(round_up(n, 8), st);
    *shift = ar.alloc_n<float>(round_up(n, 8), st);
    if (!*scale || !*shift) return 1;
    hipLaunchKernelGGL(rv_bn_fold_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, g->data, b->data, m->data, v->data, *scale, *shift, n);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// Conv2d weight [N][Cin][kh][kw] -> [Npad128][taps * cin_ld], tap = kh * 3 + kw (kh: time, kw: bin), optional row scale
int rv_pack_conv(const float* src, int N, int Cin, int taps, int cin_ld, const float* scale, Arena& ar, hipStream_t st,
                 svc_rmvpe::Conv* out) {
    out->N = N;
    out->ldw = (long)taps * cin_ld;
    out->w = ar.alloc_n<float>((size_t)round_up(N, 128) * out->ldw, st);
    if (!out->w) return 1;
    for (int t = 0; t < taps; ++t)
        if (pack_f32_launch(src + t, out->w + (long)t * cin_ld, N, Cin, 1, (long)Cin * taps, taps, 0, out->ldw, 1, 0, scale, st)) return 1;
    return 0;
}

}  // namespace

#define GETW(var, name, ...)                                              \
    const svc_tensor_desc_t* var = sd.get(name);                          \
    if (require_shape(var, name, {__VA_ARGS__})) return 1;

// ConvBlockRes(cin, cout): conv.0 (3 x 3, no bias) + conv.1 (BatchNorm) + ReLU, conv.3 + conv.4 + ReLU, + shortcut (1 x 1 with
// bias when cin != cout)
int svc_rmvpe::pack_block(const StateDict& sd, const std::string& p, int cin, int cin_ld, int cout, Block* b, hipStream_t st) {
    const int cout_ld = std::max(32, cout);
    float *s, *h;
    {
        GETW(w, p + ".conv.0.weight", cout, cin, 3, 3);
        if (rv_bn_fold(sd, p + ".conv.1", cout, wts, st, &s, &h)) return 1;
        b->c1.b = h;
        if (rv_pack_conv(w->data, cout, cin, 9, cin_ld, s, wts, st, &b->c1)) return 1;
    }
    {
        GETW(w, p + ".conv.3.weight", cout, cout, 3, 3);
        if (rv_bn_fold(sd, p + ".conv.4", cout, wts, st, &s, &h)) return 1;
        b->c2.b = h;
        if (rv_pack_conv(w->data, cout, cout, 9, cout_ld, s, wts, st, &b->c2)) return 1;
    }
    b->has_sc = cin != cout;
    if (b->has_sc) {
        GETW(w, p + ".shortcut.weight", cout, cin, 1, 1);
        GETW(bias, p + ".shortcut.bias", cout);
        if (!(b->sc.b = copy_f32(bias->data, cout, wts, st))) return 1;
        if (rv_pack_conv(w->data, cout, cin, 1, cin_ld, nullptr, wts, st, &b->sc)) return 1;
    }
    return 0;
}

int svc_rmvpe::pack(const StateDict& sd, const float* mel_basis, hipStream_t st) {
    L = cfg.en_de_layers;
    for (int l = 0; l <= L; ++l) C[l] = cfg.en_out_channels << l;
    const int nb = cfg.n_blocks, Hd = cfg.gru_hidden, W = cfg.n_mels;
    if (rv_bn_fold(sd, "unet.encoder.bn", 1, wts, st, &in_s, &in_h)) return 1;
    for (int l = 0; l < L; ++l) {
        enc[l].resize(nb);
        for (int j = 0; j < nb; ++j) {
            const int cin = j == 0 ? (l == 0 ? 1 : C[l - 1]) : C[l];
            if (pack_block(sd, "unet.encoder.layers." + std::to_string(l) + ".conv." + std::to_string(j), cin, std::max(32, cin), C[l],
                           &enc[l][j], st)) return 1;
        }
    }
    inter.resize((size_t)cfg.inter_layers * nb);
    for (int i = 0; i < cfg.inter_layers; ++i)
        for (int j = 0; j < nb; ++j) {
            const int cin = (i == 0 && j == 0) ? C[L - 1] : C[L];
            if (pack_block(sd, "unet.intermediate.layers." + std::to_string(i) + ".conv." + std::to_string(j), cin, std::max(32, cin), C[L],
                           &inter[(size_t)i * nb + j], st)) return 1;
        }
    // decoder layer d: level L - d (2 c channels) -> level l = L - d - 1 (c channels)
    static const int ph_taps[4][4][2] = {{{1, 1}}, {{1, 2}, {1, 0}}, {{2, 1}, {0, 1}}, {{2, 2}, {2, 0}, {0, 2}, {0, 0}}};   // (kh, kw) per tap
    static const int ph_n[4] = {1, 2, 2, 4};
    for (int d = 0; d < L; ++d) {
        const int l = L - d - 1, c = C[l], cin = 2 * c;
        const std::string p = "unet.decoder.layers." + std::to_string(d);
        GETW(w, p + ".conv1.0.weight", cin, c, 3, 3);
        float *s, *h;
        if (rv_bn_fold(sd, p + ".conv1.1", c, wts, st, &s, &h)) return 1;
        for (int ph = 0; ph < 4; ++ph) {
            Conv& u = up[d][ph];
            u.N = c; u.b = h; u.ldw = (long)ph_n[ph] * cin;
            u.w = wts.alloc_n<float>((size_t)round_up(c, 128) * u.ldw, st);
            if (!u.w) return 1;
            for (int t = 0; t < ph_n[ph]; ++t)      // ConvTranspose2d weight [cin][c][kh][kw]
                if (pack_f32_launch(w->data + ph_taps[ph][t][0] * 3 + ph_taps[ph][t][1], u.w + (long)t * cin, c, cin, 1, 9, (long)c * 9, 0,
                                    u.ldw, 1, 0, s, st)) return 1;
        }
        dec[d].resize(nb);
        for (int j = 0; j < nb; ++j) {
            const int bc = j == 0 ? 2 * c : c;
            if (pack_block(sd, p + ".conv2." + std::to_string(j), bc, std::max(32, bc), c, &dec[d][j], st)) return 1;
        }
    }
    {   // head conv: Conv2d(c0, 3, 3 x 3, bias)
        GETW(w, "cnn.weight", 3, C[0], 3, 3);
        GETW(b, "cnn.bias", 3);
        if (!(cnn.b = copy_f32(b->data, 3, wts, st))) return 1;
        if (rv_pack_conv(w->data, 3, C[0], 9, ldl(0), nullptr, wts, st, &cnn)) return 1;
    }
    {   // GRU: the reference's feature index is c * W + bin, the head conv's rows are [bin][4] (channel 3 = zero)
        const int K = 4 * W;
        gru_in.N = 6 * Hd; gru_in.ldw = K;
        gru_in.w = wts.alloc_n<float>((size_t)round_up(6 * Hd, 128) * K, st);
        gru_in.b = wts.alloc_n<float>(6 * Hd, st);
        w_hh4 = wts.alloc_n<float>((size_t)2 * 3 * Hd * Hd, st);
        b_hh = wts.alloc_n<float>(6 * Hd, st);
        if (!gru_in.w || !gru_in.b || !w_hh4 || !b_hh) return 1;
        for (int dir = 0; dir < 2; ++dir) {
            const std::string sfx = dir ? "_reverse" : "";
            GETW(wih, "fc.0.gru.weight_ih_l0" + sfx, 3 * Hd, 3 * W);
            GETW(whh, "fc.0.gru.weight_hh_l0" + sfx, 3 * Hd, Hd);
            GETW(bih, "fc.0.gru.bias_ih_l0" + sfx, 3 * Hd);
            GETW(bhh, "fc.0.gru.bias_hh_l0" + sfx, 3 * Hd);
            if (pack_f32_launch(wih->data, gru_in.w + (long)dir * 3 * Hd * K, 3 * Hd, 3, W, 3L * W, W, 1, K, 1, 4, nullptr, st)) return 1;
            if (pack_f32_launch(whh->data, w_hh4 + (long)dir * 3 * Hd * Hd, 3 * Hd, Hd / 4, 4, Hd, 4, 1, 4, 12L * Hd, 1, nullptr, st)) return 1;
            SVC_CHECK_HIP(hipMemcpyAsync(gru_in.b + dir * 3 * Hd, bih->data, (size_t)3 * Hd * 4, hipMemcpyDeviceToDevice, st));
            SVC_CHECK_HIP(hipMemcpyAsync(b_hh + dir * 3 * Hd, bhh->data, (size_t)3 * Hd * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    {
        GETW(w, "fc.1.weight", cfg.n_bins, 2 * Hd);
        GETW(b, "fc.1.bias", cfg.n_bins);
        if (!(fc.b = copy_f32(b->data, cfg.n_bins, wts, st))) return 1;
        fc.N = cfg.n_bins; fc.ldw = 2 * Hd;
        fc.w = wts.alloc_n<float>((size_t)round_up(cfg.n_bins, 128) * fc.ldw, st);
        if (!fc.w) return 1;
        if (pack_f32_launch(w->data, fc.w, cfg.n_bins, 2 * Hd, 1, 2L * Hd, 1, 0, fc.ldw, 1, 0, nullptr, st)) return 1;
    }
    {   // mel front-end: periodic Hann window folded into the DFT basis (float64 trigonometry), mel basis [n_mels][513] padded
        std::vector<float> basis((size_t)round_up(2 * RV_NB, 128) * RV_NFFT, 0.f);
        for (int k = 0; k < RV_NB; ++k)
            for (int n = 0; n < RV_NFFT; ++n) {
                const double ang = 2.0 * M_PI * (double)(((long)k * n) % RV_NFFT) / (double)RV_NFFT;
                const double hw = 0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)RV_NFFT);
                basis[(size_t)k * RV_NFFT + n] = (float)(cos(ang) * hw);
                basis[(size_t)(RV_NB + k) * RV_NFFT + n] = (float)(-sin(ang) * hw);
            }
        dft = wts.alloc_n<float>(basis.size(), st);
        ld_fb = round_up(RV_NB, 32);
        fb = wts.alloc_n<float>((size_t)round_up(W, 128) * ld_fb, st);
        if (!dft || !fb) return 1;
        SVC_CHECK_HIP(hipMemcpyAsync(dft, basis.data(), basis.size() * 4, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        if (pack_f32_launch(mel_basis, fb, W, 1, RV_NB, RV_NB, 0, 1, ld_fb, 0, 1, nullptr, st)) return 1;
    }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_rmvpe::reserve(int B, int H, hipStream_t st) {
    if (B <= cap_B && H <= cap_H) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws.release();
    cap_B = std::max(B, cap_B); cap_H = std::max(H, cap_H);
    const int W = cfg.n_mels, Hd = cfg.gru_hidden;
    auto plane = [&](Plane& pl, int l, int ld) -> int {
        const long guard = (long)(W >> l) * ld, n = (long)cap_B * ((cap_H >> l) + 2) * (W >> l) * ld;
        pl.base = ws.alloc_n<float>((size_t)(n + 2 * guard), st);
        if (!pl.base) return 1;
        pl.p = pl.base + guard;
        return 0;
    };
    for (int l = 0; l <= L; ++l) {
        if (plane(pin[l], l, l == 0 ? 32 : ldl(l - 1)) || plane(pa[l], l, ldl(l)) || plane(pb[l], l, ldl(l)) || plane(pt[l], l, ldl(l))) return 1;
        if (l < L && plane(pk[l], l, 2 * C[l])) return 1;
    }
    phases = ws.alloc_n<float>((size_t)cap_B * ((cap_H >> 1) + 2) * (W >> 1) * 4 * C[0], st);     // level 1 -> 0 is the largest
    cnn_out = ws.alloc_n<float>((size_t)cap_B * (cap_H + 2) * W * 4, st);
    xp = ws.alloc_n<float>((size_t)cap_B * cap_H * 6 * Hd, st);
    gru_out = ws.alloc_n<float>((size_t)cap_B * cap_H * 2 * Hd, st);
    if (!phases || !cnn_out || !xp || !gru_out) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// x [B][H_l + 2][W_l][ldx] -> columns [0, c.N) of y [B][H_l + 2][W_l][ldy]: bias, act (ReLU), then + res.  taps 9 (3 x 3, pad 1) or 1
int svc_rmvpe::conv(const Conv& c, const float* x, long ldx, float* y, long ldy, int lvl, int taps, const float* res, long ldres, int act,
                    bool zero_tail, const Rows& fr, int B, int H, hipStream_t st) {
    const int Hl = H >> lvl, Wl = cfg.n_mels >> lvl, Hp = Hl + 2;
    SVC_REQUIRE((long)B * Hp * Wl < (1L << 30), "RMVPE: a group's plane rows must stay below 2^30 (lower the plane budget)");
    Gemm g((long)B * Hp * Wl, c.N, Wl);
    g.p.pad_mode = KG_PAD_ZERO;
    g.p.n_taps = taps;
    for (int t = 0; t < taps; ++t) {
        const int dt = taps == 9 ? t / 3 : 1, df = taps == 9 ? t % 3 : 1;
        g.p.a_ptr[t] = x + (long)(dt - 1) * Wl * ldx;        // the t - 1 / t + 1 neighbour = one whole sequence away
        g.p.a_ld[t] = ldx; g.p.a_ktiles[t] = (int)(ldx / 32); g.p.a_shift[t] = df - 1;
    }
    g.p.w = c.w; g.p.ldw = c.ldw; g.p.bias = c.b;
    g.p.c32 = y; g.p.ldc32 = ldy;
    g.p.res = res; g.p.ldres = ldres;
    g.p.act = act; g.p.act_slope = 0.f;
    if (g.run(st)) return 1;
    if (zero_tail) {
        const int n4 = c.N / 4;
        hipLaunchKernelGGL(rv_zero_tail_kernel, dim3(cdiv((long)B * Hp * Wl * n4, 256)), dim3(256), 0, st, y, ldy, n4, fr, lvl, B, Hp, Wl);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

// a chain of ConvBlockRes at one level; the last block writes to last_dst (ld last_ld) when given.  *out = where the result is
int svc_rmvpe::run_blocks(const std::vector<Block>& blocks, const float* x, long ldx, int lvl, float* last_dst, long last_ld, const Rows& fr,
                          int B, int H, const float** out, hipStream_t st) {
    const int LR = KG_ACT_LRELU;                             // leaky ReLU with slope 0 = ReLU
    const long ld = ldl(lvl);
    float* t1 = pt[lvl].p;
    for (size_t j = 0; j < blocks.size(); ++j) {
        const Block& b = blocks[j];
        float* y = x == pa[lvl].p ? pb[lvl].p : pa[lvl].p;
        long ldy = ld;
        if (j + 1 == blocks.size() && last_dst) { y = last_dst; ldy = last_ld; }
        if (conv(b.c1, x, ldx, t1, ld, lvl, 9, nullptr, 0, LR, true, fr, B, H, st)) return 1;
        const float* shortcut = x;
        long ldsc = ldx;
        if (b.has_sc) {                                      // 1 x 1 shortcut into y, then y = relu(bn(conv(t1))) + y in place
            if (conv(b.sc, x, ldx, y, ldy, lvl, 1, nullptr, 0, KG_ACT_NONE, false, fr, B, H, st)) return 1;
            shortcut = y; ldsc = ldy;
        }
        if (conv(b.c2, t1, ld, y, ldy, lvl, 9, shortcut, ldsc, LR, true, fr, B, H, st)) return 1;
        x = y; ldx = ldy;
    }
    *out = x;
    return 0;
}

// mel [B][n_mels][Tm] (frames at and above fr.n[b] never read) -> out [B][T][n_bins]; H = padded frames of the longest clip
int svc_rmvpe::salience_group(const float* mel, int Tm, const Rows& fr, int B, int T, float* out, hipStream_t st) {
    const int W = cfg.n_mels, Hd = cfg.gru_hidden;
    int H = 0;
    for (int b = 0; b < B; ++b) H = std::max(H, (fr.n[b] + RV_TMULT - 1) / RV_TMULT * RV_TMULT);
    if (reserve(B, H, st) || tm.mark(0, st)) return 1;
    hipLaunchKernelGGL(rv_input_kernel, dim3(cdiv((long)B * (H + 2) * W, 256)), dim3(256), 0, st, mel, Tm, pin[0].p, fr, B, H, W, in_s, in_h);
    SVC_CHECK_HIP(hipGetLastError());
    const float* x = pin[0].p;
    for (int l = 0; l < L; ++l) {                            // encoder: the level's output is the skip, written into the concat buffer
        const float* skip;
        if (run_blocks(enc[l], x, l == 0 ? 32 : ldl(l - 1), l, pk[l].p + C[l], 2 * C[l], fr, B, H, &skip, st)) return 1;
        const int ldo = ldl(l);                              // input plane of level l + 1 carries C[l] channels
        hipLaunchKernelGGL(rv_pool_kernel, dim3(cdiv((long)B * ((H >> (l + 1)) + 2) * (W >> (l + 1)) * ldo, 256)), dim3(256), 0, st, skip,
                           2L * C[l], pin[l + 1].p, ldo, C[l], B, H >> l, W >> l);
        SVC_CHECK_HIP(hipGetLastError());
        x = pin[l + 1].p;
    }
    if (run_blocks(inter, x, ldl(L - 1), L, nullptr, 0, fr, B, H, &x, st)) return 1;
    static const int ph_d[4][4][2] = {{{0, 0}}, {{0, 0}, {0, 1}}, {{0, 0}, {1, 0}}, {{0, 0}, {0, 1}, {1, 0}, {1, 1}}};       // (dy, dx) per tap
    static const int ph_n[4] = {1, 2, 2, 4};
    for (int d = 0; d < L; ++d) {
        const int l = L - d - 1, c = C[l], Hi = H >> (l + 1), Wi = W >> (l + 1);
        const long ldx = 2 * c;
        for (int ph = 0; ph < 4; ++ph) {                     // transposed conv: out[2 m + py][2 n + px] from in[m + dy][n + dx]
            Gemm g((long)B * (Hi + 2) * Wi, c, Wi);
            g.p.pad_mode = KG_PAD_ZERO;
            g.p.n_taps = ph_n[ph];
            for (int t = 0; t < ph_n[ph]; ++t) {
                g.p.a_ptr[t] = x + (long)ph_d[ph][t][0] * Wi * ldx;
                g.p.a_ld[t] = ldx; g.p.a_ktiles[t] = (int)(ldx / 32); g.p.a_shift[t] = ph_d[ph][t][1];
            }
            g.p.w = up[d][ph].w; g.p.ldw = up[d][ph].ldw; g.p.bias = up[d][ph].b;
            g.p.c32 = phases + ph * c; g.p.ldc32 = 4 * c;
            g.p.act = KG_ACT_LRELU;
            if (g.run(st)) return 1;
        }
        hipLaunchKernelGGL(rv_interleave_kernel, dim3(cdiv((long)B * (2 * Hi + 2) * 2 * Wi * (c / 4), 256)), dim3(256), 0, st, phases, pk[l].p,
                           2L * c, c / 4, fr, l, B, Hi, Wi);
        SVC_CHECK_HIP(hipGetLastError());
        if (run_blocks(dec[d], pk[l].p, 2 * c, l, nullptr, 0, fr, B, H, &x, st)) return 1;
    }
    if (conv(cnn, x, ldl(0), cnn_out, 4, 0, 9, nullptr, 0, KG_ACT_NONE, false, fr, B, H, st) || tm.mark(1, st)) return 1;
    {   // GRU input projection, all frames and both directions: rows 1 .. H of every clip, K = [bin][4]
        Gemm g((long)B * H, 6 * Hd, H);
        g.p.a_seq_rows = H + 2; g.p.a_off = 1; g.p.a_len = H;
        g.p.a_ptr[0] = cnn_out; g.p.a_ld[0] = 4L * W; g.p.a_ktiles[0] = 4 * W / 32;
        g.p.w = gru_in.w; g.p.ldw = gru_in.ldw; g.p.bias = gru_in.b;
        g.p.c32 = xp; g.p.ldc32 = 6 * Hd;
        if (g.run(st) || tm.mark(2, st)) return 1;
    }
    if (B >= 4) hipLaunchKernelGGL(rv_gru_kernel<4>, dim3(cdiv(B, 4), 2), dim3(Hd), 0, st, xp, w_hh4, b_hh, gru_out, fr, B, H, Hd);
    else if (B >= 2) hipLaunchKernelGGL(rv_gru_kernel<2>, dim3(cdiv(B, 2), 2), dim3(Hd), 0, st, xp, w_hh4, b_hh, gru_out, fr, B, H, Hd);
    else hipLaunchKernelGGL(rv_gru_kernel<1>, dim3(1, 2), dim3(Hd), 0, st, xp, w_hh4, b_hh, gru_out, fr, B, H, Hd);
    SVC_CHECK_HIP(hipGetLastError());
    if (tm.mark(3, st)) return 1;
    {   // fc.1 + sigmoid, cropped to the caller's T frames.  Rows [Tpad_b, T) of a shorter clip hold whatever an earlier call left in
        // gru_out (finite: the workspace starts as zero and only results are ever stored): a GEMM row depends on nothing but its
        // own input row, and rv_zero_rows_kernel overwrites every row at and above T_b, so none of it reaches a result
        Gemm g((long)B * T, cfg.n_bins, T);
        g.p.a_seq_rows = H; g.p.a_len = H;
        g.p.a_ptr[0] = gru_out; g.p.a_ld[0] = 2 * Hd; g.p.a_ktiles[0] = 2 * Hd / 32;
        g.p.w = fc.w; g.p.ldw = fc.ldw; g.p.bias = fc.b; g.p.act = KG_ACT_SIGMOID;
        g.p.c32 = out; g.p.ldc32 = cfg.n_bins;
        if (g.run(st)) return 1;
    }
    hipLaunchKernelGGL(rv_zero_rows_kernel, dim3(cdiv((long)B * T * cfg.n_bins, 256)), dim3(256), 0, st, out, fr, B, T, cfg.n_bins);
    SVC_CHECK_HIP(hipGetLastError());
    return tm.mark(4, st);
}

// clips in groups that keep one level-0 plane inside plane_budget; a row's bits do not depend on its group
int svc_rmvpe::salience(const float* mel, const int32_t* frame_lens, int B, int T, float* out, hipStream_t st) {
    int H = 0;
    for (int b = 0; b < B; ++b) H = std::max(H, (frame_lens[b] + RV_TMULT - 1) / RV_TMULT * RV_TMULT);
    const int G = group_size(B, H);
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = std::min(G, B - b0);
        Rows fr;
        memset(&fr, 0, sizeof(fr));
        for (int b = 0; b < nb; ++b) fr.n[b] = frame_lens[b0 + b];
        if (salience_group(mel + (long)b0 * cfg.n_mels * T, T, fr, nb, T, out + (long)b0 * T * cfg.n_bins, st)) return 1;
    }
    return 0;
}

// wave [B][L] -> out [B][n_mels][frames(L)]; lens: samples per clip
int svc_rmvpe::mel(const float* wave, const Rows& lens, int B, int L, float* out, hipStream_t st) {
    const int frames = 1 + L / RV_HOP, W = cfg.n_mels;
    const long rows = (long)B * frames, stride = round_up((long)L + 2 * RV_PAD + RV_NFFT, RV_HOP);
    const long ld_s = round_up(2 * RV_NB, 8), ld_c = round_up(W, 32);
    if (rows > mel_cap_rows || stride > mel_cap_stride || B > mel_cap_B) {
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        mws.release();
        mel_cap_rows = std::max(rows, mel_cap_rows); mel_cap_stride = std::max(stride, mel_cap_stride); mel_cap_B = std::max(B, mel_cap_B);
        padded = mws.alloc_n<float>((size_t)mel_cap_B * mel_cap_stride + RV_NFFT, st);
        spec = mws.alloc_n<float>((size_t)mel_cap_rows * ld_s, st);
        mag = mws.alloc_n<float>((size_t)mel_cap_rows * ld_fb, st);
        melc = mws.alloc_n<float>((size_t)mel_cap_rows * ld_c, st);
        if (!padded || !spec || !mag || !melc) { mel_cap_rows = mel_cap_stride = 0; mel_cap_B = 0; return 1; }
    }
    hipLaunchKernelGGL(rv_pad_kernel, dim3(cdiv(stride, 256), B), dim3(256), 0, st, wave, lens, L, padded, stride);
    SVC_CHECK_HIP(hipGetLastError());
    {   // STFT: rows = frames, overlapping in memory (row stride = hop), K = n_fft
        Gemm g(rows, 2 * RV_NB, frames);
        g.p.a_seq_rows = (int)(stride / RV_HOP); g.p.a_len = g.p.a_seq_rows;
        g.p.a_ptr[0] = padded; g.p.a_ld[0] = RV_HOP; g.p.a_ktiles[0] = RV_NFFT / 32;
        g.p.w = dft; g.p.ldw = RV_NFFT;
        g.p.c32 = spec; g.p.ldc32 = ld_s; g.p.vec_ok = 1;    // pad columns (zero weight rows) land in the ld padding
        if (kgemm_launch(g.p, 1, KG_EPI_STORE, st)) return 1;
    }
    hipLaunchKernelGGL(rv_mag_kernel, dim3(rows, cdiv(ld_fb, 128)), dim3(128), 0, st, spec, ld_s, mag, ld_fb, RV_NB);
    SVC_CHECK_HIP(hipGetLastError());
    {
        Gemm g(rows, W, frames);
        g.p.a_ptr[0] = mag; g.p.a_ld[0] = ld_fb; g.p.a_ktiles[0] = (int)(ld_fb / 32);
        g.p.w = fb; g.p.ldw = ld_fb;
        g.p.c32 = melc; g.p.ldc32 = ld_c; g.p.vec_ok = 1;
        if (kgemm_launch(g.p, 1, KG_EPI_STORE, st)) return 1;
    }
    hipLaunchKernelGGL(rv_mellog_kernel, dim3(cdiv(frames, 128), W, B), dim3(128), 0, st, melc, ld_c, out, lens, W, frames);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

namespace {
// host checks of a ragged audio batch; every message names the offending argument
int rv_check_wave(const char* fn, const void* wave, const int32_t* lens, int B, int L, bool lens_required) {
    const std::string f(fn);
    if (lens_required && !lens) { set_error(f + ": lens is NULL"); return 1; }
    if (B < 1 || B > RV_MAX_B) { set_error(f + ": B must be 1 .. 64 clips"); return 1; }
    if (L < RV_PAD + 1) { set_error(f + ": L is below svc_rmvpe_min_len() = n_fft / 2 + 1 samples"); return 1; }
    if (lens)
        for (int b = 0; b < B; ++b)
            if (lens[b] < RV_PAD + 1 || lens[b] > L) { set_error(f + ": lens outside [svc_rmvpe_min_len(), L]"); return 1; }
    if (!wave) { set_error(f + ": wave is NULL"); return 1; }
    return 0;
}
int rv_check_frames(const char* fn, const int32_t* frame_lens, int B, int T) {
    const std::string f(fn);
    if (!frame_lens) { set_error(f + ": frame_lens is NULL"); return 1; }
    if (B < 1 || B > RV_MAX_B) { set_error(f + ": B must be 1 .. 64 clips"); return 1; }
    if (T < 1) { set_error(f + ": T must be at least 1 frame"); return 1; }
    for (int b = 0; b < B; ++b)
        if (frame_lens[b] < 1 || frame_lens[b] > T) { set_error(f + ": frame_lens outside [1, T]"); return 1; }
    return 0;
}
}  // namespace

extern "C" {

int svc_rmvpe_create(const svc_rmvpe_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, const float* mel_basis, void* stream,
                     svc_rmvpe_t** out) {
    SVC_REQUIRE(cfg && weights && mel_basis && out, "svc_rmvpe_create: null argument");
    SVC_REQUIRE(cfg->en_de_layers >= 1 && cfg->en_de_layers <= RV_MAX_LEVELS && cfg->inter_layers >= 1 && cfg->n_blocks >= 1,
                "svc_rmvpe_create: en_de_layers 1 .. 5, at least one intermediate layer and one block");
    SVC_REQUIRE(cfg->en_out_channels == 16 || (cfg->en_out_channels > 0 && cfg->en_out_channels % 32 == 0),
                "svc_rmvpe_create: en_out_channels 16 or a multiple of 32");
    SVC_REQUIRE(cfg->n_mels >= 8 && cfg->n_mels % 8 == 0 && cfg->n_mels % (1 << cfg->en_de_layers) == 0,
                "svc_rmvpe_create: n_mels a multiple of 8 and of 2^en_de_layers");
    SVC_REQUIRE(cfg->gru_hidden >= 64 && cfg->gru_hidden <= 256 && cfg->gru_hidden % 64 == 0, "svc_rmvpe_create: gru_hidden 64 | 128 | 192 | 256");
    SVC_REQUIRE(cfg->n_bins >= 9, "svc_rmvpe_create: n_bins");
    auto* m = new svc_rmvpe();
    m->cfg = *cfg;
    StateDict sd(weights, n_weights);
    if (m->pack(sd, mel_basis, (hipStream_t)stream)) { delete m; return 1; }
    *out = m;
    return 0;
}

void svc_rmvpe_destroy(svc_rmvpe_t* m) { delete m; }

int svc_rmvpe_frames(int n_samples) { return n_samples >= 0 ? 1 + n_samples / RV_HOP : 0; }
int svc_rmvpe_min_len(void) { return RV_PAD + 1; }

int svc_rmvpe_set_plane_budget(svc_rmvpe_t* m, long long bytes) {
    SVC_REQUIRE(m && bytes >= 0, "svc_rmvpe_set_plane_budget: bad argument");
    m->plane_budget = bytes ? (long)bytes : 256L << 20;
    return 0;
}

int svc_rmvpe_set_timing(svc_rmvpe_t* m, int on) {
    SVC_REQUIRE(m, "svc_rmvpe_set_timing: null handle");
    m->tm.on = on != 0;
    return 0;
}

int svc_rmvpe_last_timing(svc_rmvpe_t* m, float* ms4) {
    const char* msg = "svc_rmvpe_last_timing: timing is off or no call was made";
    SVC_REQUIRE(m, msg);
    return m->tm.last(ms4, msg);
}

int svc_rmvpe_mel(svc_rmvpe_t* m, const float* wave, const int32_t* lens, int B, int L, float* mel_out, void* stream) {
    if (rv_check_wave("svc_rmvpe_mel", wave, lens, B, L, true)) return 1;
    SVC_REQUIRE(m && mel_out, "svc_rmvpe_mel: null handle or output");
    Rows r;
    memset(&r, 0, sizeof(r));
    for (int b = 0; b < B; ++b) r.n[b] = lens[b];
    return m->mel(wave, r, B, L, mel_out, (hipStream_t)stream);
}

int svc_rmvpe_salience(svc_rmvpe_t* m, const float* mel, const int32_t* frame_lens, int B, int T, float* out, void* stream) {
    if (rv_check_frames("svc_rmvpe_salience", frame_lens, B, T)) return 1;
    SVC_REQUIRE(m && mel && out, "svc_rmvpe_salience: null handle, mel or output");
    return m->salience(mel, frame_lens, B, T, out, (hipStream_t)stream);
}

int svc_rmvpe_decode(const float* salience, const int32_t* frame_lens, int B, int T, float thred, float* f0_out, void* stream) {
    if (rv_check_frames("svc_rmvpe_decode", frame_lens, B, T)) return 1;
    SVC_REQUIRE(salience && f0_out, "svc_rmvpe_decode: null salience or output");
    const int n_bins = 360;
    Rows r;
    memset(&r, 0, sizeof(r));
    for (int b = 0; b < B; ++b) r.n[b] = frame_lens[b];
    hipLaunchKernelGGL(rv_decode_kernel, dim3(cdiv((long)B * T, 4)), dim3(256), 0, (hipStream_t)stream, salience, r, B, T, n_bins, thred, f0_out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int svc_rmvpe_f0(svc_rmvpe_t* m, const float* wave, const int32_t* lens, int B, int L, float thred, float* f0_out, void* stream) {
    if (rv_check_wave("svc_rmvpe_f0", wave, lens, B, L, false)) return 1;
    SVC_REQUIRE(m && f0_out, "svc_rmvpe_f0: null handle or output");
    hipStream_t st = (hipStream_t)stream;
    const int T = svc_rmvpe_frames(L), W = m->cfg.n_mels, nbins = m->cfg.n_bins;
    int32_t fl[RV_MAX_B];
    int H = 0;
    for (int b = 0; b < B; ++b) {
        fl[b] = svc_rmvpe_frames(lens ? lens[b] : L);
        H = std::max(H, (fl[b] + RV_TMULT - 1) / RV_TMULT * RV_TMULT);
    }
    const int G = m->group_size(B, H);
    const long need = (long)G * T;
    if (need > m->f0_cap) {
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        m->tmp.release();
        m->f0_cap = 0;
        m->f0_mel = m->tmp.alloc_n<float>((size_t)need * W, st);
        m->f0_sal = m->tmp.alloc_n<float>((size_t)need * nbins, st);
        if (!m->f0_mel || !m->f0_sal) return 1;
        m->f0_cap = need;
    }
    for (int b0 = 0; b0 < B; b0 += G) {                      // the whole path group by group: scratch stays inside the budget
        const int nb = std::min(G, B - b0);
        Rows sm, fr;
        memset(&sm, 0, sizeof(sm));
        memset(&fr, 0, sizeof(fr));
        for (int b = 0; b < nb; ++b) { sm.n[b] = lens ? lens[b0 + b] : L; fr.n[b] = fl[b0 + b]; }
        if (m->mel(wave + (long)b0 * L, sm, nb, L, m->f0_mel, st)) return 1;
        if (m->salience_group(m->f0_mel, T, fr, nb, T, m->f0_sal, st)) return 1;
        hipLaunchKernelGGL(rv_decode_kernel, dim3(cdiv((long)nb * T, 4)), dim3(256), 0, st, m->f0_sal, fr, nb, T, nbins, thred,
                           f0_out + (long)b0 * T);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

int svc_f0_adjust(const float* f0_alt, const int32_t* alt_lens, const float* f0_ori, const int32_t* ori_lens, int B, int Talt, int Tori,
                  int auto_adjust, const float* semitones, float* out, float* medians, void* stream) {
    SVC_REQUIRE(alt_lens != nullptr, "svc_f0_adjust: alt_lens is NULL");
    SVC_REQUIRE(ori_lens != nullptr, "svc_f0_adjust: ori_lens is NULL");
    SVC_REQUIRE(B >= 1 && B <= RV_MAX_B, "svc_f0_adjust: B must be 1 .. 64 rows");
    SVC_REQUIRE(Talt >= 1 && Tori >= 1, "svc_f0_adjust: Talt and Tori must be at least 1");
    Rows a, o;
    RowsF s;
    memset(&a, 0, sizeof(a)); memset(&o, 0, sizeof(o)); memset(&s, 0, sizeof(s));
    for (int b = 0; b < B; ++b) {
        SVC_REQUIRE(alt_lens[b] >= 0 && alt_lens[b] <= Talt, "svc_f0_adjust: alt_lens outside [0, Talt]");
        SVC_REQUIRE(ori_lens[b] >= 0 && ori_lens[b] <= Tori, "svc_f0_adjust: ori_lens outside [0, Tori]");
        a.n[b] = alt_lens[b]; o.n[b] = ori_lens[b];
        s.v[b] = semitones ? semitones[b] : 0.f;
    }
    SVC_REQUIRE(f0_alt && f0_ori && out, "svc_f0_adjust: null f0_alt, f0_ori or out");
    hipLaunchKernelGGL(f0_adjust_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, f0_alt, a, f0_ori, o, Talt, Tori, auto_adjust, s, out,
                       medians);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
