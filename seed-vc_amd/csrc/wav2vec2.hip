// wav2vec 2.0 content encoder for gfx950 (XLS-R-300m / HuBERT-large family: layer-norm feature extractor, "stable layer norm"
// transformer, grouped positional conv): 16 kHz audio -> content features at 50 rows/s (`semantic_fn` of the reference drivers for
// the xlsr models: Wav2Vec2FeatureExtractor + the first layers of facebook/wav2vec2-xls-r-300m in float16).
//
// Stages.  Normalisation: per window (x - mean) / sqrt(var + 1e-7), mean first, then the variance about it, both from 64 block
// partials folded in a fixed order (double accumulation, no atomics).  Extractor: conv0 (1 -> C) fused with its LayerNorm and
// erf-GELU in one row kernel (one wave per output row, the raw 3200 rows/s x C plane is never written), convs 1..n-1 as 2- and
// 3-tap tap-GEMMs on channels-last rows (stride in the row map, no padding) each followed by the LayerNorm+GELU row kernel, the
// last of which also applies the feature projection's LayerNorm; then Linear C -> D.  Positional conv: a grouped Conv1d of k taps
// as a Toeplitz product per (group, 64-position tile, window), input rows resident in LDS (w2v_posconv_kernel); precision 0 runs
// it on the fp32 tap-GEMM, one accumulating launch per group and 48 taps.  Encoder: pre-LN blocks on the tap-GEMM and the
// attention kernel with per-window key counts, then encoder.layer_norm.  Residual stream, LayerNorm statistics and softmax are
// fp32.  Windows of long clips travel as a table in kernel arguments, exactly as in whisper.hip; every window is computed as if
// alone (row-local kernels, per-element k order in the GEMMs, tile-independent tap order in the positional conv, pinned attention
// form), so its bits do not depend on its companions, their order or the group size.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "model_util.h"

using namespace svc;

namespace {

constexpr int WV_MAX_WIN = 64, WV_MAX_B = 64, WV_NBLK = 64, WV_DEFAULT_GROUP = 16, WV_MAX_CONV = 8, WV_SPR = 320;
constexpr int WV_PC_BM = 64, WV_PC_MAXK = 128, WV_PC_AHEAD = 4;    // positional conv: positions per workgroup, most taps, taps of weights in flight
constexpr float WV_QSCALE = 0.125f * 1.4426950408889634f;     // 1 / sqrt(64), and the attention kernel's exp2

struct WinTab {                                   // one group of windows as a kernel argument
    int clip[WV_MAX_WIN], start[WV_MAX_WIN], n[WV_MAX_WIN];           // source clip, first sample, samples
    int dst0[WV_MAX_WIN], drop[WV_MAX_WIN], keep[WV_MAX_WIN];         // assemble: rows [drop, keep) go to out[clip][dst0 ...]
    int zero_from[WV_MAX_WIN];                                        // last window of its clip: the clip's row count; else -1
};
struct LenTab { int v[WV_MAX_CONV + 1][WV_MAX_WIN]; };                // samples, then rows after each conv, per window

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void wv_lens_kernel(LenTab lt, int* __restrict__ dst, int n_rows) {
    const int i = threadIdx.x;
    if (i < WV_MAX_WIN)
        for (int r = 0; r < n_rows; ++r) dst[r * WV_MAX_WIN + i] = lt.v[r][i];
}

// part[g][blk] = sum over the block's share of window g of (x - sub)^POW, sub = 0 (POW 1) or the window's mean (POW 2): the
// share depends on the window's own length only, the 64 partials are folded in index order once per consuming block
__device__ __forceinline__ double wv_fold(const double* part) {
    double s = 0.0;
    for (int i = 0; i < WV_NBLK; ++i) s += part[i];
    return s;
}
template <int POW>
__global__ __launch_bounds__(256) void wv_stat_kernel(const float* __restrict__ wave, WinTab wt, long Lrow, const double* __restrict__ sums,
                                                      double* __restrict__ part) {
    __shared__ double red[4];
    const int g = blockIdx.y, blk = blockIdx.x, n = wt.n[g];
    const float* x = wave + (long)wt.clip[g] * Lrow + wt.start[g];
    const int per = (n + WV_NBLK - 1) / WV_NBLK, i0 = blk * per, i1 = min(n, i0 + per);
    if (POW == 2 && threadIdx.x == 0) red[0] = wv_fold(sums + g * WV_NBLK) / (double)n;      // folded once per block, in index order
    __syncthreads();
    const double mean = POW == 2 ? red[0] : 0.0;
    __syncthreads();
    double s = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) {
        const double d = (double)x[i] - mean;
        s += POW == 2 ? d * d : d;
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[g * WV_NBLK + blk] = (red[0] + red[1]) + (red[2] + red[3]);
}
// dst[g][i] = (x - mean) / sqrt(var + 1e-7), i < n; nothing at or above n is read or written
__global__ void wv_norm_kernel(const float* __restrict__ wave, WinTab wt, long Lrow, const double* __restrict__ sums, const double* __restrict__ sq,
                               float* __restrict__ dst, long stride) {
    __shared__ double mr[2];
    const int g = blockIdx.y, n = wt.n[g];
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if ((long)blockIdx.x * blockDim.x >= n) return;          // uniform over the block
    if (threadIdx.x < 2) mr[threadIdx.x] = wv_fold((threadIdx.x ? sq : sums) + g * WV_NBLK) / (double)n;   // once per block, in index order
    __syncthreads();
    if (i >= n) return;
    const double mean = mr[0], var = mr[1];
    const float rstd = (float)(1.0 / sqrt(var + 1e-7));
    dst[(long)g * stride + i] = (float)((double)wave[(long)wt.clip[g] * Lrow + wt.start[g] + i] - mean) * rstd;
}

// LayerNorm statistics of a row held by one wave (v[i] = channel lane + 64 i): mean, then the variance about it
template <int NMAX>
__device__ __forceinline__ void wv_row_norm(float (&v)[NMAX], int n, int D, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                            int lane, bool gelu) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) s += v[i];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) { const float d = v[i] - mean; q = fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) {
            const int c = lane + 64 * i;
            const float o = (v[i] - mean) * rstd * gamma[c] + beta[c];
            v[i] = gelu ? gelu_erf(o) : o;
        }
}

// Row kernel of the extractor and the encoder, one wave per row.  MODE 0: LayerNorm; 1: LayerNorm, erf-GELU; 2: LayerNorm, erf-GELU,
// then a second LayerNorm (gamma2, beta2: the feature projection's).  Rows at and above lens[seq] (seq = row / seq_rows) are
// neither read nor written; lens may be null.
template <int MODE>
__global__ __launch_bounds__(256) void wv_rownorm_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y32, half_t* __restrict__ y16,
                                                         long ldy, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ gamma2, const float* __restrict__ beta2, long rows, int D,
                                                         float eps, const int* __restrict__ lens, int seq_rows) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, n = D / 64;
    if (row >= rows) return;
    if (lens && (int)(row % seq_rows) >= lens[row / seq_rows]) return;
    const float* xr = x + row * ldx;
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) v[i] = xr[lane + 64 * i];
    wv_row_norm<32>(v, n, D, eps, gamma, beta, lane, MODE >= 1);
    if (MODE == 2) wv_row_norm<32>(v, n, D, eps, gamma2, beta2, lane, false);
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) {
            const int c = lane + 64 * i;
            if (y32) y32[row * ldy + c] = v[i];
            if (y16) y16[row * ldy + c] = (half_t)v[i];
        }
}

// conv0 (1 -> C channels, k0 taps, stride s0, bias) + LayerNorm(C) + erf-GELU: one wave per output row, weights [k0][C] in LDS
__global__ __launch_bounds__(256) void wv_conv0_kernel(const float* __restrict__ wn, long stride, const float* __restrict__ w /*[k0][C]*/,
                                                       const float* __restrict__ bias, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ y32, half_t* __restrict__ y16, int C, int k0, int s0, int L0,
                                                       const int* __restrict__ lens0, float eps) {
    extern __shared__ float w_s[];
    const int g = blockIdx.y, lane = threadIdx.x & 63, n = C / 64, len = lens0[g];
    for (int i = threadIdx.x; i < k0 * C; i += 256) w_s[i] = w[i];
    __syncthreads();
    const float* xg = wn + (long)g * stride;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < len; row += gridDim.x * 4) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < n) v[i] = bias[lane + 64 * i];
        for (int t = 0; t < k0; ++t) {
            const float xv = xg[(long)row * s0 + t];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < n) v[i] = fmaf(xv, w_s[t * C + lane + 64 * i], v[i]);
        }
        wv_row_norm<8>(v, n, C, eps, gamma, beta, lane, true);
        const long o = ((long)g * L0 + row) * C;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < n) {
                if (y32) y32[o + lane + 64 * i] = v[i];
                if (y16) y16[o + lane + 64 * i] = (half_t)v[i];
            }
    }
}

// ---- positional conv, fp16 operands: out = x32 + gelu(conv(x16) + bias) on channels-last rows [G][P][D], groups of 64 channels.
// Workgroup = (group, tile of 64 positions, window), group-major so that a group's 2 k 64 64 weight bytes stay in L2 across its
// tiles.  The 64 + k - 1 input rows of the group's channel slice (128 bytes each) are loaded into LDS once, rows below 0 and at or
// above the window's own T as zeros (never loaded); 16-byte chunks XOR-swizzled by the row so that the 16 consecutive rows of an
// MFMA A fragment read conflict-free.  Wave w owns output channels 16 w .. 16 w + 15 of the group for all 64 positions (4
// accumulator tiles): the waves share the rows in LDS, and no two waves need the same weights, so the pre-packed weight fragments
// (1 KiB per (tap, k-step, wave), lane order) go straight from L2 to registers, four taps ahead, with no LDS ring.  Every output element
// accumulates (tap 0 .. k-1) x (channels 0..31, 32..63) in that order in fp32, whatever T, the batch or the tile.
__device__ __forceinline__ int wv_pc_swz(int row) { return (row >> 1) & 7; }

__global__ __launch_bounds__(256) void w2v_posconv_kernel(const half_t* __restrict__ x16, const float* __restrict__ x32, const half_t* __restrict__ wp,
                                                          const float* __restrict__ bias, float* __restrict__ out, const int* __restrict__ lens,
                                                          int P, int D, int k, int n_win, int n_tiles) {
    __shared__ __attribute__((aligned(16))) char rows_s[(WV_PC_BM + WV_PC_MAXK - 1) * 128];
    const int tile = blockIdx.x % n_tiles, win = (blockIdx.x / n_tiles) % n_win, grp = blockIdx.x / (n_tiles * n_win);
    const int T = lens[win], p0 = tile * WV_PC_BM;
    if (p0 >= T) return;                                    // uniform over the workgroup, before any barrier
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    const int R = WV_PC_BM + k - 1, half = k / 2;
    const half_t* xg = x16 + (long)win * P * D + grp * 64;
    for (int idx = tid; idx < R * 8; idx += 256) {
        const int r = idx >> 3, c = idx & 7, q = p0 + r - half;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q >= 0 && q < T) v = *reinterpret_cast<const uint4*>(xg + (long)q * D + c * 8);
        *reinterpret_cast<uint4*>(rows_s + r * 128 + ((c ^ wv_pc_swz(r)) << 4)) = v;
    }
    __syncthreads();
    float4v acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (float4v){0.f, 0.f, 0.f, 0.f};
    // fragment (tap t, k-step ks, wave w): wp[(((grp k + t) 2 + ks) 4 + w) 64 + lane] (16 bytes)
    const uint4* wf = reinterpret_cast<const uint4*>(wp) + ((long)grp * k * 8 + wave) * 64 + lane;
    // the weights of the next WV_PC_AHEAD taps are in flight under the MFMAs of a tap (a tap's 8 MFMAs are shorter than an L2 round trip)
    uint4 wb[WV_PC_AHEAD][2];
#pragma unroll
    for (int u = 0; u < WV_PC_AHEAD; ++u)
        if (u < k) { wb[u][0] = wf[(long)u * 8 * 64]; wb[u][1] = wf[(long)u * 8 * 64 + 4 * 64]; }
    for (int t0 = 0; t0 < k; t0 += WV_PC_AHEAD) {
#pragma unroll
        for (int u = 0; u < WV_PC_AHEAD; ++u) {
            const int t = t0 + u;
            if (t >= k) break;
            const uint4 c0 = wb[u][0], c1 = wb[u][1];
            if (t + WV_PC_AHEAD < k) { wb[u][0] = wf[(long)(t + WV_PC_AHEAD) * 8 * 64]; wb[u][1] = wf[(long)(t + WV_PC_AHEAD) * 8 * 64 + 4 * 64]; }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = mt * 16 + fr + t;
                const char* rp = rows_s + row * 128;
                const int sw = wv_pc_swz(row);
                const uint4 a0 = *reinterpret_cast<const uint4*>(rp + ((fq ^ sw) << 4));
                const uint4 a1 = *reinterpret_cast<const uint4*>(rp + (((4 + fq) ^ sw) << 4));
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a0), __builtin_bit_cast(half8, c0), acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a1), __builtin_bit_cast(half8, c1), acc[mt], 0, 0, 0);
            }
        }
    }
    // acc[mt][r] = C[position p0 + 16 mt + 4 fq + r][channel 16 wave + fr]
    const int nch = grp * 64 + wave * 16 + fr;
    const float bv = bias[nch];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = p0 + mt * 16 + fq * 4 + r;
            if (p < T) {
                const long o = ((long)win * P + p) * D + nch;
                out[o] = x32[o] + gelu_erf(acc[mt][r] + bv);
            }
        }
}

// precision 0: out = x + gelu(acc + bias) over the valid rows (acc from the accumulating fp32 tap-GEMM launches)
__global__ void wv_posadd_kernel(const float* __restrict__ x, const float* __restrict__ acc, const float* __restrict__ bias, float* __restrict__ out,
                                 const int* __restrict__ lens, int P, int D) {
    const int win = blockIdx.y, p = blockIdx.x;
    if (p >= lens[win]) return;
    const long o = ((long)win * P + p) * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) out[o + c] = x[o + c] + gelu_erf(acc[o + c] + bias[c]);
}

// per-tap scale of the weight-normed positional conv: sc[t] = g[t] / || v[:, :, t] ||  (norm over dims 0 and 1; one block per tap)
__global__ __launch_bounds__(256) void wv_wn_scale_kernel(const float* __restrict__ g, const float* __restrict__ v, long n01, int k, float* __restrict__ sc) {
    __shared__ double red[4];
    const int t = blockIdx.x;
    double s = 0.0;
    for (long i = threadIdx.x; i < n01; i += 256) { const double a = v[i * k + t]; s += a * a; }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sc[t] = (float)((double)g[t] / sqrt((red[0] + red[1]) + (red[2] + red[3])));
}
// v [D][64][k] (x sc[t], or as it is when sc is null) -> the fp16 fragment stream of w2v_posconv_kernel and / or the fp32 tap-GEMM
// rows w32[(grp 64 + n)][t 64 + c]
__global__ void wv_pack_pos_kernel(const float* __restrict__ v, const float* __restrict__ sc, int D, int k, half_t* __restrict__ wp, float* __restrict__ w32) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)D * 64 * k) return;
    const int t = (int)(i % k), c = (int)((i / k) % 64), no = (int)(i / ((long)k * 64));
    const float val = v[i] * (sc ? sc[t] : 1.f);
    const int grp = no / 64, n = no % 64;
    if (wp) {
        const int w = n >> 4, fr = n & 15, ks = c >> 5, fq = (c & 31) >> 3, j = c & 7;
        wp[((((long)(grp * k + t) * 2 + ks) * 4 + w) * 64 + fq * 16 + fr) * 8 + j] = (half_t)val;
    }
    if (w32) w32[((long)no * k + t) * 64 + c] = val;
}

// V columns of qkv [G * P][3 D] (fp16) -> vt [G][D][vt_ld] in the attention's column order; columns at and above the window's rows are zero
__global__ __launch_bounds__(256) void wv_vt_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ vt, const int* __restrict__ lens, int P, int D,
                                                    long vt_ld, int mode) {
    __shared__ half_t tile[32][34];
    const int g = blockIdx.z, p0 = blockIdx.x * 32, d0 = blockIdx.y * 32, T = lens[g];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i;
        tile[i][tx] = p < T ? qkv[((long)g * P + p) * 3 * D + 2 * D + d0 + tx] : (half_t)0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + tx;
        if (p < vt_ld) vt[((long)g * D + d0 + i) * vt_ld + vt_pos(p, mode)] = tile[tx][i];
    }
}

// src [G][P][D] rows below lens[g] -> dst [G][T][D]; the other rows of dst are not touched
__global__ void wv_copy_rows_kernel(const float* __restrict__ src, int P, float* __restrict__ dst, int T, const int* __restrict__ lens, int D) {
    const int g = blockIdx.y, r = blockIdx.x;
    if (r >= lens[g]) return;
    const float4* s = reinterpret_cast<const float4*>(src + ((long)g * P + r) * D);
    float4* d = reinterpret_cast<float4*>(dst + ((long)g * T + r) * D);
    for (int i = threadIdx.x; i < D / 4; i += blockDim.x) d[i] = s[i];
}

// enc [G][P][D] -> out [B][Rmax][D]: block (r, g).  r < P: row r of window g, when kept, goes to its place in the clip's rows;
// r >= P: row r - P of the clip is zeroed when window g is the clip's last and the row is at or above the clip's count
__global__ void wv_assemble_kernel(const float* __restrict__ enc, WinTab wt, float* __restrict__ out, int P, int D, int Rmax) {
    const int g = blockIdx.y, r = blockIdx.x;
    float4* dst = nullptr;
    const float4* src = nullptr;
    if (r < P) {
        if (r < wt.drop[g] || r >= wt.keep[g]) return;
        dst = reinterpret_cast<float4*>(out + ((long)wt.clip[g] * Rmax + wt.dst0[g] + r - wt.drop[g]) * D);
        src = reinterpret_cast<const float4*>(enc + ((long)g * P + r) * D);
    } else {
        const int z = r - P;
        if (wt.zero_from[g] < 0 || z < wt.zero_from[g]) return;
        dst = reinterpret_cast<float4*>(out + ((long)wt.clip[g] * Rmax + z) * D);
    }
    for (int i = threadIdx.x; i < D / 4; i += blockDim.x) dst[i] = src ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

KGemmParams wv_gemm(long M, int N, int Lout) {
    KGemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = (int)M; p.N = N; p.Lout = Lout; p.a_seq_rows = Lout; p.c_seq_rows = Lout; p.a_stride = 1; p.a_len = Lout; p.n_taps = 1;
    p.vec_ok = 1;
    return p;
}

long wv_n_windows(long W, long O, long n) { return n <= W ? 1 : 1 + (n - W + (W - O) - 1) / (W - O); }

long wv_frames(const svc_w2v_config_t& c, long n, int upto = WV_MAX_CONV) {
    for (int l = 0; l < c.n_conv && l < upto; ++l) n = n >= c.conv_kernel[l] ? (n - c.conv_kernel[l]) / c.conv_stride[l] + 1 : 0;
    return n;
}

int wv_check_cfg(const svc_w2v_config_t* c, const char* who) {
    auto bad = [&](const char* msg) { set_error(std::string(who) + ": " + msg); return 1; };
    if (!c) return bad("null config");
    if (c->n_conv < 2 || c->n_conv > WV_MAX_CONV) return bad("n_conv must be 2 .. 8");
    for (int l = 0; l < c->n_conv; ++l)
        if (c->conv_kernel[l] < 1 || c->conv_stride[l] < 1 || c->conv_kernel[l] > (l ? 8 : 64)) return bad("conv_kernel / conv_stride out of range");
    long hop = 1;
    for (int l = 0; l < c->n_conv; ++l) hop *= c->conv_stride[l];
    if (hop != WV_SPR) return bad("the conv strides must multiply to 320 samples per row (the drivers' window plan counts rows of 320 samples)");
    if ((long)c->conv_kernel[0] * c->conv_dim > 8192) return bad("conv_kernel[0] * conv_dim must not exceed 8192 (conv0 keeps its weights in 32 KB of LDS)");
    if (c->window_samples < WV_SPR || c->window_samples % WV_SPR) return bad("window_samples must be a positive multiple of 320");
    if (wv_frames(*c, c->window_samples) < 1) return bad("window_samples is shorter than the extractor's receptive field");
    return 0;
}

}  // namespace

struct svc_w2v {
    svc_w2v_config_t cfg;
    int dt = 0;                      // tap-GEMM dtype of the convs and linears: 0 fp16 (precision 1), 1 fp32 (precision 0)
    int group = WV_DEFAULT_GROUP, qt_form = 1;
    Arena wts, ws_fe, ws_enc;
    struct Lin { void* w = nullptr; float* b = nullptr; long ldw = 0; int N = 0; };
    struct Layer { Lin qkv, o, fc1, fc2; float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; };
    float* w0 = nullptr; float* b0 = nullptr;                           // conv0 [k0][C], bias
    Lin conv[WV_MAX_CONV], proj;
    float *cg[WV_MAX_CONV] = {}, *cb[WV_MAX_CONV] = {}, *pg = nullptr, *pb = nullptr, *gf = nullptr, *bf = nullptr;
    half_t* pos16 = nullptr; float* pos32 = nullptr; float* posb = nullptr;
    std::vector<Layer> layers;
    // extractor workspace for cap_g windows of cap_n samples; encoder workspace for ecap_g windows of ecap_p rows
    int cap_g = 0; long cap_n = 0; int ecap_g = 0, ecap_p = 0;
    int Ls[WV_MAX_CONV + 1] = {};    // row strides of the stage buffers of the current call (its longest window)
    long nstride = 0;
    float* wn = nullptr; double* part = nullptr; int* dlens = nullptr;
    void *actA = nullptr, *actB = nullptr; float* raw = nullptr;
    float *h32 = nullptr, *x = nullptr, *n32 = nullptr, *ao32 = nullptr, *ff32 = nullptr, *enc = nullptr, *acc32 = nullptr;
    half_t *h16 = nullptr, *n16 = nullptr, *qkv16 = nullptr, *vt = nullptr, *ao16 = nullptr, *ff16 = nullptr;
    long vt_ld = 0;
    bool timing = false;
    hipEvent_t ev[5] = {};
    ~svc_w2v() {
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    }
    int mark(int i, hipStream_t st) {
        if (!timing) return 0;
        if (!ev[i]) SVC_CHECK_HIP(hipEventCreate(&ev[i]));
        SVC_CHECK_HIP(hipEventRecord(ev[i], st));
        return 0;
    }
    int pack_lin(const float* w, const float* bias, int N, int K, const float* scale, Lin* out, hipStream_t st);
    int pack(const StateDict& sd, const std::string& pre, hipStream_t st);
    int reserve_fe(int G, long nmax, hipStream_t st);
    int reserve_enc(int G, int P, hipStream_t st);
    int put_lens(const LenTab& lt, hipStream_t st);
    int lin(const Lin& l, const void* a, long K, long M, int Lout, int act, const float* res, float* c32, half_t* c16, hipStream_t st);
    int rownorm(int mode, const float* x, long ldx, float* y32, half_t* y16, long ldy, const float* g, const float* b, const float* g2, const float* b2,
                long rows, int D, const int* lens, int seq_rows, hipStream_t st);
    int normalize_group(const float* wave, long Lrow, const WinTab& wt, int G, float* dst, long stride, hipStream_t st);
    int features_group(const float* wnorm, long stride, int G, hipStream_t st);            // -> h32 (+ h16) [G][Ls[n_conv]][D]
    int posconv_group(const float* h, const half_t* h16v, int G, int P, float* out, hipStream_t st);
    int encode_group(const float* h, const half_t* h16v, int G, int P, float* out, hipStream_t st);
};

namespace {

float* wv_copy(const float* src, long n, Arena& ar, hipStream_t st) {
    float* p = ar.alloc_n<float>(round_up(n, 8), st);
    if (!p) return nullptr;
    if (hipMemcpyAsync(p, src, (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("weight copy failed"); return nullptr; }
    return p;
}

int wv_require(const svc_tensor_desc_t* d, const std::string& name, const std::vector<long>& shp) {
    if (!d) { set_error("svc_w2v_create: state_dict is missing " + name); return 1; }
    bool ok = d->ndim == (int)shp.size();
    for (size_t i = 0; ok && i < shp.size(); ++i) ok = d->shape[i] == shp[i];
    if (!ok) { set_error("svc_w2v_create: shape mismatch for " + name); return 1; }
    return 0;
}

struct KeyShape { std::string name; std::vector<long> shape; };

std::vector<KeyShape> wv_keys(const svc_w2v_config_t& c) {
    const long D = c.d_model, F = c.ffn_dim, C = c.conv_dim;
    std::vector<KeyShape> k;
    for (int l = 0; l < c.n_conv; ++l) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(l) + ".";
        k.push_back({p + "conv.weight", {C, l ? C : 1, c.conv_kernel[l]}});
        k.push_back({p + "conv.bias", {C}});
        k.push_back({p + "layer_norm.weight", {C}});
        k.push_back({p + "layer_norm.bias", {C}});
    }
    k.push_back({"feature_projection.layer_norm.weight", {C}});
    k.push_back({"feature_projection.layer_norm.bias", {C}});
    k.push_back({"feature_projection.projection.weight", {D, C}});
    k.push_back({"feature_projection.projection.bias", {D}});
    k.push_back({"encoder.pos_conv_embed.conv.bias", {D}});
    k.push_back({"encoder.layer_norm.weight", {D}});
    k.push_back({"encoder.layer_norm.bias", {D}});
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string p = "encoder.layers." + std::to_string(i) + ".";
        for (const char* n : {"k_proj", "v_proj", "q_proj", "out_proj"}) {
            k.push_back({p + "attention." + n + ".weight", {D, D}});
            k.push_back({p + "attention." + n + ".bias", {D}});
        }
        k.push_back({p + "layer_norm.weight", {D}});
        k.push_back({p + "layer_norm.bias", {D}});
        k.push_back({p + "feed_forward.intermediate_dense.weight", {F, D}});
        k.push_back({p + "feed_forward.intermediate_dense.bias", {F}});
        k.push_back({p + "feed_forward.output_dense.weight", {D, F}});
        k.push_back({p + "feed_forward.output_dense.bias", {D}});
        k.push_back({p + "final_layer_norm.weight", {D}});
        k.push_back({p + "final_layer_norm.bias", {D}});
    }
    return k;
}

}  // namespace

// nn.Linear weight [N][K] -> [Npad128][K] in the GEMM's dtype, rows optionally scaled
int svc_w2v::pack_lin(const float* w, const float* bias, int N, int K, const float* scale, Lin* out, hipStream_t st) {
    out->N = N; out->ldw = K;
    out->w = wts.alloc((size_t)round_up(N, 128) * K * esize(dt), st);
    if (!out->w) return 1;
    if (pack_any(dt, w, out->w, 0, N, 1, K, K, 0, 1, K, 0, 1, scale, st)) return 1;
    if (bias && !(out->b = wv_copy(bias, N, wts, st))) return 1;
    return 0;
}

int svc_w2v::pack(const StateDict& sd, const std::string& pre, hipStream_t st) {
    const int D = cfg.d_model, F = cfg.ffn_dim, C = cfg.conv_dim, k = cfg.pos_k;
    auto get = [&](const std::string& key) { return sd.get(pre + key)->data; };       // every key was checked by the caller
    const std::string fe = "feature_extractor.conv_layers.";
    for (int l = 0; l < cfg.n_conv; ++l) {
        const std::string p = fe + std::to_string(l) + ".";
        const int kl = cfg.conv_kernel[l];
        if (l == 0) {   // [C][1][k0] -> [k0][C] fp32
            w0 = wts.alloc_n<float>((size_t)kl * C, st);
            if (!w0 || pack_f32_launch(get(p + "conv.weight"), w0, kl, C, 1, 1, kl, 0, C, 1, 0, nullptr, st)) return 1;
            if (!(b0 = wv_copy(get(p + "conv.bias"), C, wts, st))) return 1;
        } else {        // [C][C][kl] -> [Cpad128][kl * C], tap-major
            Lin& c = conv[l];
            c.N = C; c.ldw = (long)kl * C;
            c.w = wts.alloc((size_t)round_up(C, 128) * c.ldw * esize(dt), st);
            if (!c.w) return 1;
            for (int t = 0; t < kl; ++t)
                if (pack_any(dt, get(p + "conv.weight") + t, c.w, (long)t * C, C, C, 1, (long)kl * C, kl, 0, c.ldw, 1, 0, nullptr, st)) return 1;
            if (!(c.b = wv_copy(get(p + "conv.bias"), C, wts, st))) return 1;
        }
        if (!(cg[l] = wv_copy(get(p + "layer_norm.weight"), C, wts, st)) || !(cb[l] = wv_copy(get(p + "layer_norm.bias"), C, wts, st))) return 1;
    }
    if (!(pg = wv_copy(get("feature_projection.layer_norm.weight"), C, wts, st)) || !(pb = wv_copy(get("feature_projection.layer_norm.bias"), C, wts, st)))
        return 1;
    if (pack_lin(get("feature_projection.projection.weight"), get("feature_projection.projection.bias"), D, C, nullptr, &proj, st)) return 1;
    {   // positional conv: weight norm (per tap, over dims 0 and 1) folded here
        const std::string pc = pre + "encoder.pos_conv_embed.conv.";
        const float *v = nullptr, *g = nullptr;
        if (sd.has(pc + "weight")) v = sd.get(pc + "weight")->data;
        else if (sd.has(pc + "parametrizations.weight.original1")) { g = sd.get(pc + "parametrizations.weight.original0")->data; v = sd.get(pc + "parametrizations.weight.original1")->data; }
        else { g = sd.get(pc + "weight_g")->data; v = sd.get(pc + "weight_v")->data; }
        float* sc = nullptr;
        if (g) {
            if (!(sc = wts.alloc_n<float>(k, st))) return 1;
            hipLaunchKernelGGL(wv_wn_scale_kernel, dim3(k), dim3(256), 0, st, g, v, (long)D * 64, k, sc);
            SVC_CHECK_HIP(hipGetLastError());
        }
        const size_t nw = (size_t)D * 64 * k;
        if (dt == 0) { if (!(pos16 = wts.alloc_n<half_t>(nw, st))) return 1; }
        else if (!(pos32 = wts.alloc_n<float>(nw + (size_t)128 * k * 64, st))) return 1;      // slack: the tap-GEMM stages whole weight tiles
        hipLaunchKernelGGL(wv_pack_pos_kernel, dim3(cdiv((long)nw, 256)), dim3(256), 0, st, v, sc, D, k, pos16, pos32);
        SVC_CHECK_HIP(hipGetLastError());
        if (!(posb = wv_copy(get("encoder.pos_conv_embed.conv.bias"), D, wts, st))) return 1;
    }
    float* qs = wts.alloc_n<float>(D, st);
    if (!qs) return 1;
    {
        std::vector<float> h(D, WV_QSCALE);
        SVC_CHECK_HIP(hipMemcpyAsync(qs, h.data(), (size_t)D * 4, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
    }
    layers.resize(cfg.n_layers);
    for (int i = 0; i < cfg.n_layers; ++i) {
        Layer& ly = layers[i];
        const std::string p = "encoder.layers." + std::to_string(i) + ".";
        // q | k | v rows of one [3 D][D] weight; the q rows and bias carry 1 / 8 and log2(e)
        ly.qkv.N = 3 * D; ly.qkv.ldw = D;
        ly.qkv.w = wts.alloc((size_t)round_up(3 * D, 128) * D * esize(dt), st);
        ly.qkv.b = wts.alloc_n<float>(3 * D, st);
        if (!ly.qkv.w || !ly.qkv.b) return 1;
        if (pack_any(dt, get(p + "attention.q_proj.weight"), ly.qkv.w, 0, D, 1, D, D, 0, 1, D, 0, 1, qs, st)) return 1;
        if (pack_any(dt, get(p + "attention.k_proj.weight"), ly.qkv.w, (long)D * D, D, 1, D, D, 0, 1, D, 0, 1, nullptr, st)) return 1;
        if (pack_any(dt, get(p + "attention.v_proj.weight"), ly.qkv.w, 2L * D * D, D, 1, D, D, 0, 1, D, 0, 1, nullptr, st)) return 1;
        if (pack_f32_launch(get(p + "attention.q_proj.bias"), ly.qkv.b, D, 1, 1, 1, 0, 0, 1, 0, 0, qs, st)) return 1;
        SVC_CHECK_HIP(hipMemcpyAsync(ly.qkv.b + D, get(p + "attention.k_proj.bias"), (size_t)D * 4, hipMemcpyDeviceToDevice, st));
        SVC_CHECK_HIP(hipMemcpyAsync(ly.qkv.b + 2 * D, get(p + "attention.v_proj.bias"), (size_t)D * 4, hipMemcpyDeviceToDevice, st));
        if (pack_lin(get(p + "attention.out_proj.weight"), get(p + "attention.out_proj.bias"), D, D, nullptr, &ly.o, st)) return 1;
        if (pack_lin(get(p + "feed_forward.intermediate_dense.weight"), get(p + "feed_forward.intermediate_dense.bias"), F, D, nullptr, &ly.fc1, st)) return 1;
        if (pack_lin(get(p + "feed_forward.output_dense.weight"), get(p + "feed_forward.output_dense.bias"), D, F, nullptr, &ly.fc2, st)) return 1;
        if (!(ly.g1 = wv_copy(get(p + "layer_norm.weight"), D, wts, st)) || !(ly.b1 = wv_copy(get(p + "layer_norm.bias"), D, wts, st)) ||
            !(ly.g2 = wv_copy(get(p + "final_layer_norm.weight"), D, wts, st)) || !(ly.b2 = wv_copy(get(p + "final_layer_norm.bias"), D, wts, st)))
            return 1;
    }
    if (!(gf = wv_copy(get("encoder.layer_norm.weight"), D, wts, st)) || !(bf = wv_copy(get("encoder.layer_norm.bias"), D, wts, st))) return 1;
    if (!(dlens = wts.alloc_n<int>((size_t)(WV_MAX_CONV + 1) * WV_MAX_WIN, st))) return 1;
    if (!(part = wts.alloc_n<double>((size_t)2 * WV_MAX_WIN * WV_NBLK, st))) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// The row strides of a call's stage buffers come from THIS call's longest window (the GEMMs run over the windows x strides
// rectangle, so a call must not pay for a longer one the handle saw earlier); the allocation only has to be at least as large.
int svc_w2v::reserve_fe(int G, long nmax, hipStream_t st) {
    Ls[0] = (int)nmax;
    for (int l = 0; l < cfg.n_conv; ++l) Ls[l + 1] = (int)wv_frames(cfg, nmax, l + 1);
    nstride = round_up(nmax, 64);
    if (G <= cap_g && nmax <= cap_n) return 0;
    G = std::max(G, cap_g); nmax = std::max(nmax, cap_n);
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws_fe.release();
    cap_g = 0; cap_n = 0;
    const long C = cfg.conv_dim, L1 = wv_frames(cfg, nmax, 1), L2 = wv_frames(cfg, nmax, 2);
    SVC_REQUIRE((long)G * L1 < (1L << 31), "w2v: the window group is too large for 32-bit row offsets");
    const size_t es = dt == 0 ? 2 : 4;
    wn = ws_fe.alloc_n<float>((size_t)G * round_up(nmax, 64), st);
    actA = ws_fe.alloc((size_t)G * L1 * C * es, st);
    actB = ws_fe.alloc((size_t)G * L2 * C * es, st);
    raw = ws_fe.alloc_n<float>((size_t)G * L2 * C, st);
    if (!wn || !actA || !actB || !raw) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    cap_g = G; cap_n = nmax;
    return 0;
}

int svc_w2v::reserve_enc(int G, int P, hipStream_t st) {
    if (G <= ecap_g && P <= ecap_p) return 0;
    G = std::max(G, ecap_g); P = std::max(P, ecap_p);
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws_enc.release();
    ecap_g = 0; ecap_p = 0;
    const long D = cfg.d_model, F = cfg.ffn_dim, MP = (long)G * P;
    SVC_REQUIRE(MP * std::max(3 * D, F) < (1L << 31), "w2v: the window group is too large for 32-bit row offsets");
    const long vld = round_up(P, 64);
    h32 = ws_enc.alloc_n<float>((size_t)MP * D, st);
    x = ws_enc.alloc_n<float>((size_t)MP * D, st);
    enc = ws_enc.alloc_n<float>((size_t)MP * D, st);
    qkv16 = ws_enc.alloc_n<half_t>((size_t)MP * 3 * D, st);
    vt = ws_enc.alloc_n<half_t>((size_t)G * D * vld, st);
    ao16 = ws_enc.alloc_n<half_t>((size_t)MP * D, st);
    if (!h32 || !x || !enc || !qkv16 || !vt || !ao16) return 1;
    if (dt == 0) {
        h16 = ws_enc.alloc_n<half_t>((size_t)MP * D, st);
        n16 = ws_enc.alloc_n<half_t>((size_t)MP * D, st);
        ff16 = ws_enc.alloc_n<half_t>((size_t)MP * F, st);
        if (!h16 || !n16 || !ff16) return 1;
    } else {
        n32 = ws_enc.alloc_n<float>((size_t)MP * D, st);
        ao32 = ws_enc.alloc_n<float>((size_t)MP * D, st);
        ff32 = ws_enc.alloc_n<float>((size_t)MP * F, st);
        acc32 = ws_enc.alloc_n<float>((size_t)MP * D, st);
        if (!n32 || !ao32 || !ff32 || !acc32) return 1;
    }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ecap_g = G; ecap_p = P;
    return 0;
}

int svc_w2v::put_lens(const LenTab& lt, hipStream_t st) {
    hipLaunchKernelGGL(wv_lens_kernel, dim3(1), dim3(64), 0, st, lt, dlens, cfg.n_conv + 1);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// c = act(a [M][K] W^T + b) (+ res): fp32 and / or fp16 out, leading dimension N
int svc_w2v::lin(const Lin& l, const void* a, long K, long M, int Lout, int act, const float* res, float* c32, half_t* c16, hipStream_t st) {
    KGemmParams p = wv_gemm(M, l.N, Lout);
    p.a_ptr[0] = a; p.a_ld[0] = K; p.a_ktiles[0] = (int)(K / ktile_elems(dt));
    p.w = l.w; p.ldw = l.ldw; p.bias = l.b; p.act = act;
    p.res = res; p.ldres = l.N;
    p.c32 = c32; p.ldc32 = l.N; p.c16 = c16; p.ldc16 = l.N;
    return kgemm_launch(p, dt, KG_EPI_STORE, st);
}

int svc_w2v::rownorm(int mode, const float* xin, long ldx, float* y32, half_t* y16, long ldy, const float* g, const float* b, const float* g2,
                     const float* b2, long rows, int D, const int* lens, int seq_rows, hipStream_t st) {
    SVC_REQUIRE(D >= 64 && D % 64 == 0 && D <= 2048, "layernorm: D must be a multiple of 64, at most 2048");
    if (rows == 0) return 0;
    const dim3 grid(cdiv(rows, 4)), blk(256);
    if (mode == 0) hipLaunchKernelGGL(wv_rownorm_kernel<0>, grid, blk, 0, st, xin, ldx, y32, y16, ldy, g, b, g2, b2, rows, D, 1e-5f, lens, seq_rows);
    else if (mode == 1) hipLaunchKernelGGL(wv_rownorm_kernel<1>, grid, blk, 0, st, xin, ldx, y32, y16, ldy, g, b, g2, b2, rows, D, 1e-5f, lens, seq_rows);
    else hipLaunchKernelGGL(wv_rownorm_kernel<2>, grid, blk, 0, st, xin, ldx, y32, y16, ldy, g, b, g2, b2, rows, D, 1e-5f, lens, seq_rows);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int svc_w2v::normalize_group(const float* wave, long Lrow, const WinTab& wt, int G, float* dst, long stride, hipStream_t st) {
    int nmax = 0;
    for (int g = 0; g < G; ++g) nmax = std::max(nmax, wt.n[g]);
    double* sq = part + WV_MAX_WIN * WV_NBLK;
    hipLaunchKernelGGL(wv_stat_kernel<1>, dim3(WV_NBLK, G), dim3(256), 0, st, wave, wt, Lrow, (const double*)nullptr, part);
    hipLaunchKernelGGL(wv_stat_kernel<2>, dim3(WV_NBLK, G), dim3(256), 0, st, wave, wt, Lrow, (const double*)part, sq);
    hipLaunchKernelGGL(wv_norm_kernel, dim3(cdiv(nmax, 256), G), dim3(256), 0, st, wave, wt, Lrow, (const double*)part, (const double*)sq, dst, stride);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// normalised windows wnorm [G][stride], lengths in dlens (row l = rows after conv l - 1) -> h32 (+ h16) [G][P][D], P = Ls[n_conv]
int svc_w2v::features_group(const float* wnorm, long stride, int G, hipStream_t st) {
    const int C = cfg.conv_dim, nc = cfg.n_conv;
    const bool f16 = dt == 0;
    {
        const int blocks = std::min(cdiv(Ls[1], 4), 2048);
        hipLaunchKernelGGL(wv_conv0_kernel, dim3(blocks, G), dim3(256), (size_t)cfg.conv_kernel[0] * C * 4, st, wnorm, stride, w0, b0, cg[0], cb[0],
                           f16 ? nullptr : (float*)actA, f16 ? (half_t*)actA : nullptr, C, cfg.conv_kernel[0], cfg.conv_stride[0], Ls[1],
                           dlens + WV_MAX_WIN, 1e-5f);
        SVC_CHECK_HIP(hipGetLastError());
    }
    void* cur = actA;
    void* nxt = actB;
    for (int l = 1; l < nc; ++l) {
        const int kl = cfg.conv_kernel[l];
        KGemmParams p = wv_gemm((long)G * Ls[l + 1], C, Ls[l + 1]);
        p.a_seq_rows = Ls[l]; p.a_len = Ls[l]; p.seq_len = dlens + l * WV_MAX_WIN; p.a_stride = cfg.conv_stride[l]; p.pad_mode = KG_PAD_ZERO;
        p.n_taps = kl;
        for (int t = 0; t < kl; ++t) { p.a_ptr[t] = cur; p.a_ld[t] = C; p.a_ktiles[t] = C / ktile_elems(dt); p.a_shift[t] = t; }
        p.w = conv[l].w; p.ldw = conv[l].ldw; p.bias = conv[l].b;
        p.c32 = raw; p.ldc32 = C;
        if (kgemm_launch(p, dt, KG_EPI_STORE, st)) return 1;
        const bool last = l == nc - 1;
        if (rownorm(last ? 2 : 1, raw, C, f16 ? nullptr : (float*)nxt, f16 ? (half_t*)nxt : nullptr, C, cg[l], cb[l], pg, pb, (long)G * Ls[l + 1], C,
                    dlens + (l + 1) * WV_MAX_WIN, Ls[l + 1], st))
            return 1;
        std::swap(cur, nxt);
    }
    const int P = Ls[nc];
    return lin(proj, cur, C, (long)G * P, P, KG_ACT_NONE, nullptr, h32, f16 ? h16 : nullptr, st);
}

// h [G][P][D] (+ its fp16 copy in precision 1), rows per window in dlens row n_conv -> out = h + gelu(posconv(h)) on the valid rows
int svc_w2v::posconv_group(const float* h, const half_t* h16v, int G, int P, float* out, hipStream_t st) {
    const int D = cfg.d_model, k = cfg.pos_k, NG = cfg.pos_groups;
    const int* lens = dlens + cfg.n_conv * WV_MAX_WIN;
    if (dt == 0) {
        const int n_tiles = cdiv(P, WV_PC_BM);
        hipLaunchKernelGGL(w2v_posconv_kernel, dim3((unsigned)(n_tiles * G * NG)), dim3(256), 0, st, h16v, h, pos16, posb, out, lens, P, D, k, G, n_tiles);
        SVC_CHECK_HIP(hipGetLastError());
        return 0;
    }
    for (int g = 0; g < NG; ++g)
        for (int t0 = 0; t0 < k; t0 += KG_MAX_TAPS) {
            const int nt = std::min(KG_MAX_TAPS, k - t0);
            KGemmParams p = wv_gemm((long)G * P, 64, P);
            p.seq_len = lens; p.pad_mode = KG_PAD_ZERO; p.n_taps = nt;
            for (int t = 0; t < nt; ++t) { p.a_ptr[t] = h + g * 64; p.a_ld[t] = D; p.a_ktiles[t] = 2; p.a_shift[t] = t0 + t - k / 2; }
            p.w = pos32 + (long)g * 64 * k * 64 + (long)t0 * 64; p.ldw = (long)k * 64;
            p.c32 = acc32 + g * 64; p.ldc32 = D;
            if (t0) { p.res = acc32 + g * 64; p.ldres = D; }
            if (kgemm_launch(p, 1, KG_EPI_STORE, st)) return 1;
        }
    hipLaunchKernelGGL(wv_posadd_kernel, dim3(P, G), dim3(256), 0, st, h, (const float*)acc32, posb, out, lens, P, D);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// h [G][P][D] -> out [G][P][D] (final LayerNorm); rows at and above a window's count are not written
int svc_w2v::encode_group(const float* h, const half_t* h16v, int G, int P, float* out, hipStream_t st) {
    const int D = cfg.d_model, F = cfg.ffn_dim, H = cfg.n_heads;
    const long MP = (long)G * P;
    const bool f16 = dt == 0;
    const int* lens = dlens + cfg.n_conv * WV_MAX_WIN;
    const long vld = round_up(P, 64);
    if (posconv_group(h, h16v, G, P, x, st)) return 1;
    if (mark(2, st)) return 1;
    const void* nrm = f16 ? (const void*)n16 : (const void*)n32;
    const int vmode = attention_vt_mode(G, H, P);
    for (const Layer& ly : layers) {
        if (rownorm(0, x, D, f16 ? nullptr : n32, f16 ? n16 : nullptr, D, ly.g1, ly.b1, nullptr, nullptr, MP, D, lens, P, st)) return 1;
        if (lin(ly.qkv, nrm, D, MP, P, KG_ACT_NONE, nullptr, nullptr, qkv16, st)) return 1;
        hipLaunchKernelGGL(wv_vt_kernel, dim3(cdiv(vld, 32), D / 32, G), dim3(256), 0, st, qkv16, vt, lens, P, D, vld, vmode);
        SVC_CHECK_HIP(hipGetLastError());
        AttnParams a;
        memset(&a, 0, sizeof(a));
        a.q = qkv16; a.k = qkv16 + D; a.ld_qk = 3 * D;
        a.vt = vt; a.vt_seq_stride = (long)D * vld; a.vt_ld = vld; a.vt_perm = vmode;
        a.out = ao16; a.ld_out = D;
        a.out32 = f16 ? nullptr : ao32;
        a.n_seq = G; a.H = H; a.seq_rows = P; a.Tq = P; a.kv_len = lens; a.kv_len_const = P;
        a.qt_form = qt_form;
        if (attention_launch(a, st)) return 1;
        if (lin(ly.o, f16 ? (const void*)ao16 : (const void*)ao32, D, MP, P, KG_ACT_NONE, x, x, nullptr, st)) return 1;
        if (rownorm(0, x, D, f16 ? nullptr : n32, f16 ? n16 : nullptr, D, ly.g2, ly.b2, nullptr, nullptr, MP, D, lens, P, st)) return 1;
        if (lin(ly.fc1, nrm, D, MP, P, KG_ACT_GELU, nullptr, f16 ? nullptr : ff32, f16 ? ff16 : nullptr, st)) return 1;
        if (lin(ly.fc2, f16 ? (const void*)ff16 : (const void*)ff32, F, MP, P, KG_ACT_NONE, x, x, nullptr, st)) return 1;
    }
    if (rownorm(0, x, D, out, nullptr, D, gf, bf, nullptr, nullptr, MP, D, lens, P, st)) return 1;
    return mark(3, st);
}

extern "C" {

int svc_w2v_create(const svc_w2v_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream, svc_w2v_t** out) {
    SVC_REQUIRE(cfg && weights && out, "svc_w2v_create: null argument");
    SVC_REQUIRE(cfg->feat_extract_norm_layer == 1 && cfg->do_stable_layer_norm == 1 && cfg->conv_bias == 1,
                "svc_w2v_create: only feat_extract_norm = \"layer\" with do_stable_layer_norm and conv_bias is supported (group-norm extractors and "
                "post-LN encoders are refused)");
    if (wv_check_cfg(cfg, "svc_w2v_create")) return 1;
    SVC_REQUIRE(cfg->conv_dim >= 64 && cfg->conv_dim % 64 == 0 && cfg->conv_dim <= 512, "svc_w2v_create: conv_dim must be a multiple of 64, at most 512");
    SVC_REQUIRE(cfg->d_model >= 64 && cfg->d_model % 64 == 0 && cfg->d_model <= 2048 && cfg->n_heads >= 1 && cfg->n_heads * 64 == cfg->d_model,
                "svc_w2v_create: d_model must be a multiple of 64 (at most 2048) and the head dimension 64 (n_heads * 64 == d_model)");
    SVC_REQUIRE(cfg->n_layers >= 1 && cfg->ffn_dim >= 64 && cfg->ffn_dim % 64 == 0, "svc_w2v_create: n_layers >= 1, ffn_dim a multiple of 64");
    SVC_REQUIRE(cfg->pos_k >= 2 && cfg->pos_k % 2 == 0 && cfg->pos_k <= WV_PC_MAXK, "svc_w2v_create: num_conv_pos_embeddings must be even, 2 .. 128");
    SVC_REQUIRE(cfg->pos_groups >= 1 && cfg->pos_groups * 64 == cfg->d_model, "svc_w2v_create: the positional conv needs groups of 64 channels");
    SVC_REQUIRE(cfg->precision == 0 || cfg->precision == 1, "svc_w2v_create: precision 0 (fp32 GEMMs) or 1 (fp16 GEMMs)");
    StateDict sd(weights, n_weights);
    std::string pre;
    for (const char* p : {"", "wav2vec2.", "hubert.", "model."})
        if (sd.has(std::string(p) + "feature_projection.projection.weight")) { pre = p; break; }
    for (const auto& k : wv_keys(*cfg))
        if (wv_require(sd.get(pre + k.name), pre + k.name, k.shape)) return 1;
    {
        const std::string pc = pre + "encoder.pos_conv_embed.conv.";
        const long D = cfg->d_model, k = cfg->pos_k;
        if (sd.has(pc + "weight")) { if (wv_require(sd.get(pc + "weight"), pc + "weight", {D, 64, k})) return 1; }
        else if (sd.has(pc + "parametrizations.weight.original1")) {
            if (wv_require(sd.get(pc + "parametrizations.weight.original0"), pc + "parametrizations.weight.original0", {1, 1, k}) ||
                wv_require(sd.get(pc + "parametrizations.weight.original1"), pc + "parametrizations.weight.original1", {D, 64, k}))
                return 1;
        } else if (wv_require(sd.get(pc + "weight_g"), pc + "weight_g", {1, 1, k}) || wv_require(sd.get(pc + "weight_v"), pc + "weight_v", {D, 64, k}))
            return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    auto* m = new svc_w2v();
    m->cfg = *cfg;
    m->dt = cfg->precision ? 0 : 1;
    // the attention's query-tile form, from the configuration alone: what a group of four full windows would get from the grid-size rule
    const long Pw = wv_frames(*cfg, cfg->window_samples);
    m->qt_form = (long)cdiv(Pw, 128) * cfg->n_heads * 4 <= 256 ? 1 : 2;
    if (m->pack(sd, pre, st)) { delete m; return 1; }
    *out = m;
    return 0;
}

void svc_w2v_destroy(svc_w2v_t* m) { delete m; }

long svc_w2v_frames(const svc_w2v_config_t* cfg, long n_samples) {
    if (wv_check_cfg(cfg, "svc_w2v_frames")) return -1;
    if (n_samples < 0) { set_error("svc_w2v_frames: n_samples must not be negative"); return -1; }
    return wv_frames(*cfg, n_samples);
}

static int wv_plan_check(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples, const char* who) {
    if (wv_check_cfg(cfg, who)) return 1;
    if (overlap_rows < 0 || (long)overlap_rows * WV_SPR >= cfg->window_samples) { set_error(std::string(who) + ": overlap_rows outside [0, window_samples / 320)"); return 1; }
    if (n_samples < 1 || wv_frames(*cfg, std::min<long>(n_samples, cfg->window_samples)) < 1) {
        set_error(std::string(who) + ": n_samples is shorter than the extractor's receptive field");
        return 1;
    }
    return 0;
}

int svc_w2v_n_windows(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples) {
    if (wv_plan_check(cfg, overlap_rows, n_samples, "svc_w2v_n_windows")) return -1;
    const long nw = wv_n_windows(cfg->window_samples, (long)overlap_rows * WV_SPR, n_samples);
    if (nw > 0x7fffffffL) { set_error("svc_w2v_n_windows: n_samples is too large"); return -1; }
    return (int)nw;
}

int svc_w2v_rows(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples) {
    if (wv_plan_check(cfg, overlap_rows, n_samples, "svc_w2v_rows")) return -1;
    const long W = cfg->window_samples, O = (long)overlap_rows * WV_SPR, nw = wv_n_windows(W, O, n_samples);
    long rows = 0;
    for (long j = 0; j < nw; ++j) {
        const long f = wv_frames(*cfg, std::min(W, n_samples - j * (W - O)));
        rows += std::max(0L, f - (j ? overlap_rows : 0));
    }
    if (rows > 0x7fffffffL) { set_error("svc_w2v_rows: n_samples is too large"); return -1; }
    return (int)rows;
}

int svc_w2v_set_window_group(svc_w2v_t* m, int windows) {
    SVC_REQUIRE(windows >= 0 && windows <= WV_MAX_WIN, "svc_w2v_set_window_group: windows must be 0 (default) .. 64");
    SVC_REQUIRE(m, "svc_w2v_set_window_group: null handle");
    m->group = windows ? windows : WV_DEFAULT_GROUP;
    return 0;
}

int svc_w2v_set_timing(svc_w2v_t* m, int on) {
    SVC_REQUIRE(m, "svc_w2v_set_timing: null handle");
    m->timing = on != 0;
    return 0;
}

int svc_w2v_last_timing(svc_w2v_t* m, float* ms4) {
    SVC_REQUIRE(m && ms4 && m->timing && m->ev[0] && m->ev[4], "svc_w2v_last_timing: timing is off or no svc_w2v_content call was made");
    SVC_CHECK_HIP(hipEventSynchronize(m->ev[4]));
    for (int i = 0; i < 4; ++i) SVC_CHECK_HIP(hipEventElapsedTime(&ms4[i], m->ev[i], m->ev[i + 1]));
    return 0;
}

int svc_w2v_normalize(svc_w2v_t* m, const float* wave, const int32_t* lens, int B, int L, float* out, void* stream) {
    SVC_REQUIRE(lens != nullptr, "svc_w2v_normalize: lens is NULL");
    SVC_REQUIRE(B >= 1 && B <= WV_MAX_B, "svc_w2v_normalize: B must be 1 .. 64 clips");
    SVC_REQUIRE(L >= 1, "svc_w2v_normalize: L must be at least 1 sample");
    for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 1 && lens[b] <= L, "svc_w2v_normalize: lens outside [1, L]");
    SVC_REQUIRE(wave && out, "svc_w2v_normalize: null wave or out");
    SVC_REQUIRE(m, "svc_w2v_normalize: null handle");
    WinTab wt;
    memset(&wt, 0, sizeof(wt));
    for (int b = 0; b < B; ++b) { wt.clip[b] = b; wt.n[b] = lens[b]; }
    return m->normalize_group(wave, L, wt, B, out, L, (hipStream_t)stream);
}

int svc_w2v_features(svc_w2v_t* m, const float* wave_norm, const int32_t* lens, int B, int L, float* out, int Tmax, void* stream) {
    SVC_REQUIRE(lens != nullptr, "svc_w2v_features: lens is NULL");
    SVC_REQUIRE(B >= 1 && B <= WV_MAX_B, "svc_w2v_features: B must be 1 .. 64 clips");
    SVC_REQUIRE(L >= 1, "svc_w2v_features: L must be at least 1 sample");
    for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 1 && lens[b] <= L, "svc_w2v_features: lens outside [1, L]");
    SVC_REQUIRE(wave_norm && out, "svc_w2v_features: null wave or out");
    SVC_REQUIRE(m, "svc_w2v_features: null handle");
    long nmax = 0;
    for (int b = 0; b < B; ++b) {
        const long f = wv_frames(m->cfg, lens[b]);
        SVC_REQUIRE(f >= 1, "svc_w2v_features: lens shorter than the extractor's receptive field");
        SVC_REQUIRE(f <= Tmax, "svc_w2v_features: Tmax is smaller than the longest clip's rows (svc_w2v_frames)");
        nmax = std::max<long>(nmax, lens[b]);
    }
    hipStream_t st = (hipStream_t)stream;
    const int G = std::min(m->group, B), nc = m->cfg.n_conv, D = m->cfg.d_model;
    if (m->reserve_fe(G, nmax, st)) return 1;
    const int P = m->Ls[nc];                                 // this call's rows per window
    if (m->reserve_enc(G, P, st)) return 1;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = std::min(G, B - b0);
        LenTab lt;
        memset(&lt, 0, sizeof(lt));
        for (int g = 0; g < nb; ++g)
            for (int l = 0; l <= nc; ++l) lt.v[l][g] = (int)wv_frames(m->cfg, lens[b0 + g], l);
        if (m->put_lens(lt, st)) return 1;
        if (m->features_group(wave_norm + (long)b0 * L, L, nb, st)) return 1;
        hipLaunchKernelGGL(wv_copy_rows_kernel, dim3(P, nb), dim3(256), 0, st, (const float*)m->h32, P, out + (long)b0 * Tmax * D, Tmax,
                           (const int*)(m->dlens + nc * WV_MAX_WIN), D);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

static int wv_seam_rows(svc_w2v_t* m, const float* h, const int32_t* rows, int B, int T, float* out, void* stream, bool layers, const char* who) {
    const std::string w(who);
    if (!rows) { set_error(w + ": rows is NULL"); return 1; }
    if (B < 1 || B > WV_MAX_B) { set_error(w + ": B must be 1 .. 64 clips"); return 1; }
    if (T < 1) { set_error(w + ": T must be at least 1 row"); return 1; }
    for (int b = 0; b < B; ++b)
        if (rows[b] < 1 || rows[b] > T) { set_error(w + ": rows outside [1, T]"); return 1; }
    if (!h || !out) { set_error(w + ": null h or out"); return 1; }
    if (!m) { set_error(w + ": null handle"); return 1; }
    hipStream_t st = (hipStream_t)stream;
    const int G = std::min(m->group, B), nc = m->cfg.n_conv, D = m->cfg.d_model;
    if (m->reserve_enc(G, T, st)) return 1;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = std::min(G, B - b0);
        LenTab lt;
        memset(&lt, 0, sizeof(lt));
        for (int g = 0; g < nb; ++g) lt.v[nc][g] = rows[b0 + g];
        if (m->put_lens(lt, st)) return 1;
        const float* hg = h + (long)b0 * T * D;
        float* og = out + (long)b0 * T * D;
        if (m->dt == 0 && cast_rows_launch(hg, D, m->h16, D, nb * T, D, st)) return 1;
        if (layers) { if (m->encode_group(hg, m->h16, nb, T, og, st)) return 1; }
        else if (m->posconv_group(hg, m->h16, nb, T, og, st)) return 1;
    }
    return 0;
}

int svc_w2v_posconv(svc_w2v_t* m, const float* h, const int32_t* rows, int B, int T, float* out, void* stream) {
    return wv_seam_rows(m, h, rows, B, T, out, stream, false, "svc_w2v_posconv");
}

int svc_w2v_encode(svc_w2v_t* m, const float* h, const int32_t* rows, int B, int T, float* out, void* stream) {
    return wv_seam_rows(m, h, rows, B, T, out, stream, true, "svc_w2v_encode");
}

int svc_w2v_content(svc_w2v_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, float* out, int Rmax, void* stream) {
    SVC_REQUIRE(B >= 1 && B <= WV_MAX_B, "svc_w2v_content: B must be 1 .. 64 clips");
    SVC_REQUIRE(L >= 1, "svc_w2v_content: L must be at least 1 sample");
    if (lens)
        for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 1 && lens[b] <= L, "svc_w2v_content: lens outside [1, L]");
    SVC_REQUIRE(overlap_rows >= 0, "svc_w2v_content: overlap_rows outside [0, window_samples / 320)");
    SVC_REQUIRE(Rmax >= 1, "svc_w2v_content: Rmax is smaller than the longest clip's rows (svc_w2v_rows)");
    SVC_REQUIRE(wave && out, "svc_w2v_content: null wave or out");
    SVC_REQUIRE(m, "svc_w2v_content: null handle");
    const svc_w2v_config_t& c = m->cfg;
    const int D = c.d_model, nc = c.n_conv;
    const long W = c.window_samples, O = (long)overlap_rows * WV_SPR;
    SVC_REQUIRE(O < W, "svc_w2v_content: overlap_rows outside [0, window_samples / 320)");
    struct Win { int clip, start, n, dst0, drop, keep, zero_from; };
    std::vector<Win> wins;
    long nmax = 0;
    for (int b = 0; b < B; ++b) {
        const long n = lens ? lens[b] : L;
        SVC_REQUIRE(wv_frames(c, std::min(n, W)) >= 1, "svc_w2v_content: lens shorter than the extractor's receptive field");
        const int rows = svc_w2v_rows(&c, overlap_rows, n);
        SVC_REQUIRE(rows >= 0 && rows <= Rmax, "svc_w2v_content: Rmax is smaller than the longest clip's rows (svc_w2v_rows)");
        const long nw = wv_n_windows(W, O, n);
        int dst = 0;
        for (long j = 0; j < nw; ++j) {
            const long s = j * (W - O), ns = std::min(W, n - s);
            const int keep = (int)wv_frames(c, ns), drop = j ? overlap_rows : 0;
            if (keep <= drop) continue;                          // a later window no longer than the overlap contributes nothing
            wins.push_back({b, (int)s, (int)ns, dst, drop, keep, -1});
            dst += keep - drop;
            nmax = std::max(nmax, ns);
        }
        wins.back().zero_from = rows;                            // the clip's last computed window zeroes the rows above its count
    }
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)std::min((size_t)m->group, wins.size());
    if (m->reserve_fe(G, nmax, st)) return 1;
    const int P = m->Ls[nc];                                 // this call's rows per window
    if (m->reserve_enc(G, P, st)) return 1;
    for (size_t w0 = 0; w0 < wins.size(); w0 += G) {
        const int nb = (int)std::min((size_t)G, wins.size() - w0);
        WinTab wt;
        LenTab lt;
        memset(&wt, 0, sizeof(wt));
        memset(&lt, 0, sizeof(lt));
        for (int g = 0; g < nb; ++g) {
            const Win& w = wins[w0 + g];
            wt.clip[g] = w.clip; wt.start[g] = w.start; wt.n[g] = w.n; wt.dst0[g] = w.dst0; wt.drop[g] = w.drop;
            wt.keep[g] = w.keep;
            wt.zero_from[g] = w.zero_from;
            for (int l = 0; l <= nc; ++l) lt.v[l][g] = (int)wv_frames(c, w.n, l);
        }
        if (m->mark(0, st)) return 1;
        if (m->put_lens(lt, st)) return 1;
        if (m->normalize_group(wave, L, wt, nb, m->wn, m->nstride, st)) return 1;
        if (m->features_group(m->wn, m->nstride, nb, st) || m->mark(1, st)) return 1;
        if (m->encode_group(m->h32, m->h16, nb, P, m->enc, st)) return 1;
        hipLaunchKernelGGL(wv_assemble_kernel, dim3(P + Rmax, nb), dim3(256), 0, st, (const float*)m->enc, wt, out, P, D, Rmax);
        SVC_CHECK_HIP(hipGetLastError());
        if (m->mark(4, st)) return 1;
    }
    return 0;
}

/* y = gelu(LayerNorm(x) * gamma + beta) over rows of D (op seam of the extractor's LayerNorm + erf-GELU row kernel) */
int svc_op_layernorm_gelu(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, void* stream) {
    SVC_REQUIRE(x && gamma && beta && y && rows >= 0, "svc_op_layernorm_gelu: null argument or negative rows");
    SVC_REQUIRE(D >= 64 && D % 64 == 0 && D <= 2048, "svc_op_layernorm_gelu: D must be a multiple of 64, at most 2048");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(wv_rownorm_kernel<1>, dim3(cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, (long)D, y, (half_t*)nullptr, (long)D, gamma, beta,
                       (const float*)nullptr, (const float*)nullptr, (long)rows, D, eps, (const int*)nullptr, 1);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
