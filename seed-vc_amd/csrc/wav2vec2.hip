// wav2vec 2.0 content encoder for gfx950 (XLS-R-300m / HuBERT-large family: layer-norm feature extractor, "stable layer norm"
// transformer, grouped positional conv): 16 kHz audio -> content features at 50 rows/s (`semantic_fn` of the reference drivers for
// the xlsr models: Wav2Vec2FeatureExtractor + the first layers of facebook/wav2vec2-xls-r-300m in float16).
//
// Normalisation: per window (x - mean) / sqrt(var + 1e-7), mean first, then the variance about it, both from 64 block partials
// folded in a fixed order (double accumulation, no atomics).  Extractor: conv0 (1 -> C) fused with its LayerNorm and erf-GELU in
// one row kernel (one wave per output row, the raw 3200 rows/s x C plane is never written), convs 1..n-1 as 2- and 3-tap
// tap-GEMMs on channels-last rows (stride in the row map, no padding) each followed by the LayerNorm+GELU row kernel, the last of
// which also applies the feature projection's LayerNorm; then Linear C -> D.  Positional conv: a grouped Conv1d of k taps as a
// Toeplitz product per (group, 64-position tile, window), input rows resident in LDS (w2v_posconv_kernel); precision 0 runs it on
// the fp32 tap-GEMM, one accumulating launch per group and 48 taps.  The transformer stack (with per-window key counts), the
// window plan of long clips and the row gather are content_encoder.h's.  Every window is computed as if alone (tile-independent
// tap order in the positional conv), so its bits do not depend on its companions, their order or the group size.
//
// The base family (HuBERT-base / wav2vec2-base, through svc_w2v_create_ex): a group norm over the window's own conv0
// frames instead of the LayerNorms (statistics from the window's samples: wv_gn_*_kernel below), positional-conv groups of 16 .. 64
// channels (the kernel is a template on the width) and the stack's post-LN order.
#include <math.h>
#include <string.h>

#include "w2v_internal.h"

using namespace svc;

namespace {

constexpr int WV_NBLK = 64;
constexpr int WV_PC_BM = 64, WV_PC_MAXK = 128, WV_PC_AHEAD = 4;    // positional conv: positions per workgroup, most taps, taps of weights in flight
constexpr StackNames WV_NAMES = {"encoder.layers.", "attention.q_proj", "attention.k_proj", "attention.k_proj.bias", "attention.v_proj",
                                 "attention.out_proj", "layer_norm", "feed_forward.intermediate_dense", "feed_forward.output_dense",
                                 "final_layer_norm", "encoder.layer_norm"};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void wv_lens_kernel(LenTab lt, int* __restrict__ dst, int n_rows) {
    const int i = threadIdx.x;
    if (i < MAX_WIN)
        for (int r = 0; r < n_rows; ++r) dst[r * MAX_WIN + i] = lt.v[r][i];
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
        row_norm<8>(v, n, C, eps, gamma, beta, lane, true);
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
// Groups of WD = 16, 32 or 48 channels (the base family: 768 / 16 = 48) keep the 128-byte rows and the K steps of 32: the 16-byte
// chunks at and above WD / 8 of every row are WRITTEN as zeros (0 x a stale NaN would be NaN), the weight fragments of the channels
// at and above WD are zeros from the pack, WD / 16 waves own output channels (the others only help to load the rows) and WD <= 32
// runs one K step.  WD = 64 is the kernel it was, instruction for instruction.
__device__ __forceinline__ int wv_pc_swz(int row) { return (row >> 1) & 7; }

template <int WD>
__global__ __launch_bounds__(256) void w2v_posconv_kernel(const half_t* __restrict__ x16, const float* __restrict__ x32, const half_t* __restrict__ wp,
                                                          const float* __restrict__ bias, float* __restrict__ out, const int* __restrict__ lens,
                                                          int P, int D, int k, int n_win, int n_tiles) {
    __shared__ __attribute__((aligned(16))) char rows_s[(WV_PC_BM + WV_PC_MAXK - 1) * 128];
    const int tile = blockIdx.x % n_tiles, win = (blockIdx.x / n_tiles) % n_win, grp = blockIdx.x / (n_tiles * n_win);
    const int T = lens[win], p0 = tile * WV_PC_BM;
    if (p0 >= T) return;                                    // uniform over the workgroup, before any barrier
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
    constexpr int NW = WD / 16, KS = WD > 32 ? 2 : 1;        // waves that own output channels, K steps of 32 channels
    const int R = WV_PC_BM + k - 1, half = k / 2;
    const half_t* xg = x16 + (long)win * P * D + grp * WD;
    for (int idx = tid; idx < R * 8; idx += 256) {
        const int r = idx >> 3, c = idx & 7, q = p0 + r - half;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if ((WD == 64 || c < WD / 8) && q >= 0 && q < T) v = *reinterpret_cast<const uint4*>(xg + (long)q * D + c * 8);
        *reinterpret_cast<uint4*>(rows_s + r * 128 + ((c ^ wv_pc_swz(r)) << 4)) = v;
    }
    __syncthreads();
    if (NW < 4 && wave >= NW) return;                        // after the only barrier
    float4v acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (float4v){0.f, 0.f, 0.f, 0.f};
    // fragment (tap t, k-step ks, wave w): wp[(((grp k + t) KS + ks) NW + w) 64 + lane] (16 bytes)
    constexpr int TS = KS * NW * 64, K1 = (KS - 1) * NW * 64;   // fragments per tap; offset of the second K step (0: there is none)
    const uint4* wf = reinterpret_cast<const uint4*>(wp) + ((long)grp * k * KS * NW + wave) * 64 + lane;
    // the weights of the next WV_PC_AHEAD taps are in flight under the MFMAs of a tap (a tap's 8 MFMAs are shorter than an L2 round trip)
    uint4 wb[WV_PC_AHEAD][2];
#pragma unroll
    for (int u = 0; u < WV_PC_AHEAD; ++u)
        if (u < k) { wb[u][0] = wf[(long)u * TS]; wb[u][1] = wf[(long)u * TS + K1]; }
    for (int t0 = 0; t0 < k; t0 += WV_PC_AHEAD) {
#pragma unroll
        for (int u = 0; u < WV_PC_AHEAD; ++u) {
            const int t = t0 + u;
            if (t >= k) break;
            const uint4 c0 = wb[u][0], c1 = wb[u][1];
            if (t + WV_PC_AHEAD < k) { wb[u][0] = wf[(long)(t + WV_PC_AHEAD) * TS]; wb[u][1] = wf[(long)(t + WV_PC_AHEAD) * TS + K1]; }
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int row = mt * 16 + fr + t;
                const char* rp = rows_s + row * 128;
                const int sw = wv_pc_swz(row);
                const uint4 a0 = *reinterpret_cast<const uint4*>(rp + ((fq ^ sw) << 4));
                const uint4 a1 = *reinterpret_cast<const uint4*>(rp + (((4 + fq) ^ sw) << 4));
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a0), __builtin_bit_cast(half8, c0), acc[mt], 0, 0, 0);
                if (KS == 2) acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a1), __builtin_bit_cast(half8, c1), acc[mt], 0, 0, 0);
            }
        }
    }
    // acc[mt][r] = C[position p0 + 16 mt + 4 fq + r][channel 16 wave + fr]
    const int nch = grp * WD + wave * 16 + fr;
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
// v [D][wd][k] (x sc[t], or as it is when sc is null), groups of wd channels -> the fp16 fragment stream of w2v_posconv_kernel and /
// or the fp32 tap-GEMM rows w32[(grp wd + n)][t 64 + c].  With wd < 64 the slots of the channels wd .. 63 (wd .. 31 at wd = 16) are
// not written here: the caller zeroed the whole destination first.
__global__ void wv_pack_pos_kernel(const float* __restrict__ v, const float* __restrict__ sc, int D, int wd, int k, half_t* __restrict__ wp,
                                   float* __restrict__ w32) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)D * wd * k) return;
    const int t = (int)(i % k), c = (int)((i / k) % wd), no = (int)(i / ((long)k * wd));
    const float val = v[i] * (sc ? sc[t] : 1.f);
    const int grp = no / wd, n = no % wd, nw = wd / 16, nks = wd > 32 ? 2 : 1;
    if (wp) {
        const int w = n >> 4, fr = n & 15, ks = c >> 5, fq = (c & 31) >> 3, j = c & 7;
        wp[((((long)(grp * k + t) * nks + ks) * nw + w) * 64 + fq * 16 + fr) * 8 + j] = (half_t)val;
    }
    if (w32) w32[((long)no * k + t) * 64 + c] = val;
}
// precision 0, groups narrower than 64 channels: dst [rows][NG 64] = the rows of h [rows][NG wd] with every group zero-padded to 64
// channels (the fp32 tap-GEMM reads K in steps of 32).  Rows at and above the window's count are written as zeros, never read.
__global__ void wv_padgroups_kernel(const float* __restrict__ h, float* __restrict__ dst, const int* __restrict__ lens, int P, int D, int wd) {
    const int win = blockIdx.y, p = blockIdx.x, ng = D / wd;
    const bool live = p < lens[win];
    const long i = (long)win * P + p;
    for (int c = threadIdx.x; c < ng * 64; c += blockDim.x) {
        const int g = c >> 6, cc = c & 63;
        dst[i * ng * 64 + c] = live && cc < wd ? h[i * D + g * wd + cc] : 0.f;
    }
}

// ---- group-norm extractor (the base family).  GroupNorm with one channel per group normalises channel c of conv0
// over the window's own T0 frames.  conv0 is linear in its k0 taps, so with m_j = mean_t x[s0 t + j] and Cov_jk = mean_t (x[s0 t + j]
// - m_j)(x[s0 t + k] - m_k) the channel's mean is b_c + sum_j w_cj m_j and its variance sum_jk w_cj w_ck Cov_jk: the raw T0 x C plane
// is never written.  Statistics: item = a tap j (POW 1) or a pair j <= k (POW 2); block blk of 64 sums its share of the frames (the
// share depends on T0 only), thread (item, frame lane fl) sums the frames fl, fl + FL, ... of the share in order, the FL lanes are
// folded in index order; the 64 block partials are folded in index order by the consumer.  Double throughout, no atomics.
constexpr int WV_GN_MAXK = 16, WV_GN_MAXP = WV_GN_MAXK * (WV_GN_MAXK + 1) / 2;      // most taps of conv0 in this family, most pairs
template <int POW>
__global__ __launch_bounds__(256) void wv_gn_stat_kernel(const float* __restrict__ x, long stride, const int* __restrict__ lens0, int k0, int s0,
                                                         int n_items, int items_pad, const double* __restrict__ sums, double* __restrict__ part) {
    __shared__ double red[256];
    __shared__ double mean_s[WV_GN_MAXK];
    const int g = blockIdx.y, blk = blockIdx.x, T0 = lens0[g];
    const float* xg = x + (long)g * stride;
    const int per = (T0 + WV_NBLK - 1) / WV_NBLK, i0 = blk * per, i1 = min(T0, i0 + per);
    const int item = threadIdx.x % items_pad, fl = threadIdx.x / items_pad, FL = 256 / items_pad;
    if (POW == 2 && threadIdx.x < k0) {
        double m = 0.0;
        for (int b = 0; b < WV_NBLK; ++b) m += sums[((long)g * WV_NBLK + b) * k0 + threadIdx.x];
        mean_s[threadIdx.x] = m / (double)T0;
    }
    __syncthreads();
    int j = item, kk = item;
    if (POW == 2) {                                          // pair index -> (j <= kk), rows of the upper triangle in order
        j = 0;
        int left = item;
        while (j < k0 - 1 && left >= k0 - j) { left -= k0 - j; ++j; }
        kk = j + left;
    }
    double s = 0.0;
    if (item < n_items) {
        const double mj = POW == 2 ? mean_s[j] : 0.0, mk = POW == 2 ? mean_s[kk] : 0.0;
        for (int t = i0 + fl; t < i1; t += FL) {
            const float* xt = xg + (long)t * s0;
            s += POW == 2 ? ((double)xt[j] - mj) * ((double)xt[kk] - mk) : (double)xt[j];
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (fl == 0 && item < n_items) {
        double a = 0.0;
        for (int f = 0; f < FL; ++f) a += red[f * items_pad + item];
        part[((long)g * WV_NBLK + blk) * n_items + item] = a;
    }
}
// one block per window: fold the partials, then per channel y = (conv0 of the centred samples) * scale + shift with
// scale = gamma / sqrt(var_c + eps), shift = beta (the conv bias cancels against the channel's mean); the tap means go to `mean`
__global__ __launch_bounds__(256) void wv_gn_affine_kernel(const double* __restrict__ psum, const double* __restrict__ pcov, const int* __restrict__ lens0,
                                                           const float* __restrict__ w /*[k0][C]*/, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int C, int k0, float eps, float* __restrict__ mean,
                                                           float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ double cov_s[WV_GN_MAXK][WV_GN_MAXK];
    const int g = blockIdx.x, T0 = lens0[g], np = k0 * (k0 + 1) / 2;
    if (T0 < 1) return;
    for (int item = threadIdx.x; item < np + k0; item += 256) {
        const bool is_mean = item >= np;
        const int it = is_mean ? item - np : item, n_items = is_mean ? k0 : np;
        const double* p = (is_mean ? psum : pcov) + (long)g * WV_NBLK * n_items + it;
        double a = 0.0;
        for (int b = 0; b < WV_NBLK; ++b) a += p[(long)b * n_items];
        a /= (double)T0;
        if (is_mean) mean[g * WV_GN_MAXK + it] = (float)a;
        else {
            int j = 0, left = it;
            while (j < k0 - 1 && left >= k0 - j) { left -= k0 - j; ++j; }
            cov_s[j][j + left] = a;
            cov_s[j + left][j] = a;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        double var = 0.0;
        for (int j = 0; j < k0; ++j) {
            double r = 0.0;
            for (int kk = 0; kk < k0; ++kk) r += (double)w[kk * C + c] * cov_s[j][kk];
            var += (double)w[j * C + c] * r;
        }
        scale[(long)g * C + c] = (float)((double)gamma[c] / sqrt(fmax(var, 0.0) + (double)eps));
        shift[(long)g * C + c] = beta[c];
    }
}
// conv0 on the centred samples + the channel's scale and shift + erf-GELU: one wave per output row, weights [k0][C] in LDS
__global__ __launch_bounds__(256) void wv_conv0_gn_kernel(const float* __restrict__ wn, long stride, const float* __restrict__ w /*[k0][C]*/,
                                                          const float* __restrict__ mean, const float* __restrict__ scale, const float* __restrict__ shift,
                                                          float* __restrict__ y32, half_t* __restrict__ y16, int C, int k0, int s0, int L0,
                                                          const int* __restrict__ lens0) {
    extern __shared__ float w_s[];
    const int g = blockIdx.y, lane = threadIdx.x & 63, n = C / 64, len = lens0[g];
    for (int i = threadIdx.x; i < k0 * C; i += 256) w_s[i] = w[i];
    __syncthreads();
    const float* xg = wn + (long)g * stride;
    const float* mg = mean + g * WV_GN_MAXK;
    float sc[8], sh[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i < n && len > 0) { sc[i] = scale[(long)g * C + lane + 64 * i]; sh[i] = shift[(long)g * C + lane + 64 * i]; }
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < len; row += gridDim.x * 4) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
        for (int t = 0; t < k0; ++t) {
            const float xv = xg[(long)row * s0 + t] - mg[t];
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (i < n) v[i] = fmaf(xv, w_s[t * C + lane + 64 * i], v[i]);
        }
        const long o = ((long)g * L0 + row) * C;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < n) {
                const float yv = gelu_erf(fmaf(v[i], sc[i], sh[i]));
                if (y32) y32[o + lane + 64 * i] = yv;
                if (y16) y16[o + lane + 64 * i] = (half_t)yv;
            }
    }
}
// do_normalize = 0: dst[g][i] = the window's samples as they are, i < n; nothing at or above n is read or written
__global__ void wv_copy_kernel(const float* __restrict__ wave, WinTab wt, long Lrow, float* __restrict__ dst, long stride) {
    const int g = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < wt.n[g]) dst[(long)g * stride + i] = wave[(long)wt.clip[g] * Lrow + wt.start[g] + i];
}

}  // namespace

namespace svc {

long wv_frames(const svc_w2v_config_t& c, long n, int upto) {
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
    if (hop != SAMPLES_PER_ROW) return bad("the conv strides must multiply to 320 samples per row (the drivers' window plan counts rows of 320 samples)");
    if ((long)c->conv_kernel[0] * c->conv_dim > 8192) return bad("conv_kernel[0] * conv_dim must not exceed 8192 (conv0 keeps its weights in 32 KB of LDS)");
    if (c->window_samples < SAMPLES_PER_ROW || c->window_samples % SAMPLES_PER_ROW) return bad("window_samples must be a positive multiple of 320");
    if (wv_frames(*c, c->window_samples) < 1) return bad("window_samples is shorter than the extractor's receptive field");
    return 0;
}

}  // namespace svc

namespace {

std::vector<KeyShape> wv_keys(const svc_w2v_config_t& c, bool final_ln) {
    const long D = c.d_model, F = c.ffn_dim, C = c.conv_dim;
    std::vector<KeyShape> k;
    for (int l = 0; l < c.n_conv; ++l) {
        const std::string p = "feature_extractor.conv_layers." + std::to_string(l) + ".";
        k.push_back({p + "conv.weight", {C, l ? C : 1, c.conv_kernel[l]}});
        if (c.conv_bias) k.push_back({p + "conv.bias", {C}});
        if (!c.feat_extract_norm_layer && l) continue;       // group norm: conv 0 alone has a norm (a GroupNorm, under the same name)
        k.push_back({p + "layer_norm.weight", {C}});
        k.push_back({p + "layer_norm.bias", {C}});
    }
    k.push_back({"feature_projection.layer_norm.weight", {C}});
    k.push_back({"feature_projection.layer_norm.bias", {C}});
    k.push_back({"feature_projection.projection.weight", {D, C}});
    k.push_back({"feature_projection.projection.bias", {D}});
    k.push_back({"encoder.pos_conv_embed.conv.bias", {D}});
    EncoderStack::keys(WV_NAMES, c.n_layers, D, F, k, final_ln);
    return k;
}

}  // namespace

int svc_w2v::pack(const StateDict& sd, const std::string& pre, hipStream_t st) {
    const int D = cfg.d_model, C = cfg.conv_dim, k = cfg.pos_k;
    auto get = [&](const std::string& key) { return sd.get(pre + key)->data; };       // every key was checked by the caller
    const std::string fe = "feature_extractor.conv_layers.";
    for (int l = 0; l < cfg.n_conv; ++l) {
        const std::string p = fe + std::to_string(l) + ".";
        const int kl = cfg.conv_kernel[l];
        if (l == 0) {   // [C][1][k0] -> [k0][C] fp32
            w0 = wts.alloc_n<float>((size_t)kl * C, st);
            if (!w0 || pack_f32_launch(get(p + "conv.weight"), w0, kl, C, 1, 1, kl, 0, C, 1, 0, nullptr, st)) return 1;
            if (cfg.conv_bias) { if (!(b0 = copy_f32(get(p + "conv.bias"), C, wts, st))) return 1; }
            else {               // the layer-norm conv0 kernel adds a bias: zeros (the group-norm one has none: it cancels against the mean)
                if (!(b0 = wts.alloc_n<float>(C, st))) return 1;
                SVC_CHECK_HIP(hipMemsetAsync(b0, 0, (size_t)C * 4, st));
            }
        } else {        // [C][C][kl] -> [Cpad128][kl * C], tap-major
            Lin& c = conv[l];
            c.N = C; c.ldw = (long)kl * C;
            c.w = wts.alloc((size_t)round_up(C, 128) * c.ldw * esize(dt), st);
            if (!c.w) return 1;
            for (int t = 0; t < kl; ++t)
                if (pack_any(dt, get(p + "conv.weight") + t, c.w, (long)t * C, C, C, 1, (long)kl * C, kl, 0, c.ldw, 1, 0, nullptr, st)) return 1;
            if (cfg.conv_bias && !(c.b = copy_f32(get(p + "conv.bias"), C, wts, st))) return 1;
        }
        if (group_norm && l) continue;
        if (!(cg[l] = copy_f32(get(p + "layer_norm.weight"), C, wts, st)) || !(cb[l] = copy_f32(get(p + "layer_norm.bias"), C, wts, st))) return 1;
    }
    if (!(pg = copy_f32(get("feature_projection.layer_norm.weight"), C, wts, st)) || !(pb = copy_f32(get("feature_projection.layer_norm.bias"), C, wts, st)))
        return 1;
    if (pack_lin(dt, wts, get("feature_projection.projection.weight"), get("feature_projection.projection.bias"), D, C, nullptr, &proj, st)) return 1;
    {   // positional conv: weight norm (per tap, over dims 0 and 1) folded here
        const std::string pc = pre + "encoder.pos_conv_embed.conv.";
        const float *v = nullptr, *g = nullptr;
        if (sd.has(pc + "weight")) v = sd.get(pc + "weight")->data;
        else if (sd.has(pc + "parametrizations.weight.original1")) { g = sd.get(pc + "parametrizations.weight.original0")->data; v = sd.get(pc + "parametrizations.weight.original1")->data; }
        else { g = sd.get(pc + "weight_g")->data; v = sd.get(pc + "weight_v")->data; }
        float* sc = nullptr;
        if (g) {
            if (!(sc = wts.alloc_n<float>(k, st))) return 1;
            hipLaunchKernelGGL(wv_wn_scale_kernel, dim3(k), dim3(256), 0, st, g, v, (long)D * pos_w, k, sc);
            SVC_CHECK_HIP(hipGetLastError());
        }
        const size_t nw = (size_t)D * pos_w * k;            // weights; fp16 fragment slots: whole K steps of 32 channels; fp32 rows: 64 channels
        const size_t n16 = (size_t)D * (pos_w > 32 ? 64 : 32) * k, n32 = (size_t)D * 64 * k + (size_t)128 * k * 64;   // slack: the tap-GEMM stages whole weight tiles
        if (dt == 0) { if (!(pos16 = wts.alloc_n<half_t>(n16, st))) return 1; }
        else if (!(pos32 = wts.alloc_n<float>(n32, st))) return 1;
        if (pos_w < 64) SVC_CHECK_HIP(dt == 0 ? hipMemsetAsync(pos16, 0, n16 * 2, st) : hipMemsetAsync(pos32, 0, n32 * 4, st));   // the padded channels' slots
        hipLaunchKernelGGL(wv_pack_pos_kernel, dim3(cdiv((long)nw, 256)), dim3(256), 0, st, v, sc, D, pos_w, k, pos16, pos32);
        SVC_CHECK_HIP(hipGetLastError());
        if (!(posb = copy_f32(get("encoder.pos_conv_embed.conv.bias"), D, wts, st))) return 1;
    }
    if (stack.pack(sd, pre, WV_NAMES, cfg.n_layers, wts, st)) return 1;
    if (!(dlens = wts.alloc_n<int>((size_t)(WV_MAX_CONV + 1) * MAX_WIN, st))) return 1;
    if (!(part = wts.alloc_n<double>((size_t)2 * MAX_WIN * WV_NBLK, st))) return 1;
    if (group_norm) {
        const int k0 = cfg.conv_kernel[0];
        if (!(gpart = wts.alloc_n<double>((size_t)MAX_WIN * WV_NBLK * (k0 + k0 * (k0 + 1) / 2), st)) ||
            !(gmean = wts.alloc_n<float>((size_t)MAX_WIN * WV_GN_MAXK, st)) || !(gscale = wts.alloc_n<float>((size_t)MAX_WIN * C, st)) ||
            !(gshift = wts.alloc_n<float>((size_t)MAX_WIN * C, st)))
            return 1;
    }
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
    const long D = cfg.d_model, MP = (long)G * P;
    h32 = ws_enc.alloc_n<float>((size_t)MP * D, st);
    enc = ws_enc.alloc_n<float>((size_t)MP * D, st);
    if (!h32 || !enc || stack.reserve(ws_enc, G, P, st)) return 1;
    if (dt == 0 && !(h16 = ws_enc.alloc_n<half_t>((size_t)MP * D, st))) return 1;
    if (dt == 1 && !(acc32 = ws_enc.alloc_n<float>((size_t)MP * D, st))) return 1;
    if (dt == 1 && pos_w < 64 && !(hpad = ws_enc.alloc_n<float>((size_t)MP * cfg.pos_groups * 64, st))) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ecap_g = G; ecap_p = P;
    return 0;
}

int svc_w2v::put_lens(const LenTab& lt, hipStream_t st) {
    hipLaunchKernelGGL(wv_lens_kernel, dim3(1), dim3(64), 0, st, lt, dlens, cfg.n_conv + 1);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int svc_w2v::normalize_group(const float* wave, long Lrow, const WinTab& wt, int G, float* dst, long stride, hipStream_t st) {
    int nmax = 0;
    for (int g = 0; g < G; ++g) nmax = std::max(nmax, wt.n[g]);
    if (!do_normalize) {
        hipLaunchKernelGGL(wv_copy_kernel, dim3(cdiv(nmax, 256), G), dim3(256), 0, st, wave, wt, Lrow, dst, stride);
        SVC_CHECK_HIP(hipGetLastError());
        return 0;
    }
    double* sq = part + MAX_WIN * WV_NBLK;
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
    if (group_norm) {
        const int k0 = cfg.conv_kernel[0], s0 = cfg.conv_stride[0], np = k0 * (k0 + 1) / 2;
        auto pad = [](int n) { int p = 16; while (p < n) p *= 2; return p; };
        double* pcov = gpart + (size_t)MAX_WIN * WV_NBLK * k0;
        const int* lens0 = dlens + MAX_WIN;
        hipLaunchKernelGGL(wv_gn_stat_kernel<1>, dim3(WV_NBLK, G), dim3(256), 0, st, wnorm, stride, lens0, k0, s0, k0, pad(k0), (const double*)nullptr, gpart);
        hipLaunchKernelGGL(wv_gn_stat_kernel<2>, dim3(WV_NBLK, G), dim3(256), 0, st, wnorm, stride, lens0, k0, s0, np, pad(np), (const double*)gpart, pcov);
        hipLaunchKernelGGL(wv_gn_affine_kernel, dim3(G), dim3(256), 0, st, (const double*)gpart, (const double*)pcov, lens0, w0, cg[0], cb[0], C, k0, 1e-5f,
                           gmean, gscale, gshift);
        const int blocks = std::min(cdiv(Ls[1], 4), 2048);
        hipLaunchKernelGGL(wv_conv0_gn_kernel, dim3(blocks, G), dim3(256), (size_t)k0 * C * 4, st, wnorm, stride, w0, gmean, gscale, gshift,
                           f16 ? nullptr : (float*)actA, f16 ? (half_t*)actA : nullptr, C, k0, s0, Ls[1], lens0);
        SVC_CHECK_HIP(hipGetLastError());
    } else {
        const int blocks = std::min(cdiv(Ls[1], 4), 2048);
        hipLaunchKernelGGL(wv_conv0_kernel, dim3(blocks, G), dim3(256), (size_t)cfg.conv_kernel[0] * C * 4, st, wnorm, stride, w0, b0, cg[0], cb[0],
                           f16 ? nullptr : (float*)actA, f16 ? (half_t*)actA : nullptr, C, cfg.conv_kernel[0], cfg.conv_stride[0], Ls[1],
                           dlens + MAX_WIN, 1e-5f);
        SVC_CHECK_HIP(hipGetLastError());
    }
    void* cur = actA;
    void* nxt = actB;
    for (int l = 1; l < nc; ++l) {
        const int kl = cfg.conv_kernel[l];
        KGemmParams p = kgemm_rows((long)G * Ls[l + 1], C, Ls[l + 1]);
        p.a_seq_rows = Ls[l]; p.a_len = Ls[l]; p.seq_len = dlens + l * MAX_WIN; p.a_stride = cfg.conv_stride[l]; p.pad_mode = KG_PAD_ZERO;
        p.n_taps = kl;
        for (int t = 0; t < kl; ++t) { p.a_ptr[t] = cur; p.a_ld[t] = C; p.a_ktiles[t] = C / ktile_elems(dt); p.a_shift[t] = t; }
        p.w = conv[l].w; p.ldw = conv[l].ldw; p.bias = conv[l].b;
        const bool last = l == nc - 1;
        if (group_norm) {       // conv, GELU (in the epilogue), no norm; the last one is followed by the feature projection's LayerNorm
            p.act = KG_ACT_GELU;
            if (last || !f16) { p.c32 = last ? raw : (float*)nxt; p.ldc32 = C; }
            else { p.c16 = (half_t*)nxt; p.ldc16 = C; }
            if (kgemm_launch(p, dt, KG_EPI_STORE, st)) return 1;
            if (last && rownorm_launch(0, raw, C, f16 ? nullptr : (float*)nxt, f16 ? (half_t*)nxt : nullptr, C, pg, pb, nullptr, nullptr,
                                       (long)G * Ls[l + 1], C, 1e-5f, dlens + (l + 1) * MAX_WIN, Ls[l + 1], st))
                return 1;
            std::swap(cur, nxt);
            continue;
        }
        p.c32 = raw; p.ldc32 = C;
        if (kgemm_launch(p, dt, KG_EPI_STORE, st)) return 1;
        if (rownorm_launch(last ? 2 : 1, raw, C, f16 ? nullptr : (float*)nxt, f16 ? (half_t*)nxt : nullptr, C, cg[l], cb[l], pg, pb,
                           (long)G * Ls[l + 1], C, 1e-5f, dlens + (l + 1) * MAX_WIN, Ls[l + 1], st))
            return 1;
        std::swap(cur, nxt);
    }
    const int P = Ls[nc];
    return linear_launch(dt, proj, cur, C, (long)G * P, P, KG_ACT_NONE, nullptr, h32, f16 ? h16 : nullptr, st);
}

// h [G][P][D] (+ its fp16 copy in precision 1), rows per window in dlens row n_conv -> out = h + gelu(posconv(h)) on the valid rows
int svc_w2v::posconv_group(const float* h, const half_t* h16v, int G, int P, float* out, hipStream_t st) {
    const int D = cfg.d_model, k = cfg.pos_k, NG = cfg.pos_groups;
    const int* lens = dlens + cfg.n_conv * MAX_WIN;
    if (dt == 0) {
        const int n_tiles = cdiv(P, WV_PC_BM);
        const auto kernel = pos_w == 64 ? w2v_posconv_kernel<64> : pos_w == 48 ? w2v_posconv_kernel<48> : pos_w == 32 ? w2v_posconv_kernel<32> : w2v_posconv_kernel<16>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)(n_tiles * G * NG)), dim3(256), 0, st, h16v, h, pos16, posb, out, lens, P, D, k, G, n_tiles);
        SVC_CHECK_HIP(hipGetLastError());
        return 0;
    }
    const int wd = pos_w;
    const float* a = h;                                      // groups of 64 channels are read in place; narrower ones from their padded copy
    long lda = D;
    if (wd < 64) {
        hipLaunchKernelGGL(wv_padgroups_kernel, dim3(P, G), dim3(256), 0, st, h, hpad, lens, P, D, wd);
        SVC_CHECK_HIP(hipGetLastError());
        a = hpad; lda = (long)NG * 64;
    }
    for (int g = 0; g < NG; ++g)
        for (int t0 = 0; t0 < k; t0 += KG_MAX_TAPS) {
            const int nt = std::min(KG_MAX_TAPS, k - t0);
            KGemmParams p = kgemm_rows((long)G * P, wd, P);
            p.seq_len = lens; p.pad_mode = KG_PAD_ZERO; p.n_taps = nt;
            for (int t = 0; t < nt; ++t) { p.a_ptr[t] = a + g * 64; p.a_ld[t] = lda; p.a_ktiles[t] = 2; p.a_shift[t] = t0 + t - k / 2; }
            p.w = pos32 + (long)g * wd * k * 64 + (long)t0 * 64; p.ldw = (long)k * 64;
            p.c32 = acc32 + g * wd; p.ldc32 = D;
            if (t0) { p.res = acc32 + g * wd; p.ldres = D; }
            if (kgemm_launch(p, 1, KG_EPI_STORE, st)) return 1;
        }
    hipLaunchKernelGGL(wv_posadd_kernel, dim3(P, G), dim3(256), 0, st, h, (const float*)acc32, posb, out, lens, P, D);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// h [G][P][D] -> out [G][P][D] (final LayerNorm); rows at and above a window's count are not written.  A handle made without the
// final LayerNorm leaves the residual stream in stack.x and does not use `out`.
int svc_w2v::encode_group(const float* h, const half_t* h16v, int G, int P, float* out, hipStream_t st) {
    if (posconv_group(h, h16v, G, P, stack.x, st)) return 1;
    if (tm.mark(2, st) || stack.run(G, P, dlens + cfg.n_conv * MAX_WIN, out, st)) return 1;
    return tm.mark(3, st);
}

int svc::w2v_create(const svc_w2v_config_t* cfg, const svc_w2v_ext_t* ext, const svc_tensor_desc_t* weights, int n_weights, void* stream, bool final_ln,
                    svc_w2v_t** out) {
    SVC_REQUIRE(cfg && weights && out, "svc_w2v_create: null argument");
    if (!ext)
        SVC_REQUIRE(cfg->feat_extract_norm_layer == 1 && cfg->do_stable_layer_norm == 1 && cfg->conv_bias == 1,
                    "svc_w2v_create: only feat_extract_norm = \"layer\" with do_stable_layer_norm and conv_bias is supported (group-norm extractors and "
                    "post-LN encoders are refused)");
    else {
        const int fl = cfg->feat_extract_norm_layer, sl = cfg->do_stable_layer_norm;
        SVC_REQUIRE((fl == 0 || fl == 1) && (sl == 0 || sl == 1) && (cfg->conv_bias == 0 || cfg->conv_bias == 1),
                    "svc_w2v_create_ex: feat_extract_norm_layer, do_stable_layer_norm and conv_bias must each be 0 or 1");
        SVC_REQUIRE(!(fl == 0 && sl == 1), "svc_w2v_create_ex: feat_extract_norm = \"group\" with do_stable_layer_norm is a mixed form no released model "
                                           "has (the group-norm extractor goes with the post-LN encoder)");
        SVC_REQUIRE(!(fl == 1 && sl == 0), "svc_w2v_create_ex: feat_extract_norm = \"layer\" without do_stable_layer_norm is a mixed form no released "
                                           "model has (the layer-norm extractor goes with the stable-layer-norm encoder)");
        SVC_REQUIRE(ext->do_normalize == 0 || ext->do_normalize == 1, "svc_w2v_create_ex: do_normalize must be 0 or 1");
        SVC_REQUIRE(ext->feat_proj_layer_norm == 1, "svc_w2v_create_ex: feat_proj_layer_norm must be 1 (a feature projection without its LayerNorm is not "
                                                    "supported)");
        SVC_REQUIRE(final_ln || sl == 1, "svc_w2v_create_ex: the post-LN encoder cannot run without encoder.layer_norm");
    }
    if (wv_check_cfg(cfg, "svc_w2v_create")) return 1;
    SVC_REQUIRE(cfg->feat_extract_norm_layer == 1 || cfg->conv_kernel[0] <= WV_GN_MAXK,
                "svc_w2v_create_ex: a group-norm extractor needs conv_kernel[0] <= 16 (its statistics hold every pair of taps)");
    SVC_REQUIRE(cfg->conv_dim >= 64 && cfg->conv_dim % 64 == 0 && cfg->conv_dim <= 512, "svc_w2v_create: conv_dim must be a multiple of 64, at most 512");
    SVC_REQUIRE(cfg->d_model >= 64 && cfg->d_model % 64 == 0 && cfg->d_model <= 2048 && cfg->n_heads >= 1 && cfg->n_heads * 64 == cfg->d_model,
                "svc_w2v_create: d_model must be a multiple of 64 (at most 2048) and the head dimension 64 (n_heads * 64 == d_model)");
    SVC_REQUIRE(cfg->n_layers >= 1 && cfg->ffn_dim >= 64 && cfg->ffn_dim % 64 == 0, "svc_w2v_create: n_layers >= 1, ffn_dim a multiple of 64");
    SVC_REQUIRE(cfg->pos_k >= 2 && cfg->pos_k % 2 == 0 && cfg->pos_k <= WV_PC_MAXK, "svc_w2v_create: num_conv_pos_embeddings must be even, 2 .. 128");
    if (!ext) SVC_REQUIRE(cfg->pos_groups >= 1 && cfg->pos_groups * 64 == cfg->d_model, "svc_w2v_create: the positional conv needs groups of 64 channels");
    else
        SVC_REQUIRE(cfg->pos_groups >= 1 && cfg->d_model % cfg->pos_groups == 0 && (cfg->d_model / cfg->pos_groups) % 16 == 0 &&
                        cfg->d_model / cfg->pos_groups <= 64,
                    "svc_w2v_create_ex: the positional conv needs groups of 16, 32, 48 or 64 channels (d_model / pos_groups a multiple of 16, at most 64)");
    SVC_REQUIRE(cfg->precision == 0 || cfg->precision == 1, "svc_w2v_create: precision 0 (fp32 GEMMs) or 1 (fp16 GEMMs)");
    const char* who = "svc_w2v_create";
    const long pos_w = cfg->d_model / cfg->pos_groups;
    StateDict sd(weights, n_weights);
    std::string pre;
    for (const char* p : {"", "wav2vec2.", "hubert.", "model."})
        if (sd.has(std::string(p) + "feature_projection.projection.weight")) { pre = p; break; }
    for (const auto& k : wv_keys(*cfg, final_ln))
        if (require_shape(sd.get(pre + k.name), pre + k.name, k.shape, who)) return 1;
    {
        const std::string pc = pre + "encoder.pos_conv_embed.conv.";
        const long D = cfg->d_model, k = cfg->pos_k;
        if (sd.has(pc + "weight")) { if (require_shape(sd.get(pc + "weight"), pc + "weight", {D, pos_w, k}, who)) return 1; }
        else if (sd.has(pc + "parametrizations.weight.original1")) {
            if (require_shape(sd.get(pc + "parametrizations.weight.original0"), pc + "parametrizations.weight.original0", {1, 1, k}, who) ||
                require_shape(sd.get(pc + "parametrizations.weight.original1"), pc + "parametrizations.weight.original1", {D, pos_w, k}, who))
                return 1;
        } else if (require_shape(sd.get(pc + "weight_g"), pc + "weight_g", {1, 1, k}, who) || require_shape(sd.get(pc + "weight_v"), pc + "weight_v", {D, pos_w, k}, who))
            return 1;
    }
    hipStream_t st = (hipStream_t)stream;
    auto* m = new svc_w2v();
    m->cfg = *cfg;
    m->dt = cfg->precision ? 0 : 1;
    m->group_norm = cfg->feat_extract_norm_layer == 0;
    m->do_normalize = !ext || ext->do_normalize == 1;
    m->pos_w = (int)pos_w;
    // the attention's query-tile form, from the configuration alone: what a group of four full windows would get from the grid-size rule
    const long Pw = wv_frames(*cfg, cfg->window_samples);
    m->stack.dt = m->dt; m->stack.D = cfg->d_model; m->stack.F = cfg->ffn_dim; m->stack.H = cfg->n_heads;
    m->stack.final_ln = final_ln;
    m->stack.post_ln = cfg->do_stable_layer_norm == 0;
    m->stack.qt_form = (long)cdiv(Pw, 128) * cfg->n_heads * 4 <= 256 ? 1 : 2;
    if (m->pack(sd, pre, st)) { delete m; return 1; }
    *out = m;
    return 0;
}

extern "C" {

int svc_w2v_create(const svc_w2v_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream, svc_w2v_t** out) {
    return w2v_create(cfg, nullptr, weights, n_weights, stream, true, out);
}

int svc_w2v_create_ex(const svc_w2v_config_t* cfg, const svc_w2v_ext_t* ext, const svc_tensor_desc_t* weights, int n_weights, void* stream,
                      svc_w2v_t** out) {
    return w2v_create(cfg, ext, weights, n_weights, stream, true, out);
}

void svc_w2v_destroy(svc_w2v_t* m) { delete m; }

long svc_w2v_frames(const svc_w2v_config_t* cfg, long n_samples) {
    if (wv_check_cfg(cfg, "svc_w2v_frames")) return -1;
    if (n_samples < 0) { set_error("svc_w2v_frames: n_samples must not be negative"); return -1; }
    return wv_frames(*cfg, n_samples);
}

static int wv_plan_check(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples, const char* who) {
    if (wv_check_cfg(cfg, who)) return 1;
    if (overlap_rows < 0 || (long)overlap_rows * SAMPLES_PER_ROW >= cfg->window_samples) { set_error(std::string(who) + ": overlap_rows outside [0, window_samples / 320)"); return 1; }
    if (n_samples < 1 || wv_frames(*cfg, std::min<long>(n_samples, cfg->window_samples)) < 1) {
        set_error(std::string(who) + ": n_samples is shorter than the extractor's receptive field");
        return 1;
    }
    return 0;
}

int svc_w2v_n_windows(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples) {
    if (wv_plan_check(cfg, overlap_rows, n_samples, "svc_w2v_n_windows")) return -1;
    const long nw = window_count(cfg->window_samples, (long)overlap_rows * SAMPLES_PER_ROW, n_samples);
    if (nw > 0x7fffffffL) { set_error("svc_w2v_n_windows: n_samples is too large"); return -1; }
    return (int)nw;
}

int svc_w2v_rows(const svc_w2v_config_t* cfg, int overlap_rows, long n_samples) {
    if (wv_plan_check(cfg, overlap_rows, n_samples, "svc_w2v_rows")) return -1;
    const long W = cfg->window_samples, O = (long)overlap_rows * SAMPLES_PER_ROW, nw = window_count(W, O, n_samples);
    long rows = 0;
    for (long j = 0; j < nw; ++j) {
        const long f = wv_frames(*cfg, std::min(W, n_samples - j * (W - O)));
        rows += std::max(0L, f - (j ? overlap_rows : 0));
    }
    if (rows > 0x7fffffffL) { set_error("svc_w2v_rows: n_samples is too large"); return -1; }
    return (int)rows;
}

int svc_w2v_set_window_group(svc_w2v_t* m, int windows) {
    SVC_REQUIRE(windows >= 0 && windows <= MAX_WIN, "svc_w2v_set_window_group: windows must be 0 (default) .. 64");
    SVC_REQUIRE(m, "svc_w2v_set_window_group: null handle");
    m->group = windows ? windows : WV_DEFAULT_GROUP;
    return 0;
}

int svc_w2v_set_timing(svc_w2v_t* m, int on) {
    SVC_REQUIRE(m, "svc_w2v_set_timing: null handle");
    m->tm.on = on != 0;
    return 0;
}

int svc_w2v_last_timing(svc_w2v_t* m, float* ms4) {
    const char* msg = "svc_w2v_last_timing: timing is off or no svc_w2v_content call was made";
    SVC_REQUIRE(m, msg);
    return m->tm.last(ms4, msg);
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
        if (copy_rows_launch(m->h32, P, out + (long)b0 * Tmax * D, Tmax, m->dlens + nc * MAX_WIN, nb, P, D, st)) return 1;
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
    const long W = c.window_samples;
    SVC_REQUIRE((long)overlap_rows * SAMPLES_PER_ROW < W, "svc_w2v_content: overlap_rows outside [0, window_samples / 320)");
    std::vector<Win> wins;                                   // the window plan of the whole call, in clip order
    for (int b = 0; b < B; ++b) {
        const long n = lens ? lens[b] : L;
        SVC_REQUIRE(wv_frames(c, std::min(n, W)) >= 1, "svc_w2v_content: lens shorter than the extractor's receptive field");
        const int rows = plan_clip(wins, b, n, W, overlap_rows, [&c](long ns) { return wv_frames(c, ns); });
        SVC_REQUIRE(rows <= Rmax, "svc_w2v_content: Rmax is smaller than the longest clip's rows (svc_w2v_rows)");
    }
    long nmax = 0;
    for (const Win& w : wins) nmax = std::max<long>(nmax, w.n);
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)std::min((size_t)m->group, wins.size());
    if (m->reserve_fe(G, nmax, st)) return 1;
    const int P = m->Ls[nc];                                 // this call's rows per window
    if (m->reserve_enc(G, P, st)) return 1;
    for (size_t w0 = 0; w0 < wins.size(); w0 += G) {
        const int nb = (int)std::min((size_t)G, wins.size() - w0);
        const WinTab wt = win_table(wins, w0, nb);
        LenTab lt;
        memset(&lt, 0, sizeof(lt));
        for (int g = 0; g < nb; ++g)
            for (int l = 0; l <= nc; ++l) lt.v[l][g] = (int)wv_frames(c, wt.n[g], l);
        if (m->tm.mark(0, st)) return 1;
        if (m->put_lens(lt, st)) return 1;
        if (m->normalize_group(wave, L, wt, nb, m->wn, m->nstride, st)) return 1;
        if (m->features_group(m->wn, m->nstride, nb, st) || m->tm.mark(1, st)) return 1;
        if (m->encode_group(m->h32, m->h16, nb, P, m->enc, st)) return 1;
        if (assemble_launch(m->enc, wt, nb, out, P, D, Rmax, 256, st)) return 1;
        if (m->tm.mark(4, st)) return 1;
    }
    return 0;
}

/* y = gelu(LayerNorm(x) * gamma + beta) over rows of D (op seam of the extractor's LayerNorm + erf-GELU row kernel) */
int svc_op_layernorm_gelu(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, void* stream) {
    SVC_REQUIRE(x && gamma && beta && y && rows >= 0, "svc_op_layernorm_gelu: null argument or negative rows");
    SVC_REQUIRE(D >= 64 && D % 64 == 0 && D <= 2048, "svc_op_layernorm_gelu: D must be a multiple of 64, at most 2048");
    return rownorm_launch(1, x, D, y, nullptr, D, gamma, beta, nullptr, nullptr, rows, D, eps, nullptr, 1, (hipStream_t)stream);
}

}  // extern "C"
