// ASTRAL tokenizer for gfx950 (the content tokens of the v2 model): 16 kHz audio -> HuBERT-large rows (the
// wav2vec 2.0 encoder of wav2vec2.hip, cut after `ssl.n_layers` layers, without encoder.layer_norm) -> per head a ConvNeXt V2
// stage and a binary spherical quantizer -> int32 tokens at 50 rows/s.  One SSL pass feeds every head (the reference runs HuBERT
// once per tokenizer).
//
// Head, on channels-last rows [G][P][C] with the window's own row count from a device table: input_projection on the packed
// linear; per block a row kernel for the depthwise conv (7 taps over the window's OWN rows, zeros outside, never loaded) with its
// bias and the LayerNorm (eps 1e-6) straight into pwconv1's operand dtype, pwconv1 + erf-GELU and pwconv2 + residual on the
// packed linears, and between them GRN: sums of squares per (window, channel) from partials over tiles of 64 of the window's own
// rows folded in index order, the factor 1 + gamma Nx, and one pass y (1 + gamma Nx) + beta over pwconv1's output.  BSQ:
// project_in in fp32 from the fp32 residual rows, one wave per row, the signs packed MSB first in the same kernel.  Residual
// stream, statistics and logits are fp32, reductions have a fixed order and no atomics, so a window's bits do not depend on its
// companions, their order or the group size.
#include <math.h>
#include <string.h>

#include "w2v_internal.h"

using namespace svc;

namespace {

constexpr int AS_MAX_HEADS = SVC_ASTRAL_MAX_HEADS, AS_DW_K = 7, AS_TILE = 64, AS_MAX_BITS = 16;

struct RowTab { int v[MAX_WIN]; };
struct HeadMap { int v[AS_MAX_HEADS]; };                     // output plane -> head (svc_astral_tokens_heads)

__global__ void as_rows_kernel(RowTab t, int* __restrict__ dst) {
    if (threadIdx.x < MAX_WIN) dst[threadIdx.x] = t.v[threadIdx.x];
}

// x [G][P][C] fp32 -> y [G][P][C]: depthwise conv (w [7][C], bias) over the window's own rows, then LayerNorm over channels.
// One wave per output row; rows at and above rows[g] are neither read nor written.
template <int NMAX, typename OutT>
__global__ __launch_bounds__(256) void as_dwln_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, OutT* __restrict__ y,
                                                      const int* __restrict__ rows, int P, int C, float eps) {
    const int g = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, n = C / 64, len = rows[g];
    if (row >= len) return;
    float v[NMAX];
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) v[i] = bias[lane + 64 * i];
#pragma unroll
    for (int t = 0; t < AS_DW_K; ++t) {
        const int r = row + t - AS_DW_K / 2;
        if (r < 0 || r >= len) continue;                     // uniform over the wave
        const float* xr = x + ((long)g * P + r) * C;
#pragma unroll
        for (int i = 0; i < NMAX; ++i)
            if (i < n) v[i] = fmaf(xr[lane + 64 * i], w[t * C + lane + 64 * i], v[i]);
    }
    row_norm<NMAX>(v, n, C, eps, gamma, beta, lane, false);
    OutT* yr = y + ((long)g * P + row) * C;
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) yr[lane + 64 * i] = (OutT)v[i];
}

// part[g][tile][c] = sum over the rows [64 tile, 64 tile + 64) below rows[g] of y[g][row][c]^2, in row order
template <typename T>
__global__ __launch_bounds__(256) void as_grn_part_kernel(const T* __restrict__ y, float* __restrict__ part, const int* __restrict__ rows, int P, int F,
                                                          int n_tiles) {
    const int g = blockIdx.z, tile = blockIdx.x, c = blockIdx.y * 256 + threadIdx.x, len = rows[g];
    const int r0 = tile * AS_TILE, r1 = min(len, r0 + AS_TILE);
    if (r0 >= len || c >= F) return;
    const T* yp = y + ((long)g * P + r0) * F + c;
    float s = 0.f;
    for (int r = r0; r < r1; ++r, yp += F) { const float a = (float)*yp; s = fmaf(a, a, s); }
    part[((long)g * n_tiles + tile) * F + c] = s;
}

// fac[g][c] = 1 + gamma[c] Gx[c] / (mean_c Gx + 1e-6), Gx[c] = sqrt(the window's partials folded in index order); one workgroup
// per window, the channel mean from per-thread sums in channel order, a wave butterfly and the four waves in order
__global__ __launch_bounds__(256) void as_grn_fac_kernel(const float* __restrict__ part, const float* __restrict__ gamma, float* __restrict__ fac,
                                                         const int* __restrict__ rows, int F, int n_tiles) {
    __shared__ float red[4];
    const int g = blockIdx.x, nt = (rows[g] + AS_TILE - 1) / AS_TILE;
    float gx[8], s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = threadIdx.x + 256 * i;
        gx[i] = 0.f;
        if (c < F) {
            float q = 0.f;
            for (int t = 0; t < nt; ++t) q += part[((long)g * n_tiles + t) * F + c];
            gx[i] = sqrtf(q);
            s += gx[i];
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float inv = 1.0f / (((red[0] + red[1]) + (red[2] + red[3])) / (float)F + 1e-6f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = threadIdx.x + 256 * i;
        if (c < F) fac[(long)g * F + c] = fmaf(gamma[c], gx[i] * inv, 1.0f);
    }
}

// y[g][row][c] = y fac[g][c] + beta[c] on the window's own rows, in place (pwconv2's operand); one wave per row, four rows per
// workgroup, V elements of 16 bytes per lane and step
template <typename T, int V>
__global__ __launch_bounds__(256) void as_grn_apply_kernel(T* __restrict__ y, const float* __restrict__ fac, const float* __restrict__ beta,
                                                           const int* __restrict__ rows, int P, int F) {
    struct __attribute__((aligned(16))) Vec { T e[V]; };
    const int g = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows[g]) return;
    Vec* yr = reinterpret_cast<Vec*>(y + ((long)g * P + row) * F);
    const float* fg = fac + (long)g * F;
    for (int i = lane; i < F / V; i += 64) {
        Vec a = yr[i];
#pragma unroll
        for (int j = 0; j < V; ++j) a.e[j] = (T)fmaf((float)a.e[j], fg[i * V + j], beta[i * V + j]);
        yr[i] = a;
    }
}

// MSB-first index of the strictly positive logits (both zeros and NaN give bit 0)
__device__ __forceinline__ int as_bit(float z, int j, int bits) { return z > 0.f ? 1 << (bits - 1 - j) : 0; }

// x [G][P][C] fp32 -> index[g][row] = sum_j [x . w[j] + b[j] > 0] 2^(bits - 1 - j), or the logits z[g][row][j] when z is given;
// one wave per row, each dot product in channel order lane + 64 i, then a wave butterfly
template <int NMAX>
__global__ __launch_bounds__(256) void as_bsq_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                     int* __restrict__ index, float* __restrict__ z, const int* __restrict__ rows, int P, int C, int bits) {
    const int g = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, n = C / 64;
    if (row >= rows[g]) return;
    const float* xr = x + ((long)g * P + row) * C;
    float v[NMAX];
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) v[i] = xr[lane + 64 * i];
    int idx = 0;
    for (int j = 0; j < bits; ++j) {
        const float* wj = w + (long)j * C;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NMAX; ++i)
            if (i < n) s = fmaf(v[i], wj[lane + 64 * i], s);
        s = wave_sum(s) + b[j];
        if (z) { if (lane == 0) z[((long)g * P + row) * bits + j] = s; }
        else idx |= as_bit(s, j, bits);
    }
    if (!z && lane == 0) index[(long)g * P + row] = idx;
}

__global__ void as_index_kernel(const float* __restrict__ z, int* __restrict__ index, long rows, int bits) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int idx = 0;
    for (int j = 0; j < bits; ++j) idx |= as_bit(z[r * bits + j], j, bits);
    index[r] = idx;
}

// idx [heads][G * P] -> tokens [planes][B][Rmax]: thread (r, g, plane), plane p holding head hm.v[p].  r < P: row r of window g,
// when kept, goes to its place in the clip's tokens; r >= P: token r - P of the clip becomes -1 when window g is the clip's last
// and r - P is at or above the count
__global__ void as_assemble_kernel(const int* __restrict__ idx, WinTab wt, int* __restrict__ tokens, int P, int G, int B, int Rmax, long idx_stride,
                                   HeadMap hm) {
    const int g = blockIdx.y, plane = blockIdx.z, head = hm.v[plane], r = blockIdx.x * blockDim.x + threadIdx.x;
    int* out = tokens + ((long)plane * B + wt.clip[g]) * Rmax;
    if (r < P) {
        if (r >= wt.drop[g] && r < wt.keep[g]) out[wt.dst0[g] + r - wt.drop[g]] = idx[(long)head * idx_stride + (long)g * P + r];
    } else if (r < P + Rmax) {
        const int zr = r - P;
        if (wt.zero_from[g] >= 0 && zr >= wt.zero_from[g]) out[zr] = -1;
    }
}

// Duration reduction (unique_consecutive) of clip b0 + blockIdx.x: a ragged compaction in chunks of 256 tokens, kept tokens in
// order, -1 above the count, the count by a plain vector store.  in and out must not overlap.
__global__ __launch_bounds__(256) void as_reduce_kernel(const int* __restrict__ in, RowTab rows, int b0, int R, int* __restrict__ out,
                                                        int* __restrict__ counts) {
    __shared__ int wsum[4];
    const int b = b0 + blockIdx.x, n = rows.v[blockIdx.x], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int* src = in + (long)b * R;
    int* dst = out + (long)b * R;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        int tok = 0;
        bool keep = false;
        if (i < n) { tok = src[i]; keep = i == 0 || src[i - 1] != tok; }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int k = 0; k < wave; ++k) off += wsum[k];
        if (keep) dst[off + before] = tok;
        base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    for (int i = base + threadIdx.x; i < R; i += 256) dst[i] = -1;
    if (threadIdx.x == 0) counts[b] = base;
}

struct Block {
    float *dw = nullptr, *dwb = nullptr, *ng = nullptr, *nb = nullptr, *gamma = nullptr, *beta = nullptr;   // dw [7][dim]
    Lin pw1, pw2;
};
struct Head {
    svc_astral_head_config_t c;
    Lin inp;
    std::vector<Block> blocks;
    float *pin_w = nullptr, *pin_b = nullptr;                // project_in [bits][dim], fp32
    float* x = nullptr;                                      // workspace: the head's residual stream [G * P][dim]
};

long as_rows_of(const svc_w2v_config_t& c, long ns) { return std::min(wv_frames(c, ns), ns / SAMPLES_PER_ROW); }

int as_check_cfg(const svc_astral_config_t* c, const char* who) {
    auto bad = [&](const std::string& msg) { set_error(std::string(who) + ": " + msg); return 1; };
    if (!c) return bad("null config");
    if (c->n_heads < 1 || c->n_heads > AS_MAX_HEADS) return bad("n_heads must be 1 or 2");
    for (int k = 0; k < c->n_heads; ++k) {
        const svc_astral_head_config_t& h = c->head[k];
        if (h.dim < 64 || h.dim % 64 || h.dim > 2048) return bad("dim must be a multiple of 64, at most 2048");
        if (h.intermediate_dim < 64 || h.intermediate_dim % 64 || h.intermediate_dim > 2048) return bad("intermediate_dim must be a multiple of 64, at most 2048");
        if (h.n_blocks < 1 || h.n_blocks > 64) return bad("n_blocks must be 1 .. 64");
        if (h.bits < 1 || h.bits > AS_MAX_BITS) return bad("bits must be 1 .. 16 (codebook_size = 2^bits)");
        if (h.dw_kernel != AS_DW_K) return bad("only a depthwise conv of 7 taps (padding 3, dilation 1) is supported");
    }
    return 0;
}

int as_plan_check(const svc_astral_config_t* cfg, int overlap_rows, long n_samples, const char* who) {
    if (!cfg) { set_error(std::string(who) + ": null config"); return 1; }
    if (wv_check_cfg(&cfg->ssl, who)) return 1;
    if (overlap_rows < 0 || (long)overlap_rows * SAMPLES_PER_ROW >= cfg->ssl.window_samples) { set_error(std::string(who) + ": overlap_rows outside [0, window_samples / 320)"); return 1; }
    if (n_samples < 1 || as_rows_of(cfg->ssl, std::min<long>(n_samples, cfg->ssl.window_samples)) < 1) {
        set_error(std::string(who) + ": n_samples is shorter than the extractor's receptive field");
        return 1;
    }
    return 0;
}

}  // namespace

struct svc_astral {
    svc_astral_config_t cfg;
    int dt = 0, group = WV_DEFAULT_GROUP;
    svc_w2v* ssl = nullptr;
    Head heads[AS_MAX_HEADS];
    Arena wts, ws;
    int cap_g = 0, cap_p = 0;
    void *nrm = nullptr, *y = nullptr;                       // [G * P][dim] and [G * P][F] in the GEMM's dtype
    half_t* h16 = nullptr;                                   // precision 1: the SSL rows as input_projection's operand
    float *part = nullptr, *fac = nullptr;
    int *idx = nullptr, *hrows = nullptr;                    // idx [heads][G * P]; hrows [MAX_WIN]: the current group's rows per window
    StageTimer tm;
    ~svc_astral() { svc_w2v_destroy(ssl); }
    int pack_head(int k, const StateDict& sd, hipStream_t st);
    int reserve(int G, int P, hipStream_t st);
    int put_rows(const int* rows, int G, hipStream_t st);
    int convnext_group(int k, const float* h, int G, int P, hipStream_t st);          // h [G][P][Din] -> heads[k].x
    int bsq_group(int k, const float* x, int G, int P, int* index, float* z, hipStream_t st);
};

namespace {

// the keys of head k and their shapes; input_projection.weight and the GRN parameters are checked by element count
int as_check_head(const svc_astral_config_t& c, int k, const StateDict& sd, const char* who) {
    const svc_astral_head_config_t& h = c.head[k];
    const long D = h.dim, F = h.intermediate_dim, Din = c.ssl.d_model;
    const std::string hw = std::string(who) + " (head " + std::to_string(k) + ")";
    auto numel = [&](const std::string& key, long n, int max_dim) {
        const svc_tensor_desc_t* d = sd.get(key);
        if (!d) { set_error(hw + ": state_dict is missing " + key); return 1; }
        if (StateDict::numel(d) != n || d->ndim > max_dim) { set_error(hw + ": shape mismatch for " + key); return 1; }
        return 0;
    };
    const svc_tensor_desc_t* ip = sd.get("encoder.input_projection.weight");
    if (!ip) { set_error(hw + ": state_dict is missing encoder.input_projection.weight"); return 1; }
    if (!((ip->ndim == 2 || (ip->ndim == 3 && ip->shape[2] == 1)) && ip->shape[0] == D && ip->shape[1] == Din)) {
        set_error(hw + ": shape mismatch for encoder.input_projection.weight (expected (dim, d_model) or (dim, d_model, 1))");
        return 1;
    }
    if (require_shape(sd.get("encoder.input_projection.bias"), "encoder.input_projection.bias", {D}, hw)) return 1;
    for (int i = 0; i < h.n_blocks; ++i) {
        const std::string p = "encoder.blocks." + std::to_string(i) + ".";
        if (require_shape(sd.get(p + "dwconv.weight"), p + "dwconv.weight", {D, 1, AS_DW_K}, hw) || require_shape(sd.get(p + "dwconv.bias"), p + "dwconv.bias", {D}, hw) ||
            require_shape(sd.get(p + "norm.weight"), p + "norm.weight", {D}, hw) || require_shape(sd.get(p + "norm.bias"), p + "norm.bias", {D}, hw) ||
            require_shape(sd.get(p + "pwconv1.weight"), p + "pwconv1.weight", {F, D}, hw) || require_shape(sd.get(p + "pwconv1.bias"), p + "pwconv1.bias", {F}, hw) ||
            numel(p + "grn.gamma", F, 3) || numel(p + "grn.beta", F, 3) ||
            require_shape(sd.get(p + "pwconv2.weight"), p + "pwconv2.weight", {D, F}, hw) || require_shape(sd.get(p + "pwconv2.bias"), p + "pwconv2.bias", {D}, hw))
            return 1;
    }
    return require_shape(sd.get("quantizer.project_in.weight"), "quantizer.project_in.weight", {h.bits, D}, hw) ||
           require_shape(sd.get("quantizer.project_in.bias"), "quantizer.project_in.bias", {h.bits}, hw);
}

template <typename F>
int as_dispatch_nmax(int C, F f) { return C <= 512 ? f(std::integral_constant<int, 8>()) : f(std::integral_constant<int, 32>()); }

}  // namespace

int svc_astral::pack_head(int k, const StateDict& sd, hipStream_t st) {
    Head& h = heads[k];
    h.c = cfg.head[k];
    const int D = h.c.dim, F = h.c.intermediate_dim, Din = cfg.ssl.d_model;
    auto get = [&](const std::string& key) { return sd.get(key)->data; };            // every key was checked by the caller
    if (pack_lin(dt, wts, get("encoder.input_projection.weight"), get("encoder.input_projection.bias"), D, Din, nullptr, &h.inp, st)) return 1;
    h.blocks.resize(h.c.n_blocks);
    for (int i = 0; i < h.c.n_blocks; ++i) {
        Block& b = h.blocks[i];
        const std::string p = "encoder.blocks." + std::to_string(i) + ".";
        if (!(b.dw = wts.alloc_n<float>((size_t)AS_DW_K * D, st))) return 1;
        if (pack_f32_launch(get(p + "dwconv.weight"), b.dw, AS_DW_K, D, 1, 1, AS_DW_K, 0, D, 1, 0, nullptr, st)) return 1;      // [D][1][7] -> [7][D]
        if (!(b.dwb = copy_f32(get(p + "dwconv.bias"), D, wts, st)) || !(b.ng = copy_f32(get(p + "norm.weight"), D, wts, st)) ||
            !(b.nb = copy_f32(get(p + "norm.bias"), D, wts, st)) || !(b.gamma = copy_f32(get(p + "grn.gamma"), F, wts, st)) ||
            !(b.beta = copy_f32(get(p + "grn.beta"), F, wts, st)))
            return 1;
        if (pack_lin(dt, wts, get(p + "pwconv1.weight"), get(p + "pwconv1.bias"), F, D, nullptr, &b.pw1, st)) return 1;
        if (pack_lin(dt, wts, get(p + "pwconv2.weight"), get(p + "pwconv2.bias"), D, F, nullptr, &b.pw2, st)) return 1;
    }
    if (!(h.pin_w = copy_f32(get("quantizer.project_in.weight"), (long)h.c.bits * D, wts, st)) ||
        !(h.pin_b = copy_f32(get("quantizer.project_in.bias"), h.c.bits, wts, st)))
        return 1;
    return 0;
}

int svc_astral::reserve(int G, int P, hipStream_t st) {
    if (G <= cap_g && P <= cap_p) return 0;
    G = std::max(G, cap_g); P = std::max(P, cap_p);
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws.release();
    cap_g = 0; cap_p = 0;
    long Dm = 0, Fm = 0;
    for (int k = 0; k < cfg.n_heads; ++k) { Dm = std::max<long>(Dm, cfg.head[k].dim); Fm = std::max<long>(Fm, cfg.head[k].intermediate_dim); }
    const long MP = (long)G * P;
    SVC_REQUIRE(MP * std::max<long>(Fm, cfg.ssl.d_model) < (1L << 31), "astral: the window group is too large for 32-bit row offsets");
    for (int k = 0; k < cfg.n_heads; ++k)
        if (!(heads[k].x = ws.alloc_n<float>((size_t)MP * cfg.head[k].dim, st))) return 1;
    nrm = ws.alloc((size_t)MP * Dm * esize(dt), st);
    y = ws.alloc((size_t)MP * Fm * esize(dt), st);
    part = ws.alloc_n<float>((size_t)G * cdiv(P, AS_TILE) * Fm, st);
    fac = ws.alloc_n<float>((size_t)G * Fm, st);
    idx = ws.alloc_n<int>((size_t)AS_MAX_HEADS * MP, st);
    if (!nrm || !y || !part || !fac || !idx) return 1;
    if (dt == 0 && !(h16 = ws.alloc_n<half_t>((size_t)MP * cfg.ssl.d_model, st))) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    cap_g = G; cap_p = P;
    return 0;
}

int svc_astral::put_rows(const int* rows, int G, hipStream_t st) {
    RowTab t;
    memset(&t, 0, sizeof(t));
    for (int g = 0; g < G; ++g) t.v[g] = rows[g];
    hipLaunchKernelGGL(as_rows_kernel, dim3(1), dim3(64), 0, st, t, hrows);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// per block six launches: dwconv + LayerNorm, pwconv1 + GELU, GRN partials, GRN factor, GRN apply, pwconv2 + residual
int svc_astral::convnext_group(int k, const float* h, int G, int P, hipStream_t st) {
    const Head& hd = heads[k];
    const int D = hd.c.dim, F = hd.c.intermediate_dim, Din = cfg.ssl.d_model, n_tiles = cdiv(P, AS_TILE);
    const long MP = (long)G * P;
    const bool f16 = dt == 0;
    if (f16 && cast_rows_launch(h, Din, h16, Din, (int)MP, Din, st)) return 1;
    if (linear_launch(dt, hd.inp, f16 ? (const void*)h16 : (const void*)h, Din, MP, P, KG_ACT_NONE, nullptr, hd.x, nullptr, st)) return 1;
    for (const Block& b : hd.blocks) {
        as_dispatch_nmax(D, [&](auto nmax) {
            constexpr int N = decltype(nmax)::value;
            if (f16) hipLaunchKernelGGL((as_dwln_kernel<N, half_t>), dim3(cdiv(P, 4), G), dim3(256), 0, st, (const float*)hd.x, (const float*)b.dw, (const float*)b.dwb,
                                        (const float*)b.ng, (const float*)b.nb, (half_t*)nrm, (const int*)hrows, P, D, 1e-6f);
            else hipLaunchKernelGGL((as_dwln_kernel<N, float>), dim3(cdiv(P, 4), G), dim3(256), 0, st, (const float*)hd.x, (const float*)b.dw, (const float*)b.dwb,
                                    (const float*)b.ng, (const float*)b.nb, (float*)nrm, (const int*)hrows, P, D, 1e-6f);
            return 0;
        });
        SVC_CHECK_HIP(hipGetLastError());
        if (linear_launch(dt, b.pw1, nrm, D, MP, P, KG_ACT_GELU, nullptr, f16 ? nullptr : (float*)y, f16 ? (half_t*)y : nullptr, st)) return 1;
        const dim3 pg(n_tiles, cdiv(F, 256), G);
        if (f16) {
            hipLaunchKernelGGL(as_grn_part_kernel<half_t>, pg, dim3(256), 0, st, (const half_t*)y, part, (const int*)hrows, P, F, n_tiles);
            hipLaunchKernelGGL(as_grn_fac_kernel, dim3(G), dim3(256), 0, st, (const float*)part, (const float*)b.gamma, fac, (const int*)hrows, F, n_tiles);
            hipLaunchKernelGGL((as_grn_apply_kernel<half_t, 8>), dim3(cdiv(P, 4), G), dim3(256), 0, st, (half_t*)y, (const float*)fac, (const float*)b.beta, (const int*)hrows, P, F);
        } else {
            hipLaunchKernelGGL(as_grn_part_kernel<float>, pg, dim3(256), 0, st, (const float*)y, part, (const int*)hrows, P, F, n_tiles);
            hipLaunchKernelGGL(as_grn_fac_kernel, dim3(G), dim3(256), 0, st, (const float*)part, (const float*)b.gamma, fac, (const int*)hrows, F, n_tiles);
            hipLaunchKernelGGL((as_grn_apply_kernel<float, 4>), dim3(cdiv(P, 4), G), dim3(256), 0, st, (float*)y, (const float*)fac, (const float*)b.beta, (const int*)hrows, P, F);
        }
        SVC_CHECK_HIP(hipGetLastError());
        if (linear_launch(dt, b.pw2, y, F, MP, P, KG_ACT_NONE, hd.x, hd.x, nullptr, st)) return 1;
    }
    return 0;
}

int svc_astral::bsq_group(int k, const float* x, int G, int P, int* index, float* z, hipStream_t st) {
    const Head& hd = heads[k];
    as_dispatch_nmax(hd.c.dim, [&](auto nmax) {
        hipLaunchKernelGGL(as_bsq_kernel<decltype(nmax)::value>, dim3(cdiv(P, 4), G), dim3(256), 0, st, x, (const float*)hd.pin_w, (const float*)hd.pin_b, index, z,
                           (const int*)hrows, P, hd.c.dim, hd.c.bits);
        return 0;
    });
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

namespace {

// the checks the row seams share; `rows` against T, B against the batch limit, before the handle is touched
int as_seam_check(const svc_astral_t* m, int k, const void* in, const int32_t* rows, int B, int T, const void* out, const char* who) {
    const std::string w(who);
    if (!rows) { set_error(w + ": rows is NULL"); return 1; }
    if (B < 1 || B > WV_MAX_B) { set_error(w + ": B must be 1 .. 64 clips"); return 1; }
    if (T < 1) { set_error(w + ": T must be at least 1 row"); return 1; }
    for (int b = 0; b < B; ++b)
        if (rows[b] < 1 || rows[b] > T) { set_error(w + ": rows outside [1, T]"); return 1; }
    if (!in || !out) { set_error(w + ": null input or output"); return 1; }
    if (!m) { set_error(w + ": null handle"); return 1; }
    if (k < 0 || k >= m->cfg.n_heads) { set_error(w + ": head outside [0, n_heads)"); return 1; }
    return 0;
}

int as_reduce_launch(const int* tokens, const int32_t* rows, int B, int R, int* out, int* counts, hipStream_t st) {
    for (int b0 = 0; b0 < B; b0 += MAX_WIN) {
        const int nb = std::min(MAX_WIN, B - b0);
        RowTab t;
        memset(&t, 0, sizeof(t));
        for (int b = 0; b < nb; ++b) t.v[b] = rows[b0 + b];
        hipLaunchKernelGGL(as_reduce_kernel, dim3(nb), dim3(256), 0, st, tokens, t, b0, R, out, counts);
    }
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int svc_astral_create(const svc_astral_config_t* cfg, const svc_tensor_desc_t* ssl_weights, int n_ssl_weights,
                      const svc_tensor_desc_t* const* head_weights, const int* n_head_weights, void* stream, svc_astral_t** out) {
    const char* who = "svc_astral_create";
    SVC_REQUIRE(cfg && ssl_weights && head_weights && n_head_weights && out, "svc_astral_create: null argument");
    if (as_check_cfg(cfg, who)) return 1;
    for (int k = 0; k < cfg->n_heads; ++k) SVC_REQUIRE(head_weights[k] && n_head_weights[k] >= 0, "svc_astral_create: null head weights");
    hipStream_t st = (hipStream_t)stream;
    auto* m = new svc_astral();
    m->cfg = *cfg;
    m->dt = cfg->ssl.precision ? 0 : 1;
    if (w2v_create(&cfg->ssl, nullptr, ssl_weights, n_ssl_weights, stream, false, &m->ssl)) {
        set_error(std::string(who) + ": the SSL front: " + get_error());
        delete m;
        return 1;
    }
    for (int k = 0; k < cfg->n_heads; ++k) {
        StateDict sd(head_weights[k], n_head_weights[k]);
        if (as_check_head(*cfg, k, sd, who) || m->pack_head(k, sd, st)) { delete m; return 1; }
    }
    if (!(m->hrows = m->wts.alloc_n<int>(MAX_WIN, st)) || hipStreamSynchronize(st) != hipSuccess) { delete m; set_error("svc_astral_create: allocation failed"); return 1; }
    *out = m;
    return 0;
}

void svc_astral_destroy(svc_astral_t* m) { delete m; }

int svc_astral_n_windows(const svc_astral_config_t* cfg, int overlap_rows, long n_samples) {
    if (as_plan_check(cfg, overlap_rows, n_samples, "svc_astral_n_windows")) return -1;
    const long nw = window_count(cfg->ssl.window_samples, (long)overlap_rows * SAMPLES_PER_ROW, n_samples);
    if (nw > 0x7fffffffL) { set_error("svc_astral_n_windows: n_samples is too large"); return -1; }
    return (int)nw;
}

int svc_astral_rows(const svc_astral_config_t* cfg, int overlap_rows, long n_samples) {
    if (as_plan_check(cfg, overlap_rows, n_samples, "svc_astral_rows")) return -1;
    const long W = cfg->ssl.window_samples, O = (long)overlap_rows * SAMPLES_PER_ROW, nw = window_count(W, O, n_samples);
    long rows = 0;
    for (long j = 0; j < nw; ++j) rows += std::max(0L, as_rows_of(cfg->ssl, std::min(W, n_samples - j * (W - O))) - (j ? overlap_rows : 0));
    if (rows > 0x7fffffffL) { set_error("svc_astral_rows: n_samples is too large"); return -1; }
    return (int)rows;
}

int svc_astral_set_window_group(svc_astral_t* m, int windows) {
    SVC_REQUIRE(windows >= 0 && windows <= MAX_WIN, "svc_astral_set_window_group: windows must be 0 (default) .. 64");
    SVC_REQUIRE(m, "svc_astral_set_window_group: null handle");
    m->group = windows ? windows : WV_DEFAULT_GROUP;
    return svc_w2v_set_window_group(m->ssl, windows);
}

int svc_astral_set_timing(svc_astral_t* m, int on) {
    SVC_REQUIRE(m, "svc_astral_set_timing: null handle");
    m->tm.on = on != 0;
    return 0;
}

int svc_astral_last_timing(svc_astral_t* m, float* ms4) {
    const char* msg = "svc_astral_last_timing: timing is off or no svc_astral_tokens call was made";
    SVC_REQUIRE(m, msg);
    return m->tm.last(ms4, msg);
}

}  // extern "C"

namespace {

// One window group of the SSL front: windows wt[0 .. nb) of `wave` -> m->ssl->stack.x [nb][P][Dssl] (the residual stream after the
// last layer, where the stack leaves it), and the head's rows per window min(frames(n), n / 320) in m->hrows
int as_ssl_group(svc_astral_t* m, const float* wave, long L, const WinTab& wt, int nb, int P, hipStream_t st) {
    svc_w2v* s = m->ssl;
    const svc_w2v_config_t& c = s->cfg;
    const int nc = c.n_conv;
    LenTab lt;
    memset(&lt, 0, sizeof(lt));
    int hr[MAX_WIN];
    for (int g = 0; g < nb; ++g) {
        for (int l = 0; l <= nc; ++l) lt.v[l][g] = (int)wv_frames(c, wt.n[g], l);
        hr[g] = (int)as_rows_of(c, wt.n[g]);
    }
    if (s->put_lens(lt, st) || m->put_rows(hr, nb, st)) return 1;
    if (s->normalize_group(wave, L, wt, nb, s->wn, s->nstride, st)) return 1;
    if (s->features_group(s->wn, s->nstride, nb, st)) return 1;
    return s->encode_group(s->h32, s->h16, nb, P, nullptr, st);
}

}  // namespace

extern "C" {

int svc_astral_ssl(svc_astral_t* m, const float* wave, const int32_t* lens, int B, int L, float* out, int T, void* stream) {
    SVC_REQUIRE(lens != nullptr, "svc_astral_ssl: lens is NULL");
    SVC_REQUIRE(B >= 1 && B <= WV_MAX_B, "svc_astral_ssl: B must be 1 .. 64 clips");
    SVC_REQUIRE(L >= 1 && T >= 1, "svc_astral_ssl: L and T must be at least 1");
    for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 1 && lens[b] <= L, "svc_astral_ssl: lens outside [1, L]");
    SVC_REQUIRE(wave && out, "svc_astral_ssl: null wave or out");
    SVC_REQUIRE(m, "svc_astral_ssl: null handle");
    const svc_w2v_config_t& c = m->ssl->cfg;
    long nmax = 0;
    for (int b = 0; b < B; ++b) {
        SVC_REQUIRE(lens[b] <= c.window_samples, "svc_astral_ssl: one window per clip (lens must not exceed window_samples)");
        const long r = as_rows_of(c, lens[b]);
        SVC_REQUIRE(r >= 1, "svc_astral_ssl: lens shorter than the extractor's receptive field");
        SVC_REQUIRE(r <= T, "svc_astral_ssl: T is smaller than the longest clip's rows (svc_astral_rows)");
        nmax = std::max<long>(nmax, lens[b]);
    }
    hipStream_t st = (hipStream_t)stream;
    const int G = std::min(m->group, B), D = c.d_model;
    if (m->ssl->reserve_fe(G, nmax, st)) return 1;
    const int P = m->ssl->Ls[c.n_conv];
    if (m->ssl->reserve_enc(G, P, st)) return 1;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = std::min(G, B - b0);
        WinTab wt;
        memset(&wt, 0, sizeof(wt));
        for (int g = 0; g < nb; ++g) { wt.clip[g] = b0 + g; wt.n[g] = lens[b0 + g]; }
        if (as_ssl_group(m, wave, L, wt, nb, P, st)) return 1;
        if (copy_rows_launch(m->ssl->stack.x, P, out + (long)b0 * T * D, T, m->hrows, nb, std::min(P, T), D, st)) return 1;
    }
    return 0;
}

int svc_astral_convnext(svc_astral_t* m, int head, const float* h, const int32_t* rows, int B, int T, float* x, void* stream) {
    if (as_seam_check(m, head, h, rows, B, T, x, "svc_astral_convnext")) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int G = std::min(m->group, B), Din = m->cfg.ssl.d_model, D = m->cfg.head[head].dim;
    if (m->reserve(G, T, st)) return 1;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = std::min(G, B - b0);
        if (m->put_rows(rows + b0, nb, st)) return 1;
        if (m->convnext_group(head, h + (long)b0 * T * Din, nb, T, st)) return 1;
        if (copy_rows_launch(m->heads[head].x, T, x + (long)b0 * T * D, T, m->hrows, nb, T, D, st)) return 1;
    }
    return 0;
}

int svc_astral_logits(svc_astral_t* m, int head, const float* x, const int32_t* rows, int B, int T, float* z, void* stream) {
    if (as_seam_check(m, head, x, rows, B, T, z, "svc_astral_logits")) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int D = m->cfg.head[head].dim, bits = m->cfg.head[head].bits;
    for (int b0 = 0; b0 < B; b0 += MAX_WIN) {
        const int nb = std::min(MAX_WIN, B - b0);
        if (m->put_rows(rows + b0, nb, st)) return 1;
        if (m->bsq_group(head, x + (long)b0 * T * D, nb, T, nullptr, z + (long)b0 * T * bits, st)) return 1;
    }
    return 0;
}

int svc_op_bsq_index(const float* z, int32_t* index, long rows, int bits, void* stream) {
    SVC_REQUIRE(rows >= 0 && bits >= 1 && bits <= AS_MAX_BITS, "svc_op_bsq_index: rows must not be negative, bits 1 .. 16");
    SVC_REQUIRE(rows < (1L << 31), "svc_op_bsq_index: too many rows");
    if (rows == 0) return 0;
    SVC_REQUIRE(z && index, "svc_op_bsq_index: null argument");
    hipLaunchKernelGGL(as_index_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0, (hipStream_t)stream, z, index, rows, bits);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int svc_tokens_reduce(const int32_t* tokens, const int32_t* rows, int B, int R, int32_t* out, int32_t* counts, void* stream) {
    SVC_REQUIRE(rows != nullptr, "svc_tokens_reduce: rows is NULL");
    SVC_REQUIRE(B >= 1 && R >= 1, "svc_tokens_reduce: B and R must be at least 1");
    for (int b = 0; b < B; ++b) SVC_REQUIRE(rows[b] >= 0 && rows[b] <= R, "svc_tokens_reduce: rows outside [0, R]");
    SVC_REQUIRE(tokens && out && counts, "svc_tokens_reduce: null tokens, out or counts");
    SVC_REQUIRE(out + (long)B * R <= tokens || tokens + (long)B * R <= out, "svc_tokens_reduce: tokens and out must not overlap");
    return as_reduce_launch(tokens, rows, B, R, out, counts, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// The one code path of svc_astral_tokens and svc_astral_tokens_heads; full: every head, whatever their number (the mask is not read)
int as_tokens(const char* who, svc_astral_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, bool full,
              unsigned head_mask, int32_t* tokens, int Rmax, int reduce_head, int32_t* reduced, int32_t* counts, void* stream) {
    const std::string w(who);
#define AS_REQ(cond, msg) do { if (!(cond)) { set_error(w + msg); return 1; } } while (0)
    AS_REQ(B >= 1 && B <= WV_MAX_B, ": B must be 1 .. 64 clips");
    AS_REQ(L >= 1, ": L must be at least 1 sample");
    if (lens)
        for (int b = 0; b < B; ++b) AS_REQ(lens[b] >= 1 && lens[b] <= L, ": lens outside [1, L]");
    AS_REQ(overlap_rows >= 0, ": overlap_rows outside [0, window_samples / 320)");
    AS_REQ(Rmax >= 1, ": Rmax is smaller than the longest clip's rows (svc_astral_rows)");
    AS_REQ(wave && tokens, ": null wave or tokens");
    AS_REQ(reduce_head < 0 || (reduced && counts), ": reduce_head needs reduced and counts");
    AS_REQ(full || (head_mask != 0 && head_mask < (1u << AS_MAX_HEADS)), ": head_mask must be non-zero and inside (1 << n_heads) - 1");
    AS_REQ(m, ": null handle");
    const int nh = m->cfg.n_heads;
    if (full) head_mask = (1u << nh) - 1u;
    AS_REQ(head_mask < (1u << nh), ": head_mask must be non-zero and inside (1 << n_heads) - 1");
    AS_REQ(reduce_head < nh, ": reduce_head outside [-1, n_heads)");
    AS_REQ(reduce_head < 0 || (head_mask >> reduce_head & 1u), ": reduce_head is not a selected head");
    HeadMap hm;
    memset(&hm, 0, sizeof(hm));
    int np = 0, reduce_plane = -1;                           // selected heads in ascending order: plane p holds head hm.v[p]
    for (int k = 0; k < nh; ++k)
        if (head_mask >> k & 1u) {
            if (k == reduce_head) reduce_plane = np;
            hm.v[np++] = k;
        }
    AS_REQ(reduce_head < 0 || reduced + (long)B * Rmax <= tokens || tokens + (long)np * B * Rmax <= reduced, ": reduced must not overlap tokens");
    const svc_w2v_config_t& c = m->ssl->cfg;
    const int nc = c.n_conv;
    const long W = c.window_samples;
    AS_REQ((long)overlap_rows * SAMPLES_PER_ROW < W, ": overlap_rows outside [0, window_samples / 320)");
    std::vector<Win> wins;                                   // the window plan of the whole call, in clip order
    int clip_rows[WV_MAX_B];
    for (int b = 0; b < B; ++b) {
        const long n = lens ? lens[b] : L;
        AS_REQ(as_rows_of(c, std::min(n, W)) >= 1, ": lens shorter than the extractor's receptive field");
        clip_rows[b] = plan_clip(wins, b, n, W, overlap_rows, [&c](long ns) { return as_rows_of(c, ns); });
        AS_REQ(clip_rows[b] <= Rmax, ": Rmax is smaller than the longest clip's rows (svc_astral_rows)");
    }
#undef AS_REQ
    long nmax = 0;
    for (const Win& wn : wins) nmax = std::max<long>(nmax, wn.n);
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)std::min((size_t)m->group, wins.size());
    if (m->ssl->reserve_fe(G, nmax, st)) return 1;
    const int P = m->ssl->Ls[nc];                            // this call's rows per window
    if (m->ssl->reserve_enc(G, P, st) || m->reserve(G, P, st)) return 1;
    for (size_t w0 = 0; w0 < wins.size(); w0 += G) {
        const int nb = (int)std::min((size_t)G, wins.size() - w0);
        const WinTab wt = win_table(wins, w0, nb);
        if (m->tm.mark(0, st)) return 1;
        if (as_ssl_group(m, wave, L, wt, nb, P, st) || m->tm.mark(1, st)) return 1;
        for (int p = 0; p < np; ++p)                         // every selected head on the group's SSL rows before the workspace is reused
            if (m->convnext_group(hm.v[p], m->ssl->stack.x, nb, P, st)) return 1;
        if (m->tm.mark(2, st)) return 1;
        for (int p = 0; p < np; ++p)
            if (m->bsq_group(hm.v[p], m->heads[hm.v[p]].x, nb, P, m->idx + (long)hm.v[p] * m->cap_g * m->cap_p, nullptr, st)) return 1;
        if (m->tm.mark(3, st)) return 1;
        hipLaunchKernelGGL(as_assemble_kernel, dim3(cdiv(P + Rmax, 256), nb, np), dim3(256), 0, st, (const int*)m->idx, wt, tokens, P, nb, B, Rmax,
                           (long)m->cap_g * m->cap_p, hm);
        SVC_CHECK_HIP(hipGetLastError());
        if (m->tm.mark(4, st)) return 1;
    }
    if (reduce_plane >= 0) return as_reduce_launch(tokens + (long)reduce_plane * B * Rmax, clip_rows, B, Rmax, reduced, counts, st);
    return 0;
}

}  // namespace

extern "C" {

int svc_astral_tokens(svc_astral_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, int32_t* tokens, int Rmax,
                      int reduce_head, int32_t* reduced, int32_t* counts, void* stream) {
    return as_tokens("svc_astral_tokens", m, wave, lens, B, L, overlap_rows, true, 0u, tokens, Rmax, reduce_head, reduced, counts, stream);
}

int svc_astral_tokens_heads(svc_astral_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, unsigned head_mask,
                            int32_t* tokens, int Rmax, int reduce_head, int32_t* reduced, int32_t* counts, void* stream) {
    return as_tokens("svc_astral_tokens_heads", m, wave, lens, B, L, overlap_rows, false, head_mask, tokens, Rmax, reduce_head, reduced, counts,
                     stream);
}

}  // extern "C"
