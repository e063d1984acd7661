// Whisper content encoder for gfx950: 16 kHz audio -> content features at 50 rows/s (`semantic_fn` of the reference drivers:
// WhisperFeatureExtractor + the encoder half of openai/whisper-small in float16, one 30 s window at a time).
//
// Three stages.  Log-mel: the window's samples zero-padded to W = 320 P, reflect padding of 200 on the padded window, the
// STFT (n_fft 400, hop 160, periodic Hann) as one fp32 tap-GEMM over overlapping signal rows, power, the caller's mel basis,
// log10, the clamp to the window's own maximum - 8 (a reduction of its own: per-block maxima, then every thread folds
// them; no atomics) and (x + 4) / 4.  Encoder: conv1 + GELU, conv2 (stride 2) + GELU, + positions, n_layers pre-LN blocks
// (q/k/v in one GEMM with the 1/8 and the attention's log2(e) folded into the q rows, fp16 rows for the attention, a small
// transpose for V^T), final LayerNorm.  Residual stream, LayerNorm statistics and softmax are fp32; convs and linears run on
// the fp16 tap-GEMM (precision 1) or the fp32 one (precision 0).  Windows of long clips: a table (clip, start, samples) of
// up to 64 windows travels as a kernel argument; no window is copied out of its clip, nothing above a clip's end is read,
// and one kernel gathers the kept rows.  Every window is computed as if alone: its bits do not depend on its companions,
// their order or the group size (the GEMMs keep each element's k order in every tile form, the attention form is pinned
// per handle, everything else is row-local).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "model_util.h"

using namespace svc;

namespace {

constexpr int WH_NFFT = 400, WH_HOP = 160, WH_PAD = WH_NFFT / 2, WH_NB = WH_NFFT / 2 + 1, WH_KP = 416 /* n_fft padded to k-tiles */;
constexpr int WH_SPR = 320;                       // samples per output row (hop 160, conv2 stride 2)
constexpr int WH_MAX_WIN = 64, WH_MAX_B = 64, WH_NBLK = 64, WH_DEFAULT_GROUP = 16;
constexpr float WH_QSCALE = 0.125f * 1.4426950408889634f;     // 1 / sqrt(64), and the attention kernel's exp2

struct WinTab {                                   // one group of windows as a kernel argument
    int clip[WH_MAX_WIN], start[WH_MAX_WIN], n[WH_MAX_WIN];           // source clip, first sample, samples (1 .. W)
    int dst0[WH_MAX_WIN], drop[WH_MAX_WIN], keep[WH_MAX_WIN];         // assemble: rows [drop, keep) go to out[clip][dst0 ...]
    int zero_from[WH_MAX_WIN];                                        // last window of its clip: the clip's row count; else -1
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// window g zero-padded to W samples, then center=True reflect padding of n_fft / 2 on the PADDED window: dst [G][stride]
__global__ void wh_pad_kernel(const float* __restrict__ wave, WinTab wt, long Lrow, float* __restrict__ dst, long stride, int W) {
    const int g = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= stride) return;
    float v = 0.f;
    if (i < (long)W + 2 * WH_PAD) {
        long q = i - WH_PAD;
        q = q < 0 ? -q : (q >= W ? 2L * (W - 1) - q : q);
        if (q < wt.n[g]) v = wave[(long)wt.clip[g] * Lrow + wt.start[g] + q];
    }
    dst[(long)g * stride + i] = v;
}

// spec [M][ld_s] = (re | im) -> pw [M][ld_p] = re^2 + im^2, pad columns zero
__global__ void wh_power_kernel(const float* __restrict__ spec, long ld_s, float* __restrict__ pw, long ld_p) {
    const long m = blockIdx.x;
    const int k = threadIdx.x;
    if (k >= ld_p) return;
    float v = 0.f;
    if (k < WH_NB) {
        const float re = spec[m * ld_s + k], im = spec[m * ld_s + WH_NB + k];
        v = re * re + im * im;
    }
    pw[m * ld_p + k] = v;
}

// c [G * NF][ldc] -> log10(max(c, 1e-10)) in place; part[g][blk] = the block's maximum (blocks without frames: -inf)
__global__ __launch_bounds__(256) void wh_log_kernel(float* __restrict__ c, long ldc, int n_mels, int NF, float* __restrict__ part) {
    __shared__ float red[4];
    const int g = blockIdx.y, blk = blockIdx.x;
    const int fpb = (NF + WH_NBLK - 1) / WH_NBLK, f0 = blk * fpb, f1 = min(NF, f0 + fpb);
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < (f1 - f0) * n_mels; i += 256) {
        const int f = f0 + i / n_mels, j = i % n_mels;
        float* p = c + ((long)g * NF + f) * ldc + j;
        const float x = *p;
        const float v = fmaxf(x > 1e-10f ? log10f(x) : -10.f, -10.f);
        *p = v;
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) part[g * WH_NBLK + blk] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// out[g][mel][f] = (max(c[g * NF + f][mel], m_g - 8) + 4) / 4, m_g = the window's maximum
__global__ void wh_norm_kernel(const float* __restrict__ c, long ldc, const float* __restrict__ part, float* __restrict__ out, int n_mels,
                               int NF) {
    const int g = blockIdx.z, j = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= NF) return;
    float m = -INFINITY;
    for (int i = 0; i < WH_NBLK; ++i) m = fmaxf(m, part[g * WH_NBLK + i]);
    out[((long)g * n_mels + j) * NF + f] = (fmaxf(c[((long)g * NF + f) * ldc + j], m - 8.f) + 4.f) * 0.25f;
}

// affine LayerNorm, one wave per row, the row in registers: mean, then the variance about it (two passes), fp32
__global__ __launch_bounds__(256) void wh_layernorm_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y32, long ldy32,
                                                           half_t* __restrict__ y16, long ldy16, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int rows, int D, float eps) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, n = D / 64;
    if (row >= rows) return;
    const float* xr = x + row * ldx;
    float v[32], s = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) { v[i] = xr[lane + 64 * i]; s += v[i]; }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) { const float d = v[i] - mean; q = fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) {
            const int c = lane + 64 * i;
            const float o = (v[i] - mean) * rstd * gamma[c] + beta[c];
            if (y32) y32[row * ldy32 + c] = o;
            if (y16) y16[row * ldy16 + c] = (half_t)o;
        }
}

// x [G][P][D] += pos [P][D]
__global__ void wh_add_pos_kernel(float* __restrict__ x, const float* __restrict__ pos, long PD4, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    float4 a = reinterpret_cast<float4*>(x)[i];
    const float4 b = reinterpret_cast<const float4*>(pos)[i % PD4];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4*>(x)[i] = a;
}

// V columns of qkv [G * P][3 D] (fp16) -> vt [G][D][vt_ld] in the attention's column order; columns at and above P stay zero
__global__ __launch_bounds__(256) void wh_vt_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ vt, int P, int D, long vt_ld, int mode) {
    __shared__ half_t tile[32][34];
    const int g = blockIdx.z, p0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + i;
        tile[i][tx] = p < P ? qkv[((long)g * P + p) * 3 * D + 2 * D + d0 + tx] : (half_t)0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int p = p0 + tx;
        if (p < P) vt[((long)g * D + d0 + i) * vt_ld + vt_pos(p, mode)] = tile[tx][i];
    }
}

// enc [G][P][D] -> out [B][Rmax][D]: block (r, g).  r < P: row r of window g, when kept, goes to its place in the clip's rows;
// r >= P: row r - P of the clip is zeroed when window g is the clip's last and the row is at or above the clip's count
__global__ void wh_assemble_kernel(const float* __restrict__ enc, WinTab wt, float* __restrict__ out, int P, int D, int Rmax) {
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

KGemmParams wh_gemm(long M, int N, int Lout) {
    KGemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = (int)M; p.N = N; p.Lout = Lout; p.a_seq_rows = Lout; p.c_seq_rows = Lout; p.a_stride = 1; p.a_len = Lout; p.n_taps = 1;
    p.vec_ok = 1;
    return p;
}

// the drivers' window plan of a clip of n samples: number of windows (>= 1)
long wh_n_windows(long W, long O, long n) { return n <= W ? 1 : 1 + (n - W + (W - O) - 1) / (W - O); }

int wh_layernorm_launch(const float* x, long ldx, float* y32, long ldy32, half_t* y16, long ldy16, const float* gamma, const float* beta,
                        long rows, int D, float eps, hipStream_t st) {
    SVC_REQUIRE(D >= 64 && D % 64 == 0 && D <= 2048, "layernorm: D must be a multiple of 64, at most 2048");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(wh_layernorm_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, ldx, y32, ldy32, y16, ldy16, gamma, beta, (int)rows, D, eps);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

struct svc_whisper {
    svc_whisper_config_t cfg;
    int dt = 0;                      // tap-GEMM dtype of the convs and linears: 0 fp16 (precision 1), 1 fp32 (precision 0)
    int W = 0, NF = 0;               // samples and mel frames of a window
    int group = WH_DEFAULT_GROUP, qt_form = 1;
    long cin_ld = 0, ld_fb = 0, ld_c = 0, ld_s = 0, stride = 0, vt_ld = 0;
    Arena wts, ws;
    struct Lin { void* w = nullptr; float* b = nullptr; long ldw = 0; int N = 0; };
    struct Layer { Lin qkv, o, fc1, fc2; float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; };
    Lin conv1, conv2;
    std::vector<Layer> layers;
    float *pos = nullptr, *gf = nullptr, *bf = nullptr, *dft = nullptr, *fb = nullptr;
    // workspace for `cap` windows
    int cap = 0;
    float *padded = nullptr, *spec = nullptr, *pw = nullptr, *melc = nullptr, *part = nullptr, *feat = nullptr, *enc = nullptr;
    float *xin32 = nullptr, *h32 = nullptr, *x = nullptr, *n32 = nullptr, *ao32 = nullptr, *ff32 = nullptr;
    half_t *xin16 = nullptr, *h16 = nullptr, *n16 = nullptr, *qkv16 = nullptr, *vt = nullptr, *ao16 = nullptr, *ff16 = nullptr;
    // measurement aid: events around the stages of the last group of the last call
    bool timing = false;
    hipEvent_t ev[5] = {};
    ~svc_whisper() {
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    }
    int mark(int i, hipStream_t st) {
        if (!timing) return 0;
        if (!ev[i]) SVC_CHECK_HIP(hipEventCreate(&ev[i]));
        SVC_CHECK_HIP(hipEventRecord(ev[i], st));
        return 0;
    }
    int pack_lin(const float* w, const float* bias, int N, int K, Lin* out, hipStream_t st);
    int pack_conv(const float* w, const float* bias, int N, int Cin, long cin_pad, Lin* out, hipStream_t st);
    int pack(const StateDict& sd, const std::string& pre, const float* mel_basis, hipStream_t st);
    int reserve(int G, hipStream_t st);
    int lin(const Lin& l, const void* a, long K, long M, int Lout, int act, const float* res, float* c32, half_t* c16, hipStream_t st);
    int mel_group(const float* wave, long Lrow, const WinTab& wt, int G, float* out, hipStream_t st);
    int encode_group(const float* feats, int G, float* out, hipStream_t st);
};

namespace {

struct KeyShape { std::string name; std::vector<long> shape; };

std::vector<KeyShape> wh_keys(const svc_whisper_config_t& c) {
    const long D = c.d_model, F = c.ffn_dim;
    std::vector<KeyShape> k = {{"conv1.weight", {D, c.n_mels, 3}}, {"conv1.bias", {D}}, {"conv2.weight", {D, D, 3}}, {"conv2.bias", {D}},
                               {"embed_positions.weight", {c.max_source_positions, D}}};
    for (int i = 0; i < c.n_layers; ++i) {
        const std::string p = "layers." + std::to_string(i) + ".";
        k.push_back({p + "self_attn.k_proj.weight", {D, D}});
        for (const char* n : {"v_proj", "q_proj", "out_proj"}) {
            k.push_back({p + "self_attn." + n + ".weight", {D, D}});
            k.push_back({p + "self_attn." + n + ".bias", {D}});
        }
        k.push_back({p + "self_attn_layer_norm.weight", {D}});
        k.push_back({p + "self_attn_layer_norm.bias", {D}});
        k.push_back({p + "fc1.weight", {F, D}});
        k.push_back({p + "fc1.bias", {F}});
        k.push_back({p + "fc2.weight", {D, F}});
        k.push_back({p + "fc2.bias", {D}});
        k.push_back({p + "final_layer_norm.weight", {D}});
        k.push_back({p + "final_layer_norm.bias", {D}});
    }
    k.push_back({"layer_norm.weight", {D}});
    k.push_back({"layer_norm.bias", {D}});
    return k;
}

int wh_require(const svc_tensor_desc_t* d, const std::string& name, const std::vector<long>& shp) {
    if (!d) { set_error("svc_whisper_create: state_dict is missing " + name); return 1; }
    bool ok = d->ndim == (int)shp.size();
    for (size_t i = 0; ok && i < shp.size(); ++i) ok = d->shape[i] == shp[i];
    if (!ok) { set_error("svc_whisper_create: shape mismatch for " + name); return 1; }
    return 0;
}

float* wh_copy(const float* src, long n, Arena& ar, hipStream_t st) {
    float* p = ar.alloc_n<float>(round_up(n, 8), st);
    if (!p) return nullptr;
    if (hipMemcpyAsync(p, src, (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("weight copy failed"); return nullptr; }
    return p;
}

}  // namespace

// nn.Linear weight [N][K] -> [Npad128][K] in the GEMM's dtype
int svc_whisper::pack_lin(const float* w, const float* bias, int N, int K, Lin* out, hipStream_t st) {
    out->N = N; out->ldw = K;
    out->w = wts.alloc((size_t)round_up(N, 128) * K * esize(dt), st);
    if (!out->w) return 1;
    if (pack_any(dt, w, out->w, 0, N, 1, K, K, 0, 1, K, 0, 1, nullptr, st)) return 1;
    if (bias && !(out->b = wh_copy(bias, N, wts, st))) return 1;
    return 0;
}

// Conv1d weight [N][Cin][3] -> [Npad128][3 * cin_pad], tap-major
int svc_whisper::pack_conv(const float* w, const float* bias, int N, int Cin, long cin_pad, Lin* out, hipStream_t st) {
    out->N = N; out->ldw = 3 * cin_pad;
    out->w = wts.alloc((size_t)round_up(N, 128) * out->ldw * esize(dt), st);
    if (!out->w) return 1;
    for (int t = 0; t < 3; ++t)
        if (pack_any(dt, w + t, out->w, t * cin_pad, N, Cin, 1, 3L * Cin, 3, 0, out->ldw, 1, 0, nullptr, st)) return 1;
    if (!(out->b = wh_copy(bias, N, wts, st))) return 1;
    return 0;
}

int svc_whisper::pack(const StateDict& sd, const std::string& pre, const float* mel_basis, hipStream_t st) {
    const int D = cfg.d_model, F = cfg.ffn_dim, P = cfg.max_source_positions;
    auto get = [&](const std::string& k) { return sd.get(pre + k)->data; };       // every key was checked by the caller
    if (pack_conv(get("conv1.weight"), get("conv1.bias"), D, cfg.n_mels, cin_ld, &conv1, st)) return 1;
    if (pack_conv(get("conv2.weight"), get("conv2.bias"), D, D, D, &conv2, st)) return 1;
    if (!(pos = wh_copy(get("embed_positions.weight"), (long)P * D, wts, st))) return 1;
    float* qs = wts.alloc_n<float>(D, st);
    if (!qs) return 1;
    {
        std::vector<float> h(D, WH_QSCALE);
        SVC_CHECK_HIP(hipMemcpyAsync(qs, h.data(), (size_t)D * 4, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
    }
    layers.resize(cfg.n_layers);
    for (int i = 0; i < cfg.n_layers; ++i) {
        Layer& ly = layers[i];
        const std::string p = "layers." + std::to_string(i) + ".";
        // q | k | v rows of one [3 D][D] weight; the q rows and bias carry 1 / 8 and log2(e), k has no bias
        ly.qkv.N = 3 * D; ly.qkv.ldw = D;
        ly.qkv.w = wts.alloc((size_t)round_up(3 * D, 128) * D * esize(dt), st);
        ly.qkv.b = wts.alloc_n<float>(3 * D, st);
        if (!ly.qkv.w || !ly.qkv.b) return 1;
        if (pack_any(dt, get(p + "self_attn.q_proj.weight"), ly.qkv.w, 0, D, 1, D, D, 0, 1, D, 0, 1, qs, st)) return 1;
        if (pack_any(dt, get(p + "self_attn.k_proj.weight"), ly.qkv.w, (long)D * D, D, 1, D, D, 0, 1, D, 0, 1, nullptr, st)) return 1;
        if (pack_any(dt, get(p + "self_attn.v_proj.weight"), ly.qkv.w, 2L * D * D, D, 1, D, D, 0, 1, D, 0, 1, nullptr, st)) return 1;
        if (pack_f32_launch(get(p + "self_attn.q_proj.bias"), ly.qkv.b, D, 1, 1, 1, 0, 0, 1, 0, 0, qs, st)) return 1;
        SVC_CHECK_HIP(hipMemcpyAsync(ly.qkv.b + 2 * D, get(p + "self_attn.v_proj.bias"), (size_t)D * 4, hipMemcpyDeviceToDevice, st));
        if (pack_lin(get(p + "self_attn.out_proj.weight"), get(p + "self_attn.out_proj.bias"), D, D, &ly.o, st)) return 1;
        if (pack_lin(get(p + "fc1.weight"), get(p + "fc1.bias"), F, D, &ly.fc1, st)) return 1;
        if (pack_lin(get(p + "fc2.weight"), get(p + "fc2.bias"), D, F, &ly.fc2, st)) return 1;
        if (!(ly.g1 = wh_copy(get(p + "self_attn_layer_norm.weight"), D, wts, st)) || !(ly.b1 = wh_copy(get(p + "self_attn_layer_norm.bias"), D, wts, st)) ||
            !(ly.g2 = wh_copy(get(p + "final_layer_norm.weight"), D, wts, st)) || !(ly.b2 = wh_copy(get(p + "final_layer_norm.bias"), D, wts, st)))
            return 1;
    }
    if (!(gf = wh_copy(get("layer_norm.weight"), D, wts, st)) || !(bf = wh_copy(get("layer_norm.bias"), D, wts, st))) return 1;
    {   // periodic Hann window folded into the DFT basis (float64 trigonometry): rows (cos | -sin), n_fft padded to 416 with zeros
        std::vector<float> basis((size_t)round_up(2 * WH_NB, 128) * WH_KP, 0.f);
        for (int k = 0; k < WH_NB; ++k)
            for (int n = 0; n < WH_NFFT; ++n) {
                const double ang = 2.0 * M_PI * (double)((k * n) % WH_NFFT) / (double)WH_NFFT;
                const double hw = 0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)WH_NFFT);
                basis[(size_t)k * WH_KP + n] = (float)(cos(ang) * hw);
                basis[(size_t)(WH_NB + k) * WH_KP + n] = (float)(-sin(ang) * hw);
            }
        dft = wts.alloc_n<float>(basis.size(), st);
        fb = wts.alloc_n<float>((size_t)round_up(cfg.n_mels, 128) * ld_fb, st);
        if (!dft || !fb) return 1;
        SVC_CHECK_HIP(hipMemcpyAsync(dft, basis.data(), basis.size() * 4, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        if (pack_f32_launch(mel_basis, fb, cfg.n_mels, 1, WH_NB, WH_NB, 0, 1, ld_fb, 0, 1, nullptr, st)) return 1;
    }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_whisper::reserve(int G, hipStream_t st) {
    if (G <= cap) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws.release();
    cap = 0;
    const long D = cfg.d_model, F = cfg.ffn_dim, P = cfg.max_source_positions, MF = (long)G * NF, MP = (long)G * P;
    SVC_REQUIRE(MF * std::max(3 * D, F) < (1L << 31), "whisper: the window group is too large for 32-bit row offsets");
    padded = ws.alloc_n<float>((size_t)G * stride + WH_KP, st);
    spec = ws.alloc_n<float>((size_t)MF * ld_s, st);
    pw = ws.alloc_n<float>((size_t)MF * ld_fb, st);
    melc = ws.alloc_n<float>((size_t)MF * ld_c, st);
    part = ws.alloc_n<float>((size_t)G * WH_NBLK, st);
    feat = ws.alloc_n<float>((size_t)MF * cfg.n_mels, st);
    enc = ws.alloc_n<float>((size_t)MP * D, st);
    x = ws.alloc_n<float>((size_t)MP * D, st);
    qkv16 = ws.alloc_n<half_t>((size_t)MP * 3 * D, st);
    vt = ws.alloc_n<half_t>((size_t)G * D * vt_ld, st);
    ao16 = ws.alloc_n<half_t>((size_t)MP * D, st);
    if (!padded || !spec || !pw || !melc || !part || !feat || !enc || !x || !qkv16 || !vt || !ao16) return 1;
    if (dt == 0) {
        xin16 = ws.alloc_n<half_t>((size_t)MF * cin_ld, st);
        h16 = ws.alloc_n<half_t>((size_t)MF * D, st);
        n16 = ws.alloc_n<half_t>((size_t)MP * D, st);
        ff16 = ws.alloc_n<half_t>((size_t)MP * F, st);
        if (!xin16 || !h16 || !n16 || !ff16) return 1;
    } else {
        xin32 = ws.alloc_n<float>((size_t)MF * cin_ld, st);
        h32 = ws.alloc_n<float>((size_t)MF * D, st);
        n32 = ws.alloc_n<float>((size_t)MP * D, st);
        ao32 = ws.alloc_n<float>((size_t)MP * D, st);
        ff32 = ws.alloc_n<float>((size_t)MP * F, st);
        if (!xin32 || !h32 || !n32 || !ao32 || !ff32) return 1;
    }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    cap = G;
    return 0;
}

// c = act(a [M][K] W^T + b) (+ res): fp32 and / or fp16 out, leading dimension N
int svc_whisper::lin(const Lin& l, const void* a, long K, long M, int Lout, int act, const float* res, float* c32, half_t* c16, hipStream_t st) {
    KGemmParams p = wh_gemm(M, l.N, Lout);
    p.a_ptr[0] = a; p.a_ld[0] = K; p.a_ktiles[0] = (int)(K / ktile_elems(dt));
    p.w = l.w; p.ldw = l.ldw; p.bias = l.b; p.act = act;
    p.res = res; p.ldres = l.N;
    p.c32 = c32; p.ldc32 = l.N; p.c16 = c16; p.ldc16 = l.N;
    return kgemm_launch(p, dt, KG_EPI_STORE, st);
}

// G windows of `wave` (rows of Lrow samples) -> out [G][n_mels][NF]
int svc_whisper::mel_group(const float* wave, long Lrow, const WinTab& wt, int G, float* out, hipStream_t st) {
    const long M = (long)G * NF;
    hipLaunchKernelGGL(wh_pad_kernel, dim3(cdiv(stride, 256), G), dim3(256), 0, st, wave, wt, Lrow, padded, stride, W);
    SVC_CHECK_HIP(hipGetLastError());
    {   // STFT: rows = frames, overlapping in memory (row stride = hop), K = n_fft (padded: the basis is zero there)
        KGemmParams p = wh_gemm(M, 2 * WH_NB, NF);
        p.a_seq_rows = (int)(stride / WH_HOP); p.a_len = p.a_seq_rows;
        p.a_ptr[0] = padded; p.a_ld[0] = WH_HOP; p.a_ktiles[0] = WH_KP / 32;
        p.w = dft; p.ldw = WH_KP;
        p.c32 = spec; p.ldc32 = ld_s;                        // pad columns (zero weight rows) land in the ld padding
        if (kgemm_launch(p, 1, KG_EPI_STORE, st)) return 1;
    }
    hipLaunchKernelGGL(wh_power_kernel, dim3(M), dim3(256), 0, st, spec, ld_s, pw, ld_fb);
    SVC_CHECK_HIP(hipGetLastError());
    {
        KGemmParams p = wh_gemm(M, cfg.n_mels, NF);
        p.a_ptr[0] = pw; p.a_ld[0] = ld_fb; p.a_ktiles[0] = (int)(ld_fb / 32);
        p.w = fb; p.ldw = ld_fb;
        p.c32 = melc; p.ldc32 = ld_c;
        if (kgemm_launch(p, 1, KG_EPI_STORE, st)) return 1;
    }
    hipLaunchKernelGGL(wh_log_kernel, dim3(WH_NBLK, G), dim3(256), 0, st, melc, ld_c, cfg.n_mels, NF, part);
    SVC_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(wh_norm_kernel, dim3(cdiv(NF, 128), cfg.n_mels, G), dim3(128), 0, st, melc, ld_c, part, out, cfg.n_mels, NF);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// feats [G][n_mels][NF] -> out [G][P][D]
int svc_whisper::encode_group(const float* feats, int G, float* out, hipStream_t st) {
    const int D = cfg.d_model, F = cfg.ffn_dim, P = cfg.max_source_positions, H = cfg.n_heads;
    const long MF = (long)G * NF, MP = (long)G * P;
    const bool f16 = dt == 0;
    // channels-last input rows; the pad columns of xin stay zero from the allocation
    if (bct_to_btc_launch(feats, G, cfg.n_mels, NF, f16 ? nullptr : xin32, cin_ld, f16 ? xin16 : nullptr, cin_ld, NF, NF, 1.f, st)) return 1;
    auto conv = [&](const Lin& c, const void* a, long lda, int astride, int Lout, float* c32, half_t* c16) -> int {
        KGemmParams p = wh_gemm((long)G * Lout, c.N, Lout);
        p.a_seq_rows = NF; p.a_len = NF; p.a_stride = astride; p.pad_mode = KG_PAD_ZERO;
        p.n_taps = 3;
        for (int t = 0; t < 3; ++t) { p.a_ptr[t] = a; p.a_ld[t] = lda; p.a_ktiles[t] = (int)(lda / ktile_elems(dt)); p.a_shift[t] = t - 1; }
        p.w = c.w; p.ldw = c.ldw; p.bias = c.b; p.act = KG_ACT_GELU;
        p.c32 = c32; p.ldc32 = c.N; p.c16 = c16; p.ldc16 = c.N;
        return kgemm_launch(p, dt, KG_EPI_STORE, st);
    };
    if (conv(conv1, f16 ? (const void*)xin16 : (const void*)xin32, cin_ld, 1, NF, f16 ? nullptr : h32, f16 ? h16 : nullptr)) return 1;
    if (conv(conv2, f16 ? (const void*)h16 : (const void*)h32, D, 2, P, x, nullptr)) return 1;
    hipLaunchKernelGGL(wh_add_pos_kernel, dim3(cdiv(MP * D / 4, 256)), dim3(256), 0, st, x, pos, (long)P * D / 4, MP * D / 4);
    SVC_CHECK_HIP(hipGetLastError());
    if (mark(2, st)) return 1;
    const void* nrm = f16 ? (const void*)n16 : (const void*)n32;
    const int vmode = attention_vt_mode(G, H, P);
    for (const Layer& ly : layers) {
        if (wh_layernorm_launch(x, D, f16 ? nullptr : n32, D, f16 ? n16 : nullptr, D, ly.g1, ly.b1, MP, D, 1e-5f, st)) return 1;
        if (lin(ly.qkv, nrm, D, MP, P, KG_ACT_NONE, nullptr, nullptr, qkv16, st)) return 1;
        hipLaunchKernelGGL(wh_vt_kernel, dim3(cdiv(P, 32), D / 32, G), dim3(256), 0, st, qkv16, vt, P, D, vt_ld, vmode);
        SVC_CHECK_HIP(hipGetLastError());
        AttnParams a;
        memset(&a, 0, sizeof(a));
        a.q = qkv16; a.k = qkv16 + D; a.ld_qk = 3 * D;
        a.vt = vt; a.vt_seq_stride = (long)D * vt_ld; a.vt_ld = vt_ld; a.vt_perm = vmode;
        a.out = ao16; a.ld_out = D;
        a.out32 = f16 ? nullptr : ao32;                      // precision 0: the fp32 out_proj reads the attention's fp32 rows
        a.n_seq = G; a.H = H; a.seq_rows = P; a.Tq = P; a.kv_len_const = P;
        a.qt_form = qt_form;
        if (attention_launch(a, st)) return 1;
        if (lin(ly.o, f16 ? (const void*)ao16 : (const void*)ao32, D, MP, P, KG_ACT_NONE, x, x, nullptr, st)) return 1;
        if (wh_layernorm_launch(x, D, f16 ? nullptr : n32, D, f16 ? n16 : nullptr, D, ly.g2, ly.b2, MP, D, 1e-5f, st)) return 1;
        if (lin(ly.fc1, nrm, D, MP, P, KG_ACT_GELU, nullptr, f16 ? nullptr : ff32, f16 ? ff16 : nullptr, st)) return 1;
        if (lin(ly.fc2, f16 ? (const void*)ff16 : (const void*)ff32, F, MP, P, KG_ACT_NONE, x, x, nullptr, st)) return 1;
    }
    if (wh_layernorm_launch(x, D, out, D, nullptr, 0, gf, bf, MP, D, 1e-5f, st)) return 1;
    return mark(3, st);
}

extern "C" {

int svc_whisper_create(const svc_whisper_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, const float* mel_basis, void* stream,
                       svc_whisper_t** out) {
    SVC_REQUIRE(cfg && weights && mel_basis && out, "svc_whisper_create: null argument");
    SVC_REQUIRE(cfg->d_model >= 64 && cfg->d_model % 64 == 0 && cfg->d_model <= 2048 && cfg->n_heads >= 1 && cfg->n_heads * 64 == cfg->d_model,
                "svc_whisper_create: d_model must be a multiple of 64 (at most 2048) and n_heads * 64 == d_model");
    SVC_REQUIRE(cfg->n_mels >= 8 && cfg->n_mels % 8 == 0, "svc_whisper_create: n_mels must be a multiple of 8");
    SVC_REQUIRE(cfg->n_layers >= 1 && cfg->ffn_dim >= 64 && cfg->ffn_dim % 64 == 0, "svc_whisper_create: n_layers >= 1, ffn_dim a multiple of 64");
    SVC_REQUIRE(cfg->max_source_positions >= 2 && cfg->max_source_positions <= 6000, "svc_whisper_create: max_source_positions 2 .. 6000");
    SVC_REQUIRE(cfg->precision == 0 || cfg->precision == 1, "svc_whisper_create: precision 0 (fp32 GEMMs) or 1 (fp16 GEMMs)");
    StateDict sd(weights, n_weights);
    std::string pre;
    for (const char* p : {"", "encoder.", "model.encoder."})
        if (sd.has(std::string(p) + "conv1.weight")) { pre = p; break; }
    for (const auto& k : wh_keys(*cfg))
        if (wh_require(sd.get(pre + k.name), pre + k.name, k.shape)) return 1;
    hipStream_t st = (hipStream_t)stream;
    auto* m = new svc_whisper();
    m->cfg = *cfg;
    m->dt = cfg->precision ? 0 : 1;
    const int P = cfg->max_source_positions;
    m->W = P * WH_SPR; m->NF = 2 * P;
    m->cin_ld = round_up(cfg->n_mels, ktile_elems(m->dt));
    m->ld_fb = round_up(WH_NB, 32); m->ld_c = round_up(cfg->n_mels, 32); m->ld_s = round_up(2 * WH_NB, 8);
    m->stride = round_up((long)m->W + 2 * WH_PAD + WH_KP, WH_HOP);
    m->vt_ld = round_up(P, 64);
    // the attention's query-tile form, from (P, n_heads) alone: what a group of four windows would get from the grid-size rule
    m->qt_form = (long)cdiv(P, 128) * cfg->n_heads * 4 <= 256 ? 1 : 2;
    if (m->pack(sd, pre, mel_basis, st)) { delete m; return 1; }
    *out = m;
    return 0;
}

void svc_whisper_destroy(svc_whisper_t* m) { delete m; }

int svc_whisper_n_windows(int P, int overlap_rows, long n_samples) {
    if (P < 1 || overlap_rows < 0 || overlap_rows >= P) { set_error("svc_whisper_n_windows: overlap_rows outside [0, P)"); return -1; }
    if (n_samples < 1) { set_error("svc_whisper_n_windows: n_samples must be at least 1"); return -1; }
    const long nw = wh_n_windows((long)P * WH_SPR, (long)overlap_rows * WH_SPR, n_samples);
    if (nw > 0x7fffffffL) { set_error("svc_whisper_n_windows: n_samples is too large"); return -1; }
    return (int)nw;
}

int svc_whisper_rows(int P, int overlap_rows, long n_samples) {
    const int nw = svc_whisper_n_windows(P, overlap_rows, n_samples);
    if (nw < 0) { set_error(std::string("svc_whisper_rows: ") + get_error()); return -1; }
    const long W = (long)P * WH_SPR, O = (long)overlap_rows * WH_SPR;
    long rows = 0;
    for (long j = 0; j < nw; ++j) {
        const long n = std::min(W, n_samples - j * (W - O));
        rows += std::min((long)P, n / WH_SPR + 1) - (j ? overlap_rows : 0);
    }
    if (rows > 0x7fffffffL) { set_error("svc_whisper_rows: n_samples is too large"); return -1; }
    return (int)rows;
}

int svc_whisper_set_window_group(svc_whisper_t* m, int windows) {
    SVC_REQUIRE(windows >= 0 && windows <= WH_MAX_WIN, "svc_whisper_set_window_group: windows must be 0 (default) .. 64");
    SVC_REQUIRE(m, "svc_whisper_set_window_group: null handle");
    m->group = windows ? windows : WH_DEFAULT_GROUP;
    return 0;
}

int svc_whisper_set_timing(svc_whisper_t* m, int on) {
    SVC_REQUIRE(m, "svc_whisper_set_timing: null handle");
    m->timing = on != 0;
    return 0;
}

int svc_whisper_last_timing(svc_whisper_t* m, float* ms4) {
    SVC_REQUIRE(m && ms4 && m->timing && m->ev[0] && m->ev[4], "svc_whisper_last_timing: timing is off or no svc_whisper_content call was made");
    SVC_CHECK_HIP(hipEventSynchronize(m->ev[4]));
    for (int i = 0; i < 4; ++i) SVC_CHECK_HIP(hipEventElapsedTime(&ms4[i], m->ev[i], m->ev[i + 1]));
    return 0;
}

int svc_whisper_mel(svc_whisper_t* m, const float* wave, const int32_t* lens, int B, int L, float* feat, void* stream) {
    SVC_REQUIRE(lens != nullptr, "svc_whisper_mel: lens is NULL");
    SVC_REQUIRE(B >= 1 && B <= WH_MAX_B, "svc_whisper_mel: B must be 1 .. 64 clips");
    SVC_REQUIRE(L >= 1, "svc_whisper_mel: L must be at least 1 sample");
    for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 1 && lens[b] <= L, "svc_whisper_mel: lens outside [1, min(L, W)]");
    SVC_REQUIRE(wave && feat, "svc_whisper_mel: null wave or feat");
    SVC_REQUIRE(m, "svc_whisper_mel: null handle");
    for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] <= m->W, "svc_whisper_mel: lens outside [1, min(L, W)] (one window per clip)");
    hipStream_t st = (hipStream_t)stream;
    const int G = std::min(m->group, B);
    if (m->reserve(G, st)) return 1;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = std::min(G, B - b0);
        WinTab wt;
        memset(&wt, 0, sizeof(wt));
        for (int g = 0; g < nb; ++g) { wt.clip[g] = b0 + g; wt.n[g] = lens[b0 + g]; }
        if (m->mel_group(wave, L, wt, nb, feat + (long)b0 * m->cfg.n_mels * m->NF, st)) return 1;
    }
    return 0;
}

int svc_whisper_encode(svc_whisper_t* m, const float* feat, int B, float* out, void* stream) {
    SVC_REQUIRE(B >= 1, "svc_whisper_encode: B must be at least 1");
    SVC_REQUIRE(feat && out, "svc_whisper_encode: null feat or out");
    SVC_REQUIRE(m, "svc_whisper_encode: null handle");
    hipStream_t st = (hipStream_t)stream;
    const int G = std::min(m->group, B);
    const long P = m->cfg.max_source_positions;
    if (m->reserve(G, st)) return 1;
    for (int b0 = 0; b0 < B; b0 += G) {
        const int nb = std::min(G, B - b0);
        if (m->encode_group(feat + (long)b0 * m->cfg.n_mels * m->NF, nb, out + (long)b0 * P * m->cfg.d_model, st)) return 1;
    }
    return 0;
}

int svc_whisper_content(svc_whisper_t* m, const float* wave, const int32_t* lens, int B, int L, int overlap_rows, float* out, int Rmax,
                        void* stream) {
    SVC_REQUIRE(B >= 1 && B <= WH_MAX_B, "svc_whisper_content: B must be 1 .. 64 clips");
    SVC_REQUIRE(L >= 1, "svc_whisper_content: L must be at least 1 sample");
    if (lens)
        for (int b = 0; b < B; ++b) SVC_REQUIRE(lens[b] >= 1 && lens[b] <= L, "svc_whisper_content: lens outside [1, L]");
    SVC_REQUIRE(overlap_rows >= 0, "svc_whisper_content: overlap_rows outside [0, P)");
    SVC_REQUIRE(Rmax >= 1, "svc_whisper_content: Rmax is smaller than the longest clip's rows (svc_whisper_rows)");
    SVC_REQUIRE(wave && out, "svc_whisper_content: null wave or out");
    SVC_REQUIRE(m, "svc_whisper_content: null handle");
    const int P = m->cfg.max_source_positions, D = m->cfg.d_model;
    SVC_REQUIRE(overlap_rows < P, "svc_whisper_content: overlap_rows outside [0, P)");
    const long W = m->W, O = (long)overlap_rows * WH_SPR;
    // the window table of the whole call, in clip order
    struct Win { int clip, start, n, dst0, drop, keep, zero_from; };
    std::vector<Win> wins;
    for (int b = 0; b < B; ++b) {
        const long n = lens ? lens[b] : L;
        const int rows = svc_whisper_rows(P, overlap_rows, n);
        SVC_REQUIRE(rows >= 0 && rows <= Rmax, "svc_whisper_content: Rmax is smaller than the longest clip's rows (svc_whisper_rows)");
        const long nw = wh_n_windows(W, O, n);
        int dst = 0;
        for (long j = 0; j < nw; ++j) {
            const long s = j * (W - O), ns = std::min(W, n - s);
            const int keep = (int)std::min((long)P, ns / WH_SPR + 1), drop = j ? overlap_rows : 0;
            wins.push_back({b, (int)s, (int)ns, dst, drop, keep, j + 1 == nw ? rows : -1});
            dst += keep - drop;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)std::min((size_t)m->group, wins.size());
    if (m->reserve(G, st)) return 1;
    for (size_t w0 = 0; w0 < wins.size(); w0 += G) {
        const int nb = (int)std::min((size_t)G, wins.size() - w0);
        WinTab wt;
        memset(&wt, 0, sizeof(wt));
        for (int g = 0; g < nb; ++g) {
            const Win& w = wins[w0 + g];
            wt.clip[g] = w.clip; wt.start[g] = w.start; wt.n[g] = w.n; wt.dst0[g] = w.dst0; wt.drop[g] = w.drop; wt.keep[g] = w.keep;
            wt.zero_from[g] = w.zero_from;
        }
        if (m->mark(0, st)) return 1;
        if (m->mel_group(wave, L, wt, nb, m->feat, st) || m->mark(1, st)) return 1;
        if (m->encode_group(m->feat, nb, m->enc, st)) return 1;
        hipLaunchKernelGGL(wh_assemble_kernel, dim3(P + Rmax, nb), dim3(192), 0, st, m->enc, wt, out, P, D, Rmax);
        SVC_CHECK_HIP(hipGetLastError());
        if (m->mark(4, st)) return 1;
    }
    return 0;
}

/* y = LayerNorm(x) * gamma + beta over rows of D (op seam of the encoder's LayerNorm kernel) */
int svc_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, void* stream) {
    SVC_REQUIRE(x && gamma && beta && y && rows >= 0, "svc_op_layernorm: null argument or negative rows");
    return wh_layernorm_launch(x, D, y, D, nullptr, 0, gamma, beta, rows, D, eps, (hipStream_t)stream);
}

}  // extern "C"
