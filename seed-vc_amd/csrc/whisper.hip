// Whisper content encoder for gfx950: 16 kHz audio -> content features at 50 rows/s (`semantic_fn` of the reference drivers:
// WhisperFeatureExtractor + the encoder half of openai/whisper-small in float16, one 30 s window at a time).
//
// Log-mel: the window's samples zero-padded to W = 320 P, reflect padding of 200 on the padded window, the STFT (n_fft 400,
// hop 160, periodic Hann) as one fp32 tap-GEMM over overlapping signal rows, power, the caller's mel basis, log10, the clamp
// to the window's own maximum - 8 (a reduction of its own: per-block maxima, then every thread folds them; no atomics) and
// (x + 4) / 4.  Stem: conv1 + GELU, conv2 (stride 2) + GELU, + positions, on the fp16 tap-GEMM (precision 1) or the fp32 one
// (precision 0).  The transformer stack, the window plan of long clips and the row gather are content_encoder.h's.  No window
// is copied out of its clip, nothing above a clip's end is read, and every window is computed as if alone.
#include <math.h>
#include <string.h>

#include "content_encoder.h"

using namespace svc;

namespace {

constexpr int WH_NFFT = 400, WH_HOP = 160, WH_PAD = WH_NFFT / 2, WH_NB = WH_NFFT / 2 + 1, WH_KP = 416 /* n_fft padded to k-tiles */;
constexpr int WH_SPR = SAMPLES_PER_ROW;           // hop 160, conv2 stride 2
constexpr int WH_MAX_B = 64, WH_NBLK = 64, WH_DEFAULT_GROUP = 16;
constexpr StackNames WH_NAMES = {"layers.", "self_attn.q_proj", "self_attn.k_proj", nullptr, "self_attn.v_proj", "self_attn.out_proj",
                                 "self_attn_layer_norm", "fc1", "fc2", "final_layer_norm", "layer_norm"};

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

// x [G][P][D] += pos [P][D]
__global__ void wh_add_pos_kernel(float* __restrict__ x, const float* __restrict__ pos, long PD4, long total4) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    float4 a = reinterpret_cast<float4*>(x)[i];
    const float4 b = reinterpret_cast<const float4*>(pos)[i % PD4];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4*>(x)[i] = a;
}

}  // namespace

struct svc_whisper {
    svc_whisper_config_t cfg;
    int dt = 0;                      // tap-GEMM dtype of the convs and linears: 0 fp16 (precision 1), 1 fp32 (precision 0)
    int W = 0, NF = 0;               // samples and mel frames of a window
    int group = WH_DEFAULT_GROUP;
    long cin_ld = 0, ld_fb = 0, ld_c = 0, ld_s = 0, stride = 0;
    Arena wts, ws;
    Lin conv1, conv2;
    EncoderStack stack;
    float *pos = nullptr, *dft = nullptr, *fb = nullptr;
    // workspace for `cap` windows
    int cap = 0;
    float *padded = nullptr, *spec = nullptr, *pw = nullptr, *melc = nullptr, *part = nullptr, *feat = nullptr, *enc = nullptr;
    float *xin32 = nullptr, *h32 = nullptr;
    half_t *xin16 = nullptr, *h16 = nullptr;
    StageTimer tm;
    int pack_conv(const float* w, const float* bias, int N, int Cin, long cin_pad, Lin* out, hipStream_t st);
    int pack(const StateDict& sd, const std::string& pre, const float* mel_basis, hipStream_t st);
    int reserve(int G, hipStream_t st);
    int mel_group(const float* wave, long Lrow, const WinTab& wt, int G, float* out, hipStream_t st);
    int encode_group(const float* feats, int G, float* out, hipStream_t st);
};

namespace {

std::vector<KeyShape> wh_keys(const svc_whisper_config_t& c) {
    const long D = c.d_model;
    std::vector<KeyShape> k = {{"conv1.weight", {D, c.n_mels, 3}}, {"conv1.bias", {D}}, {"conv2.weight", {D, D, 3}}, {"conv2.bias", {D}},
                               {"embed_positions.weight", {c.max_source_positions, D}}};
    EncoderStack::keys(WH_NAMES, c.n_layers, D, c.ffn_dim, k);
    return k;
}

}  // namespace

// Conv1d weight [N][Cin][3] -> [Npad128][3 * cin_pad], tap-major
int svc_whisper::pack_conv(const float* w, const float* bias, int N, int Cin, long cin_pad, Lin* out, hipStream_t st) {
    out->N = N; out->ldw = 3 * cin_pad;
    out->w = wts.alloc((size_t)round_up(N, 128) * out->ldw * esize(dt), st);
    if (!out->w) return 1;
    for (int t = 0; t < 3; ++t)
        if (pack_any(dt, w + t, out->w, t * cin_pad, N, Cin, 1, 3L * Cin, 3, 0, out->ldw, 1, 0, nullptr, st)) return 1;
    if (!(out->b = copy_f32(bias, N, wts, st))) return 1;
    return 0;
}

int svc_whisper::pack(const StateDict& sd, const std::string& pre, const float* mel_basis, hipStream_t st) {
    const int D = cfg.d_model, P = cfg.max_source_positions;
    auto get = [&](const std::string& k) { return sd.get(pre + k)->data; };       // every key was checked by the caller
    if (pack_conv(get("conv1.weight"), get("conv1.bias"), D, cfg.n_mels, cin_ld, &conv1, st)) return 1;
    if (pack_conv(get("conv2.weight"), get("conv2.bias"), D, D, D, &conv2, st)) return 1;
    if (!(pos = copy_f32(get("embed_positions.weight"), (long)P * D, wts, st))) return 1;
    if (stack.pack(sd, pre, WH_NAMES, cfg.n_layers, wts, st)) return 1;
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
    if (!padded || !spec || !pw || !melc || !part || !feat || !enc || stack.reserve(ws, G, (int)P, st)) return 1;
    if (dt == 0) {
        xin16 = ws.alloc_n<half_t>((size_t)MF * cin_ld, st);
        h16 = ws.alloc_n<half_t>((size_t)MF * D, st);
        if (!xin16 || !h16) return 1;
    } else {
        xin32 = ws.alloc_n<float>((size_t)MF * cin_ld, st);
        h32 = ws.alloc_n<float>((size_t)MF * D, st);
        if (!xin32 || !h32) return 1;
    }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    cap = G;
    return 0;
}

// G windows of `wave` (rows of Lrow samples) -> out [G][n_mels][NF]
int svc_whisper::mel_group(const float* wave, long Lrow, const WinTab& wt, int G, float* out, hipStream_t st) {
    const long M = (long)G * NF;
    hipLaunchKernelGGL(wh_pad_kernel, dim3(cdiv(stride, 256), G), dim3(256), 0, st, wave, wt, Lrow, padded, stride, W);
    SVC_CHECK_HIP(hipGetLastError());
    {   // STFT: rows = frames, overlapping in memory (row stride = hop), K = n_fft (padded: the basis is zero there)
        KGemmParams p = kgemm_rows(M, 2 * WH_NB, NF);
        p.a_seq_rows = (int)(stride / WH_HOP); p.a_len = p.a_seq_rows;
        p.a_ptr[0] = padded; p.a_ld[0] = WH_HOP; p.a_ktiles[0] = WH_KP / 32;
        p.w = dft; p.ldw = WH_KP;
        p.c32 = spec; p.ldc32 = ld_s;                        // pad columns (zero weight rows) land in the ld padding
        if (kgemm_launch(p, 1, KG_EPI_STORE, st)) return 1;
    }
    hipLaunchKernelGGL(wh_power_kernel, dim3(M), dim3(256), 0, st, spec, ld_s, pw, ld_fb);
    SVC_CHECK_HIP(hipGetLastError());
    {
        KGemmParams p = kgemm_rows(M, cfg.n_mels, NF);
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
    const int D = cfg.d_model, P = cfg.max_source_positions;
    const long MP = (long)G * P;
    const bool f16 = dt == 0;
    // channels-last input rows; the pad columns of xin stay zero from the allocation
    if (bct_to_btc_launch(feats, G, cfg.n_mels, NF, f16 ? nullptr : xin32, cin_ld, f16 ? xin16 : nullptr, cin_ld, NF, NF, 1.f, st)) return 1;
    auto conv = [&](const Lin& c, const void* a, long lda, int astride, int Lout, float* c32, half_t* c16) -> int {
        KGemmParams p = kgemm_rows((long)G * Lout, c.N, Lout);
        p.a_seq_rows = NF; p.a_len = NF; p.a_stride = astride; p.pad_mode = KG_PAD_ZERO;
        p.n_taps = 3;
        for (int t = 0; t < 3; ++t) { p.a_ptr[t] = a; p.a_ld[t] = lda; p.a_ktiles[t] = (int)(lda / ktile_elems(dt)); p.a_shift[t] = t - 1; }
        p.w = c.w; p.ldw = c.ldw; p.bias = c.b; p.act = KG_ACT_GELU;
        p.c32 = c32; p.ldc32 = c.N; p.c16 = c16; p.ldc16 = c.N;
        return kgemm_launch(p, dt, KG_EPI_STORE, st);
    };
    if (conv(conv1, f16 ? (const void*)xin16 : (const void*)xin32, cin_ld, 1, NF, f16 ? nullptr : h32, f16 ? h16 : nullptr)) return 1;
    if (conv(conv2, f16 ? (const void*)h16 : (const void*)h32, D, 2, P, stack.x, nullptr)) return 1;
    hipLaunchKernelGGL(wh_add_pos_kernel, dim3(cdiv(MP * D / 4, 256)), dim3(256), 0, st, stack.x, pos, (long)P * D / 4, MP * D / 4);
    SVC_CHECK_HIP(hipGetLastError());
    if (tm.mark(2, st) || stack.run(G, P, nullptr, out, st)) return 1;
    return tm.mark(3, st);
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
        if (require_shape(sd.get(pre + k.name), pre + k.name, k.shape, "svc_whisper_create")) return 1;
    hipStream_t st = (hipStream_t)stream;
    auto* m = new svc_whisper();
    m->cfg = *cfg;
    m->dt = cfg->precision ? 0 : 1;
    const int P = cfg->max_source_positions;
    m->W = P * WH_SPR; m->NF = 2 * P;
    m->cin_ld = round_up(cfg->n_mels, ktile_elems(m->dt));
    m->ld_fb = round_up(WH_NB, 32); m->ld_c = round_up(cfg->n_mels, 32); m->ld_s = round_up(2 * WH_NB, 8);
    m->stride = round_up((long)m->W + 2 * WH_PAD + WH_KP, WH_HOP);
    m->stack.dt = m->dt; m->stack.D = cfg->d_model; m->stack.F = cfg->ffn_dim; m->stack.H = cfg->n_heads;
    // the attention's query-tile form, from (P, n_heads) alone: what a group of four windows would get from the grid-size rule
    m->stack.qt_form = (long)cdiv(P, 128) * cfg->n_heads * 4 <= 256 ? 1 : 2;
    if (m->pack(sd, pre, mel_basis, st)) { delete m; return 1; }
    *out = m;
    return 0;
}

void svc_whisper_destroy(svc_whisper_t* m) { delete m; }

int svc_whisper_n_windows(int P, int overlap_rows, long n_samples) {
    if (P < 1 || overlap_rows < 0 || overlap_rows >= P) { set_error("svc_whisper_n_windows: overlap_rows outside [0, P)"); return -1; }
    if (n_samples < 1) { set_error("svc_whisper_n_windows: n_samples must be at least 1"); return -1; }
    const long nw = window_count((long)P * WH_SPR, (long)overlap_rows * WH_SPR, n_samples);
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
    SVC_REQUIRE(windows >= 0 && windows <= MAX_WIN, "svc_whisper_set_window_group: windows must be 0 (default) .. 64");
    SVC_REQUIRE(m, "svc_whisper_set_window_group: null handle");
    m->group = windows ? windows : WH_DEFAULT_GROUP;
    return 0;
}

int svc_whisper_set_timing(svc_whisper_t* m, int on) {
    SVC_REQUIRE(m, "svc_whisper_set_timing: null handle");
    m->tm.on = on != 0;
    return 0;
}

int svc_whisper_last_timing(svc_whisper_t* m, float* ms4) {
    const char* msg = "svc_whisper_last_timing: timing is off or no svc_whisper_content call was made";
    SVC_REQUIRE(m, msg);
    return m->tm.last(ms4, msg);
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
    std::vector<Win> wins;                                   // the window plan of the whole call, in clip order
    for (int b = 0; b < B; ++b) {
        const int rows = plan_clip(wins, b, lens ? lens[b] : L, m->W, overlap_rows, [P](long ns) { return std::min((long)P, ns / WH_SPR + 1); });
        SVC_REQUIRE(rows <= Rmax, "svc_whisper_content: Rmax is smaller than the longest clip's rows (svc_whisper_rows)");
    }
    hipStream_t st = (hipStream_t)stream;
    const int G = (int)std::min((size_t)m->group, wins.size());
    if (m->reserve(G, st)) return 1;
    for (size_t w0 = 0; w0 < wins.size(); w0 += G) {
        const int nb = (int)std::min((size_t)G, wins.size() - w0);
        const WinTab wt = win_table(wins, w0, nb);
        if (m->tm.mark(0, st)) return 1;
        if (m->mel_group(wave, L, wt, nb, m->feat, st) || m->tm.mark(1, st)) return 1;
        if (m->encode_group(m->feat, nb, m->enc, st)) return 1;
        if (assemble_launch(m->enc, wt, nb, out, P, D, Rmax, 192, st)) return 1;
        if (m->tm.mark(4, st)) return 1;
    }
    return 0;
}

/* y = LayerNorm(x) * gamma + beta over rows of D (op seam of the encoder's LayerNorm kernel) */
int svc_op_layernorm(const float* x, const float* gamma, const float* beta, float* y, int rows, int D, float eps, void* stream) {
    SVC_REQUIRE(x && gamma && beta && y && rows >= 0, "svc_op_layernorm: null argument or negative rows");
    return rownorm_launch(0, x, D, y, nullptr, D, gamma, beta, nullptr, nullptr, rows, D, eps, nullptr, 1, (hipStream_t)stream);
}

}  // extern "C"
