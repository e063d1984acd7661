// Kernels and host code shared by the content encoders (content_encoder.h).
#include <string.h>

#include "content_encoder.h"

namespace svc {

namespace {

constexpr float QSCALE = 0.125f * 1.4426950408889634f;        // 1 / sqrt(64), and the attention kernel's exp2

template <int MODE>
__global__ __launch_bounds__(256) void rownorm_kernel(const float* __restrict__ x, long ldx, float* __restrict__ y32, half_t* __restrict__ y16,
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
    row_norm<32>(v, n, D, eps, gamma, beta, lane, MODE >= 1);
    if (MODE == 2) row_norm<32>(v, n, D, eps, gamma2, beta2, lane, false);
#pragma unroll
    for (int i = 0; i < 32; ++i)
        if (i < n) {
            const int c = lane + 64 * i;
            if (y32) y32[row * ldy + c] = v[i];
            if (y16) y16[row * ldy + c] = (half_t)v[i];
        }
}

__global__ __launch_bounds__(256) void vt_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ vt, const int* __restrict__ lens, int P, int D,
                                                 long vt_ld, int mode) {
    __shared__ half_t tile[32][34];
    const int g = blockIdx.z, p0 = blockIdx.x * 32, d0 = blockIdx.y * 32, T = lens ? lens[g] : P;
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

// Attention on fp32 operands (precision 0 of the post-LN order, where the fp16 rounding of q, k, v and the softmax weights alone is
// 1.4e-4 of the output): one wave per (query row, head, window), head dimension 64.  qkv [G * P][3 D] fp32 with
// 1 / 8 and log2(e) already in q.  Keys in chunks of 64 in ascending order: lane j scores key t0 + j (q from LDS, the key's row from
// memory), the running maximum and sum are the online softmax's, lane d accumulates output dimension d over the chunk's keys in
// ascending order.  Keys at and above the window's own count are never read.  A row's result depends on its window alone.
__global__ __launch_bounds__(256) void attn_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, const int* __restrict__ lens, int P, int D,
                                                       int H) {
    __shared__ float q_s[4][64];
    const int g = blockIdx.z, h = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int T = lens ? lens[g] : P, row = blockIdx.x * 4 + wave;
    const float* base = qkv + (long)g * P * 3 * D + h * 64;
    if (row < T) q_s[wave][lane] = base[(long)row * 3 * D + lane];
    __syncthreads();
    if (row >= T) return;                                    // per wave, after the only barrier
    float m = -1e30f, l = 0.f, acc = 0.f;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        float s = -1e30f;
        if (t < T) {
            const float4* kr = reinterpret_cast<const float4*>(base + (long)t * 3 * D + D);
            float a = 0.f;
#pragma unroll
            for (int d4 = 0; d4 < 16; ++d4) {
                const float4 kv = kr[d4];
                a = fmaf(q_s[wave][4 * d4], kv.x, a); a = fmaf(q_s[wave][4 * d4 + 1], kv.y, a);
                a = fmaf(q_s[wave][4 * d4 + 2], kv.z, a); a = fmaf(q_s[wave][4 * d4 + 3], kv.w, a);
            }
            s = a;
        }
        float cm = s;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cm = fmaxf(cm, __shfl_xor(cm, o));
        const float mn = fmaxf(m, cm), sc = exp2f(m - mn);
        const float p = t < T ? exp2f(s - mn) : 0.f;
        l = l * sc + wave_sum(p);
        acc *= sc;
        const int nk = min(64, T - t0);
        const float* vr = base + (long)t0 * 3 * D + 2 * D + lane;
        for (int j = 0; j < nk; ++j) acc = fmaf(__shfl(p, j), vr[(long)j * 3 * D], acc);
        m = mn;
    }
    out[((long)g * P + row) * D + h * 64 + lane] = acc / l;
}

// block (r, g).  r < P: row r of window g, when kept, goes to its place in the clip's rows; r >= P: row r - P of the clip is
// zeroed when window g is the clip's last and the row is at or above the clip's count
__global__ void assemble_kernel(const float* __restrict__ enc, WinTab wt, float* __restrict__ out, int P, int D, int Rmax) {
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

// src [G][P][D] rows below lens[g] -> dst [G][T][D]; the other rows of dst are not touched
__global__ void copy_rows_kernel(const float* __restrict__ src, int P, float* __restrict__ dst, int T, const int* __restrict__ lens, int D) {
    const int g = blockIdx.y, r = blockIdx.x;
    if (r >= lens[g]) return;
    const float4* s = reinterpret_cast<const float4*>(src + ((long)g * P + r) * D);
    float4* d = reinterpret_cast<float4*>(dst + ((long)g * T + r) * D);
    for (int i = threadIdx.x; i < D / 4; i += blockDim.x) d[i] = s[i];
}

}  // namespace

int copy_rows_launch(const float* src, int P, float* dst, int T, const int* lens, int G, int rows, int D, hipStream_t st) {
    hipLaunchKernelGGL(copy_rows_kernel, dim3(rows, G), dim3(256), 0, st, src, P, dst, T, lens, D);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

WinTab win_table(const std::vector<Win>& wins, size_t w0, int G) {
    WinTab wt;
    memset(&wt, 0, sizeof(wt));
    for (int g = 0; g < G; ++g) {
        const Win& w = wins[w0 + g];
        wt.clip[g] = w.clip; wt.start[g] = w.start; wt.n[g] = w.n; wt.dst0[g] = w.dst0; wt.drop[g] = w.drop; wt.keep[g] = w.keep;
        wt.zero_from[g] = w.zero_from;
    }
    return wt;
}

int assemble_launch(const float* enc, const WinTab& wt, int G, float* out, int P, int D, int Rmax, int block, hipStream_t st) {
    hipLaunchKernelGGL(assemble_kernel, dim3(P + Rmax, G), dim3(block), 0, st, enc, wt, out, P, D, Rmax);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int rownorm_launch(int mode, const float* x, long ldx, float* y32, half_t* y16, long ldy, const float* gamma, const float* beta,
                   const float* gamma2, const float* beta2, long rows, int D, float eps, const int* lens, int seq_rows, hipStream_t st) {
    SVC_REQUIRE(D >= 64 && D % 64 == 0 && D <= 2048, "layernorm: D must be a multiple of 64, at most 2048");
    if (rows == 0) return 0;
    const auto kernel = mode == 0 ? rownorm_kernel<0> : mode == 1 ? rownorm_kernel<1> : rownorm_kernel<2>;
    hipLaunchKernelGGL(kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, ldx, y32, y16, ldy, gamma, beta, gamma2, beta2, rows, D, eps, lens, seq_rows);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int vt_launch(const half_t* qkv, half_t* vt, const int* lens, int G, int P, int D, long vt_ld, int mode, hipStream_t st) {
    hipLaunchKernelGGL(vt_kernel, dim3(cdiv(vt_ld, 32), D / 32, G), dim3(256), 0, st, qkv, vt, lens, P, D, vt_ld, mode);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

float* copy_f32(const float* src, long n, Arena& ar, hipStream_t st) {
    float* p = ar.alloc_n<float>(round_up(n, 8), st);
    if (!p) return nullptr;
    if (hipMemcpyAsync(p, src, (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) { set_error("weight copy failed"); return nullptr; }
    return p;
}

int pack_lin(int dt, Arena& wts, const float* w, const float* bias, int N, int K, const float* scale, Lin* out, hipStream_t st) {
    out->N = N; out->ldw = K;
    out->w = wts.alloc((size_t)round_up(N, 128) * K * esize(dt), st);
    if (!out->w) return 1;
    if (pack_any(dt, w, out->w, 0, N, 1, K, K, 0, 1, K, 0, 1, scale, st)) return 1;
    if (bias && !(out->b = copy_f32(bias, N, wts, st))) return 1;
    return 0;
}

KGemmParams kgemm_rows(long M, int N, int Lout) {
    KGemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = (int)M; p.N = N; p.Lout = Lout; p.a_seq_rows = Lout; p.c_seq_rows = Lout; p.a_stride = 1; p.a_len = Lout; p.n_taps = 1;
    p.vec_ok = 1;
    return p;
}

int linear_launch(int dt, const Lin& l, const void* a, long K, long M, int Lout, int act, const float* res, float* c32, half_t* c16, hipStream_t st) {
    KGemmParams p = kgemm_rows(M, l.N, Lout);
    p.a_ptr[0] = a; p.a_ld[0] = K; p.a_ktiles[0] = (int)(K / ktile_elems(dt));
    p.w = l.w; p.ldw = l.ldw; p.bias = l.b; p.act = act;
    p.res = res; p.ldres = l.N;
    p.c32 = c32; p.ldc32 = l.N; p.c16 = c16; p.ldc16 = l.N;
    return kgemm_launch(p, dt, KG_EPI_STORE, st);
}

void EncoderStack::keys(const StackNames& nm, int n_layers, long D, long F, std::vector<KeyShape>& out, bool final_ln) {
    for (int i = 0; i < n_layers; ++i) {
        const std::string p = nm.layers + std::to_string(i) + ".";
        for (const char* m : {nm.q, nm.k, nm.v, nm.o}) out.push_back({p + m + ".weight", {D, D}});
        for (const char* m : {nm.q, nm.v, nm.o}) out.push_back({p + m + ".bias", {D}});
        if (nm.k_bias) out.push_back({p + nm.k_bias, {D}});
        out.push_back({p + nm.fc1 + ".weight", {F, D}});
        out.push_back({p + nm.fc1 + ".bias", {F}});
        out.push_back({p + nm.fc2 + ".weight", {D, F}});
        out.push_back({p + nm.fc2 + ".bias", {D}});
        for (const char* m : {nm.ln1, nm.ln2}) {
            out.push_back({p + m + ".weight", {D}});
            out.push_back({p + m + ".bias", {D}});
        }
    }
    if (!final_ln) return;
    out.push_back({std::string(nm.ln_final) + ".weight", {D}});
    out.push_back({std::string(nm.ln_final) + ".bias", {D}});
}

int EncoderStack::pack(const StateDict& sd, const std::string& pre, const StackNames& nm, int n_layers, Arena& wts, hipStream_t st) {
    auto get = [&](const std::string& k) { return sd.get(pre + k)->data; };
    float* qs = wts.alloc_n<float>(D, st);
    if (!qs) return 1;
    {
        std::vector<float> h(D, QSCALE);
        SVC_CHECK_HIP(hipMemcpyAsync(qs, h.data(), (size_t)D * 4, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
    }
    layers.resize(n_layers);
    for (int i = 0; i < n_layers; ++i) {
        Layer& ly = layers[i];
        const std::string p = nm.layers + std::to_string(i) + ".";
        // q | k | v rows of one [3 D][D] weight; the q rows and bias carry 1 / 8 and log2(e); without a k bias its zeros stay
        ly.qkv.N = 3 * D; ly.qkv.ldw = D;
        ly.qkv.w = wts.alloc((size_t)round_up(3 * D, 128) * D * esize(dt), st);
        ly.qkv.b = wts.alloc_n<float>(3 * D, st);
        if (!ly.qkv.w || !ly.qkv.b) return 1;
        if (pack_any(dt, get(p + nm.q + ".weight"), ly.qkv.w, 0, D, 1, D, D, 0, 1, D, 0, 1, qs, st)) return 1;
        if (pack_any(dt, get(p + nm.k + ".weight"), ly.qkv.w, (long)D * D, D, 1, D, D, 0, 1, D, 0, 1, nullptr, st)) return 1;
        if (pack_any(dt, get(p + nm.v + ".weight"), ly.qkv.w, 2L * D * D, D, 1, D, D, 0, 1, D, 0, 1, nullptr, st)) return 1;
        if (pack_f32_launch(get(p + nm.q + ".bias"), ly.qkv.b, D, 1, 1, 1, 0, 0, 1, 0, 0, qs, st)) return 1;
        if (nm.k_bias) SVC_CHECK_HIP(hipMemcpyAsync(ly.qkv.b + D, get(p + nm.k_bias), (size_t)D * 4, hipMemcpyDeviceToDevice, st));
        SVC_CHECK_HIP(hipMemcpyAsync(ly.qkv.b + 2 * D, get(p + nm.v + ".bias"), (size_t)D * 4, hipMemcpyDeviceToDevice, st));
        if (pack_lin(dt, wts, get(p + nm.o + ".weight"), get(p + nm.o + ".bias"), D, D, nullptr, &ly.o, st)) return 1;
        if (pack_lin(dt, wts, get(p + nm.fc1 + ".weight"), get(p + nm.fc1 + ".bias"), F, D, nullptr, &ly.fc1, st)) return 1;
        if (pack_lin(dt, wts, get(p + nm.fc2 + ".weight"), get(p + nm.fc2 + ".bias"), D, F, nullptr, &ly.fc2, st)) return 1;
        if (!(ly.g1 = copy_f32(get(p + nm.ln1 + ".weight"), D, wts, st)) || !(ly.b1 = copy_f32(get(p + nm.ln1 + ".bias"), D, wts, st)) ||
            !(ly.g2 = copy_f32(get(p + nm.ln2 + ".weight"), D, wts, st)) || !(ly.b2 = copy_f32(get(p + nm.ln2 + ".bias"), D, wts, st)))
            return 1;
    }
    if (!final_ln) return 0;
    if (!(gf = copy_f32(get(std::string(nm.ln_final) + ".weight"), D, wts, st)) ||
        !(bf = copy_f32(get(std::string(nm.ln_final) + ".bias"), D, wts, st)))
        return 1;
    return 0;
}

int EncoderStack::reserve(Arena& ws, int G, int P, hipStream_t st) {
    const long MP = (long)G * P;
    SVC_REQUIRE(MP * std::max(3L * D, (long)F) < (1L << 31), "content encoder: the window group is too large for 32-bit row offsets");
    x = ws.alloc_n<float>((size_t)MP * D, st);
    qkv16 = ws.alloc_n<half_t>((size_t)MP * 3 * D, st);
    vt = ws.alloc_n<half_t>((size_t)G * D * round_up(P, 64), st);
    ao16 = ws.alloc_n<half_t>((size_t)MP * D, st);
    if (!x || !qkv16 || !vt || !ao16) return 1;
    if (post_ln && !(y = ws.alloc_n<float>((size_t)MP * D, st))) return 1;
    if (post_ln && dt == 1 && !(qkv32 = ws.alloc_n<float>((size_t)MP * 3 * D, st))) return 1;
    if (dt == 0) {
        n16 = ws.alloc_n<half_t>((size_t)MP * D, st);
        ff16 = ws.alloc_n<half_t>((size_t)MP * F, st);
        if (!n16 || !ff16) return 1;
    } else {
        n32 = ws.alloc_n<float>((size_t)MP * D, st);
        ao32 = ws.alloc_n<float>((size_t)MP * D, st);
        ff32 = ws.alloc_n<float>((size_t)MP * F, st);
        if (!n32 || !ao32 || !ff32) return 1;
    }
    return 0;
}

int EncoderStack::run(int G, int P, const int* lens, float* out, hipStream_t st) {
    const long MP = (long)G * P, vt_ld = round_up(P, 64);
    const bool f16 = dt == 0;
    const void* nrm = f16 ? (const void*)n16 : (const void*)n32;
    const int vmode = attention_vt_mode(G, H, P);
    auto norm = [&](const float* g, const float* b, float* y32, half_t* y16) {
        return rownorm_launch(0, x, D, y32, y16, D, g, b, nullptr, nullptr, MP, D, 1e-5f, lens, P, st);
    };
    if (post_ln) return run_post(G, P, lens, out, st);
    for (const Layer& ly : layers) {
        if (norm(ly.g1, ly.b1, f16 ? nullptr : n32, f16 ? n16 : nullptr)) return 1;
        if (linear_launch(dt, ly.qkv, nrm, D, MP, P, KG_ACT_NONE, nullptr, nullptr, qkv16, st)) return 1;
        if (vt_launch(qkv16, vt, lens, G, P, D, vt_ld, vmode, st)) return 1;
        AttnParams a;
        memset(&a, 0, sizeof(a));
        a.q = qkv16; a.k = qkv16 + D; a.ld_qk = 3 * D;
        a.vt = vt; a.vt_seq_stride = (long)D * vt_ld; a.vt_ld = vt_ld; a.vt_perm = vmode;
        a.ld_out = D;                                        // one of the two: precision 0's fp32 out_proj reads the attention's fp32 rows
        a.out = f16 ? ao16 : nullptr;
        a.out32 = f16 ? nullptr : ao32;
        a.n_seq = G; a.H = H; a.seq_rows = P; a.Tq = P; a.kv_len = lens; a.kv_len_const = P;
        a.qt_form = qt_form;
        if (attention_launch(a, st)) return 1;
        if (linear_launch(dt, ly.o, f16 ? (const void*)ao16 : (const void*)ao32, D, MP, P, KG_ACT_NONE, x, x, nullptr, st)) return 1;
        if (norm(ly.g2, ly.b2, f16 ? nullptr : n32, f16 ? n16 : nullptr)) return 1;
        if (linear_launch(dt, ly.fc1, nrm, D, MP, P, KG_ACT_GELU, nullptr, f16 ? nullptr : ff32, f16 ? ff16 : nullptr, st)) return 1;
        if (linear_launch(dt, ly.fc2, f16 ? (const void*)ff16 : (const void*)ff32, F, MP, P, KG_ACT_NONE, x, x, nullptr, st)) return 1;
    }
    if (!final_ln) return 0;                                 // the result is the residual stream x itself
    return norm(gf, bf, out, nullptr);
}

// Post-LN order.  The residual stream r lives in y once ln_final has normalised the stem's rows out of x; x then takes the sums
// r + branch(r) of the residual epilogues and each LayerNorm brings them back to r (and its fp16 copy, the next GEMM's operand).
// The last LayerNorm writes `out`.  No buffer is read and written by one launch except by the residual epilogues' own element.
int EncoderStack::run_post(int G, int P, const int* lens, float* out, hipStream_t st) {
    SVC_REQUIRE(final_ln && y, "content encoder: the post-LN order needs encoder.layer_norm and its workspace");
    const long MP = (long)G * P, vt_ld = round_up(P, 64);
    const bool f16 = dt == 0;
    float* r = y;
    float* s = x;
    const void* nrm = f16 ? (const void*)n16 : (const void*)r;
    const int vmode = attention_vt_mode(G, H, P);
    auto norm = [&](const float* g, const float* b, float* y32) {
        return rownorm_launch(0, s, D, y32, f16 && y32 == r ? n16 : nullptr, D, g, b, nullptr, nullptr, MP, D, 1e-5f, lens, P, st);
    };
    if (norm(gf, bf, r)) return 1;
    for (size_t i = 0; i < layers.size(); ++i) {
        const Layer& ly = layers[i];
        if (f16) {
            if (linear_launch(dt, ly.qkv, nrm, D, MP, P, KG_ACT_NONE, nullptr, nullptr, qkv16, st)) return 1;
            if (vt_launch(qkv16, vt, lens, G, P, D, vt_ld, vmode, st)) return 1;
            AttnParams a;
            memset(&a, 0, sizeof(a));
            a.q = qkv16; a.k = qkv16 + D; a.ld_qk = 3 * D;
            a.vt = vt; a.vt_seq_stride = (long)D * vt_ld; a.vt_ld = vt_ld; a.vt_perm = vmode;
            a.ld_out = D;
            a.out = ao16;
            a.n_seq = G; a.H = H; a.seq_rows = P; a.Tq = P; a.kv_len = lens; a.kv_len_const = P;
            a.qt_form = qt_form;
            if (attention_launch(a, st)) return 1;
        } else {
            if (linear_launch(dt, ly.qkv, nrm, D, MP, P, KG_ACT_NONE, nullptr, qkv32, nullptr, st)) return 1;
            hipLaunchKernelGGL(attn_f32_kernel, dim3(cdiv(P, 4), H, G), dim3(256), 0, st, (const float*)qkv32, ao32, lens, P, D, H);
            SVC_CHECK_HIP(hipGetLastError());
        }
        if (linear_launch(dt, ly.o, f16 ? (const void*)ao16 : (const void*)ao32, D, MP, P, KG_ACT_NONE, r, s, nullptr, st)) return 1;
        if (norm(ly.g1, ly.b1, r)) return 1;
        if (linear_launch(dt, ly.fc1, nrm, D, MP, P, KG_ACT_GELU, nullptr, f16 ? nullptr : ff32, f16 ? ff16 : nullptr, st)) return 1;
        if (linear_launch(dt, ly.fc2, f16 ? (const void*)ff16 : (const void*)ff32, F, MP, P, KG_ACT_NONE, r, s, nullptr, st)) return 1;
        if (norm(ly.g2, ly.b2, i + 1 == layers.size() ? out : r)) return 1;
    }
    return 0;
}

}  // namespace svc
