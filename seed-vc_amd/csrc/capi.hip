// C ABI glue that is not tied to one model: error reporting, the anti-aliased activation seam and the
// op-level entry points used by the parity tests (tests/test_gpu_ops.py).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "model_util.h"
#include "noise.h"

namespace svc {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
const char* get_error() { return g_err.c_str(); }
}  // namespace svc

using namespace svc;

namespace {
struct Scratch {   // test-path temporaries (allocates; never used by the model paths)
    Arena ar;
};
}  // namespace

extern "C" {

const char* svc_last_error(void) { return svc::get_error(); }
int svc_abi_version(void) { return SVC_ABI_VERSION; }

int svc_anti_alias_act_fwd(const void* x, void* y, const float* up12, const float* down12, const float* log_alpha,
                           const float* log_beta, int B, int C, int L, int dtype, void* stream) {
    SVC_REQUIRE(B >= 0 && C >= 0 && L >= 0, "negative shape");
    if (B == 0 || C == 0 || L == 0) return 0;      // empty input: nothing to do (pointers may be null)
    SVC_REQUIRE(x && y && up12 && down12 && log_alpha && log_beta, "null argument");
    SVC_REQUIRE(C <= 65535 && B <= 65535, "grid limit: B, C <= 65535");
    return aa_act_rows_launch(x, y, up12, down12, log_alpha, log_beta, B, C, L, dtype, (hipStream_t)stream);
}

// ---- exporters of the seeded draws (noise.h): the tensors the explicit calls take, from the device functions the seeded kernels use
extern "C++" namespace {
// out[row][pos] = the normal of (seed, domain, row, pos), rows x n; one Philox call per four rows
__global__ __launch_bounds__(256) void noise_normal_rows_kernel(unsigned long long seed, unsigned domain, int rows, long n,
                                                                float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long q = i / n, pos = i - q * n;
    if (4 * q >= rows) return;
    float v[4];
    noise_normal4(seed, domain, (unsigned)q, (unsigned)pos, v);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * q + j < rows) out[(4 * q + j) * n + pos] = v[j];
}

int noise_normal_rows_launch(unsigned long long seed, unsigned domain, int rows, long n, float* out, hipStream_t st) {
    const long total = (long)cdiv(rows, 4) * n;
    hipLaunchKernelGGL(noise_normal_rows_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, seed, domain, rows, n, out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}
}  // namespace

int svc_cfm_noise_draws(uint64_t seed, int C, int T, float* z, void* stream) {
    SVC_REQUIRE(z, "null argument");
    SVC_REQUIRE(C >= 1 && T >= 1, "svc_cfm_noise_draws: C and T must be at least 1");
    return noise_normal_rows_launch(seed, NOISE_CFM_Z, C, T, z, (hipStream_t)stream);
}

int svc_hift_noise_draws(uint64_t seed, int NH, long n, float* phase0, float* noise, void* stream) {
    SVC_REQUIRE(phase0 && noise, "null argument");
    SVC_REQUIRE(NH >= 1 && n >= 1 && n <= 0x7fffffffL, "svc_hift_noise_draws: NH >= 1 and 1 <= n < 2^31 (the sample index is a 32-bit counter word)");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(noise_phase0_kernel, dim3(cdiv(NH, 64)), dim3(64), 0, st, (const unsigned long long*)nullptr,
                       (unsigned long long)seed, 1, NH, phase0);
    SVC_CHECK_HIP(hipGetLastError());
    return noise_normal_rows_launch(seed, NOISE_HIFT_SOURCE, NH, n, noise, st);
}

int svc_op_linear(const float* a, const float* w, const float* bias, float* c, int M, int N, int K, int dtype, int act,
                  void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Scratch s;
    const int kt = ktile_elems(dtype);
    const long Kp = round_up(K, kt), Np = round_up(N, 128);
    void* ap = s.ar.alloc((size_t)M * Kp * esize(dtype), st);
    void* wp = s.ar.alloc((size_t)Np * Kp * esize(dtype), st);
    if (!ap || !wp) return 1;
    if (pack_any(dtype, a, ap, 0, M, 1, K, K, 0, 1, Kp, 0, 1, nullptr, st)) return 1;
    if (pack_any(dtype, w, wp, 0, N, 1, K, K, 0, 1, Kp, 0, 1, nullptr, st)) return 1;
    KGemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = N; p.Lout = M > 0 ? M : 1; p.a_seq_rows = p.Lout; p.c_seq_rows = p.Lout; p.a_stride = 1; p.a_len = p.Lout;
    p.n_taps = 1; p.a_ptr[0] = ap; p.a_ld[0] = Kp; p.a_ktiles[0] = (int)(Kp / kt);
    p.w = wp; p.ldw = Kp; p.bias = bias; p.act = act; p.act_slope = 0.1f;
    p.c32 = c; p.ldc32 = N; p.vec_ok = (N % 8 == 0);
    if (kgemm_launch(p, dtype, KG_EPI_STORE, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// operands of the timing harness: pseudo-random values in (-1, 1) (the MFMA rate under the power limit depends on the data)
extern "C++" template <typename T>
__global__ void bench_fill_kernel(T* __restrict__ x, long n, unsigned seed) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u + seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        x[i] = (T)((float)(h & 0xFFFF) * (2.0f / 65536.0f) - 1.0f);
    }
}

// Timing harness for kernel tuning (not part of the product path): avg ms of `iters` launches of one tap-GEMM.
int svc_op_gemm_bench(int M, int N, int K, int dtype, int epi, int iters, int debug, float* out_ms, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Scratch s;
    const int kt = ktile_elems(dtype);
    const long Kp = round_up(K, kt), Np = round_up(N, 256);
    void* ap = s.ar.alloc((size_t)M * Kp * esize(dtype), st);
    void* wp = s.ar.alloc((size_t)Np * Kp * esize(dtype), st);
    float* c32 = s.ar.alloc_n<float>((size_t)M * N, st);
    half_t* c16 = s.ar.alloc_n<half_t>((size_t)M * N, st);
    half_t* vt = s.ar.alloc_n<half_t>((size_t)M * N + 4096, st);
    float* rope = s.ar.alloc_n<float>((size_t)8192 * 64, st);
    if (!ap || !wp || !c32 || !c16 || !vt || !rope) return 1;
    if (dtype == 0) {
        hipLaunchKernelGGL(bench_fill_kernel<half_t>, dim3(1024), dim3(256), 0, st, (half_t*)ap, (long)M * Kp, 1u);
        hipLaunchKernelGGL(bench_fill_kernel<half_t>, dim3(1024), dim3(256), 0, st, (half_t*)wp, (long)Np * Kp, 2u);
    } else {
        hipLaunchKernelGGL(bench_fill_kernel<float>, dim3(1024), dim3(256), 0, st, (float*)ap, (long)M * Kp, 1u);
        hipLaunchKernelGGL(bench_fill_kernel<float>, dim3(1024), dim3(256), 0, st, (float*)wp, (long)Np * Kp, 2u);
    }
    hipLaunchKernelGGL(bench_fill_kernel<float>, dim3(1024), dim3(256), 0, st, c32, (long)M * N, 3u);
    hipLaunchKernelGGL(bench_fill_kernel<float>, dim3(1024), dim3(256), 0, st, rope, (long)8192 * 64, 4u);
    KGemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = N; p.Lout = 864; p.a_seq_rows = 864; p.c_seq_rows = 864; p.a_stride = 1; p.a_len = 864;
    p.n_taps = 1; p.a_ptr[0] = ap; p.a_ld[0] = Kp; p.a_ktiles[0] = (int)(Kp / kt);
    p.w = wp; p.ldw = Kp; p.vec_ok = 1; p.debug = debug;
    if (epi == KG_EPI_STORE) { p.c32 = c32; p.ldc32 = N; p.res = c32; p.ldres = N; }
    else if (epi == KG_EPI_SWIGLU) { p.c16 = c16; p.ldc16 = N / 2; }
    else if (epi == KG_EPI_QKV_ROPE) { p.c16 = c16; p.ldc16 = 2 * (N / 3); p.rope = rope; p.rope_D = N / 3; p.q_scale = 1.f;
                                       p.vt = vt; p.vt_seq_stride = (long)(N / 3) * 896; p.vt_ld = 896; p.vt_mode = 1; }
    else { p.c16 = c16; p.ldc16 = N / 2; }
    hipEvent_t e0, e1;
    SVC_CHECK_HIP(hipEventCreate(&e0));
    SVC_CHECK_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) if (kgemm_launch(p, dtype, epi, st)) return 1;
    SVC_CHECK_HIP(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) if (kgemm_launch(p, dtype, epi, st)) return 1;
    SVC_CHECK_HIP(hipEventRecord(e1, st));
    SVC_CHECK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SVC_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
    *out_ms = ms / iters;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return 0;
}

extern "C++" __global__ void bench_diff_kernel(const unsigned* __restrict__ a, const unsigned* __restrict__ b, long n,
                                              unsigned long long* __restrict__ count) {
    unsigned long long c = 0;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) c += a[i] != b[i];
    if (c) atomicAdd(count, c);
}

// Test aid: runs ONE fp16 tap-GEMM (epilogue `epi`, bias + residual / RoPE / V^T as the DiT uses them) under two tile-form
// overrides (`debug_a`, `debug_b`, launch_wide's bits) on the same pseudo-random operands and counts the 32-bit words in which
// the outputs differ: every tile form accumulates each output element in the same k order, so the count must be 0.
int svc_op_gemm_forms_diff(int M, int N, int K, int epi, int debug_a, int debug_b, long long* n_diff, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(M > 0 && N > 0 && K > 0 && N % 8 == 0 && n_diff, "shape (N must be a multiple of 8)");
    SVC_REQUIRE(epi == KG_EPI_STORE || ((epi == KG_EPI_SWIGLU || epi == KG_EPI_TANHSIG) && N % 2 == 0) ||
                    (epi == KG_EPI_QKV_ROPE && N % 384 == 0), "epilogue kind / width (QKV: N = 3 D, D a multiple of 128)");
    Scratch s;
    const int L = 864;
    const long Kp = round_up(K, 64), Np = round_up(N, 256);
    const long nseq = (M + L - 1) / L;
    const long n_c = (long)nseq * L * N, n_vt = nseq * (long)(N / 3 + 1) * 896 + 4096;
    half_t* ap = s.ar.alloc_n<half_t>((size_t)nseq * L * Kp, st);
    half_t* wp = s.ar.alloc_n<half_t>((size_t)Np * Kp, st);
    float* res = s.ar.alloc_n<float>((size_t)n_c, st);
    float* bias = s.ar.alloc_n<float>((size_t)Np, st);
    float* rope = s.ar.alloc_n<float>((size_t)L * 64, st);
    float* c32[2]; half_t* c16[2]; half_t* vt[2];
    for (int v = 0; v < 2; ++v) {
        c32[v] = s.ar.alloc_n<float>((size_t)n_c, st);
        c16[v] = s.ar.alloc_n<half_t>((size_t)n_c, st);
        vt[v] = s.ar.alloc_n<half_t>((size_t)n_vt, st);
        if (!c32[v] || !c16[v] || !vt[v]) return 1;
        SVC_CHECK_HIP(hipMemsetAsync(c32[v], 0, (size_t)n_c * 4, st));
        SVC_CHECK_HIP(hipMemsetAsync(c16[v], 0, (size_t)n_c * 2, st));
        SVC_CHECK_HIP(hipMemsetAsync(vt[v], 0, (size_t)n_vt * 2, st));
    }
    unsigned long long* cnt = s.ar.alloc_n<unsigned long long>(1, st);
    if (!ap || !wp || !res || !bias || !rope || !cnt) return 1;
    SVC_CHECK_HIP(hipMemsetAsync(cnt, 0, 8, st));
    hipLaunchKernelGGL(bench_fill_kernel<half_t>, dim3(1024), dim3(256), 0, st, ap, (long)nseq * L * Kp, 11u);
    hipLaunchKernelGGL(bench_fill_kernel<half_t>, dim3(1024), dim3(256), 0, st, wp, (long)Np * Kp, 12u);
    hipLaunchKernelGGL(bench_fill_kernel<float>, dim3(1024), dim3(256), 0, st, res, n_c, 13u);
    hipLaunchKernelGGL(bench_fill_kernel<float>, dim3(64), dim3(256), 0, st, bias, Np, 14u);
    hipLaunchKernelGGL(bench_fill_kernel<float>, dim3(64), dim3(256), 0, st, rope, (long)L * 64, 15u);
    for (int v = 0; v < 2; ++v) {
        KGemmParams p;
        memset(&p, 0, sizeof(p));
        p.M = M; p.N = N; p.Lout = L; p.a_seq_rows = L; p.c_seq_rows = L; p.a_stride = 1; p.a_len = L;
        p.n_taps = 1; p.a_ptr[0] = ap; p.a_ld[0] = Kp; p.a_ktiles[0] = (int)(Kp / 64);
        p.w = wp; p.ldw = Kp; p.vec_ok = 1; p.debug = v ? debug_b : debug_a;
        if (epi != KG_EPI_QKV_ROPE) p.bias = bias;      // the QKV epilogue takes none (kgemm_launch refuses it)
        if (epi == KG_EPI_STORE) { p.c32 = c32[v]; p.ldc32 = N; p.res = res; p.ldres = N; p.c16 = c16[v]; p.ldc16 = N; }
        else if (epi == KG_EPI_QKV_ROPE) { p.c16 = c16[v]; p.ldc16 = 2 * (N / 3); p.rope = rope; p.rope_D = N / 3; p.q_scale = 0.125f;
                                           p.vt = vt[v]; p.vt_seq_stride = (long)(N / 3) * 896; p.vt_ld = 896; p.vt_mode = 1; }
        else { p.c16 = c16[v]; p.ldc16 = N / 2; }
        if (kgemm_launch(p, 0, epi, st)) return 1;
    }
    hipLaunchKernelGGL(bench_diff_kernel, dim3(1024), dim3(256), 0, st, (const unsigned*)c32[0], (const unsigned*)c32[1], n_c, cnt);
    hipLaunchKernelGGL(bench_diff_kernel, dim3(1024), dim3(256), 0, st, (const unsigned*)c16[0], (const unsigned*)c16[1], n_c / 2, cnt);
    hipLaunchKernelGGL(bench_diff_kernel, dim3(1024), dim3(256), 0, st, (const unsigned*)vt[0], (const unsigned*)vt[1], n_vt / 2, cnt);
    unsigned long long h = 0;
    SVC_CHECK_HIP(hipMemcpyAsync(&h, cnt, 8, hipMemcpyDeviceToHost, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    *n_diff = (long long)h;
    return 0;
}

// The tap-GEMM's row map on the host (kgemm_tile.h, KG_TAP_SETUP): the row of its sequence that (pos, shift) reads, or -1 where
// the kernel takes the zero page instead.
static long kgemm_host_row(long pos, int a_stride, int shift, long len, int pad_mode, int reflect_min) {
    const long q0 = pos * a_stride + shift;
    const bool oob = q0 < 0 || q0 >= len;
    if (!oob) return q0;
    if (pad_mode == KG_PAD_ZERO) return -1;
    if (pad_mode == KG_PAD_CLAMP) return q0 < 0 ? 0 : len - 1;
    const long lenx = len > reflect_min ? len : reflect_min;
    const long q = q0 < 0 ? -q0 : (q0 >= lenx ? 2 * (lenx - 1) - q0 : q0);      // [len, lenx): a row of the zero extension
    return (q < 0 || q >= len) ? -1 : q;
}

// One kgemm_launch on caller-supplied operands (tests/test_gpu_kgemm.py).  Every row the launch can address is checked on the
// host first: the kernel itself checks nothing.
int svc_op_kgemm(const svc_kgemm_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(e, "svc_op_kgemm: null argument");
    SVC_REQUIRE(e->dtype == 0 || e->dtype == 1, "svc_op_kgemm: dtype is 0 (fp16) or 1 (fp32)");
    SVC_REQUIRE(e->epi >= KG_EPI_STORE && e->epi <= KG_EPI_QKV_ROPE, "svc_op_kgemm: epi is 0 .. 3");
    SVC_REQUIRE((e->form & ~0xF0) == 0, "svc_op_kgemm: form holds launch_wide's bits 0xF0 only");
    SVC_REQUIRE(e->n_src >= 1 && e->n_src <= 4, "svc_op_kgemm: n_src is 1 .. 4");
    SVC_REQUIRE(e->n_taps >= 1 && e->n_taps <= KG_MAX_TAPS, "svc_op_kgemm: n_taps is 1 .. 48");
    SVC_REQUIRE(e->M >= 1 && e->N >= 1 && e->Lout >= 1 && e->a_stride >= 1 && e->a_seq_rows >= 0 && e->a_off >= 0,
                "svc_op_kgemm: M, N, Lout and a_stride are positive, a_seq_rows and a_off are not negative");
    SVC_REQUIRE(e->pad_mode >= KG_PAD_ZERO && e->pad_mode <= KG_PAD_CLAMP && e->reflect_min >= 0, "svc_op_kgemm: pad_mode is 0 .. 2, reflect_min >= 0");
    SVC_REQUIRE(e->w, "svc_op_kgemm: w is required");
    for (int i = 0; i < e->n_src; ++i)
        SVC_REQUIRE(e->a_src[i] && e->a_rows[i] >= 1 && e->a_K[i] >= 1, "svc_op_kgemm: every source has a buffer, rows and K");
    long Ktot = 0;
    for (int t = 0; t < e->n_taps; ++t) {
        SVC_REQUIRE(e->tap_src[t] >= 0 && e->tap_src[t] < e->n_src, "svc_op_kgemm: a tap's source lies in [0, n_src)");
        SVC_REQUIRE(e->tap_K[t] == e->a_K[e->tap_src[t]], "svc_op_kgemm: a tap's K is its source's K");
        Ktot += e->tap_K[t];
    }
    const long nseq = (e->M + (long)e->Lout - 1) / e->Lout;
    SVC_REQUIRE(e->w_rows == round_up(e->N, 256), "svc_op_kgemm: w has N rounded up to 256 rows");

    // ---- the rows the launch reads: every (m, tap), as the kernel maps them
    for (long s = 0; s < nseq; ++s) {
        const long len = e->seq_len ? e->seq_len[s] : e->a_len;
        SVC_REQUIRE(len >= 0, "svc_op_kgemm: a sequence length is negative");
        SVC_REQUIRE(e->pad_mode != KG_PAD_CLAMP || len >= 1, "svc_op_kgemm: KG_PAD_CLAMP has no row to clamp to in a sequence of length 0");
        const long smap = e->a_seq_map ? e->a_seq_map[s] : s;
        SVC_REQUIRE(smap >= 0, "svc_op_kgemm: an a_seq_map entry is negative");
        const long base = smap * e->a_seq_rows + e->a_off;
        const long npos = std::min<long>(e->Lout, e->M - s * e->Lout);
        for (int t = 0; t < e->n_taps; ++t) {
            long lo = -1, hi = -1;
            for (long pos = 0; pos < npos; ++pos) {
                const long q = kgemm_host_row(pos, e->a_stride, e->tap_shift[t], len, e->pad_mode, e->reflect_min);
                if (q < 0) continue;
                lo = lo < 0 || q < lo ? q : lo;
                hi = q > hi ? q : hi;
            }
            SVC_REQUIRE(hi < 0 || (base + lo >= 0 && base + hi < e->a_rows[e->tap_src[t]]),
                        "svc_op_kgemm: a source row addressed by the row map lies outside its buffer");
        }
    }
    // ---- the rows and columns it writes
    const bool paired = e->epi == KG_EPI_SWIGLU || e->epi == KG_EPI_TANHSIG, qkv = e->epi == KG_EPI_QKV_ROPE;
    const long width = paired ? e->N / 2 : (qkv ? 2L * e->rope_D : e->N);
    SVC_REQUIRE(e->c32 || e->c16, "svc_op_kgemm: an output (c32 or c16) is required");
    SVC_REQUIRE(!e->c16_lo || (e->post_a && e->post_ib), "svc_op_kgemm: c16_lo is an output of the Snake (post_a, post_ib)");
    SVC_REQUIRE(!e->post_a == !e->post_ib && e->post_n >= 0, "svc_op_kgemm: post_a and post_ib come together, post_n >= 0");
    SVC_REQUIRE(e->c_off >= 0 && e->c_off + (long)e->Lout <= e->c_seq_rows && nseq * e->c_seq_rows <= e->c_rows,
                "svc_op_kgemm: output rows: c_off + Lout <= c_seq_rows, nseq c_seq_rows <= c_rows");
    SVC_REQUIRE(e->ldc >= width && width >= 1, "svc_op_kgemm: ldc covers the written width");
    SVC_REQUIRE(e->ld_rowvec >= 0 && e->ld_gate >= 0, "svc_op_kgemm: ld_rowvec and ld_gate are not negative");
    if (e->vec_ok || paired || qkv) {
        auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
        SVC_REQUIRE(e->N % 8 == 0 && e->ldc % 8 == 0, "svc_op_kgemm: 16-byte access needs N and ldc to be multiples of 8");
        SVC_REQUIRE(al16(e->c32) && al16(e->c16) && al16(e->c16_lo) && al16(e->res) && al16(e->res2) && al16(e->bias) && al16(e->rope) && al16(e->vt),
                    "svc_op_kgemm: 16-byte access needs 16-byte aligned c32, c16, c16_lo, res, res2, bias, rope and vt");
    }
    if (qkv) {
        SVC_REQUIRE(e->rope && e->vt && e->rope_D >= 1, "svc_op_kgemm: QKV_ROPE needs rope, vt and rope_D");
        SVC_REQUIRE(e->rope_rows >= e->Lout, "svc_op_kgemm: rope has a row for every position below Lout");
        SVC_REQUIRE(e->vt_mode >= 0 && e->vt_mode <= 2 && e->vt_ld % 4 == 0 && e->vt_ld >= round_up(e->Lout, 32),
                    "svc_op_kgemm: vt_mode is 0 .. 2, vt_ld a multiple of 4 that covers Lout rounded up to 32 (vt_pos permutes inside 32)");
    }

    KGemmParams p;
    memset(&p, 0, sizeof(p));
    const int kt = ktile_elems(e->dtype);
    p.n_taps = e->n_taps;
    p.Lout = e->Lout; p.a_seq_rows = e->a_seq_rows; p.a_off = e->a_off; p.a_stride = e->a_stride; p.a_len = e->a_len;
    p.pad_mode = e->pad_mode; p.reflect_min = e->reflect_min; p.debug = e->form;
    p.M = e->M; p.N = e->N; p.c_seq_rows = e->c_seq_rows; p.c_off = e->c_off;
    p.c32 = e->c32; p.ldc32 = e->ldc; p.c16 = (half_t*)e->c16; p.c16_lo = (half_t*)e->c16_lo; p.ldc16 = e->ldc;
    p.post_a = e->post_a; p.post_ib = e->post_ib; p.post_n = e->post_n;
    p.bias = e->bias; p.rowvec = e->rowvec; p.ld_rowvec = e->ld_rowvec; p.gate = e->gate; p.ld_gate = e->ld_gate;
    p.res = e->res; p.ldres = e->ldc; p.res2 = e->res2; p.ldres2 = e->ldc;
    p.out_scale = e->out_scale; p.act = e->act; p.act_slope = e->act_slope; p.post_relu = e->post_relu; p.vec_ok = e->vec_ok;
    p.rope = e->rope; p.rope_D = e->rope_D; p.q_scale = e->q_scale;
    p.vt = (half_t*)e->vt; p.vt_ld = e->vt_ld; p.vt_seq_stride = (long)e->rope_D * e->vt_ld; p.vt_mode = e->vt_mode;
    if (kgemm_check(p, e->epi)) return 1;      // the launch's own refusals, ahead of the first allocation
    SVC_REQUIRE(e->dtype == 0 || e->epi == KG_EPI_STORE || e->epi == KG_EPI_TANHSIG, "svc_op_kgemm: fp32 operands: STORE and TANHSIG only");
    if (e->check_only) return 0;               // every check has passed; nothing is allocated, packed or launched

    Scratch s;
    void* src[4];
    long src_ld[4];
    for (int i = 0; i < e->n_src; ++i) {
        src_ld[i] = round_up(e->a_K[i], kt);
        src[i] = s.ar.alloc((size_t)e->a_rows[i] * src_ld[i] * esize(e->dtype), st);
        if (!src[i]) return 1;
        if (pack_any(e->dtype, e->a_src[i], src[i], 0, (int)e->a_rows[i], 1, e->a_K[i], e->a_K[i], 0, 1, src_ld[i], 0, 1, nullptr, st)) return 1;
    }
    long Kp = 0;
    for (int t = 0; t < e->n_taps; ++t) Kp += round_up(e->tap_K[t], kt);
    void* wp = s.ar.alloc((size_t)e->w_rows * Kp * esize(e->dtype), st);
    if (!wp) return 1;
    long k_in = 0, k_out = 0;
    for (int t = 0; t < e->n_taps; ++t) {
        const int i = e->tap_src[t];
        p.a_ptr[t] = src[i]; p.a_ld[t] = src_ld[i]; p.a_shift[t] = e->tap_shift[t];
        p.a_ktiles[t] = (int)(src_ld[i] * (long)esize(e->dtype) / 128);
        if (pack_any(e->dtype, e->w + k_in, wp, k_out, (int)e->w_rows, 1, e->tap_K[t], Ktot, 0, 1, Kp, 0, 1, nullptr, st)) return 1;
        k_in += e->tap_K[t];
        k_out += src_ld[i];
    }
    p.w = wp; p.ldw = Kp;
    if (e->seq_len || e->a_seq_map) {
        int* d = s.ar.alloc_n<int>((size_t)2 * nseq, st);
        if (!d) return 1;
        std::vector<int> h((size_t)2 * nseq, 0);
        for (long i = 0; i < nseq; ++i) {
            if (e->seq_len) h[i] = e->seq_len[i];
            if (e->a_seq_map) h[nseq + i] = e->a_seq_map[i];
        }
        SVC_CHECK_HIP(hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));            // `h` leaves scope below
        if (e->seq_len) p.seq_len = d;
        if (e->a_seq_map) p.a_seq_map = d + nseq;
    }
    if (kgemm_launch(p, e->dtype, e->epi, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_op_permute_vt(uint16_t* vt, int64_t rows, int64_t vt_ld, int mode, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(vt && rows >= 1 && vt_ld >= 32 && vt_ld % 32 == 0 && mode >= 0 && mode <= 2,
                "svc_op_permute_vt: vt [rows >= 1][vt_ld a positive multiple of 32], mode 0 .. 2");
    if (attention_permute_vt(reinterpret_cast<half_t*>(vt), rows, vt_ld, mode, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_op_attention(const float* q, const float* k, const float* v, float* out, int N, int T, int H,
                     const int64_t* kv_lens_host, void* stream) {
    // q,k,v,out: [N][T][H][64] fp32.  Packs into the kernel's layout: qk16 [N*Tr][2D] (q pre-scaled), vt [N][D][vt_ld].
    hipStream_t st = (hipStream_t)stream;
    Scratch s;
    const int D = H * 64;
    const int Tr = (int)round_up(T, 8);
    const int vt_ld = (int)round_up(Tr, 64);
    half_t* qk = s.ar.alloc_n<half_t>((size_t)N * Tr * 2 * D, st);
    half_t* vt = s.ar.alloc_n<half_t>((size_t)N * D * vt_ld, st);
    half_t* o16 = s.ar.alloc_n<half_t>((size_t)N * Tr * D, st);
    float* qs = s.ar.alloc_n<float>((size_t)N * T * D, st);
    int* d_len = s.ar.alloc_n<int>(N, st);
    if (!qk || !vt || !o16 || !qs || !d_len) return 1;
    std::vector<float> scale(1, 0.125f * 1.4426950408889634f);
    float* d_scale = s.ar.alloc_n<float>(1, st);
    if (!d_scale) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(d_scale, scale.data(), 4, hipMemcpyHostToDevice, st));
    // q * scale: use pack with a 1-row "scale" (dim0 = 1)
    if (pack_f32_launch(q, qs, 1, 1, N * T * D, 0, 0, 1, 0, 0, 1, d_scale, st)) return 1;
    for (int n = 0; n < N; ++n) {
        if (pack_f16_launch(qs + (long)n * T * D, qk + (long)n * Tr * 2 * D, T, 1, D, D, 0, 1, 2L * D, 0, 1, nullptr, st)) return 1;
        if (pack_f16_launch(k + (long)n * T * D, qk + (long)n * Tr * 2 * D + D, T, 1, D, D, 0, 1, 2L * D, 0, 1, nullptr, st)) return 1;
        // v [T][D] -> vt [D][vt_ld]
        if (pack_f16_launch(v + (long)n * T * D, vt + (long)n * D * vt_ld, T, 1, D, D, 0, 1, 1, 0, vt_ld, nullptr, st)) return 1;
    }
    std::vector<int> lens(N);
    for (int n = 0; n < N; ++n) lens[n] = kv_lens_host ? (int)kv_lens_host[n] : T;
    SVC_CHECK_HIP(hipMemcpyAsync(d_len, lens.data(), N * 4, hipMemcpyHostToDevice, st));
    AttnParams a;
    memset(&a, 0, sizeof(a));
    a.q = qk; a.k = qk + D; a.ld_qk = 2 * D; a.vt = vt; a.vt_seq_stride = (long)D * vt_ld; a.vt_ld = vt_ld;
    a.out = o16; a.ld_out = D; a.n_seq = N; a.H = H; a.seq_rows = Tr; a.Tq = T; a.kv_len = d_len;
    // SVC_ATTN32=1: the 32x32x16 kernels want their own V^T column order (the model's QKV epilogues write it directly; here
    // the natural-order buffer is permuted in place); by default the 16x16x32 kernels run on the natural order
    if (attention_vt_mode(N, H, T) == 2) {
        if (attention_permute_vt(vt, (long)N * D, vt_ld, 2, st)) return 1;
        a.vt_perm = 2;
    }
    if (attention_launch(a, st)) return 1;
    // back to fp32 [N][T][D]
    {
        // reuse pack kernel semantics via a tiny cast: half -> float needs its own kernel; do it through hipMemcpy + host
        std::vector<half_t> h((size_t)N * Tr * D);
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        SVC_CHECK_HIP(hipMemcpy(h.data(), o16, h.size() * 2, hipMemcpyDeviceToHost));
        std::vector<float> f((size_t)N * T * D);
        for (int n = 0; n < N; ++n)
            for (int t = 0; t < T; ++t)
                for (int d = 0; d < D; ++d) f[((size_t)n * T + t) * D + d] = (float)h[((size_t)n * Tr + t) * D + d];
        SVC_CHECK_HIP(hipMemcpy(out, f.data(), f.size() * 4, hipMemcpyHostToDevice));
    }
    return 0;
}

int svc_op_attention_x3(const float* q, const float* k, const float* v, float* out, int n_seq, int seq_rows, int H, int Tq,
                        int q_start, const int64_t* kv_lens, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(q && k && v && out && kv_lens, "svc_op_attention_x3: null argument");
    SVC_REQUIRE(n_seq >= 1 && H >= 1 && seq_rows >= 1, "svc_op_attention_x3: n_seq, H and seq_rows are positive");
    SVC_REQUIRE(Tq >= 1 && Tq <= seq_rows && q_start >= 0 && q_start < Tq, "svc_op_attention_x3: 0 <= q_start < Tq <= seq_rows");
    std::vector<int> lens(n_seq);
    for (int n = 0; n < n_seq; ++n) {
        SVC_REQUIRE(kv_lens[n] >= 0 && kv_lens[n] <= seq_rows, "svc_op_attention_x3: kv_lens within [0, seq_rows]");
        lens[n] = (int)kv_lens[n];
    }
    Scratch s;
    const int D = H * 64;
    const long rows = (long)n_seq * seq_rows;
    const long vt_ld = round_up(seq_rows, 32);
    half_t* qk = s.ar.alloc_n<half_t>((size_t)rows * 4 * D, st);          // [q_hi | k_hi | q_lo | k_lo] rows
    half_t* vt = s.ar.alloc_n<half_t>((size_t)n_seq * D * vt_ld * 2, st);  // hi planes of all sequences, then lo
    int* d_len = s.ar.alloc_n<int>(n_seq, st);
    if (!qk || !vt || !d_len) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(d_len, lens.data(), (size_t)n_seq * 4, hipMemcpyHostToDevice, st));
    half_t* vt_lo = vt + (long)n_seq * D * vt_ld;
    if (attention_x3_prepare(q, k, v, D, nullptr, 0.125f * 1.4426950408889634f, qk, qk + 2 * D, qk + D, qk + 3 * D, 4 * D, vt,
                             vt_lo, (long)D * vt_ld, vt_ld, n_seq, seq_rows, D, st)) return 1;
    AttnX3Params a;
    memset(&a, 0, sizeof(a));
    a.q_hi = qk; a.q_lo = qk + 2 * D; a.k_hi = qk + D; a.k_lo = qk + 3 * D; a.ld_qk = 4 * D;
    a.vt_hi = vt; a.vt_lo = vt_lo; a.vt_seq_stride = (long)D * vt_ld; a.vt_ld = vt_ld;
    a.out32 = out; a.ld_out = D;
    a.n_seq = n_seq; a.H = H; a.seq_rows = seq_rows; a.Tq = Tq; a.q_start = q_start; a.kv_len = d_len;
    if (attention_x3_launch(a, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// One attention_launch on buffers already in the kernels' layout (tests/test_gpu_attention.py): no packing, so the test owns every
// byte the kernels read.  Everything is checked before the first allocation; the lengths travel as a host array.
int svc_op_attention_ex(const svc_attention_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(e, "svc_op_attention_ex: null argument");
    SVC_REQUIRE(e->q && e->k && e->vt, "svc_op_attention_ex: q, k and vt are required");
    SVC_REQUIRE((e->out != nullptr) != (e->out32 != nullptr), "svc_op_attention_ex: exactly one of out and out32");
    SVC_REQUIRE(e->vt_perm >= 0 && e->vt_perm <= 2, "svc_op_attention_ex: vt_perm is 0 .. 2");
    SVC_REQUIRE(e->qt_form >= 0 && e->qt_form <= 2, "svc_op_attention_ex: qt_form is 0 .. 2");
    SVC_REQUIRE(e->n_seq >= 1 && e->H >= 1 && e->seq_rows >= 1, "svc_op_attention_ex: n_seq, H and seq_rows are positive");
    SVC_REQUIRE(e->Tq >= 1 && e->Tq <= e->seq_rows, "svc_op_attention_ex: 1 <= Tq <= seq_rows");
    SVC_REQUIRE(e->q_start >= 0 && e->q_start < e->Tq, "svc_op_attention_ex: 0 <= q_start < Tq");
    const long D = (long)e->H * 64;
    SVC_REQUIRE(e->vt_ld > 0 && e->vt_ld % 64 == 0 && e->ld_qk % 8 == 0 && e->ld_out % 4 == 0 && e->vt_seq_stride % 8 == 0,
                "svc_op_attention_ex: alignment: vt_ld a multiple of 64, ld_qk and vt_seq_stride of 8, ld_out of 4");
    SVC_REQUIRE(e->ld_qk >= D && e->ld_out >= D, "svc_op_attention_ex: ld_qk and ld_out cover H * 64 columns");
    SVC_REQUIRE(e->vt_seq_stride >= D * e->vt_ld, "svc_op_attention_ex: vt_seq_stride >= H * 64 * vt_ld");
    SVC_REQUIRE((uintptr_t)e->q % 16 == 0 && (uintptr_t)e->k % 16 == 0 && (uintptr_t)e->vt % 16 == 0 && (uintptr_t)e->out % 8 == 0 &&
                (uintptr_t)e->out32 % 16 == 0, "svc_op_attention_ex: alignment: q, k, vt and out32 to 16 bytes, out to 8");
    for (int n = 0; n < (e->kv_len ? e->n_seq : 1); ++n) {
        const long len = e->kv_len ? (long)e->kv_len[n] : (long)e->kv_len_const;
        SVC_REQUIRE(len >= 0 && len <= e->seq_rows && round_up(len, 64) <= e->vt_ld,
                    "svc_op_attention_ex: kv_len within [0, seq_rows], and within vt_ld when rounded up to a key tile of 64");
    }
    Scratch s;
    AttnParams a;
    memset(&a, 0, sizeof(a));
    if (e->kv_len) {
        int* d_len = s.ar.alloc_n<int>(e->n_seq, st);
        if (!d_len) return 1;
        std::vector<int> lens(e->n_seq);
        for (int n = 0; n < e->n_seq; ++n) lens[n] = (int)e->kv_len[n];
        SVC_CHECK_HIP(hipMemcpyAsync(d_len, lens.data(), (size_t)e->n_seq * 4, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));            // `lens` leaves scope below
        a.kv_len = d_len;
    }
    a.q = (const half_t*)e->q; a.k = (const half_t*)e->k; a.ld_qk = e->ld_qk;
    a.vt = (const half_t*)e->vt; a.vt_seq_stride = e->vt_seq_stride; a.vt_ld = e->vt_ld;
    a.out = (half_t*)e->out; a.out32 = e->out32; a.ld_out = e->ld_out;
    a.n_seq = e->n_seq; a.H = e->H; a.seq_rows = e->seq_rows; a.Tq = e->Tq; a.q_start = e->q_start;
    a.kv_len_const = e->kv_len_const; a.vt_perm = e->vt_perm; a.qt_form = e->qt_form;
    if (attention_launch(a, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_op_rmsnorm(const float* x, const float* gamma, const float* w, const float* b, int add_one, float* y, int rows,
                   int D, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    Scratch s;
    half_t* y16 = s.ar.alloc_n<half_t>((size_t)rows * D, st);
    if (!y16) return 1;
    if (rmsnorm_mod_launch(x, D, y16, D, gamma, w, b, 0, add_one, rows, D, rows, 1e-5f, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    std::vector<half_t> h((size_t)rows * D);
    SVC_CHECK_HIP(hipMemcpy(h.data(), y16, h.size() * 2, hipMemcpyDeviceToHost));
    std::vector<float> f(h.size());
    for (size_t i = 0; i < h.size(); ++i) f[i] = (float)h[i];
    SVC_CHECK_HIP(hipMemcpy(y, f.data(), f.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// One launch of the fused DiT row-panel kernel on unpacked weights (tests/test_gpu_panel.py): packs the stream of the enabled
// phases in the order dit.hip builds its streams ([merge | wo, mlp | skip | qkv | head]) and launches once.
int svc_op_dit_panel(const svc_dit_panel_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(e, "svc_op_dit_panel: null argument");
    const int D = e->D, I = e->I;
    SVC_REQUIRE(D == 384 || D == 512, "svc_op_dit_panel: D must be 384 or 512");
    SVC_REQUIRE(I >= 0 && I % 32 == 0 && (!e->do_post || I >= 32), "svc_op_dit_panel: I is a positive multiple of 32");
    SVC_REQUIRE(e->n_seq >= 1 && e->Lout >= 1 && e->M == e->n_seq * e->Lout && e->row_off >= 0 && e->row_off + e->Lout <= e->seq_rows,
                "svc_op_dit_panel: M = n_seq * Lout rows, row_off + Lout <= seq_rows");
    SVC_REQUIRE(e->x, "svc_op_dit_panel: x is null");
    SVC_REQUIRE(!e->do_post || (e->wo && e->w1 && e->w3 && e->w2 && e->ao && e->g_ffn), "svc_op_dit_panel: do_post needs wo, w1, w3, w2, ao and g_ffn");
    SVC_REQUIRE(e->do_post || !e->c16, "svc_op_dit_panel: c16 is an output of do_post");
    SVC_REQUIRE(!e->do_skip || (e->wskip && e->skip_in), "svc_op_dit_panel: do_skip needs wskip and skip_in");
    SVC_REQUIRE(!e->do_qkv || (e->wqkv && e->g_attn && e->rope && e->qk && e->vt), "svc_op_dit_panel: do_qkv needs wqkv, g_attn, rope, qk and vt");
    if (e->do_qkv) {
        const long reach = round_up(e->row_off + e->Lout, 32);      // vt_pos permutes inside groups of 32 (mode 2: 16) positions
        SVC_REQUIRE(e->vt_mode >= 0 && e->vt_mode <= 2 && e->vt_ld >= reach && e->vt_ld % 4 == 0 && e->vt_seq_stride >= (long)D * e->vt_ld &&
                    e->vt_seq_stride % 4 == 0, "svc_op_dit_panel: vt_mode 0 .. 2, vt_ld covers the positions rounded up to 32, vt_seq_stride >= D vt_ld");
    }
    SVC_REQUIRE(!e->do_final || e->g_fin, "svc_op_dit_panel: do_final needs g_fin");
    SVC_REQUIRE(!e->do_final || e->seam == PANEL_SEAM_HEAD || e->n16, "svc_op_dit_panel: do_final needs n16");
    SVC_REQUIRE(e->seam != PANEL_SEAM_MERGE || (e->w_merge && e->C >= 1 && e->C <= PANEL_MERGE_K && e->ldw >= e->C),
                "svc_op_dit_panel: the merge seam needs w_merge [D][ldw] with 1 <= C <= 128 and ldw >= C");
    SVC_REQUIRE(e->seam != PANEL_SEAM_HEAD || (e->head_wa && e->head_w2), "svc_op_dit_panel: the head seam needs head_wa and head_w2");

    const bool merge = e->seam == PANEL_SEAM_MERGE, head = e->seam == PANEL_SEAM_HEAD;
    const long slot_halfs = (long)(D / 16) * 512;
    const long merge_halfs = merge ? fused_seam_slots(D, PANEL_SEAM_MERGE, e->C) * slot_halfs : 0;
    const long body_halfs = fused_stream_halfs(D, I, e->do_post != 0, e->do_skip != 0, e->do_qkv != 0);

    PanelParams p;
    memset(&p, 0, sizeof(p));
    p.M = e->M; p.Lout = e->Lout; p.seq_rows = e->seq_rows; p.row_off = e->row_off;
    p.eps = e->eps; p.add_one = e->add_one; p.I = I;
    p.do_post = e->do_post; p.do_skip = e->do_skip; p.do_qkv = e->do_qkv; p.do_final = e->do_final; p.seam = e->seam;
    p.ao = reinterpret_cast<const half_t*>(e->ao); p.x = e->x;
    p.gate_a = e->gate_a; p.gate_f = e->gate_f; p.g_ffn = e->g_ffn; p.w_f = e->w_f; p.b_f = e->b_f;
    p.c16 = reinterpret_cast<half_t*>(e->c16);
    p.skip_in = reinterpret_cast<const half_t*>(e->skip_in); p.bskip = e->bskip;
    p.g_attn = e->g_attn; p.w_a = e->w_a; p.b_a = e->b_a; p.rope = e->rope; p.q_scale = e->q_scale;
    p.qk = reinterpret_cast<half_t*>(e->qk); p.vt = reinterpret_cast<half_t*>(e->vt);
    p.vt_seq_stride = e->vt_seq_stride; p.vt_ld = e->vt_ld; p.vt_mode = e->vt_mode;
    p.g_fin = e->g_fin; p.w_fin = e->w_fin; p.b_fin = e->b_fin; p.n16 = reinterpret_cast<half_t*>(e->n16);
    p.x16 = reinterpret_cast<const half_t*>(e->x16); p.st_term = e->st_term; p.tok_time = e->tok_time; p.tok_style = e->tok_style;
    p.zero_row = e->st_term;      // stands in until the checks have passed: they ask only that the row is there
    p.npre = e->npre; p.time_first = e->time_first; p.T = e->T;
    p.head_b0 = e->head_b0; p.head_b2 = e->head_b2; p.v32 = e->v32; p.ldv = e->ldv; p.head_C = e->head_C;
    p.n_slots = (int)((merge_halfs + body_halfs) / slot_halfs + (head ? fused_seam_slots(D, PANEL_SEAM_HEAD, e->head_C) : 0));
    if (fused_panel_check(p, D, e->tm)) return 1;      // before anything is packed: head_C sizes the head's part of the stream

    Scratch s;
    float* zero_row = s.ar.alloc_n<float>(D, st);      // the arena hands out zeroed memory
    if (!zero_row) return 1;
    p.zero_row = zero_row;
    const long total = (long)p.n_slots * slot_halfs;
    half_t* ws = s.ar.alloc_n<half_t>((size_t)total, st);
    if (!ws) return 1;
    long off = 0;
    if (merge) {
        if (fused_pack_merge(ws, D, e->w_merge, e->ldw, e->C, st) != merge_halfs) { set_error("fused stream packing failed"); return 1; }
        off += merge_halfs;
    }
    if (body_halfs) {
        const bool post = e->do_post != 0;
        if (fused_pack_stream(ws + off, D, I, post ? e->wo : nullptr, post ? e->w1 : nullptr, post ? e->w3 : nullptr, post ? e->w2 : nullptr,
                              e->do_skip ? e->wskip : nullptr, e->do_qkv ? e->wqkv : nullptr, st) != body_halfs) {
            set_error("fused stream packing failed");
            return 1;
        }
        off += body_halfs;
    }
    if (head) {
        if (fused_pack_head(ws + off, D, e->head_wa, e->head_w2, e->head_C, st) != total - off) { set_error("fused stream packing failed"); return 1; }
    }
    p.wstream = ws;
    if (fused_panel_launch(p, D, e->gated != 0, st, e->tm)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// chunk2[i] = float(double(chunk2[i]) * fade_in[i] + double(chunk1_tail[i]) * fade_out[i]), i < n: the reference's
// numpy crossfade (inference.py:343-350; float32 * float64 -> float64, stored back to float32), bit for bit
// (separately rounded products and sum, no fma contraction).
__global__ void crossfade_kernel(float* __restrict__ c2, const float* __restrict__ c1, const double* __restrict__ fin,
                                 const double* __restrict__ fout, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = __dmul_rn((double)c2[i], fin[i]);
    const double b = __dmul_rn((double)c1[i], fout[i]);
    c2[i] = (float)__dadd_rn(a, b);
}

int svc_crossfade(float* chunk2, const float* chunk1_tail, const double* fade_in, const double* fade_out, int n, void* stream) {
    SVC_REQUIRE(n >= 0, "crossfade length");
    if (n == 0) return 0;
    SVC_REQUIRE(chunk2 && chunk1_tail && fade_in && fade_out, "null argument");
    hipLaunchKernelGGL(crossfade_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, chunk2, chunk1_tail, fade_in, fade_out, n);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}
}  // extern "C"

// ---- ragged assembly of a v2 batch (modules/v2/vc_wrapper.py:657-660, :700).  Pure copies: one thread per 16 bytes of
// output along the contiguous axis where the shape allows it, coalesced 4-byte accesses otherwise; every output element
// is written, padding included.  Lengths travel as kernel arguments (up to RAG_MAXB utterances per launch), so no host
// array outlives the call and nothing synchronises.
namespace {
constexpr int RAG_MAXB = 64;
struct RagLens { int a[RAG_MAXB], b[RAG_MAXB]; };

// out[b][t][:] = t < P_b ? prompt_cond[b][t] : t < P_b + S_b ? cond[b][t - P_b] : 0.  VT = float4v (Dc % 4 == 0) or float.
template <class VT>
__global__ __launch_bounds__(256) void v2_assemble_cond_kernel(const VT* __restrict__ prompt_cond, const VT* __restrict__ cond,
                                                               const RagLens lens, int Pmax, int Smax, int Dv, int T,
                                                               VT* __restrict__ out) {
    const int b = blockIdx.y;
    const int P = lens.a[b], S = lens.b[b];
    const long n = (long)T * Dv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int t = (int)(i / Dv), c = (int)(i - (long)t * Dv);
        VT v = {};
        if (t < P) v = prompt_cond[((long)b * Pmax + t) * Dv + c];
        else if (t < P + S) v = cond[((long)b * Smax + (t - P)) * Dv + c];
        out[(long)b * n + i] = v;
    }
}

// out[b][c][s] = s < x_lens[b] - P_b ? mel[b][c][P_b + s] : pad.  P_b shifts the source by an arbitrary number of floats:
// 4-byte loads (consecutive lanes read consecutive addresses), one 16-byte store per thread when VEC (Smax % 4 == 0).
template <bool VEC>
__global__ __launch_bounds__(256) void mel_strip_prompt_kernel(const float* __restrict__ mel, const RagLens lens, int C, int T,
                                                               int Smax, float pad, float* __restrict__ out) {
    constexpr int W = VEC ? 4 : 1;
    const int b = blockIdx.y;
    const int P = lens.a[b], n_valid = lens.b[b] - P;
    const int Sv = Smax / W;
    const long n = (long)C * Sv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int c = (int)(i / Sv), s0 = (int)(i - (long)c * Sv) * W;
        const float* src = mel + ((long)b * C + c) * T + P + s0;
        float v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) v[j] = s0 + j < n_valid ? src[j] : pad;
        float* dst = out + ((long)b * C + c) * Smax + s0;
        if constexpr (VEC) *reinterpret_cast<float4v*>(dst) = (float4v){v[0], v[1], v[2], v[3]};
        else dst[0] = v[0];
    }
}


// ---- long-form conversion as a pool of chunks (inference.py:470-527 with the chunks of one or more files run side by side).
constexpr int CHUNK_MAXN = RAG_MAXB;
struct GatherChunks { int P[CHUNK_MAXN], utt[CHUNK_MAXN], row0[CHUNK_MAXN], rows[CHUNK_MAXN]; };

// mu[k][t][:] = t < P_u ? prompt_cond[u][t] : t < P_u + rows[k] ? cond[row0[k] + t - P_u] : 0 (u = utt[k]).  Windows overlap
// in the source, so some rows of cond are read by two chunks.  VT = float4v (Dc % 4 == 0) or float.
template <class VT>
__global__ __launch_bounds__(256) void chunks_gather_cond_kernel(const VT* __restrict__ prompt_cond, const VT* __restrict__ cond,
                                                                 const GatherChunks ch, int Pmax, int Dv, int T, VT* __restrict__ mu) {
    const int k = blockIdx.y;
    const int P = ch.P[k], S = ch.rows[k];
    const VT* pc = prompt_cond + (long)ch.utt[k] * Pmax * Dv;
    const VT* cd = cond + (long)ch.row0[k] * Dv;
    const long n = (long)T * Dv;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int t = (int)(i / Dv);
        VT v = {};
        if (t < P) v = pc[i];
        else if (t < P + S) v = cd[i - (long)P * Dv];
        mu[(long)k * n + i] = v;
    }
}

// One seam sample: float(double(cur) * fade_in + double(tail) * fade_out), the products and the sum rounded separately
// (crossfade_kernel's arithmetic, bit-identical to numpy's).  The one statement of it for chunks_assemble_kernel and
// chunks_emit_kernel, so a file emitted piece by piece cannot drift from the file assembled at once.
__device__ __forceinline__ float seam_sample(float cur, float tail, double fin, double fout) {
    const double a = __dmul_rn((double)cur, fin);
    const double b = __dmul_rn((double)tail, fout);
    return (float)__dadd_rn(a, b);
}

struct AssembleChunks {
    long long off[CHUNK_MAXN];      // first output sample of the chunk's body
    int len[CHUNK_MAXN], body[CHUNK_MAXN];
    int prev_len[CHUNK_MAXN];       // samples of the chunk before it in the same utterance, -1 for a first chunk
};

// out[off[k] + i] = wave[k][i] for a first chunk or i >= ov, else float(double(wave[k][i]) * fade_in[i] +
// double(wave[k-1][len[k-1] - ov + i]) * fade_out[i]) with separately rounded products and sum (crossfade_kernel's
// arithmetic), i < body[k].  Each output sample is written once; no sample at or above len[k] is read.  `wave` points at
// row k0 of the wave buffer (blockIdx.y = 0), so row k - 1 of the launch's first chunk lies before it.  VEC: 4 samples per
// thread (the caller has checked that ov, every len and off, the row stride and the pointers are multiples of 4 floats).
template <bool VEC>
__global__ __launch_bounds__(256) void chunks_assemble_kernel(const float* __restrict__ wave, long stride, const AssembleChunks ch,
                                                              const double* __restrict__ fin, const double* __restrict__ fout, int ov,
                                                              float* __restrict__ out) {
    constexpr int W = VEC ? 4 : 1;
    const int k = blockIdx.y;
    const int body = ch.body[k], prev_len = ch.prev_len[k];
    const float* cur = wave + (long)k * stride;
    float* dst = out + ch.off[k];
    const int n_fade = prev_len < 0 ? 0 : ov;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g * W < body; g += (long)gridDim.x * 256) {
        const int i0 = (int)g * W;
        float v[W];
        if constexpr (VEC) {
            const float4v x = *reinterpret_cast<const float4v*>(cur + i0);
            v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
        } else {
            v[0] = cur[i0];
        }
        if (i0 < n_fade) {           // ov is a multiple of W: the whole group lies inside the seam
            const float* tail = cur - stride + (prev_len - ov);      // prev_len >= ov: that chunk is not its utterance's last
            float p[W];
            if constexpr (VEC) {
                const float4v x = *reinterpret_cast<const float4v*>(tail + i0);
                p[0] = x[0]; p[1] = x[1]; p[2] = x[2]; p[3] = x[3];
            } else {
                p[0] = tail[i0];
            }
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = seam_sample(v[j], p[j], fin[i0 + j], fout[i0 + j]);
        }
        if constexpr (VEC) *reinterpret_cast<float4v*>(dst + i0) = (float4v){v[0], v[1], v[2], v[3]};
        else dst[i0] = v[0];
    }
}

struct EmitPieces {
    long long src[CHUNK_MAXN];      // first float of the piece's row in the wave buffer
    long long tail[CHUNK_MAXN];     // float of the wave buffer that sample 0 of the chunk is faded with, -1 without a seam
    long long dst[CHUNK_MAXN];      // out_off - begin: sample i of the chunk lands at out[dst + i]
    int begin[CHUNK_MAXN], end[CHUNK_MAXN];
};

// (wave * 32768.0).astype(np.int16) with saturation instead of numpy's wrap: the scaling is exact (a power of two),
// the conversion truncates toward zero; NaN gives 0.
__device__ __forceinline__ int16_t pcm16_sample(float v) {
    const float x = v * 32768.0f;
    if (!(x == x)) return 0;
    return (int16_t)(int)fminf(fmaxf(x, -32768.0f), 32767.0f);
}

// out[dst[p] + i] = wave[src[p] + i] for i >= ov or a piece without a seam, else seam_sample(wave[src[p] + i],
// wave[tail[p] + i], fade_in[i], fade_out[i]), begin[p] <= i < end[p]; pcm (may be null) gets pcm16_sample of the same value
// at the same offset.  Only samples begin .. end - 1 of the row and, below ov, the same indices of the tail are read, only
// the piece's range is written.  VEC: 4 samples per thread, a 16-byte load and store and an 8-byte pcm store (the caller has
// checked that ov, every begin, end, out_off, len and prev_len, the row stride and the pointers allow it: then src, tail
// and dst are multiples of 4 floats and a group of 4 lies on one side of ov).
template <bool VEC>
__global__ __launch_bounds__(256) void chunks_emit_kernel(const float* __restrict__ wave, const EmitPieces pc,
                                                          const double* __restrict__ fin, const double* __restrict__ fout, int ov,
                                                          float* __restrict__ out, int16_t* __restrict__ pcm) {
    constexpr int W = VEC ? 4 : 1;
    const int p = blockIdx.y;
    const int begin = pc.begin[p], end = pc.end[p];
    const float* cur = wave + pc.src[p];
    const long long t = pc.tail[p];
    const float* tail = wave + (t < 0 ? 0 : t);
    const int n_fade = t < 0 ? 0 : ov;
    float* dst = out + pc.dst[p];
    int16_t* dpcm = pcm ? pcm + pc.dst[p] : nullptr;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; begin + g * W < end; g += (long)gridDim.x * 256) {
        const int i0 = begin + (int)g * W;
        float v[W];
        if constexpr (VEC) {
            const float4v x = *reinterpret_cast<const float4v*>(cur + i0);
            v[0] = x[0]; v[1] = x[1]; v[2] = x[2]; v[3] = x[3];
        } else {
            v[0] = cur[i0];
        }
        if (i0 < n_fade) {
            float q[W];
            if constexpr (VEC) {
                const float4v x = *reinterpret_cast<const float4v*>(tail + i0);
                q[0] = x[0]; q[1] = x[1]; q[2] = x[2]; q[3] = x[3];
            } else {
                q[0] = tail[i0];
            }
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = seam_sample(v[j], q[j], fin[i0 + j], fout[i0 + j]);
        }
        if constexpr (VEC) *reinterpret_cast<float4v*>(dst + i0) = (float4v){v[0], v[1], v[2], v[3]};
        else dst[i0] = v[0];
        if (dpcm) {
            if constexpr (VEC) {
                typedef short short4v __attribute__((ext_vector_type(4)));
                *reinterpret_cast<short4v*>(dpcm + i0) =
                    (short4v){pcm16_sample(v[0]), pcm16_sample(v[1]), pcm16_sample(v[2]), pcm16_sample(v[3])};
            } else {
                dpcm[i0] = pcm16_sample(v[0]);
            }
        }
    }
}
}  // namespace

extern "C" {

int svc_v2_assemble_cond(const float* prompt_cond, const int32_t* prompt_lens, const float* cond, const int32_t* cond_lens, int B,
                         int Pmax, int Smax, int Dc, int T, float* out, void* stream) {
    SVC_REQUIRE(B >= 0 && Pmax >= 0 && Smax >= 0 && Dc >= 1 && T >= 0, "bad argument");
    if (B == 0 || T == 0) return 0;
    SVC_REQUIRE(out && prompt_lens && cond_lens && (prompt_cond || Pmax == 0) && (cond || Smax == 0), "null argument");
    for (int b = 0; b < B; ++b)
        SVC_REQUIRE(prompt_lens[b] >= 0 && prompt_lens[b] <= Pmax && cond_lens[b] >= 0 && cond_lens[b] <= Smax &&
                        (long)prompt_lens[b] + cond_lens[b] <= T,
                    "assemble_cond: lengths outside 0 .. Pmax / 0 .. Smax, or prompt + cond frames above T");
    const bool vec = Dc % 4 == 0 && (((uintptr_t)prompt_cond | (uintptr_t)cond | (uintptr_t)out) & 15) == 0;
    const int Dv = vec ? Dc / 4 : Dc;
    const int gx = (int)std::min<long>(cdiv((long)T * Dv, 256), 4096);
    for (int b0 = 0; b0 < B; b0 += RAG_MAXB) {
        const int nb = std::min(B - b0, RAG_MAXB);
        RagLens l;
        memset(&l, 0, sizeof(l));
        for (int b = 0; b < nb; ++b) { l.a[b] = prompt_lens[b0 + b]; l.b[b] = cond_lens[b0 + b]; }
        const float* pc = prompt_cond + (long)b0 * Pmax * Dc;
        const float* cd = cond + (long)b0 * Smax * Dc;
        float* o = out + (long)b0 * T * Dc;
        if (vec)
            hipLaunchKernelGGL(v2_assemble_cond_kernel<float4v>, dim3(gx, nb), dim3(256), 0, (hipStream_t)stream,
                               reinterpret_cast<const float4v*>(pc), reinterpret_cast<const float4v*>(cd), l, Pmax, Smax, Dv, T,
                               reinterpret_cast<float4v*>(o));
        else
            hipLaunchKernelGGL(v2_assemble_cond_kernel<float>, dim3(gx, nb), dim3(256), 0, (hipStream_t)stream, pc, cd, l, Pmax, Smax, Dv, T, o);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

int svc_mel_strip_prompt(const float* mel, const int32_t* prompt_lens, const int32_t* x_lens, int B, int C, int T, int Smax,
                         float pad_value, float* out, void* stream) {
    SVC_REQUIRE(B >= 0 && C >= 0 && T >= 0 && Smax >= 0, "bad argument");
    if (B == 0 || C == 0 || Smax == 0) return 0;
    SVC_REQUIRE(out && prompt_lens && x_lens && (mel || T == 0), "null argument");
    for (int b = 0; b < B; ++b)
        SVC_REQUIRE(prompt_lens[b] >= 0 && x_lens[b] >= 0 && x_lens[b] <= T && x_lens[b] - prompt_lens[b] <= Smax,
                    "strip_prompt: x_lens outside 0 .. T, or more than Smax frames after the prompt");
    const bool vec = Smax % 4 == 0 && ((uintptr_t)out & 15) == 0;
    const int gx = (int)std::min<long>(cdiv((long)C * (vec ? Smax / 4 : Smax), 256), 4096);
    for (int b0 = 0; b0 < B; b0 += RAG_MAXB) {
        const int nb = std::min(B - b0, RAG_MAXB);
        RagLens l;
        memset(&l, 0, sizeof(l));
        for (int b = 0; b < nb; ++b) { l.a[b] = prompt_lens[b0 + b]; l.b[b] = x_lens[b0 + b]; }
        const float* src = mel + (long)b0 * C * T;
        float* o = out + (long)b0 * C * Smax;
        if (vec) hipLaunchKernelGGL(mel_strip_prompt_kernel<true>, dim3(gx, nb), dim3(256), 0, (hipStream_t)stream, src, l, C, T, Smax, pad_value, o);
        else hipLaunchKernelGGL(mel_strip_prompt_kernel<false>, dim3(gx, nb), dim3(256), 0, (hipStream_t)stream, src, l, C, T, Smax, pad_value, o);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

int svc_chunks_gather_cond(const float* prompt_cond, const int32_t* prompt_lens, int U, int Pmax, const float* cond, int R,
                           const int32_t* utt, const int32_t* row0, const int32_t* rows, int N, int Dc, int T, float* mu,
                           void* stream) {
    SVC_REQUIRE(U >= 0 && Pmax >= 0 && R >= 0 && N >= 0 && Dc >= 1 && T >= 0, "chunks_gather_cond: bad argument");
    if (N == 0 || T == 0) return 0;
    SVC_REQUIRE(mu && prompt_lens && utt && row0 && rows && (prompt_cond || Pmax == 0) && (cond || R == 0),
                "chunks_gather_cond: null argument");
    for (int u = 0; u < U; ++u)
        SVC_REQUIRE(prompt_lens[u] >= 0 && prompt_lens[u] <= Pmax, "chunks_gather_cond: prompt_lens outside 0 .. Pmax");
    for (int k = 0; k < N; ++k) {
        SVC_REQUIRE(utt[k] >= 0 && utt[k] < U, "chunks_gather_cond: utt outside 0 .. U - 1");
        SVC_REQUIRE(rows[k] >= 0 && row0[k] >= 0 && (long)row0[k] + rows[k] <= R,
                    "chunks_gather_cond: a chunk's rows lie outside cond (0 .. R)");
        SVC_REQUIRE((long)prompt_lens[utt[k]] + rows[k] <= T, "chunks_gather_cond: prompt + chunk frames above T");
    }
    const bool vec = Dc % 4 == 0 && (((uintptr_t)prompt_cond | (uintptr_t)cond | (uintptr_t)mu) & 15) == 0;
    const int Dv = vec ? Dc / 4 : Dc;
    const int gx = (int)std::min<long>(cdiv((long)T * Dv, 256), 4096);
    for (int k0 = 0; k0 < N; k0 += CHUNK_MAXN) {
        const int nk = std::min(N - k0, CHUNK_MAXN);
        GatherChunks ch;
        memset(&ch, 0, sizeof(ch));
        for (int k = 0; k < nk; ++k) {
            ch.utt[k] = utt[k0 + k]; ch.P[k] = prompt_lens[utt[k0 + k]]; ch.row0[k] = row0[k0 + k]; ch.rows[k] = rows[k0 + k];
        }
        float* o = mu + (long)k0 * T * Dc;
        if (vec)
            hipLaunchKernelGGL(chunks_gather_cond_kernel<float4v>, dim3(gx, nk), dim3(256), 0, (hipStream_t)stream,
                               reinterpret_cast<const float4v*>(prompt_cond), reinterpret_cast<const float4v*>(cond), ch, Pmax, Dv, T,
                               reinterpret_cast<float4v*>(o));
        else
            hipLaunchKernelGGL(chunks_gather_cond_kernel<float>, dim3(gx, nk), dim3(256), 0, (hipStream_t)stream, prompt_cond, cond, ch,
                               Pmax, Dv, T, o);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

int svc_chunks_assemble(const float* wave, long long stride, const int32_t* lens, const int32_t* first, const int32_t* last, int N,
                        const double* fade_in, const double* fade_out, int ov, float* out, long long out_len, void* stream) {
    SVC_REQUIRE(N >= 0 && ov >= 0 && out_len >= 0 && stride >= 0, "chunks_assemble: bad argument");
    SVC_REQUIRE(N == 0 || (lens && first && last), "chunks_assemble: null argument");
    long long total = 0;
    int max_body = 0;
    for (int k = 0; k < N; ++k) {
        SVC_REQUIRE(lens[k] >= 0 && lens[k] <= stride, "chunks_assemble: a chunk length outside 0 .. stride");
        SVC_REQUIRE(last[k] || lens[k] >= ov, "chunks_assemble: a chunk that is not the last of its utterance is shorter than the overlap");
        SVC_REQUIRE(k == 0 ? first[k] != 0 : (first[k] != 0) == (last[k - 1] != 0),
                    "chunks_assemble: first / last flags do not form consecutive utterances");
        const int body = lens[k] - (last[k] ? 0 : ov);
        max_body = std::max(max_body, body);
        total += body;
    }
    SVC_REQUIRE(N == 0 || last[N - 1], "chunks_assemble: the last chunk is not flagged last");
    SVC_REQUIRE(total == out_len, "chunks_assemble: out_len is not the sum of the chunk bodies");
    if (out_len == 0) return 0;
    SVC_REQUIRE(wave && out && (ov == 0 || (fade_in && fade_out)), "chunks_assemble: null argument");
    bool vec = ov % 4 == 0 && stride % 4 == 0 && (((uintptr_t)wave | (uintptr_t)out) & 15) == 0;
    for (int k = 0; k < N && vec; ++k) vec = lens[k] % 4 == 0;      // then every body, and so every offset, is one too
    const int gx = (int)std::min<long>(cdiv(cdiv(max_body, vec ? 4 : 1), 256), 4096);
    long long off = 0;
    for (int k0 = 0; k0 < N; k0 += CHUNK_MAXN) {
        const int nk = std::min(N - k0, CHUNK_MAXN);
        AssembleChunks ch;
        memset(&ch, 0, sizeof(ch));
        for (int k = 0; k < nk; ++k) {
            const int g = k0 + k;
            ch.len[k] = lens[g];
            ch.body[k] = lens[g] - (last[g] ? 0 : ov);
            ch.prev_len[k] = first[g] ? -1 : lens[g - 1];
            ch.off[k] = off;
            off += ch.body[k];
        }
        const float* w = wave + (long long)k0 * stride;
        if (vec) hipLaunchKernelGGL(chunks_assemble_kernel<true>, dim3(gx, nk), dim3(256), 0, (hipStream_t)stream, w, (long)stride, ch, fade_in, fade_out, ov, out);
        else hipLaunchKernelGGL(chunks_assemble_kernel<false>, dim3(gx, nk), dim3(256), 0, (hipStream_t)stream, w, (long)stride, ch, fade_in, fade_out, ov, out);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

int svc_chunks_emit(const float* wave, long long stride, int n_rows, const int32_t* row, const int32_t* len, const int32_t* prev_row,
                    const int32_t* prev_len, const int32_t* begin, const int32_t* end, const int64_t* out_off, int N,
                    const double* fade_in, const double* fade_out, int ov, float* out, int16_t* pcm, long long out_len, void* stream) {
    SVC_REQUIRE(N >= 0 && ov >= 0 && out_len >= 0 && stride >= 0 && n_rows >= 0, "chunks_emit: bad argument");
    SVC_REQUIRE(N == 0 || (row && len && prev_row && prev_len && begin && end && out_off), "chunks_emit: null argument");
    std::vector<std::pair<long long, long long>> spans;      // [first, one past the last) output sample of every non-empty piece
    int max_n = 0;
    bool seams = false;
    bool vec = ov % 4 == 0 && stride % 4 == 0 && (((uintptr_t)wave | (uintptr_t)out) & 15) == 0 && ((uintptr_t)pcm & 7) == 0;
    for (int p = 0; p < N; ++p) {
        SVC_REQUIRE(row[p] >= 0 && row[p] < n_rows, "chunks_emit: a row outside 0 .. n_rows - 1");
        SVC_REQUIRE(len[p] >= 0 && len[p] <= stride, "chunks_emit: a chunk length outside 0 .. stride");
        SVC_REQUIRE(begin[p] >= 0 && begin[p] <= end[p] && end[p] <= len[p], "chunks_emit: a piece's range outside 0 <= begin <= end <= len");
        SVC_REQUIRE(prev_row[p] < n_rows, "chunks_emit: a prev_row outside -1 .. n_rows - 1");
        if (prev_row[p] >= 0) {
            SVC_REQUIRE(prev_len[p] <= stride, "chunks_emit: a previous chunk's length outside 0 .. stride");
            SVC_REQUIRE(prev_len[p] >= ov, "chunks_emit: a previous chunk is shorter than the overlap");
            seams = seams || begin[p] < std::min(end[p], ov);
            vec = vec && prev_len[p] % 4 == 0;
        }
        const long long n = end[p] - begin[p];
        SVC_REQUIRE(out_off[p] >= 0 && out_off[p] <= out_len - n, "chunks_emit: a piece lies outside out (0 .. out_len)");
        if (n > 0) spans.emplace_back((long long)out_off[p], (long long)out_off[p] + n);
        max_n = std::max(max_n, (int)n);
        vec = vec && len[p] % 4 == 0 && begin[p] % 4 == 0 && end[p] % 4 == 0 && out_off[p] % 4 == 0;
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        SVC_REQUIRE(spans[i - 1].second <= spans[i].first, "chunks_emit: two pieces overlap in out");
    if (max_n == 0) return 0;
    SVC_REQUIRE(wave && out && (!seams || (fade_in && fade_out)), "chunks_emit: null argument");
    const int gx = (int)std::min<long>(cdiv(cdiv(max_n, vec ? 4 : 1), 256), 4096);
    for (int p0 = 0; p0 < N; p0 += CHUNK_MAXN) {
        const int np = std::min(N - p0, CHUNK_MAXN);
        EmitPieces pc;
        memset(&pc, 0, sizeof(pc));
        for (int p = 0; p < np; ++p) {
            const int g = p0 + p;
            pc.src[p] = (long long)row[g] * stride;
            pc.tail[p] = prev_row[g] < 0 ? -1 : (long long)prev_row[g] * stride + (prev_len[g] - ov);
            pc.dst[p] = (long long)out_off[g] - begin[g];
            pc.begin[p] = begin[g];
            pc.end[p] = end[g];
        }
        if (vec) hipLaunchKernelGGL(chunks_emit_kernel<true>, dim3(gx, np), dim3(256), 0, (hipStream_t)stream, wave, pc, fade_in, fade_out, ov, out, pcm);
        else hipLaunchKernelGGL(chunks_emit_kernel<false>, dim3(gx, np), dim3(256), 0, (hipStream_t)stream, wave, pc, fade_in, fade_out, ov, out, pcm);
        SVC_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
