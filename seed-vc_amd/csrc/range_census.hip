// Range census of the fp16p8 vocoder mode: what the fp8 bytes of the "fp16 + fp8 corrections" conv form (kconv.hip) lose of
// a conv's split-precision operands.
//
// The p8 form has a fixed window: producers write lo_pair_p8(hi, lo) = (fp8(hi), fp8(2^11 lo)) with no activation scale and a
// clamp at +-448, weights carry one power-of-two scale per layer.  Outside the window the correction bytes flush to zero or
// clamp and the conv falls back to plain-fp16 operand error without saying so.  The census measures, on the operand planes an
// fp16x3 run writes (hi fp16, lo fp16 residual), the energy share of each term that its byte loses -- with the hardware
// convert lo_pair_p8 itself uses -- plus the counts that say why (clamped, subnormal, flushed).  A second kernel does the
// same per output channel for a conv's packed fp8 weight bytes against its fp16 w_hi / w_lo.
//
// Determinism: counts are integers; every sum is accumulated in double in an order fixed by the shape alone (thread-strided
// elements of a 64-row slab, a fixed LDS tree per workgroup, the workgroups' partials again thread-strided and tree-reduced
// by ONE workgroup).  No atomics.
#include "range_census.h"

namespace svc {

namespace {

constexpr int CS_ROWS = 64;     // rows of the planes per workgroup
constexpr int CS_NT = 256;

struct CensusAcc {
    unsigned long long c[5] = {0, 0, 0, 0, 0};      // n, n_hi_clamp, n_hi_sub, n_lo_flush, n_lo_clamp
    float mx = 0.f;
    double s[4] = {0.0, 0.0, 0.0, 0.0};             // hi^2, (hi - dq)^2, lo^2, (lo - dq)^2
};

__device__ __forceinline__ void census_elem(CensusAcc& a, float h, float l) {
    const int pr = (int)lo_pair_p8(h, l);       // the bytes the p8 producers would write
    const float dh = __builtin_amdgcn_cvt_f32_fp8(pr, 0), dl = __builtin_amdgcn_cvt_f32_fp8(pr, 1) * (1.0f / 2048.0f);
    const float ah = fabsf(h);
    a.c[0] += h != 0.f;
    a.c[1] += ah > 448.f;
    a.c[2] += ah > 0.f && ah < 0.015625f;
    a.c[3] += l != 0.f && dl == 0.f;
    a.c[4] += fabsf(l * 2048.0f) > 448.f;
    a.mx = fmaxf(a.mx, ah);
    const double eh = (double)h - (double)dh, el = (double)l - (double)dl;
    a.s[0] += (double)h * (double)h;
    a.s[1] += eh * eh;
    a.s[2] += (double)l * (double)l;
    a.s[3] += el * el;
}

// fixed-order reduction of the workgroup's accumulators; the result is valid in thread 0
__device__ __forceinline__ void census_block_reduce(CensusAcc& a) {
    __shared__ unsigned long long sc[5][CS_NT];
    __shared__ double ss[4][CS_NT];
    __shared__ float sm[CS_NT];
    const int t = threadIdx.x;
    for (int i = 0; i < 5; ++i) sc[i][t] = a.c[i];
    for (int i = 0; i < 4; ++i) ss[i][t] = a.s[i];
    sm[t] = a.mx;
    __syncthreads();
    for (int o = CS_NT / 2; o > 0; o >>= 1) {
        if (t < o) {
            for (int i = 0; i < 5; ++i) sc[i][t] += sc[i][t + o];
            for (int i = 0; i < 4; ++i) ss[i][t] += ss[i][t + o];
            sm[t] = fmaxf(sm[t], sm[t + o]);
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int i = 0; i < 5; ++i) a.c[i] = sc[i][0];
        for (int i = 0; i < 4; ++i) a.s[i] = ss[i][0];
        a.mx = sm[0];
    }
}

__device__ __forceinline__ void census_store(const CensusAcc& a, svc_census_t* r, bool add) {
    svc_census_t v;
    v.n = (long long)a.c[0]; v.n_hi_clamp = (long long)a.c[1]; v.n_hi_sub = (long long)a.c[2];
    v.n_lo_flush = (long long)a.c[3]; v.n_lo_clamp = (long long)a.c[4];
    v.max_hi = (double)a.mx;
    v.s_hi2 = a.s[0]; v.s_hi_err2 = a.s[1]; v.s_lo2 = a.s[2]; v.s_lo_err2 = a.s[3];
    if (add) {
        v.n += r->n; v.n_hi_clamp += r->n_hi_clamp; v.n_hi_sub += r->n_hi_sub; v.n_lo_flush += r->n_lo_flush;
        v.n_lo_clamp += r->n_lo_clamp;
        v.max_hi = fmax(v.max_hi, r->max_hi);
        v.s_hi2 += r->s_hi2; v.s_hi_err2 += r->s_hi_err2; v.s_lo2 += r->s_lo2; v.s_lo_err2 += r->s_lo_err2;
    }
    *r = v;
}

// workgroup g: rows [g * CS_ROWS, (g + 1) * CS_ROWS) of the B * L rows, four channels per 8-byte load
__global__ __launch_bounds__(CS_NT) void range_census_kernel(const uint2* __restrict__ hi, const uint2* __restrict__ lo, long rows, int L,
                                                             int C, int ld4, const int* __restrict__ lens,
                                                             svc_census_t* __restrict__ part) {
    const long r0 = (long)blockIdx.x * CS_ROWS;
    const int nrows = (int)(rows - r0 < CS_ROWS ? rows - r0 : CS_ROWS);
    const int ng = (C + 3) / 4;
    CensusAcc a;
    for (int idx = threadIdx.x; idx < nrows * ng; idx += CS_NT) {
        const int rr = idx / ng, cg = idx - rr * ng;
        const long row = r0 + rr;
        if (lens) {      // rows at and above the sequence's end may hold NaN: never loaded
            const long b = row / L;
            if ((int)(row - b * L) >= lens[b]) continue;
        }
        const uint2 vh = hi[row * ld4 + cg], vl = lo[row * ld4 + cg];
        const half4 h4 = *reinterpret_cast<const half4*>(&vh), l4 = *reinterpret_cast<const half4*>(&vl);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cg * 4 + j < C) census_elem(a, (float)h4[j], (float)l4[j]);
    }
    census_block_reduce(a);
    if (threadIdx.x == 0) census_store(a, part + blockIdx.x, false);
}

// ONE workgroup: the partials in thread-strided order, then the same tree; the total is added to *rec
__global__ __launch_bounds__(CS_NT) void range_census_sum_kernel(const svc_census_t* __restrict__ part, int n_part,
                                                                 svc_census_t* __restrict__ rec) {
    CensusAcc a;
    for (int i = threadIdx.x; i < n_part; i += CS_NT) {
        const svc_census_t p = part[i];
        a.c[0] += (unsigned long long)p.n; a.c[1] += (unsigned long long)p.n_hi_clamp; a.c[2] += (unsigned long long)p.n_hi_sub;
        a.c[3] += (unsigned long long)p.n_lo_flush; a.c[4] += (unsigned long long)p.n_lo_clamp;
        a.mx = fmaxf(a.mx, (float)p.max_hi);
        a.s[0] += p.s_hi2; a.s[1] += p.s_hi_err2; a.s[2] += p.s_lo2; a.s[3] += p.s_lo_err2;
    }
    census_block_reduce(a);
    if (threadIdx.x == 0) census_store(a, rec, true);
}

// one workgroup per output channel
__global__ __launch_bounds__(CS_NT) void weight_census_kernel(const half_t* __restrict__ w, long ldw, const half_t* __restrict__ w8,
                                                              long ldw8, int k, int cin_pad, float inv_s, double* __restrict__ out) {
    const long co = blockIdx.x;
    const half_t* w3 = w + co * ldw;
    const half_t* wp = w8 + co * ldw8;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int idx = threadIdx.x; idx < k * cin_pad; idx += CS_NT) {
        const int t = idx / cin_pad, ci = idx - t * cin_pad;
        const float wh = (float)wp[(long)t * 2 * cin_pad + ci];
        const float wl = (float)w3[(long)t * 3 * cin_pad + cin_pad + ci];
        // byte 0 = fp8(2^11 s w_lo), byte 1 = fp8(s w_hi) (pack_p8_kernel)
        const int pr = (int)reinterpret_cast<const unsigned short*>(wp)[(long)t * 2 * cin_pad + cin_pad + ci];
        const float dl = __builtin_amdgcn_cvt_f32_fp8(pr, 0) * (1.0f / 2048.0f) * inv_s, dh = __builtin_amdgcn_cvt_f32_fp8(pr, 1) * inv_s;
        const double eh = (double)wh - (double)dh, el = (double)wl - (double)dl;
        s[0] += (double)wh * (double)wh;
        s[1] += eh * eh;
        s[2] += (double)wl * (double)wl;
        s[3] += el * el;
    }
    __shared__ double ss[4][CS_NT];
    const int t = threadIdx.x;
    for (int i = 0; i < 4; ++i) ss[i][t] = s[i];
    __syncthreads();
    for (int o = CS_NT / 2; o > 0; o >>= 1) {
        if (t < o)
            for (int i = 0; i < 4; ++i) ss[i][t] += ss[i][t + o];
        __syncthreads();
    }
    if (t < 4) out[co * 4 + t] = ss[t][0];
}

}  // namespace

long census_parts(int B, int L) { return ((long)B * L + CS_ROWS - 1) / CS_ROWS; }

int census_launch(const void* hi, const void* lo, int B, int L, int C, int ld, const int* lens, svc_census_t* rec, svc_census_t* part,
                  long part_cap, hipStream_t st) {
    SVC_REQUIRE(hi && lo && rec && part && B >= 1 && L >= 1 && C >= 1 && ld >= C && ld % 4 == 0, "range census: bad argument");
    SVC_REQUIRE((uintptr_t)hi % 8 == 0 && (uintptr_t)lo % 8 == 0, "range census: the planes are 8-byte aligned");
    const long n_part = census_parts(B, L);
    SVC_REQUIRE(n_part <= part_cap && n_part <= 0x7fffffffL, "range census: the partial-sum workspace is too small");
    hipLaunchKernelGGL(range_census_kernel, dim3((unsigned)n_part), dim3(CS_NT), 0, st, (const uint2*)hi, (const uint2*)lo, (long)B * L, L, C,
                       ld / 4, lens, part);
    SVC_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(range_census_sum_kernel, dim3(1), dim3(CS_NT), 0, st, (const svc_census_t*)part, (int)n_part, rec);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int weight_census_launch(const ConvW& w, double* out, hipStream_t st) {
    SVC_REQUIRE(w.w8 && w.w && w.vd == 3 && out, "weight census: the conv has no fp8 packing");
    hipLaunchKernelGGL(weight_census_kernel, dim3(w.cout), dim3(CS_NT), 0, st, (const half_t*)w.w, w.ldw, (const half_t*)w.w8, w.ldw8, w.k,
                       w.cin_pad, ldexpf(1.0f, -w.w8_exp), out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace svc

using namespace svc;

extern "C" {

int svc_op_range_census(const svc_range_census_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(e, "svc_op_range_census: null argument");
    SVC_REQUIRE(e->hi && e->lo && e->out, "svc_op_range_census: hi, lo and out are required");
    SVC_REQUIRE(e->B >= 1 && e->L >= 1 && e->C >= 1, "svc_op_range_census: B, L and C are positive");
    SVC_REQUIRE((long)e->B * e->L <= 0x7fffffffL, "svc_op_range_census: B * L exceeds 2^31 - 1 rows");
    SVC_REQUIRE(e->ld >= e->C && e->ld % 4 == 0, "svc_op_range_census: ld covers C channels and is a multiple of 4");
    SVC_REQUIRE((uintptr_t)e->hi % 8 == 0 && (uintptr_t)e->lo % 8 == 0, "svc_op_range_census: the planes are 8-byte aligned");
    if (e->lens)
        for (int b = 0; b < e->B; ++b) SVC_REQUIRE(e->lens[b] >= 0 && e->lens[b] <= e->L, "svc_op_range_census: lens out of range");
    Arena ar;
    const long n_part = census_parts(e->B, e->L);
    svc_census_t* rec = ar.alloc_n<svc_census_t>(1, st);
    svc_census_t* part = ar.alloc_n<svc_census_t>((size_t)n_part, st);
    int* d_lens = nullptr;
    if (!rec || !part) return 1;
    if (e->lens) {
        d_lens = ar.alloc_n<int>(e->B, st);
        if (!d_lens) return 1;
        SVC_CHECK_HIP(hipMemcpyAsync(d_lens, e->lens, e->B * sizeof(int), hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));      // the caller's array is pageable
    }
    if (census_launch(e->hi, e->lo, e->B, e->L, e->C, e->ld, d_lens, rec, part, n_part, st)) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(e->out, rec, sizeof(svc_census_t), hipMemcpyDeviceToHost, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_op_weight_census(const float* w, int Cout, int Cin, int k, double* out, int* w8_exp_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(w && out, "svc_op_weight_census: w and out are required");
    SVC_REQUIRE(Cout >= 1 && Cin >= 1 && k >= 3 && k <= 16, "svc_op_weight_census: Cout and Cin are positive, 3 <= k <= 16");
    Arena ar;
    svc_tensor_desc_t d;
    d.name = "c.weight"; d.data = w; d.ndim = 3; d.shape[0] = Cout; d.shape[1] = Cin; d.shape[2] = k; d.shape[3] = 1;
    StateDict sd(&d, 1);
    ConvW cw;
    if (pack_conv1d(sd, "c", Cout, Cin, k, false, 3, ar, st, &cw)) return 1;
    SVC_REQUIRE(cw.w8 != nullptr, "svc_op_weight_census: this conv shape gets no fp8 packing");
    double* d_out = ar.alloc_n<double>((size_t)Cout * 4, st);
    if (!d_out) return 1;
    if (weight_census_launch(cw, d_out, st)) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(out, d_out, (size_t)Cout * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    if (w8_exp_out) *w8_exp_out = cw.w8_exp;
    return 0;
}

}  // extern "C"
