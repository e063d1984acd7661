// AR prefill and short-row layers: the GEMV-pair linears (S <= 8 rows), and the RoPE / cache scatter and attention kernels
// that the GEMV-pair and the tap-GEMM (S > 8) layers share.  Included by ar.hip only.
#pragma once
#include "ar_common.h"

namespace {

// ---- GEMV-pair layers (S <= 8 rows): one wave per PAIR of output rows (2w, 2w+1), fp16 weights streamed with
// 16-byte loads, fp32 accumulate.  NORM fuses the preceding RMSNorm (x fp32, rstd recomputed per wave: K floats
// from L2 -- cheaper than a launch).  Epilogues: PLAIN (+residual), GLU (rows = (w1_j, w3_j) -> silu(a) * b) and
// QKV (rows = one RoPE pair: rotate with the bf16 table, q -> q_out, k / v -> scattered into the KV cache).
enum { GV_PLAIN = 0, GV_GLU = 1, GV_QKV = 2 };
struct GemvArgs {
    const void* x; long ldx;            // NORM ? fp32 : fp16
    const float* gamma; float eps;
    const half_t* W; long ldw;
    const float* res; long ldres;
    float* out32; half_t* out16; long ldo;
    int S, N, K;
    // QKV
    float *q_out, *kc, *vc;
    const float* rope;
    const int* pos;
    int H, Hkv, Lmax;
    // the linear itself; everything else (norm, residual, outputs, QKV) starts out null / 0
    GemvArgs(const void* x_, long ldx_, const half_t* W_, long ldw_, int S_, int N_, int K_)
        : x(x_), ldx(ldx_), gamma(nullptr), eps(0.f), W(W_), ldw(ldw_), res(nullptr), ldres(0), out32(nullptr), out16(nullptr), ldo(0),
          S(S_), N(N_), K(K_), q_out(nullptr), kc(nullptr), vc(nullptr), rope(nullptr), pos(nullptr), H(0), Hkv(0), Lmax(0) {}
};

template <bool NORM, int EPI>
__global__ __launch_bounds__(256) void gemv_pair_kernel(const GemvArgs a) {
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int r0 = 2 * wave;
    if (r0 >= a.N) return;
    const bool has1 = r0 + 1 < a.N;
    const half_t* w0 = a.W + (long)r0 * a.ldw;
    const half_t* w1 = w0 + (has1 ? a.ldw : 0);
    float rstd[8];
    if constexpr (NORM) {
        const float* xf = reinterpret_cast<const float*>(a.x);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            float ss = 0.f;
            if (s < a.S)
                for (int k0 = lane * 4; k0 < a.K; k0 += 256) {
                    const float4v v = *reinterpret_cast<const float4v*>(xf + (long)s * a.ldx + k0);
                    ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
                }
            rstd[s] = rsqrtf(wave_sum_f(ss) / (float)a.K + a.eps);
        }
    }
    float acc0[8], acc1[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) acc0[s] = acc1[s] = 0.f;
    for (int k0 = lane * 8; k0 < a.K; k0 += 512) {
        const half8 wa = *reinterpret_cast<const half8*>(w0 + k0);
        const half8 wb = *reinterpret_cast<const half8*>(w1 + k0);
        float g[8];
        if constexpr (NORM) {
            const float4v g0 = *reinterpret_cast<const float4v*>(a.gamma + k0);
            const float4v g1 = *reinterpret_cast<const float4v*>(a.gamma + k0 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { g[j] = g0[j]; g[4 + j] = g1[j]; }
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (s < a.S) {
                float xv[8];
                if constexpr (NORM) {
                    const float* xf = reinterpret_cast<const float*>(a.x) + (long)s * a.ldx + k0;
                    const float4v x0 = *reinterpret_cast<const float4v*>(xf);
                    const float4v x1 = *reinterpret_cast<const float4v*>(xf + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { xv[j] = x0[j] * rstd[s] * g[j]; xv[4 + j] = x1[j] * rstd[s] * g[4 + j]; }
                } else {
                    const half8 xh = *reinterpret_cast<const half8*>(reinterpret_cast<const half_t*>(a.x) + (long)s * a.ldx + k0);
#pragma unroll
                    for (int j = 0; j < 8; ++j) xv[j] = (float)xh[j];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    acc0[s] += xv[j] * (float)wa[j];
                    acc1[s] += xv[j] * (float)wb[j];
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        if (s < a.S) {
            const float v0 = wave_sum_f(acc0[s]);
            const float v1 = wave_sum_f(acc1[s]);
            if (lane == 0) {
                if constexpr (EPI == GV_GLU) {
                    a.out16[(long)s * a.ldo + wave] = (half_t)((v0 / (1.f + __expf(-v0))) * v1);
                } else if constexpr (EPI == GV_PLAIN) {
                    float o0 = v0, o1 = v1;
                    if (a.res) { o0 += a.res[(long)s * a.ldres + r0]; if (has1) o1 += a.res[(long)s * a.ldres + r0 + 1]; }
                    if (a.out32) { a.out32[(long)s * a.ldo + r0] = o0; if (has1) a.out32[(long)s * a.ldo + r0 + 1] = o1; }
                    if (a.out16) { a.out16[(long)s * a.ldo + r0] = (half_t)o0; if (has1) a.out16[(long)s * a.ldo + r0 + 1] = (half_t)o1; }
                } else {
                    const int D = a.H * 64, kvd = a.Hkv * 64;
                    const int ip = a.pos[s], kp = a.pos[a.S + s];
                    if (r0 < D + kvd) {
                        const int pair = (r0 & 63) >> 1;
                        const float cs = a.rope[((long)ip * 32 + pair) * 2], sn = a.rope[((long)ip * 32 + pair) * 2 + 1];
                        const float o0 = v0 * cs - v1 * sn, o1 = v1 * cs + v0 * sn;
                        if (r0 < D) {
                            a.q_out[(long)s * D + r0] = o0;
                            a.q_out[(long)s * D + r0 + 1] = o1;
                        } else {
                            const int ek = r0 - D;
                            float* dst = a.kc + ((long)(ek >> 6) * a.Lmax + kp) * 64 + (ek & 63);
                            dst[0] = o0;
                            dst[1] = o1;
                        }
                    } else {
                        const int ev = r0 - D - kvd;
                        float* dst = a.vc + ((long)(ev >> 6) * a.Lmax + kp) * 64 + (ev & 63);
                        dst[0] = v0;
                        dst[1] = v1;
                    }
                }
            }
        }
    }
}

// Contract (held by tests/test_gpu_ar_step.py): S <= 8 rows, K a multiple of 8; rows [0, N) of W are read and nothing beyond
// (an odd last row is read twice and stored once); `res` may be `out32` (a lane reads its residual before it stores the same
// element); QKV writes q_out [S][D] and row kv_pos[s] of every KV head of the one cache given, nothing else.
template <bool NORM, int EPI>
int gemv_pair_launch(const GemvArgs& a, hipStream_t st) {
    const int waves = (a.N + 1) / 2;
    hipLaunchKernelGGL((gemv_pair_kernel<NORM, EPI>), dim3(cdiv(waves, 4)), dim3(256), 0, st, a);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// RoPE (bf16-rounded table) on q and k, scatter k / v into the cache at kv_pos.  qkv [S][D + 2 kvd] fp32.
__global__ void ar_rope_cache_kernel(const float* __restrict__ qkv, long ldq, float* __restrict__ q_out, float* __restrict__ kc,
                                     float* __restrict__ vc, const float* __restrict__ rope, const int* __restrict__ pos, int S,
                                     int H, int Hkv, int Lmax) {
    // pos[0..S) = input_pos (RoPE), pos[S..2S) = kv_pos (cache slot)
    const int s = blockIdx.x;
    const int D = H * 64, kvd = Hkv * 64;
    const float* row = qkv + (long)s * ldq;
    const int ip = pos[s], kp = pos[S + s];
    for (int i = threadIdx.x; i < (D + 2 * kvd) / 2; i += blockDim.x) {
        const int e = 2 * i;                       // even element index within [q | k | v]
        const float x0 = row[e], x1 = row[e + 1];
        if (e < D + kvd) {
            const int pair = (e & 63) >> 1;
            const float cs = rope[((long)ip * 32 + pair) * 2], sn = rope[((long)ip * 32 + pair) * 2 + 1];
            const float o0 = x0 * cs - x1 * sn, o1 = x1 * cs + x0 * sn;
            if (e < D) {
                q_out[(long)s * D + e] = o0;
                q_out[(long)s * D + e + 1] = o1;
            } else {
                const int ek = e - D, hk = ek >> 6, d = ek & 63;
                float* dst = kc + ((long)hk * Lmax + kp) * 64 + d;
                dst[0] = o0;
                dst[1] = o1;
            }
        } else {
            const int ev = e - D - kvd, hv = ev >> 6, d = ev & 63;
            float* dst = vc + ((long)hv * Lmax + kp) * 64 + d;
            dst[0] = x0;
            dst[1] = x1;
        }
    }
}

// Contract: writes q_out [S][D] and row kv_pos[s] of every KV head (two rows of one call may be neighbours in the cache); every
// other cache element keeps its bits.  Positions are the caller's to keep inside [0, Lmax).
int ar_rope_cache_launch(const float* qkv, long ldq, float* q_out, float* kc, float* vc, const float* rope, const int* pos, int S, int H,
                         int Hkv, int Lmax, hipStream_t st) {
    hipLaunchKernelGGL(ar_rope_cache_kernel, dim3(S), dim3(256), 0, st, qkv, ldq, q_out, kc, vc, rope, pos, S, H, Hkv, Lmax);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// One 1024-thread block per (token s, head h): softmax(q k^T / 8 over cache slots j <= kv_pos[s]) v -> y16 [S][D].
// Scores: one thread per key (16 independent 16-byte loads in flight per thread); PV: lane = d, 16 key slices.
__global__ __launch_bounds__(1024) void ar_attn_kernel(const float* __restrict__ q, const float* __restrict__ kc,
                                                       const float* __restrict__ vc, half_t* __restrict__ y, const int* __restrict__ pos,
                                                       int S, int H, int Hkv, int Lmax) {
    extern __shared__ float sm[];               // scores [Lmax] then 16 x 64 partial outputs
    __shared__ float red[16];
    const int s = blockIdx.x, h = blockIdx.y;
    const int hk = h / (H / Hkv);
    const int n_keys = pos[S + s] + 1;          // causal row of the mask: slots 0 .. kv_pos
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float4v qv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) qv[i] = *reinterpret_cast<const float4v*>(q + ((long)s * H + h) * 64 + i * 4);
    const float* kbase = kc + (long)hk * Lmax * 64;
    float mx = -1e30f;
    for (int j = tid; j < n_keys; j += 1024) {
        const float4v* kr = reinterpret_cast<const float4v*>(kbase + (long)j * 64);
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { const float4v kv = kr[i]; d += qv[i][0] * kv[0] + qv[i][1] * kv[1] + qv[i][2] * kv[2] + qv[i][3] * kv[3]; }
        d *= 0.125f;
        sm[j] = d;
        mx = fmaxf(mx, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
    __syncthreads();
    float ls = 0.f;
    for (int j = tid; j < n_keys; j += 1024) {
        const float p = expf(sm[j] - m);
        sm[j] = p;
        ls += p;
    }
    ls = wave_sum_f(ls);
    if (lane == 0) red[wave] = ls;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += red[i];
    const float inv = 1.0f / tot;
    // o[d] = sum_j p_j v_j[d]: lane = d, 16 waves split the keys
    const float* vbase = vc + (long)hk * Lmax * 64;
    float acc = 0.f;
#pragma unroll 4
    for (int j = wave; j < n_keys; j += 16) acc += sm[j] * vbase[(long)j * 64 + lane];
    float* part = sm + Lmax;
    part[wave * 64 + lane] = acc;
    __syncthreads();
    if (wave == 0) {
        float o = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) o += part[i * 64 + lane];
        y[((long)s * H + h) * 64 + lane] = (half_t)(o * inv);
    }
}

// Contract: row s addresses cache rows 0 .. kv_pos[s] and none above (NaN there cannot reach y); the cache is not written.
// Dynamic LDS is (Lmax + 1024) floats: 36 KB at the largest max_seq_len, 8192.
int ar_attn_launch(const float* q, const float* kc, const float* vc, half_t* y, const int* pos, int S, int H, int Hkv, int Lmax,
                   hipStream_t st) {
    const size_t lds = ((size_t)Lmax + 1024) * sizeof(float);
    hipLaunchKernelGGL(ar_attn_kernel, dim3(S, H), dim3(1024), lds, st, q, kc, vc, y, pos, S, H, Hkv, Lmax);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace
