// v2 AR model (NaiveTransformer, GQA 12q/2kv, KV cache): `forward_generate` (prefill and one-token decode step)
// and the top-p / repetition-penalty / exponential-race sampler, as HIP kernels for gfx950.
//
// `svc_ar::run` takes one of three forms, by the number of rows S:
//   * S = 1 on a shape the one-token kernels hold (`dec_step`, decided once in svc_ar_create): the decode step, three
//     launches per layer ("S = 1 decode step" below);
//   * S <= 8 (and S = 1 on other shapes): GEMV-pair layers, five launches per layer;
//   * S > 8 (prefill): the MFMA tap-GEMM on the same packed weights.
// The decode step is HBM-bound (every weight byte is read once per token), so its linears are wave-per-output-row GEMV
// kernels streaming fp16 weights with 16-byte loads.  The whole step (38 kernels for ar_base) is captured once into a
// hipGraph and replayed per token (the reference's answer to launch overhead is torch.compile "reduce-overhead",
// modules/v2/vc_wrapper.py:105-114); positions live in device memory and are advanced inside the graph, so a replay
// needs no host-side argument update.
//
// Up to 64 sequences decode together ("batched decode step" below): each in its own slot (KV cache, positions), the
// linears as skinny MFMA GEMMs that read every weight byte once per step for all slots, one captured graph per padded
// batch, and the generate loop's state per slot (svc_ar_set_max_batch / _prefill_slot / _decode_step_batch /
// _generate_batch).  The B = 1 entry points and kernels do not change with it: slot 0 is their cache.
//
// reference: modules/v2/ar.py:239-267 (forward_generate), :75-93 (KVCache.update), :503-567 (Attention),
//            :600-651 (RMSNorm, bf16 RoPE table), :712-763 (sample / logits_to_probs / exponential race).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "model_util.h"

using namespace svc;

namespace {

// Device-resident state of the generate loop: the captured per-token graph (decode step -> rank -> sample, which also
// embeds the drawn token and advances the positions) reads everything that changes from token to token from here, so one graph replay per token needs no host argument.
struct GenState {
    const float* noise;      // [max_new][V] Exp(1) draws, row t for token t; null = draw them from `seed` (ar_exp_draw4)
    unsigned long long seed;
    int* toks;               // [max_new] generated tokens
    int cnt;                 // index of the token being generated (>= 1 inside the loop)
    int min_before_eos, eos;
    float temperature, top_p, rep_pen;
};

// Cross-lane sums on the DPP path (one VALU instruction per step, no LDS crossbar round trip: `__shfl_xor` compiles to
// ds_bpermute_b32, ~100+ cycles each, and the one-token kernels are chains of such latencies).  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
__device__ __forceinline__ float row8_sum_f(float v) {      // every lane of an aligned 8-lane group gets the group's sum
    v += dpp_f<DPP_XOR1>(v); v += dpp_f<DPP_XOR2>(v); v += dpp_f<DPP_HALF_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float row16_sum_f(float v) {     // ... of an aligned 16-lane group (a DPP row)
    v = row8_sum_f(v); v += dpp_f<DPP_ROW_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {      // every lane gets the wave's sum
    v = row16_sum_f(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)) +
           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
}

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

// ------------------------------------------------------------------------------------------------ S = 1 decode step
// Three launches per layer, then the last layer's w2 and the output head.  The step is bound by launch boundaries and
// memory round trips, not bandwidth (13.4 MB of weights per layer); every kernel issues EVERY load a wave needs before
// anything waits:
//   dec_qkvraw (layer 0) | dec_w2qkv (layers >= 1): this layer's unnormalised QKV GEMV, fused with the previous layer's
//               w2 GEMV + residual ("three launches per layer" below)
//   dec_attn2 : RMSNorm scale, RoPE, KV-cache write, attention over the valid cache prefix and the head's slice of wo
//               -> partial residual vectors part[head][D]                     (wo's own launch disappears)
//   dec_ffn13 : h = h_in + sum_heads part[head] (summed once per workgroup in LDS; workgroup 0 stores it to the other
//               residual buffer), ffn_norm, w1/w3 GEMV, SwiGLU -> ff16        (4 rows per wave)
//   dec_w2    : h_out = h + w2 GEMV, last layer                               (2 rows per wave)
//   dec_head  : final RMSNorm + output GEMV                                   (4 rows per wave)
// A wave owns whole weight rows; lane l owns the 16-byte chunks l, l + 64, ... of every row (and of the input vector),
// so the input never goes through LDS and one wave reduction per row finishes it.
constexpr int DEC_MAXC = 5;          // chunks of 8 elements per lane: reductions up to 64 * 8 * 5 = 2560 long

template <int NR>
struct DecW { half8 w[NR][DEC_MAXC]; };

// Every weight chunk of the NR rows; rows past the end re-read the last row.  KC = the reduction length when it is known
// at compile time (the ar_base sizes), 0 = runtime K.  No lane is predicated: a chunk index past the row is CLAMPED (the
// lane re-reads the last chunk, an L1 hit) and its input element is zeroed in dec_dot -- a predicated load is a branch
// per request with conservative vmcnt(0) waits at the joins, which serialised these one-round-trip kernels; whole chunks
// past the row are skipped by a wave-uniform test (compile-time with KC).
template <int NR, int KC = 0>
__device__ __forceinline__ void dec_load_w(DecW<NR>& r, const half_t* __restrict__ W, long ldw, int row0, int n_rows, int K, int lane) {
    const int nch = KC ? KC >> 3 : K >> 3;
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        const half_t* wr = W + (long)(row0 + q < n_rows ? row0 + q : n_rows - 1) * ldw;
#pragma unroll
        for (int i = 0; i < DEC_MAXC; ++i) {
            if (64 * i < nch) {
                const int c = lane + 64 * i;
                r.w[q][i] = *reinterpret_cast<const half8*>(wr + 8 * (c < nch ? c : nch - 1));
            }
        }
    }
}

struct DecG { float4v g0[DEC_MAXC], g1[DEC_MAXC]; };      // a lane's chunks of the RMSNorm weight

template <int KC = 0>
__device__ __forceinline__ void dec_load_g(DecG& g, const float* __restrict__ gamma, int K, int lane) {
    const int nch = KC ? KC >> 3 : K >> 3;
#pragma unroll
    for (int i = 0; i < DEC_MAXC; ++i) {
        if (64 * i < nch) {
            const int c = lane + 64 * i, cc = c < nch ? c : nch - 1;
            g.g0[i] = *reinterpret_cast<const float4v*>(gamma + 8 * cc);
            g.g1[i] = *reinterpret_cast<const float4v*>(gamma + 8 * cc + 4);
        }
    }
}

// input chunks (global or LDS) -> optional RMSNorm (rstd from this wave's own sum of squares) * gamma -> NR dot products.
// `pg`: the norm weight already in registers (requested before a barrier), or null to load it here.
template <int NR, bool XF16, int KC = 0>
__device__ __forceinline__ void dec_dot(const DecW<NR>& r, int K, const void* x, const float* gamma, float eps, bool norm,
                                        float (&out)[NR], int lane, const DecG* pg = nullptr) {
    float xv[DEC_MAXC][8];
    const int nch = KC ? KC >> 3 : K >> 3;
    const int Kk = KC ? KC : K;
    DecG gl;
    if (norm && !pg) dec_load_g<KC>(gl, gamma, K, lane);
    const DecG& g = pg ? *pg : gl;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < DEC_MAXC; ++i) {
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[i][j] = 0.f;
        if (64 * i < nch) {
            const int c = lane + 64 * i, cc = c < nch ? c : nch - 1;
            if constexpr (XF16) {
                const half8 h = *reinterpret_cast<const half8*>(reinterpret_cast<const half_t*>(x) + 8 * cc);
#pragma unroll
                for (int j = 0; j < 8; ++j) xv[i][j] = c < nch ? (float)h[j] : 0.f;
            } else {
                const float* xf = reinterpret_cast<const float*>(x) + 8 * cc;
                const float4v a = *reinterpret_cast<const float4v*>(xf), b = *reinterpret_cast<const float4v*>(xf + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { xv[i][j] = c < nch ? a[j] : 0.f; xv[i][4 + j] = c < nch ? b[j] : 0.f; }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += xv[i][j] * xv[i][j];
        }
    }
    if (norm) {
        const float rstd = rsqrtf(wave_sum_f(ss) / (float)Kk + eps);
#pragma unroll
        for (int i = 0; i < DEC_MAXC; ++i) {
            if (64 * i < nch) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { xv[i][j] *= rstd * g.g0[i][j]; xv[i][4 + j] *= rstd * g.g1[i][j]; }
            }
        }
    }
    float acc[NR];
#pragma unroll
    for (int q = 0; q < NR; ++q) {
        acc[q] = 0.f;
#pragma unroll
        for (int i = 0; i < DEC_MAXC; ++i) {
            if (64 * i < nch) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[q] += xv[i][j] * (float)r.w[q][i][j];
            }
        }
    }
    // the NR reductions are independent DPP chains (the compiler interleaves them)
#pragma unroll
    for (int q = 0; q < NR; ++q) out[q] = wave_sum_f(acc[q]);
}

// 256 threads = 4 waves x 4 rows (2 SwiGLU outputs each).  h = h_in + sum_p part[p] is summed once per workgroup; the weight
// rows are requested before that prologue.
template <int NP, int KD>
__global__ __launch_bounds__(256) void dec_ffn13_kernel(const float* __restrict__ h_in, const float* __restrict__ part, int n_part,
                                                        float* __restrict__ h_out, const float* __restrict__ gamma, float eps,
                                                        const half_t* __restrict__ W, int K, int N, half_t* __restrict__ ff) {
    __shared__ __attribute__((aligned(16))) float hs[64 * 8 * DEC_MAXC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = (blockIdx.x * 4 + wave) * 4;
    DecW<4> w;
    dec_load_w<4, KD>(w, W, K, r0 < N ? r0 : 0, N, K, lane);
    DecG g;                                     // requested before the barrier (after it: one more exposed L2 round trip)
    dec_load_g<KD>(g, gamma, K, lane);
    for (int c = tid; c < (K >> 2); c += 256) {
        float4v a = *reinterpret_cast<const float4v*>(h_in + 4 * c);
        if constexpr (NP > 0) {
            float4v b[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) b[p] = *reinterpret_cast<const float4v*>(part + (long)p * K + 4 * c);
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] += b[p][j];
        } else {
            for (int p = 0; p < n_part; ++p) {
                const float4v b = *reinterpret_cast<const float4v*>(part + (long)p * K + 4 * c);
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] += b[j];
            }
        }
        *reinterpret_cast<float4v*>(hs + 4 * c) = a;
        if (blockIdx.x == 0) *reinterpret_cast<float4v*>(h_out + 4 * c) = a;
    }
    __syncthreads();
    if (r0 >= N) return;
    float v[4];
    dec_dot<4, false, KD>(w, K, hs, gamma, eps, true, v, lane, &g);
    if (lane == 0) {
        ff[r0 >> 1] = (half_t)((v[0] / (1.f + __expf(-v[0]))) * v[1]);
        if (r0 + 2 < N) ff[(r0 >> 1) + 1] = (half_t)((v[2] / (1.f + __expf(-v[2]))) * v[3]);
    }
}

// out[n] = res[n] + sum_k W[n][k] x16[k]   (w2 + residual; one wave per 2 rows)
template <int KI>
__global__ __launch_bounds__(64) void dec_w2_kernel(const half_t* __restrict__ x, const half_t* __restrict__ W, int K, int N,
                                                    const float* __restrict__ res, float* __restrict__ out) {
    const int lane = threadIdx.x, r0 = 2 * blockIdx.x;
    if (r0 >= N) return;
    DecW<2> w;
    dec_load_w<2, KI>(w, W, K, r0, N, K, lane);
    const float res0 = res[r0], res1 = r0 + 1 < N ? res[r0 + 1] : 0.f;
    float v[2];
    dec_dot<2, true, KI>(w, K, x, nullptr, 0.f, false, v, lane);
    if (lane == 0) {
        out[r0] = res0 + v[0];
        if (r0 + 1 < N) out[r0 + 1] = res1 + v[1];
    }
}

// ---- three launches per layer -------------------------------------------------------------------------------------
// The attention RMSNorm scale is ONE scalar per token, so it commutes out of the QKV projection:
//     qkv = wqkv (gamma * h / rms(h)) = (Wq' h) / rms(h),   Wq' = wqkv diag(gamma),
// and h = h_mid + w2 ff of the previous layer makes  Wq' h = Wq' h_mid + (Wq' w2) ff  -- with W' = Wq' w2 composed in fp32
// at pack time, the previous layer's w2 GEMV and this layer's QKV GEMV read the same inputs (ff, h_mid) and become ONE
// launch; the 1 / rms(h) factor, RoPE and the KV-cache write move into the attention kernel, which reads h anyway.
// A dependent launch costs ~6 us on this machine whatever it does; the second matrix costs 4.7 MB more weights per layer.

// layer 0: qkv_raw[n] = sum_k Wq'[n][k] h[k]   (no preceding w2)
template <int KD>
__global__ __launch_bounds__(64) void dec_qkvraw_kernel(const float* __restrict__ h, const half_t* __restrict__ Wq, int K, int N,
                                                        float* __restrict__ out) {
    const int lane = threadIdx.x, r0 = 2 * blockIdx.x;
    if (r0 >= N) return;
    DecW<2> w;
    dec_load_w<2, KD>(w, Wq, K, r0, N, K, lane);
    float v[2];
    dec_dot<2, false, KD>(w, K, h, nullptr, 0.f, false, v, lane);
    if (lane == 0) {
        out[r0] = v[0];
        if (r0 + 1 < N) out[r0 + 1] = v[1];
    }
}

// layers >= 1.  Rows [0, D): h_out = h_mid + w2 ff (the previous layer's output = this layer's input);
// rows [D, D + N): qkv_raw = W' ff + Wq' h_mid, Wc = [W' | Wq'] row-wise (ld = I + D).
template <int KD, int KI>
__global__ __launch_bounds__(64) void dec_w2qkv_kernel(const half_t* __restrict__ ff, const float* __restrict__ h_mid,
                                                       const half_t* __restrict__ W2, const half_t* __restrict__ Wc, int I, int D, int N,
                                                       float* __restrict__ h_out, float* __restrict__ qkv_out) {
    const int lane = threadIdx.x, r0 = 2 * blockIdx.x;
    if (r0 < D) {
        DecW<2> w;
        dec_load_w<2, KI>(w, W2, I, r0, D, I, lane);
        const float res0 = h_mid[r0], res1 = r0 + 1 < D ? h_mid[r0 + 1] : 0.f;
        float v[2];
        dec_dot<2, true, KI>(w, I, ff, nullptr, 0.f, false, v, lane);
        if (lane == 0) {
            h_out[r0] = res0 + v[0];
            if (r0 + 1 < D) h_out[r0 + 1] = res1 + v[1];
        }
        return;
    }
    const int rq = r0 - D;
    if (rq >= N) return;
    DecW<2> wa, wb;
    dec_load_w<2, KI>(wa, Wc, (long)I + D, rq, N, I, lane);
    dec_load_w<2, KD>(wb, Wc + I, (long)I + D, rq, N, D, lane);
    float va[2], vb[2];
    dec_dot<2, true, KI>(wa, I, ff, nullptr, 0.f, false, va, lane);
    dec_dot<2, false, KD>(wb, D, h_mid, nullptr, 0.f, false, vb, lane);
    if (lane == 0) {
        qkv_out[rq] = va[0] + vb[0];
        if (rq + 1 < N) qkv_out[rq + 1] = va[1] + vb[1];
    }
}

// Attention of the decode step, spread over the chip: grid = (DEC_NS wo-row slices) x (heads), 512 threads.
// q / k / v arrive unnormalised (qkv_raw).  Every workgroup of head h recomputes that head's softmax over the valid cache
// prefix [0, kv_pos] -- <= 4096 x 64 fp32 keys and values, read from L2 / Infinity Cache -- and applies 1 / DEC_NS of the
// head's wo column slice (D / DEC_NS rows x 64 columns, held in registers), so 96 workgroups carry the 12 heads of ar_base
// instead of 12 (with one workgroup per head, a CU moved 154 KB of K / V + 98 KB of wo and ran eight 1024-thread barriers).
//   * every request that does not depend on `pos` goes out first: the first two batches of cache rows (by position,
//     clamped to the cache, NOT to the valid prefix), the wo rows, the layer input, q / k / v;
//   * 1 / rms(h): every wave reduces the layer input h on its own (D floats from L2, one DPP tree: no barrier);
//   * q and the new k are rotated (bf16-rounded table, position input_pos); the new key / value are used from registers
//     for position kv_pos and stored into the cache by slice 0 of the first head of each KV group;
//   * EIGHT lanes per key (thread = key slot tid / 8, column octet c = tid % 8: columns 32 r + 4 c .. + 3, r = 0, 1, so the
//     eight lanes of a key read one whole 128-byte line per request): a score is 8 FMAs + three DPP adds and the softmax
//     bookkeeping is replicated 8x, not 16x as with one float4 column per lane (in-kernel timestamps: the key loop took
//     1.5 us of the 6.6 us a workgroup lives; four lanes per key needs 48 more registers for q / k / v and spilled);
//     64 slots x 4 keys = 256 keys per batch, two batches in flight; each slot runs its OWN online softmax (no cross-wave
//     exchange per batch);
//   * merge: the 8 slots of a wave by DPP row rotations (one (max, l, acc) per 16-lane row and wave-uniform max), the 32
//     rows through LDS in two short stages that use every thread (the serial 32-term sum of 64 threads took 2.2 us);
//   * part[h][n] = sum_d wo[n][64 h + d] y[d] for this slice's rows n (y rounded to fp16 like the stand-alone path).
constexpr int DEC_NS = 8;           // wo row slices per head
constexpr int DA_KB = 4;            // keys per thread per batch (64 slots x 4 = 256 keys)
constexpr int DA_WO = 2;            // wo rows per thread: 64 rows per pass, D / DEC_NS <= 128 rows (D <= 1024)
constexpr int DPP_ROR8 = 0x128;
struct DaKey { float4v r[2]; };     // a lane's eighth of a 64-float row: columns 32 r + 4 c .. + 3
__global__ __launch_bounds__(512) void dec_attn2_kernel(const float* __restrict__ hres, const float* __restrict__ qkv_raw, float eps,
                                                        const float* __restrict__ rope, float* __restrict__ kc, float* __restrict__ vc,
                                                        const half_t* __restrict__ wo, float* __restrict__ part,
                                                        const int* __restrict__ pos, int H, int Hkv, int Lmax) {
    __shared__ __attribute__((aligned(16))) float pacc[32 * 64];     // per 16-lane row: 64 output columns
    __shared__ __attribute__((aligned(16))) float red[8 * 64];
    __shared__ float pm[32], pl[32], redl[8], yv[64];
    const int sl = blockIdx.x, h = blockIdx.y, D = H * 64, kvd = Hkv * 64;
    const int hk = h / (H / Hkv);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slot = tid >> 3, c = tid & 7;
    const int rows_per = (D + DEC_NS - 1) / DEC_NS;
    // this slice's wo rows: row n = 8 lanes x 16 bytes of columns [64 h, 64 h + 64)
    half8 wr[DA_WO];
#pragma unroll
    for (int i = 0; i < DA_WO; ++i) {
        const int n = sl * rows_per + i * 64 + (tid >> 3);
        const int nn = n < D ? n : D - 1;
        wr[i] = *reinterpret_cast<const half8*>(wo + (long)nn * D + 64 * h + 8 * (tid & 7));
    }
    // wave-uniform bases + 32-bit lane offsets: the requests take the (SGPR base, VGPR offset, immediate) form
    const float* kbase = kc + (long)hk * Lmax * 64;
    const float* vbase = vc + (long)hk * Lmax * 64;
    DaKey ka[DA_KB], va[DA_KB], kb[DA_KB], vb[DA_KB];
    // Cache rows are requested by position only: the first two batches do not wait for `pos` to arrive.  Rows past kv_pos
    // hold zeros or stale FINITE values of an earlier run (the cache is zero-initialised and only ever written with
    // computed keys / values); their scores are masked and their p is exactly 0.
    auto load_batch = [&](DaKey (&kx)[DA_KB], DaKey (&vx)[DA_KB], int j0) {    // position kv_pos is patched from registers
#pragma unroll
        for (int i = 0; i < DA_KB; ++i) {
            const int j = j0 + slot + 64 * i;
            const unsigned o = (unsigned)(j < Lmax ? j : Lmax - 1) * 64u + 4u * (unsigned)c;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                kx[i].r[r] = *reinterpret_cast<const float4v*>(kbase + o + 32 * r);
                vx[i].r[r] = *reinterpret_cast<const float4v*>(vbase + o + 32 * r);
            }
        }
    };
    load_batch(ka, va, 0);
    load_batch(kb, vb, 64 * DA_KB);
    __builtin_amdgcn_sched_barrier(0);          // the cache rows go out first: nothing below is hoisted above their requests
    const int ip = pos[0], kp = pos[1];
    const int n_keys = kp + 1;
    // 1 / rms of the layer input, per wave: D <= 1024 floats = up to 4 float4 per lane, all requested at once
    float4v hx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = lane + 64 * i;                // clamped address + weight 0: a predicated load would be a branch with a
        hx[i] = *reinterpret_cast<const float4v*>(hres + 4 * (q < (D >> 2) ? q : 0));      // vmcnt(0) wait behind the cache rows
        if (q >= (D >> 2)) hx[i] = (float4v){0.f, 0.f, 0.f, 0.f};
    }
    DaKey q4, k4, v4;
    float4v cs[2];                              // (cos, sin) of the rotation pairs 16 r + 2 c, 16 r + 2 c + 1
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        q4.r[r] = *reinterpret_cast<const float4v*>(qkv_raw + (long)h * 64 + 32 * r + 4 * c);
        k4.r[r] = *reinterpret_cast<const float4v*>(qkv_raw + D + (long)hk * 64 + 32 * r + 4 * c);
        v4.r[r] = *reinterpret_cast<const float4v*>(qkv_raw + D + kvd + (long)hk * 64 + 32 * r + 4 * c);
        cs[r] = *reinterpret_cast<const float4v*>(rope + ((long)ip * 32 + 16 * r + 2 * c) * 2);
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) ss += hx[i][0] * hx[i][0] + hx[i][1] * hx[i][1] + hx[i][2] * hx[i][2] + hx[i][3] * hx[i][3];
    ss = wave_sum_f(ss);
    const float rstd = rsqrtf(ss / (float)D + eps);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { q4.r[r][j] *= rstd; k4.r[r][j] *= rstd; v4.r[r][j] *= rstd; }
        const float4v q0 = q4.r[r], k0 = k4.r[r], t = cs[r];
        q4.r[r][0] = q0[0] * t[0] - q0[1] * t[1]; q4.r[r][1] = q0[1] * t[0] + q0[0] * t[1];
        q4.r[r][2] = q0[2] * t[2] - q0[3] * t[3]; q4.r[r][3] = q0[3] * t[2] + q0[2] * t[3];
        k4.r[r][0] = k0[0] * t[0] - k0[1] * t[1]; k4.r[r][1] = k0[1] * t[0] + k0[0] * t[1];
        k4.r[r][2] = k0[2] * t[2] - k0[3] * t[3]; k4.r[r][3] = k0[3] * t[2] + k0[2] * t[3];
    }
    if (sl == 0 && h % (H / Hkv) == 0 && slot == 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            *reinterpret_cast<float4v*>(kc + ((long)hk * Lmax + kp) * 64 + 32 * r + 4 * c) = k4.r[r];
            *reinterpret_cast<float4v*>(vc + ((long)hk * Lmax + kp) * 64 + 32 * r + 4 * c) = v4.r[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) q4.r[r] *= 0.125f;      // 1 / sqrt(64) folded into q (exact: a power of two)
    float m_run = -1e30f, l_run = 0.f;
    DaKey acc;
#pragma unroll
    for (int r = 0; r < 2; ++r) acc.r[r] = (float4v){0.f, 0.f, 0.f, 0.f};
    auto process = [&](DaKey (&kx)[DA_KB], DaKey (&vx)[DA_KB], int j0) {
        float sc[DA_KB];
#pragma unroll
        for (int i = 0; i < DA_KB; ++i) {
            if (j0 + slot + 64 * i == kp) { kx[i] = k4; vx[i] = v4; }
            float a = 0.f;
#pragma unroll
            for (int r = 0; r < 2; ++r)
                a += q4.r[r][0] * kx[i].r[r][0] + q4.r[r][1] * kx[i].r[r][1] + q4.r[r][2] * kx[i].r[r][2] + q4.r[r][3] * kx[i].r[r][3];
            sc[i] = a;
        }
#pragma unroll
        for (int i = 0; i < DA_KB; ++i) sc[i] = row8_sum_f(sc[i]);
        float m_new = m_run;
#pragma unroll
        for (int i = 0; i < DA_KB; ++i) {
            sc[i] = j0 + slot + 64 * i < n_keys ? sc[i] : -1e30f;
            m_new = fmaxf(m_new, sc[i]);
        }
        const float scale = __expf(m_run - m_new);
        l_run *= scale;
#pragma unroll
        for (int r = 0; r < 2; ++r) acc.r[r] *= scale;
#pragma unroll
        for (int i = 0; i < DA_KB; ++i) {
            const float p = j0 + slot + 64 * i < n_keys ? __expf(sc[i] - m_new) : 0.f;
            l_run += p;                          // the eight lanes of a slot carry the same p
#pragma unroll
            for (int r = 0; r < 2; ++r) acc.r[r] += p * vx[i].r[r];
        }
        m_run = m_new;
    };
    for (int j0 = 0; j0 < n_keys; j0 += 2 * 64 * DA_KB) {
        process(ka, va, j0);
        if (j0 + 2 * 64 * DA_KB < n_keys) load_batch(ka, va, j0 + 2 * 64 * DA_KB);
        if (j0 + 64 * DA_KB < n_keys) {
            process(kb, vb, j0 + 64 * DA_KB);
            if (j0 + 3 * 64 * DA_KB < n_keys) load_batch(kb, vb, j0 + 3 * 64 * DA_KB);
        }
    }
    // merge, stage 0: the 8 slots of this wave.  Wave-uniform maximum, then per 16-lane row (2 slots) sums by a rotation:
    // lane c of a row ends up with the row's sum for its column octet.
    float mw = fmaxf(m_run, dpp_f<DPP_ROR8>(m_run));
    mw = fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mw), 0)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mw), 16))),
               fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mw), 32)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mw), 48))));
    {
        const float scale = __expf(m_run - mw);
        l_run *= scale;
        l_run += dpp_f<DPP_ROR8>(l_run);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float a = acc.r[r][j] * scale;
                a += dpp_f<DPP_ROR8>(a);
                acc.r[r][j] = a;
            }
    }
    const int g = tid >> 4;                     // 16-lane row index: 32 per workgroup
    if ((tid & 15) < 8) {
#pragma unroll
        for (int r = 0; r < 2; ++r) *reinterpret_cast<float4v*>(pacc + g * 64 + 32 * r + 4 * c) = acc.r[r];
        if ((tid & 15) == 0) { pm[g] = mw; pl[g] = l_run; }
    }
    __syncthreads();
    {
        // stage 1: every thread; wave w folds the four rows 4 w .. 4 w + 3 (they share pm) for column d = lane
        float M = pm[0];
#pragma unroll
        for (int i = 1; i < 8; ++i) M = fmaxf(M, pm[4 * i]);
        const float w = __expf(pm[4 * wave] - M);
        const float o = pacc[(4 * wave) * 64 + lane] + pacc[(4 * wave + 1) * 64 + lane] + pacc[(4 * wave + 2) * 64 + lane] +
                        pacc[(4 * wave + 3) * 64 + lane];
        red[wave * 64 + lane] = w * o;
        if (lane == 0) redl[wave] = w * (pl[4 * wave] + pl[4 * wave + 1] + pl[4 * wave + 2] + pl[4 * wave + 3]);
    }
    __syncthreads();
    if (tid < 64) {
        float o = 0.f, tot = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { o += red[i * 64 + tid]; tot += redl[i]; }
        yv[tid] = (float)(half_t)(o / tot);
    }
    __syncthreads();
    const float4v y0 = *reinterpret_cast<const float4v*>(yv + 8 * (tid & 7)), y1 = *reinterpret_cast<const float4v*>(yv + 8 * (tid & 7) + 4);
#pragma unroll
    for (int i = 0; i < DA_WO; ++i) {
        const int nl = i * 64 + (tid >> 3);
        const int n = sl * rows_per + nl;
        float o = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) o += y0[j] * (float)wr[i][j] + y1[j] * (float)wr[i][4 + j];
        o = row8_sum_f(o);
        if (nl < rows_per && n < D && (tid & 7) == 0) part[(long)h * D + n] = o;
    }
}

// logits[n] = sum_k W[n][k] norm(h)[k]   (final norm + output head; 4 rows per wave)
template <int KD>
__global__ __launch_bounds__(256) void dec_head_kernel(const float* __restrict__ h, const float* __restrict__ gamma, float eps,
                                                       const half_t* __restrict__ W, int K, int N, float* __restrict__ logits) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = (blockIdx.x * 4 + wave) * 4;
    if (r0 >= N) return;
    DecW<4> w;
    dec_load_w<4, KD>(w, W, K, r0, N, K, lane);
    float v[4];
    dec_dot<4, false, KD>(w, K, h, gamma, eps, true, v, lane);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (r0 + r < N) logits[r0 + r] = v[r];
    }
}

__global__ void advance_pos_kernel(int* pos, int* cnt) {   // S = 1: {input_pos, kv_pos} += 1 (ar.py:402-403)
    if (threadIdx.x < 2) pos[threadIdx.x] += 1;
    if (cnt && threadIdx.x == 2) cnt[0] += 1;
}

// x = embeddings[previous token]  (embed_base of the token sampled by the previous step, ar.py:188-193,414)
__global__ void ar_embed_kernel(const float* __restrict__ emb, const GenState* __restrict__ gs, float* __restrict__ x, int D) {
    const long t = gs->toks[gs->cnt - 1];
    for (int c = threadIdx.x; c < D; c += blockDim.x) x[c] = emb[t * D + c];
}

// ---- sampler: one block, vocab <= 4096.  reference: ar.py:731-763 + :723-727
constexpr int SORT_N = 4096;

// Seeded Exp(1) draws: Philox4x32-10 (Salmon et al., SC'11), key = (seed low word, seed high word), counter =
// (v / 4, token step, 0, 0); output word j of the call is the draw of vocabulary entry 4 (v / 4) + j.  A draw is a pure
// function of (seed, step, v): nothing about the slot, the batch or the other sequences enters it.
// u = ((word >> 8) + 1) * 2^-24 lies in (0, 1] and is exact in fp32, so q = -log(u) is finite (<= 16.64) and >= 0.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ void ar_exp_draw4(unsigned long long seed, int step, int v4, float (&q)[4]) {
    unsigned w[4];
    philox4x32_10((unsigned)v4, (unsigned)step, 0u, 0u, (unsigned)seed, (unsigned)(seed >> 32), w);
    // q = -log(k 2^-24) = n ln2 - log(m), k = m 2^(24 - n), m in [1, 2): log(m) <= 0.7 carries an absolute error of ~1e-7
    // and n ln2 is a two-term product whose high part is exact (n <= 24, ln2_hi has 15 significant bits), so the error of
    // q is half an fp32 ulp of q plus ~1.5e-7 -- exp(-q) reproduces u to < 1e-6 relative over the whole range (logf on u
    // itself is 2 ulp of q off: 2e-6 at q = 8 .. 16.6).
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned k = (w[j] >> 8) + 1u;
        const int e = 31 - __clz((int)k);
        const float m = ldexpf((float)k, -e), n = (float)(24 - e);
        // explicit fmaf: the sampler and svc_ar_exp_draws must round alike.  fmaxf: log(m) may overshoot ln2 by an ulp when
        // m is just below 2 (n = 1)
        q[j] = fmaxf(fmaf(n, 0.693145751953125f, fmaf(n, 1.42860682030941723212e-6f, -logf(m))), 0.f);
    }
}

// out[s][v] = the draw of (seed, step0 + s, v): what the seeded sampler uses, for svc_ar_exp_draws
__global__ __launch_bounds__(256) void ar_exp_draws_kernel(unsigned long long seed, int step0, int V, float* __restrict__ out) {
    const int v4 = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (4 * v4 >= V) return;
    float q[4];
    ar_exp_draw4(seed, step0 + s, v4, q);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * v4 + j < V) out[(size_t)s * V + 4 * v4 + j] = q[j];
}

// Sampler stage 1 (many workgroups): repetition penalty + suppression, then the RANK of every logit in the descending
// order torch.sort gives (ties: lower index first) by counting -- workgroup b ranks tokens 16 b .. 16 b + 15, 16 lanes per
// token, each lane counting over a 1/16 stride of the vocabulary held in LDS.  Writes the sorted (value, index) pairs and
// the penalised logits.  V^2 comparisons spread over V / 16 workgroups (one CU alone needs ~100 us for them; the 78-stage
// single-workgroup bitonic network this replaces took 74 us).
__device__ __forceinline__ void ar_rank_body(const float* __restrict__ logits, int V, const int* __restrict__ prev, int n_prev,
                                             int suppress, float rep_pen, const GenState* __restrict__ gs,
                                             float* __restrict__ skey, int* __restrict__ sidx, float* __restrict__ lgp) {
    if (gs) {   // generate loop: token gs->cnt; the repetition penalty sees previous_tokens[0] only (ar.py:442-444)
        prev = gs->toks; n_prev = 1;
        suppress = gs->cnt < gs->min_before_eos ? gs->eos : -1;
        rep_pen = gs->rep_pen;
    }
    __shared__ __attribute__((aligned(16))) float lg[SORT_N];
    const int tid = threadIdx.x;
    for (int i = tid; i < SORT_N; i += 256) lg[i] = i < V ? logits[i] : -INFINITY;
    __syncthreads();
    // repetition penalty from the ORIGINAL logits (gather, transform, scatter: duplicates write the same value)
    for (int i = tid; i < n_prev; i += 256) {
        const int t = prev[i];
        const float sc = logits[t];
        lg[t] = sc < 0.f ? sc * rep_pen : sc / rep_pen;
    }
    __syncthreads();
    if (tid == 0 && suppress >= 0) lg[suppress] = -INFINITY;
    __syncthreads();
    const int i = blockIdx.x * 16 + (tid >> 4), l = tid & 15;
    const float mine = i < V ? lg[i] : -INFINITY;
    int rk = 0;
    for (int j = l; j < V; j += 16) {
        const float o = lg[j];
        rk += (o > mine) || (o == mine && j < i);
    }
    rk += __shfl_xor(rk, 1); rk += __shfl_xor(rk, 2); rk += __shfl_xor(rk, 4); rk += __shfl_xor(rk, 8);
    if (l == 0 && i < V) {
        skey[rk] = mine;
        sidx[rk] = i;
        lgp[i] = mine;
    }
}

__global__ __launch_bounds__(256) void ar_rank_kernel(const float* __restrict__ logits, int V, const int* __restrict__ prev, int n_prev,
                                                      int suppress, float rep_pen, const GenState* __restrict__ gs,
                                                      float* __restrict__ skey, int* __restrict__ sidx, float* __restrict__ lgp) {
    ar_rank_body(logits, V, prev, n_prev, suppress, rep_pen, gs, skey, sidx, lgp);
}

// Sampler stage 2 (one workgroup): softmax over the sorted logits, top-p cut, temperature softmax, exponential race.
// Returns the drawn token (the same value in every thread).
__device__ __forceinline__ int ar_sample_body(const float* __restrict__ lgp, int V, const float* __restrict__ skey,
                                              const int* __restrict__ sidx, float temperature, float top_p,
                                              const float* __restrict__ exp_noise, unsigned long long seed, int step,
                                              float* __restrict__ probs_out) {
    __shared__ float key[SORT_N];
    __shared__ int idx[SORT_N];
    __shared__ float lg[SORT_N];       // penalised logits in vocabulary order, later reused
    // block-wide reductions: DPP inside a wave, 16 slots through LDS, ONE barrier each (every reduction has its own slots,
    // so nothing has to wait for the previous one to be read out); the tree reductions this replaces were ~50 barriers
    // of 16 waves per token (~4 us of the 10 us this kernel took)
    __shared__ float r_mx[16], r_sum[16], r_best[16];
    __shared__ int r_idx[16];
    __shared__ double r_scan[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // seeded draws: thread t owns vocabulary entries 4t .. 4t+3 (one Philox call; SORT_N = 4 x 1024).  Pure integer VALU
    // work issued before the first load is waited for, so it hides under the memory latency of the prologue.
    float q4[4] = {1.f, 1.f, 1.f, 1.f};
    if (!exp_noise && 4 * tid < V) ar_exp_draw4(seed, step, tid, q4);
    auto wave_max_f = [](float v) {
        v = fmaxf(v, dpp_f<DPP_XOR1>(v)); v = fmaxf(v, dpp_f<DPP_XOR2>(v));
        v = fmaxf(v, dpp_f<DPP_HALF_MIRROR>(v)); v = fmaxf(v, dpp_f<DPP_ROW_MIRROR>(v));
        return fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)),
                           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16))),
                     fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)),
                           __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48))));
    };
    for (int i = tid; i < SORT_N; i += 1024) {
        lg[i] = i < V ? lgp[i] : -INFINITY;
        key[i] = i < V ? skey[i] : -INFINITY;
        idx[i] = i < V ? sidx[i] : i;
    }
    __syncthreads();
    // softmax of the sorted logits, cumulative sum (double, like torch.cumsum on CPU floats), top-p mask
    const float m = key[0];
    // chunked scan: thread t (< 1024) owns sorted elements 4t..4t+3
    float e4[4];
    double local = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) { e4[r] = expf(key[4 * tid + r] - m); local += (double)e4[r]; }
    double incl = local;               // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(incl, o);
        if (lane >= o) incl += u;
    }
    if (lane == 63) r_scan[wave] = incl;
    __syncthreads();
    double base = 0.0, total = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double w = r_scan[i];
        if (i < wave) base += w;
        total += w;
    }
    double run = base + incl - local;  // sum of everything before this thread's first element
    for (int r = 0; r < 4; ++r) {
        const int sidx = 4 * tid + r;
        run += (double)e4[r];
        const float cum = (float)(run / total);
        const bool remove = sidx > 0 && cum > top_p;
        if (idx[sidx] < V) lg[idx[sidx]] = remove ? -INFINITY : lg[idx[sidx]];
    }
    __syncthreads();
    // final softmax over kept logits / temperature
    const float tinv = 1.0f / fmaxf(temperature, 1e-5f);
    float mx = -INFINITY;
    for (int i = tid; i < V; i += 1024) mx = fmaxf(mx, lg[i] * tinv);
    mx = wave_max_f(mx);
    if (lane == 0) r_mx[wave] = mx;
    __syncthreads();
    float m2 = r_mx[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) m2 = fmaxf(m2, r_mx[i]);
    float sum = 0.f;
    for (int i = tid; i < V; i += 1024) { const float e = expf(lg[i] * tinv - m2); key[i] = e; sum += e; }
    sum = wave_sum_f(sum);
    if (lane == 0) r_sum[wave] = sum;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) tot += r_sum[i];
    const float inv = 1.0f / tot;
    // exponential race: argmax probs / q (ties: the lower index)
    float best = -1.f;
    int besti = 0;
    if (exp_noise) {
        for (int i = tid; i < V; i += 1024) {
            const float p = key[i] * inv;
            if (probs_out) probs_out[i] = p;
            const float r = p / exp_noise[i];
            if (r > best) { best = r; besti = i; }
        }
    } else {
        // the same race over this thread's own four entries: the maximum (ties: the lower index) does not depend on
        // how the entries are spread over the threads
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 4 * tid + j;
            if (i < V) {
                const float p = key[i] * inv;
                if (probs_out) probs_out[i] = p;
                const float r = p / q4[j];
                if (r > best) { best = r; besti = i; }
            }
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float ob = __shfl_xor(best, o);
        const int oi = __shfl_xor(besti, o);
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    if (lane == 0) { r_best[wave] = best; r_idx[wave] = besti; }
    __syncthreads();
    best = r_best[0]; besti = r_idx[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) {
        const float ob = r_best[i];
        const int oi = r_idx[i];
        if (ob > best || (ob == best && oi < besti)) { best = ob; besti = oi; }
    }
    idx[0] = besti;                    // every thread holds the same winner; the callers' tails read it from LDS
    __syncthreads();
    return idx[0];
}

__global__ __launch_bounds__(1024) void ar_sample_kernel(const float* __restrict__ lgp, int V, const float* __restrict__ skey,
                                                         const int* __restrict__ sidx, float temperature, float top_p,
                                                         const float* __restrict__ exp_noise, unsigned long long seed,
                                                         int step, int* __restrict__ idx_out,
                                                         float* __restrict__ probs_out, GenState* __restrict__ gs,
                                                         const float* __restrict__ emb, float* __restrict__ next_x, int D,
                                                         int* __restrict__ pos) {
    if (gs) {
        const int t = gs->cnt;
        temperature = gs->temperature; top_p = gs->top_p;
        exp_noise = gs->noise ? gs->noise + (size_t)t * V : nullptr;
        seed = gs->seed; step = t;
        idx_out = gs->toks + t;
    }
    const int tid = threadIdx.x;
    const int win = ar_sample_body(lgp, V, skey, sidx, temperature, top_p, exp_noise, seed, step, probs_out);
    if (tid == 0) idx_out[0] = win;
    if (gs && next_x) {
        // generate loop: this workgroup also prepares the next step -- embedding row of the token just drawn into the
        // residual buffer (ar.py:188-193,414), positions and token counter advanced (ar.py:402-403) -- which saves the
        // embed, copy and advance launches of every token (a dependent launch costs ~4.5 us whatever it does)
        const long tk = win;
        for (int c = tid; c < D; c += 1024) next_x[c] = emb[tk * D + c];
        if (tid == 0) { pos[0] += 1; pos[1] += 1; gs->cnt += 1; }
    }
}


// ------------------------------------------------------------------------------------------ batched decode step (B <= 64)
// One token for each of B sequences: slot b has its own KV cache, input_pos and kv_pos.  The per-token cost of the B = 1
// step is the fp16 weight stream, which is the same for every sequence, so the linears become skinny GEMMs that read each
// weight byte once per step for all slots; five launches per layer whatever B is:
//   bgemm<NORM, QKV>   attention_norm + wqkv, RoPE, q -> bq, k / v -> each slot's cache row kv_pos[b]
//   battn              one-token attention of every slot over its own cache prefix [0, kv_pos[b]]
//   bgemm<PLAIN>       wo + residual
//   bgemm<NORM, GLU>   ffn_norm + w1 / w3 + SwiGLU
//   bgemm<PLAIN>       w2 + residual
// then bgemm<NORM, PLAIN> for the final norm + output head and the sampler over B rows.  The composed `wc` matrices of
// the B = 1 step are not used.  Nothing here uses atomics, and every reduction has a fixed order that depends on the
// model shape alone, so a slot's result is bit-identical whatever B is and whatever the other slots hold.
constexpr int MAXB = 64;

// GenState of one slot + its loop flags.  A finished slot (EOS drawn, max_new reached, or the next position would leave the
// cache) stays in the batch: it re-runs its last step in place (same positions, same cache row) and records nothing.
struct GenSlot : GenState {
    int done;
    int max_new;
};

enum { BG_PLAIN = 0, BG_GLU = 1, BG_QKV = 2 };
struct BGemmArgs {
    const void* x; long ldx;            // [Bp][K], NORM ? fp32 : fp16
    const float* gamma; float eps;
    const half_t* W; long ldw;          // [N rounded up to 16][K] fp16
    const float* res;                   // PLAIN: optional residual [Bp][ldo]
    float* out32; half_t* out16; long ldo;
    int N, K;
    // QKV
    float* q_out;                       // [Bp][H * 64]
    float* const* kc; float* const* vc; // [MAXB] cache base of every slot for this layer
    const float* rope;
    const int* pos;                     // [0, MAXB) input_pos, [MAXB, 2 MAXB) kv_pos
    const int* nb;                      // live slots: rows b >= *nb are padding of the M tile and touch no cache
    int H, Hkv, Lmax;
};

// out[b][n] = sum_k x[b][k] W[n][k] on v_mfma_f32_16x16x32_f16 with the WEIGHT rows as the MFMA's M side and the batch
// as its N side: a lane's four accumulator registers are four CONSECUTIVE output features n of one slot b, so a RoPE
// pair, a (w1_j, w3_j) SwiGLU pair and a 16-byte store all stay inside one lane.
// A workgroup (4 waves) owns 16 NT weight rows; the waves split K in four contiguous ranges, so a weight byte is read by
// exactly one wave of one workgroup: it goes straight to VGPRs with 16-byte loads (no LDS round trip), and so do the
// activation fragments (<= 64 x K, L2-resident).  The four partial tiles meet in LDS and are summed in wave order.
// NORM: x is the fp32 residual stream; the RMSNorm weight is applied to the fragment, 1 / rms(x[b]) is one scalar per
// output column and is applied after the reduction (the sum of squares rides along with the fragment loads).
// MT = M tiles of 16 slots (Bp / 16): more column tiles of the same code, nothing else changes with B; NT = 16-row weight
// tiles per workgroup; KC = K when known at compile time (the ar_base sizes: k-steps unrolled in groups whose requests all
// go out before the group's first MFMA waits), 0 = runtime K.
template <bool NORM, int EPI, int MT, int NT, int KC>
__global__ __launch_bounds__(256) void bgemm_kernel(const BGemmArgs a) {
    __shared__ __attribute__((aligned(16))) float part[4][NT * MT][4][64];
    __shared__ float ssq[NORM ? 4 : 1][MT][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * (16 * NT);
    const int K = KC ? KC : a.K;
    const int nsteps = K >> 5, per = (nsteps + 3) >> 2;          // 32-element k-steps, a contiguous quarter per wave
    constexpr bool FULL = KC != 0 && ((KC >> 5) % 4) == 0;
    const int s0 = wave * per;
    float4v acc[NT][MT];
    float ss[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        ss[m] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t][m] = (float4v){0.f, 0.f, 0.f, 0.f};
    }
    const half_t* wrow = a.W + (long)(n0 + r) * a.ldw + 8 * g;
    // one k-step = a lane's 16-byte fragments: NT weight rows, MT activation rows (NORM: 32 bytes of fp32 + the norm weight)
    struct Frag {
        half8 w[NT];
        half8 xh[NORM ? 1 : MT];
        float4v x0[NORM ? MT : 1], x1[NORM ? MT : 1], g0, g1;
    };
    auto load = [&](int s, Frag& f) {
        const int k = 32 * s + 8 * g;
#pragma unroll
        for (int t = 0; t < NT; ++t) f.w[t] = *reinterpret_cast<const half8*>(wrow + (long)16 * t * a.ldw + 32 * s);
        if constexpr (NORM) {
            f.g0 = *reinterpret_cast<const float4v*>(a.gamma + k);
            f.g1 = *reinterpret_cast<const float4v*>(a.gamma + k + 4);
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const float* xp = reinterpret_cast<const float*>(a.x) + (long)(16 * m + r) * a.ldx + k;
                f.x0[m] = *reinterpret_cast<const float4v*>(xp);
                f.x1[m] = *reinterpret_cast<const float4v*>(xp + 4);
            }
        } else {
#pragma unroll
            for (int m = 0; m < MT; ++m)
                f.xh[m] = *reinterpret_cast<const half8*>(reinterpret_cast<const half_t*>(a.x) + (long)(16 * m + r) * a.ldx + k);
        }
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            half8 xf;
            if constexpr (NORM) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ss[m] += f.x0[m][j] * f.x0[m][j] + f.x1[m][j] * f.x1[m][j];
                    xf[j] = (half_t)(f.x0[m][j] * f.g0[j]);
                    xf[4 + j] = (half_t)(f.x1[m][j] * f.g1[j]);
                }
            } else {
                xf = f.xh[m];
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.w[t], xf, acc[t][m], 0, 0, 0);
        }
    };
    if constexpr (FULL) {
        // groups of U k-steps: every request of a group is issued before its first MFMA waits (deep unroll, late vmcnt) --
        // step by step the compiler kept ~8 requests in flight per wave, and one wave per SIMD then waits out a memory
        // round trip per step
        constexpr int PER = (KC >> 5) >> 2;
        constexpr int U = NORM ? (PER % 3 == 0 ? 3 : 1) : (PER % 6 == 0 ? 6 : PER % 2 == 0 ? 2 : 1);
#pragma unroll
        for (int i0 = 0; i0 < PER; i0 += U) {
            Frag f[U];
#pragma unroll
            for (int u = 0; u < U; ++u) load(s0 + i0 + u, f[u]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < U; ++u) mma(f[u]);
        }
    } else {
        const int s1 = s0 + per < nsteps ? s0 + per : nsteps;
        for (int s = s0; s < s1; ++s) {
            Frag f;
            load(s, f);
            mma(f);
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) part[wave][t * MT + m][i][lane] = acc[t][m][i];
    if constexpr (NORM) {
#pragma unroll
        for (int m = 0; m < MT; ++m) ssq[wave][m][lane] = ss[m];
    }
    __syncthreads();
    // wave w finishes the tiles w, w + 4, ...: partials summed in wave order, then the epilogue
#pragma unroll
    for (int q0 = 0; q0 < NT * MT; q0 += 4) {
        const int q = q0 + wave;
        if (q >= NT * MT) break;
        const int t = q / MT, m = q % MT;
        float4v v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ((part[0][q][i][lane] + part[1][q][i][lane]) + part[2][q][i][lane]) + part[3][q][i][lane];
        const int b = 16 * m + r;               // slot (MFMA column)
        const int n = n0 + 16 * t + 4 * g;      // output features n .. n + 3
        if constexpr (NORM) {
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) tot += ssq[w][m][r + 16 * gg];
            const float rstd = rsqrtf(tot / (float)K + a.eps);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] *= rstd;
        }
        if (n >= a.N) continue;
        if constexpr (EPI == BG_GLU) {          // rows (2 j, 2 j + 1) = (w1_j, w3_j)
            half2v o;
            o[0] = (half_t)((v[0] / (1.f + __expf(-v[0]))) * v[1]);
            o[1] = (half_t)((v[2] / (1.f + __expf(-v[2]))) * v[3]);
            *reinterpret_cast<half2v*>(a.out16 + (long)b * a.ldo + (n >> 1)) = o;
        } else if constexpr (EPI == BG_PLAIN) {
            if (n + 3 < a.N && (a.ldo & 3) == 0) {
                if (a.res) v += *reinterpret_cast<const float4v*>(a.res + (long)b * a.ldo + n);
                *reinterpret_cast<float4v*>(a.out32 + (long)b * a.ldo + n) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (n + i < a.N) a.out32[(long)b * a.ldo + n + i] = v[i] + (a.res ? a.res[(long)b * a.ldo + n + i] : 0.f);
            }
        } else {                                // QKV: n .. n + 3 = two rotation pairs of one head
            if (b >= *a.nb) continue;
            const int D = a.H * 64, kvd = a.Hkv * 64;
            const int ip = a.pos[b], kp = a.pos[MAXB + b];
            if (n < D + kvd) {
                const float4v cs = *reinterpret_cast<const float4v*>(a.rope + ((long)ip * 32 + ((n & 63) >> 1)) * 2);
                const float4v o = {v[0] * cs[0] - v[1] * cs[1], v[1] * cs[0] + v[0] * cs[1],
                                   v[2] * cs[2] - v[3] * cs[3], v[3] * cs[2] + v[2] * cs[3]};
                if (n < D) {
                    *reinterpret_cast<float4v*>(a.q_out + (long)b * D + n) = o;
                } else {
                    const int e = n - D;
                    *reinterpret_cast<float4v*>(a.kc[b] + ((long)(e >> 6) * a.Lmax + kp) * 64 + (e & 63)) = o;
                }
            } else {
                const int e = n - D - kvd;
                *reinterpret_cast<float4v*>(a.vc[b] + ((long)(e >> 6) * a.Lmax + kp) * 64 + (e & 63)) = v;
            }
        }
    }
}

template <bool NORM, int EPI, int NT, int KC>
int bgemm_launch(const BGemmArgs& a, int Bp, hipStream_t st) {
    const dim3 grid(cdiv(a.N, 16 * NT)), block(256);
    switch (Bp / 16) {
        case 1: hipLaunchKernelGGL((bgemm_kernel<NORM, EPI, 1, NT, KC>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((bgemm_kernel<NORM, EPI, 2, NT, KC>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((bgemm_kernel<NORM, EPI, 3, NT, KC>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((bgemm_kernel<NORM, EPI, 4, NT, KC>), grid, block, 0, st, a); break;
    }
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// One-token attention of slot b = blockIdx.y for GT query heads of one KV head (GQA: they share every key / value row; GT = 3
// of the 6 heads per KV head for ar_base: the cache prefix is read twice, from L2, and the per-key arithmetic -- which is
// what a workgroup spends its time on -- is spread over twice the CUs).  512 threads, keys in chunks of 512:
//   loads  : every cache row of the chunk is requested at once -- one memory round trip per chunk; 32 groups of 16
//            lanes, group = keys j (mod 32), lane = 4 of the 64 columns, so a row is one 256-byte request (a thread that
//            reads a whole key row by itself touches 64 lines per instruction and evicts them before it comes back)
//   scores : 4 FMAs + a 16-lane DPP sum per (key, head), q (pre-scaled by 1/8) in registers; scores -> LDS
//   softmax: one thread per key; chunk maximum per head over the 8 waves, running (max, sum) across chunks (one rescale
//            per chunk); probabilities -> LDS
//   PV     : the same groups and columns as the loads
//   merge  : the 4 groups of a wave by two lane exchanges, the 8 waves through LDS in wave order.
// Only rows 0 .. kv_pos[b] of the slot's cache are ever addressed (an index past the prefix is clamped into it and its
// probability is exactly 0), so whatever an earlier, longer sequence left in the rows above cannot reach the result, not
// even as 0 x value.
constexpr int BA_CH = 512;          // one key per thread and chunk
template <int GT>
__global__ __launch_bounds__(512) void battn_kernel(const float* __restrict__ q, float* const* __restrict__ kc_tab,
                                                    float* const* __restrict__ vc_tab, half_t* __restrict__ y,
                                                    const int* __restrict__ pos, const int* __restrict__ nb, int H, int Hkv, int Lmax) {
    __shared__ __attribute__((aligned(16))) float sc[GT][BA_CH];
    __shared__ __attribute__((aligned(16))) float pw[8][GT][64];
    __shared__ float redm[8][GT], redl[8][GT];
    const int b = blockIdx.y;
    // position and cache bases are requested together with the live-slot count, not after it: one round trip, not two
    // (every slot has a valid position; the bases of a slot that was never allocated are null and are not used)
    const int n_keys = pos[MAXB + b] + 1;
    const float* kslot = kc_tab[b];
    const float* vslot = vc_tab[b];
    if (b >= *nb) return;
    const int G = H / Hkv, ngrp = G / GT;
    const int hk = blockIdx.x / ngrp, h0 = hk * G + (blockIdx.x % ngrp) * GT;
    const int D = H * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 4, c = tid & 15;
    float4v qv[GT];                             // this lane's four columns of every head's q
#pragma unroll
    for (int i = 0; i < GT; ++i) qv[i] = *reinterpret_cast<const float4v*>(q + (long)b * D + (h0 + i) * 64 + 4 * c) * 0.125f;   // 1 / sqrt(64), exact
    const float* kb = kslot + (long)hk * Lmax * 64;
    const float* vb = vslot + (long)hk * Lmax * 64;
    float4v acc[GT];
    float m_run[GT], l_run[GT];
#pragma unroll
    for (int i = 0; i < GT; ++i) {
        acc[i] = (float4v){0.f, 0.f, 0.f, 0.f};
        m_run[i] = -1e30f;
        l_run[i] = 0.f;
    }
    for (int c0 = 0; c0 < n_keys; c0 += BA_CH) {
        const int nk = n_keys - c0 < BA_CH ? n_keys - c0 : BA_CH;
        // every cache row this thread needs from the chunk is requested here, before anything waits: 16 key and 16 value
        // quarter-rows (rows group + 32 u: a row is one 256-byte request of its 16 lanes); an index past the chunk is
        // clamped into it and masked below.  Wave-uniform base + 32-bit lane offset: one address register per request.
        float4v kx[BA_CH / 32], vx[BA_CH / 32];
#pragma unroll
        for (int u = 0; u < BA_CH / 32; ++u) {
            const int jj = grp + 32 * u;
            const unsigned o = (unsigned)(c0 + (jj < nk ? jj : nk - 1)) * 64u + 4u * (unsigned)c;
            kx[u] = *reinterpret_cast<const float4v*>(kb + o);
            vx[u] = *reinterpret_cast<const float4v*>(vb + o);
        }
#pragma unroll
        for (int u = 0; u < BA_CH / 32; ++u) {
            const int jj = grp + 32 * u;
#pragma unroll
            for (int i = 0; i < GT; ++i) {
                const float a = row16_sum_f(qv[i][0] * kx[u][0] + qv[i][1] * kx[u][1] + qv[i][2] * kx[u][2] + qv[i][3] * kx[u][3]);
                if (c == 0) sc[i][jj] = jj < nk ? a : -1e30f;
            }
        }
        __syncthreads();
        const bool has_key = tid < nk;
        float s[GT];
#pragma unroll
        for (int i = 0; i < GT; ++i) s[i] = sc[i][tid];
        float mx[GT];
#pragma unroll
        for (int i = 0; i < GT; ++i) {
            mx[i] = s[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], o));
            if (lane == 0) redm[wave][i] = mx[i];
        }
        __syncthreads();
        float scale[GT], ls[GT];
#pragma unroll
        for (int i = 0; i < GT; ++i) {
            float m = m_run[i];
#pragma unroll
            for (int w = 0; w < 8; ++w) m = fmaxf(m, redm[w][i]);
            scale[i] = __expf(m_run[i] - m);
            m_run[i] = m;
            const float p = has_key ? __expf(s[i] - m) : 0.f;
            sc[i][tid] = p;
            ls[i] = wave_sum_f(p);
            if (lane == 0) redl[wave][i] = ls[i];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < GT; ++i) {
            float l = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) l += redl[w][i];
            l_run[i] = l_run[i] * scale[i] + l;
            acc[i] *= scale[i];
        }
#pragma unroll
        for (int u = 0; u < BA_CH / 32; ++u) {
            const int jj = grp + 32 * u;            // sc holds 0 for the keys past the chunk
#pragma unroll
            for (int i = 0; i < GT; ++i) acc[i] += sc[i][jj] * vx[u];
        }
        __syncthreads();                        // sc, redm and redl are rewritten by the next chunk
    }
#pragma unroll
    for (int i = 0; i < GT; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float a = acc[i][j];
            a += __shfl_xor(a, 16);
            a += __shfl_xor(a, 32);
            acc[i][j] = a;
        }
        if (lane < 16) *reinterpret_cast<float4v*>(&pw[wave][i][4 * c]) = acc[i];
    }
    __syncthreads();
    for (int e = tid; e < GT * 64; e += 512) {
        const int i = e >> 6, d = e & 63;
        float o = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) o += pw[w][i][d];
        float l = l_run[0];                     // l_run[i] without a dynamic register index
#pragma unroll
        for (int k = 1; k < GT; ++k) l = i == k ? l_run[k] : l;
        y[(long)b * D + (h0 + i) * 64 + d] = (half_t)(o / l);
    }
}

__global__ void advance_pos_batch_kernel(int* __restrict__ pos, const int* __restrict__ nb) {
    const int b = threadIdx.x;
    if (b < *nb) { pos[b] += 1; pos[MAXB + b] += 1; }
}

// x[b] = embeddings[last token of slot b]
__global__ void ar_embed_batch_kernel(const float* __restrict__ emb, const GenSlot* __restrict__ slots, float* __restrict__ x, int D) {
    const GenSlot* gs = slots + blockIdx.x;
    const long t = gs->toks[gs->cnt - 1];
    for (int c = threadIdx.x; c < D; c += blockDim.x) x[(long)blockIdx.x * D + c] = emb[t * D + c];
}

__global__ __launch_bounds__(256) void ar_rank_batch_kernel(const float* __restrict__ logits, int V, const GenSlot* __restrict__ slots,
                                                            const int* __restrict__ nb, float* __restrict__ skey,
                                                            int* __restrict__ sidx, float* __restrict__ lgp) {
    const int b = blockIdx.y;
    if (b >= *nb) return;
    ar_rank_body(logits + (long)b * V, V, nullptr, 0, -1, 1.f, slots + b, skey + (long)b * SORT_N, sidx + (long)b * SORT_N,
                 lgp + (long)b * SORT_N);
}

// Sampler stage 2 for slot b = blockIdx.x, then the slot's loop state: record the token, embed it as the next input,
// advance the positions -- or finish the slot (EOS; max_new tokens; the next position would leave the cache).
__global__ __launch_bounds__(1024) void ar_sample_batch_kernel(const float* __restrict__ lgp, int V, const float* __restrict__ skey,
                                                               const int* __restrict__ sidx, GenSlot* __restrict__ slots,
                                                               const int* __restrict__ nb, const float* __restrict__ emb,
                                                               float* __restrict__ next_x, int D, int* __restrict__ pos, int Lmax) {
    const int b = blockIdx.x;
    if (b >= *nb) return;
    GenSlot* gs = slots + b;
    const int tid = threadIdx.x;
    const int t = gs->cnt, was_done = gs->done;         // read by every thread before thread 0 changes them (barriers in the body)
    const int row = t < gs->max_new ? t : gs->max_new - 1;      // a slot finished by max_new has no noise row t (seeded: step)
    const int win = ar_sample_body(lgp + (long)b * SORT_N, V, skey + (long)b * SORT_N, sidx + (long)b * SORT_N, gs->temperature,
                                   gs->top_p, gs->noise ? gs->noise + (size_t)row * V : nullptr, gs->seed, row, nullptr);
    const bool record = !was_done && win != gs->eos;
    const long tk = record ? win : gs->toks[t - 1];     // a finished slot keeps its last input
    for (int c = tid; c < D; c += 1024) next_x[(long)b * D + c] = emb[tk * D + c];
    if (tid == 0 && !was_done) {
        gs->toks[t] = win;
        if (!record) {
            gs->done = 1;                               // EOS: cnt = tokens before it
        } else {
            const int ip = pos[b] + 1, kp = pos[MAXB + b] + 1;
            gs->cnt = t + 1;
            if (t + 1 >= gs->max_new || ip >= Lmax || kp >= Lmax) gs->done = 1;
            else { pos[b] = ip; pos[MAXB + b] = kp; }
        }
    }
}

}  // namespace

struct svc_ar {
    svc_ar_config_t cfg;
    int D, H, Hkv, L, I, V, Lmax, kvd, Nqkv;
    Arena wts, ws;
    struct Layer {
        half_t *wqkv, *wo, *w13, *w2;
        half_t* wc = nullptr;     // decode step (dec_step only): layer 0 [Nqkv][D] = wqkv diag(gamma); layers >= 1 [Nqkv][I + D] = [Wq' w2_prev | Wq']
        float *g_attn, *g_ffn;
        float *kc, *vc;
    };
    std::vector<Layer> layers;
    float* g_final;
    half_t* w_out;
    float* rope;
    int cap_S = 0;
    float *h32, *qkv32, *q32, *logits;
    float *h32b, *part;           // S = 1 step: second residual buffer, per-head wo partials
    half_t *n16, *y16, *ff16, *x16;
    int* d_pos;
    GenState* d_gen = nullptr;    // generate-loop state (device)
    float *d_skey = nullptr, *d_lgp = nullptr;   // sampler stage 1 -> stage 2
    int* d_sidx = nullptr;
    int sample(const float* lg, const int* prev, int n_prev, int suppress, float temperature, float top_p, float rep_pen,
               const float* exp_noise, int* idx_out, float* probs_out, GenState* gs, hipStream_t st, bool prepare_next = false,
               unsigned long long seed = 0, int step = 0);      // exp_noise null (and gs null): the draws of (seed, step)
    // decode graph
    hipGraphExec_t graph = nullptr;
    hipGraphExec_t gen_graph = nullptr;   // step -> rank -> sample (+ next embedding, advance), driven by d_gen
    float* gx = nullptr;          // staged input of the captured step
    float* emb = nullptr;         // model.embeddings.weight [V][D] fp32 (generate loop only)
    int ensure_graph();
    int ensure_gen_graph();
    bool dec_step = false;        // S = 1 runs the decode step (the shape fits the dec_* kernels; `wc` is composed)

    int reserve(int S, hipStream_t st);
    int run(const float* x, int S, const int* d_positions, float* logits_out, hipStream_t st);
    int run_dec_step(const float* x, const int* d_positions, float* logits_out, hipStream_t st);
    int run_gemv_layers(int S, const int* d_positions, hipStream_t st);
    int run_gemm_layers(int S, const int* d_positions, hipStream_t st);
    int run_head(int S, float* logits_out, hipStream_t st);

    // ---- batch (svc_ar_set_max_batch): slot 0 is the cache above, slots 1 .. max_batch - 1 are allocated on request.
    // The batch workspace is separate from `ws` (which reserve() may reallocate): the captured batch graphs stay valid.
    int max_batch = 1;
    Arena slot_mem, bws;
    std::vector<float*> slot_base;     // [max_batch], slot >= 1: layer i keys at + 2 i cache_elems(), values at + (2 i + 1) cache_elems()
    float** d_kvtab = nullptr;         // device [L][2][MAXB] cache bases per layer (keys, values) and slot; null = no such slot
    float *bh = nullptr, *bq = nullptr, *blogits = nullptr;      // [MAXB][D] residual / q, [MAXB][V]
    half_t *by16 = nullptr, *bff16 = nullptr;                    // [MAXB][D], [MAXB][I]
    int *d_bpos = nullptr, *d_nb = nullptr;
    GenSlot* d_slots = nullptr;
    float *b_skey = nullptr, *b_lgp = nullptr;
    int* b_sidx = nullptr;
    hipGraphExec_t bstep_graph[MAXB / 16] = {}, bgen_graph[MAXB / 16] = {};     // by padded batch: 16, 32, 48, 64 rows
    int cur_nb = 0;                    // value of *d_nb
    int bpos_n = 0;                    // slots whose device positions h_bpos mirrors (0: svc_ar_decode_step_batch needs set_pos)
    int h_bpos[2 * MAXB] = {};
    size_t cache_elems() const { return (size_t)Hkv * Lmax * 64; }
    float* slot_kc(int slot, int layer) const { return slot ? slot_base[slot] + 2 * layer * cache_elems() : layers[layer].kc; }
    float* slot_vc(int slot, int layer) const { return slot ? slot_base[slot] + (2 * layer + 1) * cache_elems() : layers[layer].vc; }
    int ensure_batch_ws(hipStream_t st);
    int upload_kvtab(hipStream_t st);
    int set_nb(int B, hipStream_t st);
    int prefill_slot(int slot, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out, hipStream_t st);
    int run_batch_step(int Bp, hipStream_t st);
    int ensure_batch_graph(int Bp, bool gen);
};

namespace {
// out[s] = (res ? res[s] : 0) + W x[s] on the tap-GEMM (S > 8 rows); GLU: rows (2j, 2j+1) of W are (w1_j, w3_j) ->
// out16[s][j] = silu(a) * b
int lin(const half_t* x, const half_t* W, long ldw, const float* res, float* out32, half_t* out16, long ldo, int S, int N, int K,
        bool glu, hipStream_t st) {
    KGemmParams p;
    memset(&p, 0, sizeof(p));
    p.M = S; p.N = N; p.Lout = S; p.a_seq_rows = S; p.c_seq_rows = S; p.a_stride = 1; p.a_len = S;
    p.n_taps = 1; p.a_ptr[0] = x; p.a_ld[0] = K; p.a_ktiles[0] = K / 64;
    p.w = W; p.ldw = ldw;
    p.res = res; p.ldres = ldo;
    p.c32 = out32; p.ldc32 = ldo;
    p.c16 = out16; p.ldc16 = ldo;
    p.vec_ok = (N % 8 == 0) && (ldo % 8 == 0);
    return kgemm_launch(p, 0, glu ? KG_EPI_SWIGLU : KG_EPI_STORE, st);
}
}  // namespace

int svc_ar::reserve(int S, hipStream_t st) {
    if (S <= cap_S) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws.release();
    cap_S = std::max(S, 8);
    const long Sr = cap_S;
    h32 = ws.alloc_n<float>(Sr * D, st);
    qkv32 = ws.alloc_n<float>(Sr * Nqkv, st);
    q32 = ws.alloc_n<float>(Sr * D, st);
    logits = ws.alloc_n<float>(round_up(V, 8), st);
    n16 = ws.alloc_n<half_t>(Sr * D, st);
    y16 = ws.alloc_n<half_t>(Sr * D, st);
    ff16 = ws.alloc_n<half_t>(Sr * I, st);
    x16 = ws.alloc_n<half_t>(Sr * D, st);
    d_pos = ws.alloc_n<int>(2 * Sr, st);
    gx = ws.alloc_n<float>(D, st);
    h32b = ws.alloc_n<float>(D, st);
    part = ws.alloc_n<float>((long)H * D, st);
    d_gen = reinterpret_cast<GenState*>(ws.alloc(sizeof(GenState), st));
    d_skey = ws.alloc_n<float>(SORT_N, st);
    d_sidx = ws.alloc_n<int>(SORT_N, st);
    d_lgp = ws.alloc_n<float>(SORT_N, st);
    if (!d_skey || !d_sidx || !d_lgp) return 1;
    if (!h32 || !qkv32 || !q32 || !logits || !n16 || !y16 || !ff16 || !x16 || !d_pos || !gx || !h32b || !part || !d_gen) return 1;
    if (graph) { (void)hipGraphExecDestroy(graph); graph = nullptr; }
    if (gen_graph) { (void)hipGraphExecDestroy(gen_graph); gen_graph = nullptr; }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// The dec_* kernels are instantiated for the ar_base sizes (KD = dim 768, KI = intermediate 2304: reduction lengths known
// at compile time, dead chunks pruned) and for runtime sizes (KD = KI = 0); dec_ffn13 adds NP = 12 head partials from
// registers (NP = 0: a runtime count).  Calls f(KD, KI, NP) with the instance for this shape, as compile-time constants.
namespace {
template <int N> using IntC = std::integral_constant<int, N>;
template <class F>
int with_dec_sizes(int D, int I, int H, F&& f) {
    const bool base = D == 768 && I == 2304;
    if (H == 12) return base ? f(IntC<768>(), IntC<2304>(), IntC<12>()) : f(IntC<0>(), IntC<0>(), IntC<12>());
    return base ? f(IntC<768>(), IntC<2304>(), IntC<0>()) : f(IntC<0>(), IntC<0>(), IntC<0>());
}
}  // namespace

int svc_ar::run(const float* x, int S, const int* d_positions, float* logits_out, hipStream_t st) {
    if (S == 1 && dec_step) return run_dec_step(x, d_positions, logits_out, st);
    if (x != h32) SVC_CHECK_HIP(hipMemcpyAsync(h32, x, (size_t)S * D * 4, hipMemcpyDeviceToDevice, st));
    if (S <= 8 ? run_gemv_layers(S, d_positions, st) : run_gemm_layers(S, d_positions, st)) return 1;
    return run_head(S, logits_out, st);
}

// S = 1 decode step: three launches per layer (dec_qkvraw | dec_w2qkv, dec_attn2, dec_ffn13) + the last w2 + head.
int svc_ar::run_dec_step(const float* x, const int* d_positions, float* logits_out, hipStream_t st) {
    if (x != h32) SVC_CHECK_HIP(hipMemcpyAsync(h32, x, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
    return with_dec_sizes(D, I, H, [&](auto KD, auto KI, auto NP) {
        for (int i = 0; i < L; ++i) {
            const Layer& ly = layers[i];
            if (i == 0)
                hipLaunchKernelGGL((dec_qkvraw_kernel<KD>), dim3(cdiv(Nqkv, 2)), dim3(64), 0, st, h32, ly.wc, D, Nqkv, qkv32);
            else
                hipLaunchKernelGGL((dec_w2qkv_kernel<KD, KI>), dim3(cdiv(D + Nqkv, 2)), dim3(64), 0, st, ff16, h32b, layers[i - 1].w2,
                                   ly.wc, I, D, Nqkv, h32, qkv32);
            hipLaunchKernelGGL(dec_attn2_kernel, dim3(DEC_NS, H), dim3(512), 0, st, h32, qkv32, cfg.norm_eps, rope, ly.kc, ly.vc, ly.wo, part,
                               d_positions, H, Hkv, Lmax);
            hipLaunchKernelGGL((dec_ffn13_kernel<NP, KD>), dim3(cdiv(2 * I, 16)), dim3(256), 0, st, h32, part, H, h32b, ly.g_ffn,
                               cfg.norm_eps, ly.w13, D, 2 * I, ff16);
            SVC_CHECK_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL((dec_w2_kernel<KI>), dim3(D / 2), dim3(64), 0, st, ff16, layers[L - 1].w2, I, D, h32b, h32);
        hipLaunchKernelGGL((dec_head_kernel<KD>), dim3(cdiv(V, 16)), dim3(256), 0, st, h32, g_final, cfg.norm_eps, w_out, D, V, logits_out);
        SVC_CHECK_HIP(hipGetLastError());
        return 0;
    });
}

// S <= 8: five launches per layer; the norms, RoPE and the cache scatter live in the GEMVs.
int svc_ar::run_gemv_layers(int S, const int* d_positions, hipStream_t st) {
    const size_t attn_lds = ((size_t)Lmax + 1024) * sizeof(float);
    for (int i = 0; i < L; ++i) {
        const Layer& ly = layers[i];
        GemvArgs a;
        memset(&a, 0, sizeof(a));
        a.x = h32; a.ldx = D; a.gamma = ly.g_attn; a.eps = cfg.norm_eps; a.W = ly.wqkv; a.ldw = D; a.S = S; a.N = Nqkv; a.K = D;
        a.q_out = q32; a.kc = ly.kc; a.vc = ly.vc; a.rope = rope; a.pos = d_positions; a.H = H; a.Hkv = Hkv; a.Lmax = Lmax;
        if (gemv_pair_launch<true, GV_QKV>(a, st)) return 1;
        hipLaunchKernelGGL(ar_attn_kernel, dim3(S, H), dim3(1024), attn_lds, st, q32, ly.kc, ly.vc, y16, d_positions, S, H, Hkv, Lmax);
        SVC_CHECK_HIP(hipGetLastError());
        memset(&a, 0, sizeof(a));
        a.x = y16; a.ldx = D; a.W = ly.wo; a.ldw = D; a.res = h32; a.ldres = D; a.out32 = h32; a.ldo = D; a.S = S; a.N = D; a.K = D;
        if (gemv_pair_launch<false, GV_PLAIN>(a, st)) return 1;
        memset(&a, 0, sizeof(a));
        a.x = h32; a.ldx = D; a.gamma = ly.g_ffn; a.eps = cfg.norm_eps; a.W = ly.w13; a.ldw = D; a.out16 = ff16; a.ldo = I;
        a.S = S; a.N = 2 * I; a.K = D;
        if (gemv_pair_launch<true, GV_GLU>(a, st)) return 1;
        memset(&a, 0, sizeof(a));
        a.x = ff16; a.ldx = I; a.W = ly.w2; a.ldw = I; a.res = h32; a.ldres = D; a.out32 = h32; a.ldo = D; a.S = S; a.N = D; a.K = I;
        if (gemv_pair_launch<false, GV_PLAIN>(a, st)) return 1;
    }
    return 0;
}

// S > 8 (prefill): RMSNorm, tap-GEMM linears, RoPE + cache scatter, attention.
int svc_ar::run_gemm_layers(int S, const int* d_positions, hipStream_t st) {
    const size_t attn_lds = ((size_t)Lmax + 1024) * sizeof(float);
    for (int i = 0; i < L; ++i) {
        const Layer& ly = layers[i];
        if (rmsnorm_mod_launch(h32, D, n16, D, ly.g_attn, nullptr, nullptr, 0, 0, S, D, S, cfg.norm_eps, st)) return 1;
        if (lin(n16, ly.wqkv, D, nullptr, qkv32, nullptr, Nqkv, S, Nqkv, D, false, st)) return 1;
        hipLaunchKernelGGL(ar_rope_cache_kernel, dim3(S), dim3(256), 0, st, qkv32, (long)Nqkv, q32, ly.kc, ly.vc, rope, d_positions,
                           S, H, Hkv, Lmax);
        SVC_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(ar_attn_kernel, dim3(S, H), dim3(1024), attn_lds, st, q32, ly.kc, ly.vc, y16, d_positions, S, H, Hkv, Lmax);
        SVC_CHECK_HIP(hipGetLastError());
        if (lin(y16, ly.wo, D, h32, h32, nullptr, D, S, D, D, false, st)) return 1;
        if (rmsnorm_mod_launch(h32, D, n16, D, ly.g_ffn, nullptr, nullptr, 0, 0, S, D, S, cfg.norm_eps, st)) return 1;
        if (lin(n16, ly.w13, D, nullptr, nullptr, ff16, I, S, 2 * I, D, true, st)) return 1;
        if (lin(ff16, ly.w2, I, h32, h32, nullptr, D, S, D, I, false, st)) return 1;
    }
    return 0;
}

// last token only (ar.py:255-259): final RMSNorm fused into the output GEMV
int svc_ar::run_head(int S, float* logits_out, hipStream_t st) {
    GemvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = h32 + (long)(S - 1) * D; a.ldx = D; a.gamma = g_final; a.eps = cfg.norm_eps; a.W = w_out; a.ldw = D;
    a.out32 = logits_out; a.ldo = V; a.S = 1; a.N = V; a.K = D;
    return gemv_pair_launch<true, GV_PLAIN>(a, st);
}

namespace {
// Captures the launches `body` issues on a fresh stream into *exec.
template <class F>
int capture_graph(hipGraphExec_t* exec, F&& body) {
    hipStream_t cs;
    SVC_CHECK_HIP(hipStreamCreate(&cs));
    hipGraph_t g = nullptr;
    SVC_CHECK_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = body(cs);
    const hipError_t e = hipStreamEndCapture(cs, &g);
    if (rc || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipStreamDestroy(cs);
        if (!rc) set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        return 1;
    }
    SVC_CHECK_HIP(hipGraphInstantiate(exec, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    (void)hipStreamDestroy(cs);
    return 0;
}
}  // namespace

int svc_ar::ensure_graph() {
    if (graph) return 0;
    return capture_graph(&graph, [&](hipStream_t cs) {
        if (run(gx, 1, d_pos, logits, cs)) return 1;
        hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(64), 0, cs, d_pos, (int*)nullptr);
        return hipGetLastError() != hipSuccess ? 1 : 0;
    });
}

int svc_ar::sample(const float* lg, const int* prev, int n_prev, int suppress, float temperature, float top_p, float rep_pen,
                   const float* exp_noise, int* idx_out, float* probs_out, GenState* gs, hipStream_t st, bool prepare_next,
                   unsigned long long seed, int step) {
    hipLaunchKernelGGL(ar_rank_kernel, dim3(cdiv(V, 16)), dim3(256), 0, st, lg, V, prev, n_prev, suppress, rep_pen, gs, d_skey, d_sidx, d_lgp);
    hipLaunchKernelGGL(ar_sample_kernel, dim3(1), dim3(1024), 0, st, d_lgp, V, d_skey, d_sidx, temperature, top_p, exp_noise, seed, step,
                       idx_out, probs_out, gs, prepare_next ? emb : nullptr, prepare_next ? h32 : nullptr, D, d_pos);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int svc_ar::ensure_gen_graph() {
    if (gen_graph) return 0;
    // the step runs in place on h32, which holds the embedding of the previous token (written by svc_ar_generate for the
    // first step and by the sampler of every step for the next one)
    return capture_graph(&gen_graph, [&](hipStream_t cs) {
        if (run(h32, 1, d_pos, logits, cs)) return 1;
        return sample(logits, nullptr, 0, -1, 1.f, 1.f, 1.f, nullptr, nullptr, nullptr, d_gen, cs, true);
    });
}

// ---- batch ---------------------------------------------------------------------------------------------------------
int svc_ar::ensure_batch_ws(hipStream_t st) {
    if (d_nb) return 0;
    bh = bws.alloc_n<float>((size_t)MAXB * D, st);
    bq = bws.alloc_n<float>((size_t)MAXB * D, st);
    blogits = bws.alloc_n<float>((size_t)MAXB * V, st);
    by16 = bws.alloc_n<half_t>((size_t)MAXB * D, st);
    bff16 = bws.alloc_n<half_t>((size_t)MAXB * I, st);
    d_bpos = bws.alloc_n<int>(2 * MAXB, st);
    d_slots = reinterpret_cast<GenSlot*>(bws.alloc(MAXB * sizeof(GenSlot), st));
    b_skey = bws.alloc_n<float>((size_t)MAXB * SORT_N, st);
    b_sidx = bws.alloc_n<int>((size_t)MAXB * SORT_N, st);
    b_lgp = bws.alloc_n<float>((size_t)MAXB * SORT_N, st);
    d_kvtab = reinterpret_cast<float**>(bws.alloc((size_t)L * 2 * MAXB * sizeof(float*), st));
    int* nb = bws.alloc_n<int>(1, st);
    if (!bh || !bq || !blogits || !by16 || !bff16 || !d_bpos || !d_slots || !b_skey || !b_sidx || !b_lgp || !d_kvtab || !nb) {
        bws.release();
        return 1;
    }
    if (slot_base.empty()) slot_base.assign(1, nullptr);
    d_nb = nb;
    cur_nb = 0;
    return upload_kvtab(st);
}

int svc_ar::upload_kvtab(hipStream_t st) {
    std::vector<float*> tab((size_t)L * 2 * MAXB, nullptr);
    for (int i = 0; i < L; ++i)
        for (int b = 0; b < max_batch; ++b) {
            tab[((size_t)i * 2) * MAXB + b] = slot_kc(b, i);
            tab[((size_t)i * 2 + 1) * MAXB + b] = slot_vc(b, i);
        }
    SVC_CHECK_HIP(hipMemcpyAsync(d_kvtab, tab.data(), tab.size() * sizeof(float*), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

int svc_ar::set_nb(int B, hipStream_t st) {
    if (B == cur_nb) return 0;
    SVC_CHECK_HIP(hipMemcpyAsync(d_nb, &B, sizeof(int), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    cur_nb = B;
    return 0;
}

// svc_ar_forward_generate on one slot's cache.  Every slot, slot 0 included, takes the GEMV-pair (S <= 8) or tap-GEMM
// layers -- never the B = 1 decode step -- so a sequence computes the same thing whichever slot it is given.
int svc_ar::prefill_slot(int slot, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out,
                         hipStream_t st) {
    if (reserve(S, st)) return 1;
    std::vector<int> pos(2 * S);
    for (int s = 0; s < S; ++s) {
        SVC_REQUIRE(input_pos[s] >= 0 && input_pos[s] < Lmax && kv_pos[s] >= 0 && kv_pos[s] < Lmax, "position out of range");
        pos[s] = (int)input_pos[s];
        pos[S + s] = (int)kv_pos[s];
    }
    SVC_CHECK_HIP(hipMemcpyAsync(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    SVC_CHECK_HIP(hipMemcpyAsync(h32, x, (size_t)S * D * 4, hipMemcpyDeviceToDevice, st));
    // the layer loops read the cache pointers from `layers`: point them at the slot while they enqueue
    std::vector<Layer> own = layers;
    for (int i = 0; i < L; ++i) { layers[i].kc = slot_kc(slot, i); layers[i].vc = slot_vc(slot, i); }
    const int rc = S <= 8 ? run_gemv_layers(S, d_pos, st) : run_gemm_layers(S, d_pos, st);
    layers = own;
    if (rc) return 1;
    return run_head(S, logits_out, st);
}

// The batched step on bh [Bp][D] (in place) -> blogits [Bp][V]; positions from d_bpos, live slots from d_nb.
int svc_ar::run_batch_step(int Bp, hipStream_t st) {
    const int G = H / Hkv;
    const int GT = G % 3 == 0 ? 3 : G % 2 == 0 ? 2 : 1;       // query heads per attention workgroup
    const bool base = D == 768 && I == 2304;       // ar_base: reduction lengths known at compile time
    auto go = [&](auto KD, auto KI) {
        for (int i = 0; i < L; ++i) {
            const Layer& ly = layers[i];
            float* const* kct = d_kvtab + ((size_t)i * 2) * MAXB;
            float* const* vct = d_kvtab + ((size_t)i * 2 + 1) * MAXB;
            BGemmArgs a;
            memset(&a, 0, sizeof(a));
            a.x = bh; a.ldx = D; a.gamma = ly.g_attn; a.eps = cfg.norm_eps; a.W = ly.wqkv; a.ldw = D; a.N = Nqkv; a.K = D;
            a.q_out = bq; a.kc = kct; a.vc = vct; a.rope = rope; a.pos = d_bpos; a.nb = d_nb; a.H = H; a.Hkv = Hkv; a.Lmax = Lmax;
            if (bgemm_launch<true, BG_QKV, 1, KD>(a, Bp, st)) return 1;
            const dim3 ag(Hkv * (G / GT), Bp);
            switch (GT) {
                case 3: hipLaunchKernelGGL(battn_kernel<3>, ag, dim3(512), 0, st, bq, kct, vct, by16, d_bpos, d_nb, H, Hkv, Lmax); break;
                case 2: hipLaunchKernelGGL(battn_kernel<2>, ag, dim3(512), 0, st, bq, kct, vct, by16, d_bpos, d_nb, H, Hkv, Lmax); break;
                default: hipLaunchKernelGGL(battn_kernel<1>, ag, dim3(512), 0, st, bq, kct, vct, by16, d_bpos, d_nb, H, Hkv, Lmax); break;
            }
            SVC_CHECK_HIP(hipGetLastError());
            memset(&a, 0, sizeof(a));
            a.x = by16; a.ldx = D; a.W = ly.wo; a.ldw = D; a.res = bh; a.out32 = bh; a.ldo = D; a.N = D; a.K = D;
            if (bgemm_launch<false, BG_PLAIN, 1, KD>(a, Bp, st)) return 1;
            memset(&a, 0, sizeof(a));
            a.x = bh; a.ldx = D; a.gamma = ly.g_ffn; a.eps = cfg.norm_eps; a.W = ly.w13; a.ldw = D; a.out16 = bff16; a.ldo = I;
            a.N = 2 * I; a.K = D;
            if (bgemm_launch<true, BG_GLU, 2, KD>(a, Bp, st)) return 1;
            memset(&a, 0, sizeof(a));
            a.x = bff16; a.ldx = I; a.W = ly.w2; a.ldw = I; a.res = bh; a.out32 = bh; a.ldo = D; a.N = D; a.K = I;
            if (bgemm_launch<false, BG_PLAIN, 1, KI>(a, Bp, st)) return 1;
        }
        BGemmArgs a;
        memset(&a, 0, sizeof(a));
        a.x = bh; a.ldx = D; a.gamma = g_final; a.eps = cfg.norm_eps; a.W = w_out; a.ldw = D; a.out32 = blogits; a.ldo = V;
        a.N = V; a.K = D;
        return bgemm_launch<true, BG_PLAIN, 1, KD>(a, Bp, st);
    };
    return base ? go(IntC<768>(), IntC<2304>()) : go(IntC<0>(), IntC<0>());
}

// One captured chain per padded batch: the step, then either the position advance (svc_ar_decode_step_batch) or the
// sampler over the live rows with the next embedding and the loop state (svc_ar_generate_batch).
int svc_ar::ensure_batch_graph(int Bp, bool gen) {
    hipGraphExec_t* ge = (gen ? bgen_graph : bstep_graph) + (Bp / 16 - 1);
    if (*ge) return 0;
    return capture_graph(ge, [&](hipStream_t cs) {
        if (run_batch_step(Bp, cs)) return 1;
        if (!gen) {
            hipLaunchKernelGGL(advance_pos_batch_kernel, dim3(1), dim3(MAXB), 0, cs, d_bpos, d_nb);
        } else {
            hipLaunchKernelGGL(ar_rank_batch_kernel, dim3(cdiv(V, 16), Bp), dim3(256), 0, cs, blogits, V, d_slots, d_nb, b_skey, b_sidx, b_lgp);
            hipLaunchKernelGGL(ar_sample_batch_kernel, dim3(Bp), dim3(1024), 0, cs, b_lgp, V, b_skey, b_sidx, d_slots, d_nb, emb, bh, D,
                               d_bpos, Lmax);
        }
        return hipGetLastError() != hipSuccess ? 1 : 0;
    });
}

extern "C" {

int svc_ar_create(const svc_ar_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, void* stream, svc_ar_t** out) {
    SVC_REQUIRE(cfg && weights && out, "null argument");
    SVC_REQUIRE(cfg->head_dim == 64 && cfg->dim == cfg->n_head * 64 && cfg->n_head % cfg->n_local_heads == 0, "AR: head_dim 64, GQA");
    SVC_REQUIRE(cfg->dim % 64 == 0 && cfg->intermediate_size % 64 == 0 && cfg->vocab_size <= SORT_N, "AR: shape limits");
    SVC_REQUIRE(cfg->max_seq_len >= 8 && cfg->max_seq_len <= 8192, "AR: max_seq_len");
    hipStream_t st = (hipStream_t)stream;
    svc_ar* m = new svc_ar();
    m->cfg = *cfg;
    m->D = cfg->dim; m->H = cfg->n_head; m->Hkv = cfg->n_local_heads; m->L = cfg->n_layer; m->I = cfg->intermediate_size;
    m->V = cfg->vocab_size; m->Lmax = cfg->max_seq_len; m->kvd = m->Hkv * 64; m->Nqkv = m->D + 2 * m->kvd;
    StateDict sd(weights, n_weights);
    auto fail = [&]() { delete m; return 1; };
    const int D = m->D, I = m->I, V = m->V;
    auto pack16 = [&](const std::string& name, int N, int K, long row0, long row_step, half_t* dst, long ld) -> int {
        const auto* w = sd.get(name);
        if (require_shape(w, name, {N, K})) return 1;
        return pack_f16_launch(w->data, dst + row0 * ld, N, 1, K, K, 0, 1, row_step * ld, 0, 1, nullptr, st);
    };
    auto vec = [&](const std::string& name, int n) -> float* {
        const auto* w = sd.get(name);
        if (require_shape(w, name, {n})) return nullptr;
        float* d = m->wts.alloc_n<float>(n, st);
        if (d) (void)hipMemcpyAsync(d, w->data, n * 4, hipMemcpyDeviceToDevice, st);
        return d;
    };
    m->layers.resize(m->L);
    for (int i = 0; i < m->L; ++i) {
        const std::string p = "model.layers." + std::to_string(i) + ".";
        auto& ly = m->layers[i];
        ly.wqkv = m->wts.alloc_n<half_t>(round_up(m->Nqkv, 128) * (long)D, st);
        ly.wo = m->wts.alloc_n<half_t>(round_up(D, 128) * (long)D, st);
        ly.w13 = m->wts.alloc_n<half_t>(round_up(2 * I, 128) * (long)D, st);
        ly.w2 = m->wts.alloc_n<half_t>(round_up(D, 128) * (long)I, st);
        ly.kc = m->wts.alloc_n<float>((long)m->Hkv * m->Lmax * 64, st);
        ly.vc = m->wts.alloc_n<float>((long)m->Hkv * m->Lmax * 64, st);
        if (!ly.wqkv || !ly.wo || !ly.w13 || !ly.w2 || !ly.kc || !ly.vc) return fail();
        if (pack16(p + "attention.wqkv.weight", m->Nqkv, D, 0, 1, ly.wqkv, D)) return fail();
        if (pack16(p + "attention.wo.weight", D, D, 0, 1, ly.wo, D)) return fail();
        if (pack16(p + "feed_forward.w1.weight", I, D, 0, 2, ly.w13, D)) return fail();
        if (pack16(p + "feed_forward.w3.weight", I, D, 1, 2, ly.w13, D)) return fail();
        if (pack16(p + "feed_forward.w2.weight", D, I, 0, 1, ly.w2, I)) return fail();
        ly.g_attn = vec(p + "attention_norm.weight", D);
        ly.g_ffn = vec(p + "ffn_norm.weight", D);
        if (!ly.g_attn || !ly.g_ffn) return fail();
    }
    // S = 1 takes the decode step when the dec_* kernels hold the shape: dec_attn2 covers 64 * DA_WO * DEC_NS wo rows per
    // head, and a lane holds DEC_MAXC chunks of 8 elements of each reduction (dim, intermediate_size).  Other shapes run
    // S = 1 on the GEMV-pair layers.
    m->dec_step = D <= 64 * DA_WO * DEC_NS && D <= 64 * 8 * DEC_MAXC && I <= 64 * 8 * DEC_MAXC;
    if (m->dec_step) {   // its weights: Wq' = wqkv diag(gamma_attn) and, for layers >= 1, W' = Wq' w2_prev composed in fp32
        const int Nq = m->Nqkv;
        Arena tmp;
        float* wq = tmp.alloc_n<float>((size_t)round_up(Nq, 128) * D, st);           // Wq'            [Nq][D]
        float* w2t = tmp.alloc_n<float>((size_t)round_up(I, 128) * D, st);           // w2_prev^T      [I][D]
        float* wp = tmp.alloc_n<float>((size_t)round_up(Nq, 128) * I, st);           // W' = Wq' w2    [Nq][I]
        bool ok = wq && w2t && wp;
        for (int i = 0; ok && i < m->L; ++i) {
            const std::string p = "model.layers." + std::to_string(i) + ".";
            auto& ly = m->layers[i];
            const auto* wqkv = sd.get(p + "attention.wqkv.weight");
            // columns scaled by gamma: dim0 of the pack = column index
            ok = ok && !pack_f32_launch(wqkv->data, wq, D, 1, Nq, 1, 0, D, 1, 0, D, ly.g_attn, st);
            if (i == 0) {
                ly.wc = m->wts.alloc_n<half_t>((size_t)round_up(Nq, 2) * D, st);
                ok = ok && ly.wc && !pack_f16_launch(wq, ly.wc, Nq, 1, D, D, 0, 1, D, 0, 1, nullptr, st);
                continue;
            }
            const auto* w2 = sd.get("model.layers." + std::to_string(i - 1) + ".feed_forward.w2.weight");        // [D][I]
            ok = ok && !pack_f32_launch(w2->data, w2t, I, 1, D, 1, 0, I, D, 0, 1, nullptr, st);                    // -> [I][D]
            if (!ok) break;
            KGemmParams g;
            memset(&g, 0, sizeof(g));
            g.M = Nq; g.N = I; g.Lout = Nq; g.a_seq_rows = Nq; g.c_seq_rows = Nq; g.a_stride = 1; g.a_len = Nq;
            g.n_taps = 1; g.a_ptr[0] = wq; g.a_ld[0] = D; g.a_ktiles[0] = D / 32;       // fp32 k-tiles of 32 elements (128 bytes)
            g.w = w2t; g.ldw = D; g.c32 = wp; g.ldc32 = I; g.vec_ok = 1;
            ok = ok && !kgemm_launch(g, 1, KG_EPI_STORE, st);                            // exact fp32 fma chain (v_mfma_f32_16x16x4_f32)
            const long ldc = (long)I + D;
            ly.wc = m->wts.alloc_n<half_t>((size_t)round_up(Nq, 2) * ldc, st);
            ok = ok && ly.wc && !pack_f16_launch(wp, ly.wc, Nq, 1, I, I, 0, 1, ldc, 0, 1, nullptr, st) &&
                 !pack_f16_launch(wq, ly.wc + I, Nq, 1, D, D, 0, 1, ldc, 0, 1, nullptr, st);
        }
        const hipError_t e = hipStreamSynchronize(st);                                 // tmp is freed on scope exit
        if (!ok || e != hipSuccess) {
            set_error(std::string("AR: composing the decode-step weights failed: ") + (ok ? hipGetErrorString(e) : get_error()));
            return fail();
        }
    }
    m->g_final = vec("model.norm.weight", D);
    m->w_out = m->wts.alloc_n<half_t>(round_up(V, 128) * (long)D, st);
    if (!m->g_final || !m->w_out) return fail();
    if (pack16("model.output.weight", V, D, 0, 1, m->w_out, D)) return fail();
    {   // bf16-rounded RoPE table over max_seq_len positions (ar.py:624-632)
        std::vector<float> tab((size_t)m->Lmax * 64);
        for (int i = 0; i < 32; ++i) {
            const float f = 1.0f / powf(cfg->rope_base, (float)(2 * i) / 64.0f);
            for (int t = 0; t < m->Lmax; ++t) {
                const float a = (float)t * f;
                float c = (float)cos((double)a), s = (float)sin((double)a);
                uint32_t u;
                memcpy(&u, &c, 4); u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000u; memcpy(&c, &u, 4);
                memcpy(&u, &s, 4); u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000u; memcpy(&s, &u, 4);
                tab[((size_t)t * 32 + i) * 2] = c;
                tab[((size_t)t * 32 + i) * 2 + 1] = s;
            }
        }
        m->rope = m->wts.alloc_n<float>(tab.size(), st);
        if (!m->rope) return fail();
        if (hipMemcpyAsync(m->rope, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) { set_error("rope upload failed"); return fail(); }
    }
    if (const auto* e = sd.get("model.embeddings.weight")) {       // optional: only svc_ar_generate needs it
        if (require_shape(e, "model.embeddings.weight", {V, D})) return fail();
        m->emb = m->wts.alloc_n<float>((size_t)V * D, st);
        if (!m->emb) return fail();
        if (hipMemcpyAsync(m->emb, e->data, (size_t)V * D * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("embedding copy failed");
            return fail();
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess) { set_error("sync failed"); return fail(); }
    *out = m;
    return 0;
}

void svc_ar_destroy(svc_ar_t* m) {
    if (m && m->graph) (void)hipGraphExecDestroy(m->graph);
    if (m && m->gen_graph) (void)hipGraphExecDestroy(m->gen_graph);
    for (int i = 0; m && i < MAXB / 16; ++i) {
        if (m->bstep_graph[i]) (void)hipGraphExecDestroy(m->bstep_graph[i]);
        if (m->bgen_graph[i]) (void)hipGraphExecDestroy(m->bgen_graph[i]);
    }
    delete m;
}

int svc_ar_reset(svc_ar_t* m, void* stream) {
    SVC_REQUIRE(m, "null argument");
    for (auto& ly : m->layers) {
        SVC_CHECK_HIP(hipMemsetAsync(ly.kc, 0, (size_t)m->Hkv * m->Lmax * 64 * 4, (hipStream_t)stream));
        SVC_CHECK_HIP(hipMemsetAsync(ly.vc, 0, (size_t)m->Hkv * m->Lmax * 64 * 4, (hipStream_t)stream));
    }
    return 0;
}

int svc_ar_forward_generate(svc_ar_t* m, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out,
                            void* stream) {
    SVC_REQUIRE(m && x && input_pos && kv_pos && logits_out && S >= 1, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (m->reserve(S, st)) return 1;
    std::vector<int> pos(2 * S);
    for (int s = 0; s < S; ++s) {
        SVC_REQUIRE(input_pos[s] >= 0 && input_pos[s] < m->Lmax && kv_pos[s] >= 0 && kv_pos[s] < m->Lmax, "position out of range");
        pos[s] = (int)input_pos[s];
        pos[S + s] = (int)kv_pos[s];
    }
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return m->run(x, S, m->d_pos, logits_out, st);
}

// One-token decode step replayed from a hipGraph.  The first call (or a call with set_pos != 0) sets the device
// positions {input_pos, kv_pos}; every replay advances both by one, as NaiveWrapper.generate does (ar.py:402-403).
int svc_ar_decode_step(svc_ar_t* m, const float* x, int set_pos, int64_t input_pos, int64_t kv_pos, float* logits_out, void* stream) {
    SVC_REQUIRE(m && x && logits_out, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (m->reserve(1, st)) return 1;
    if (set_pos) {
        SVC_REQUIRE(input_pos >= 0 && input_pos < m->Lmax && kv_pos >= 0 && kv_pos < m->Lmax, "position out of range");
        const int pos[2] = {(int)input_pos, (int)kv_pos};
        SVC_CHECK_HIP(hipMemcpyAsync(m->d_pos, pos, 8, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
    }
    if (m->ensure_graph()) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(m->gx, x, (size_t)m->D * 4, hipMemcpyDeviceToDevice, st));
    SVC_CHECK_HIP(hipGraphLaunch(m->graph, st));
    SVC_CHECK_HIP(hipMemcpyAsync(logits_out, m->logits, (size_t)m->V * 4, hipMemcpyDeviceToDevice, st));
    return 0;
}

// Whole generation loop of NaiveWrapper.generate (modules/v2/ar.py:382-422) for B = 1: prefill, then one captured
// decode step + on-device sampling per token; the host only looks at the tokens every `check_every` steps (EOS check),
// so there is no per-token synchronisation.  Tokens produced speculatively after an EOS are discarded.
int svc_ar_generate(svc_ar_t* m, const float* x_prefill, int S, const int64_t* input_pos, const int64_t* kv_pos,
                    const float* exp_noise, int max_new, int min_tokens_before_eos, float temperature, float top_p,
                    float repetition_penalty, int check_every, int32_t* tokens_out, int32_t* n_tokens, void* stream) {
    SVC_REQUIRE(m && x_prefill && input_pos && kv_pos && exp_noise && tokens_out && n_tokens && S >= 1 && max_new >= 1, "bad argument");
    SVC_REQUIRE(m->emb, "svc_ar_generate needs model.embeddings.weight in the state dict given to svc_ar_create");
    hipStream_t st = (hipStream_t)stream;
    const int V = m->V, eos = V - 1;
    if (check_every < 1) check_every = 16;
    // prefill + first token (EOS suppressed, no previous tokens: ar.py:399-401)
    if (m->reserve(S, st)) return 1;       // m->logits exists from here on
    if (svc_ar_forward_generate(m, x_prefill, S, input_pos, kv_pos, m->logits, stream)) return 1;
    if (m->sample(m->logits, nullptr, 0, eos, temperature, top_p, repetition_penalty, exp_noise, tokens_out, nullptr, nullptr, st)) return 1;
    if (m->reserve(1, st)) return 1;
    const int pos[2] = {(int)input_pos[S - 1] + 1, (int)kv_pos[S - 1] + 1};
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_pos, pos, 8, hipMemcpyHostToDevice, st));
    GenState gs;
    gs.noise = exp_noise; gs.seed = 0; gs.toks = tokens_out; gs.cnt = 1; gs.min_before_eos = min_tokens_before_eos; gs.eos = eos;
    gs.temperature = temperature; gs.top_p = top_p; gs.rep_pen = repetition_penalty;
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_gen, &gs, sizeof(gs), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ar_embed_kernel, dim3(1), dim3(256), 0, st, m->emb, m->d_gen, m->h32, m->D);   // input of the first step
    SVC_CHECK_HIP(hipGetLastError());
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    if (m->ensure_gen_graph()) return 1;
    std::vector<int32_t> host(max_new);
    int n = 1, checked = 1, t = 1;
    bool done = false;
    while (!done) {
        const int t_end = std::min(max_new, t + check_every);
        for (; t < t_end; ++t) {
            if (pos[0] + (t - 1) >= m->Lmax || pos[1] + (t - 1) >= m->Lmax) { done = true; break; }   // cache / RoPE table exhausted
            SVC_CHECK_HIP(hipGraphLaunch(m->gen_graph, st));      // decode step on embed(token t-1) -> sample token t, embed it, advance
        }
        if (t > checked) {
            SVC_CHECK_HIP(hipMemcpyAsync(host.data() + checked, tokens_out + checked, (size_t)(t - checked) * 4, hipMemcpyDeviceToHost, st));
            SVC_CHECK_HIP(hipStreamSynchronize(st));
            for (int i = checked; i < t; ++i) {
                if (host[i] == eos) { done = true; break; }
                n = i + 1;
            }
            checked = t;
        }
        if (t >= max_new) done = true;
    }
    *n_tokens = n;
    return 0;
}

int svc_ar_set_max_batch(svc_ar_t* m, int max_batch, void* stream) {
    SVC_REQUIRE(m, "null argument");
    SVC_REQUIRE(max_batch >= 1 && max_batch <= MAXB, "AR: max_batch must be 1 .. 64");
    hipStream_t st = (hipStream_t)stream;
    if (m->ensure_batch_ws(st)) return 1;
    if (max_batch == m->max_batch) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    m->slot_mem.release();
    m->slot_base.assign(1, nullptr);
    m->max_batch = 1;
    m->bpos_n = 0;
    for (int b = 1; b < max_batch; ++b) {
        float* p = m->slot_mem.alloc_n<float>((size_t)m->L * 2 * m->cache_elems(), st);
        if (!p) {
            m->slot_mem.release();
            m->slot_base.assign(1, nullptr);
            (void)m->upload_kvtab(st);
            return 1;
        }
        m->slot_base.push_back(p);
    }
    m->max_batch = max_batch;
    return m->upload_kvtab(st);
}

int svc_ar_prefill_slot(svc_ar_t* m, int slot, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out,
                        void* stream) {
    SVC_REQUIRE(m && x && input_pos && kv_pos && logits_out && S >= 1, "bad argument");
    SVC_REQUIRE(slot >= 0 && slot < m->max_batch, "AR: slot outside max_batch (svc_ar_set_max_batch)");
    hipStream_t st = (hipStream_t)stream;
    if (m->ensure_batch_ws(st)) return 1;
    return m->prefill_slot(slot, x, S, input_pos, kv_pos, logits_out, st);
}

int svc_ar_decode_step_batch(svc_ar_t* m, int B, const float* x, int set_pos, const int64_t* input_pos, const int64_t* kv_pos,
                             float* logits_out, void* stream) {
    SVC_REQUIRE(m, "null argument");
    SVC_REQUIRE(B >= 1 && B <= m->max_batch, "AR: batch outside 1 .. max_batch (svc_ar_set_max_batch)");
    SVC_REQUIRE(x && logits_out, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    int pos[2 * MAXB];
    if (set_pos) {
        SVC_REQUIRE(input_pos && kv_pos, "bad argument");
        memset(pos, 0, sizeof(pos));
        for (int b = 0; b < B; ++b) {
            SVC_REQUIRE(input_pos[b] >= 0 && input_pos[b] < m->Lmax && kv_pos[b] >= 0 && kv_pos[b] < m->Lmax, "position out of range");
            pos[b] = (int)input_pos[b];
            pos[MAXB + b] = (int)kv_pos[b];
        }
    } else {
        SVC_REQUIRE(m->bpos_n == B, "AR: svc_ar_decode_step_batch needs set_pos on the first step of a batch");
        memcpy(pos, m->h_bpos, sizeof(pos));
        for (int b = 0; b < B; ++b) SVC_REQUIRE(pos[b] < m->Lmax && pos[MAXB + b] < m->Lmax, "position out of range");
    }
    if (m->ensure_batch_ws(st)) return 1;
    if (set_pos) {
        SVC_CHECK_HIP(hipMemcpyAsync(m->d_bpos, pos, sizeof(pos), hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
    }
    m->bpos_n = 0;
    const int Bp = (int)round_up(B, 16);
    if (m->set_nb(B, st) || m->ensure_batch_graph(Bp, false)) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(m->bh, x, (size_t)B * m->D * 4, hipMemcpyDeviceToDevice, st));
    SVC_CHECK_HIP(hipGraphLaunch(m->bstep_graph[Bp / 16 - 1], st));
    SVC_CHECK_HIP(hipMemcpyAsync(logits_out, m->blogits, (size_t)B * m->V * 4, hipMemcpyDeviceToDevice, st));
    for (int b = 0; b < B; ++b) { pos[b] += 1; pos[MAXB + b] += 1; }
    memcpy(m->h_bpos, pos, sizeof(pos));
    m->bpos_n = B;
    return 0;
}

// B independent svc_ar_generate loops in one: per-slot prefill and first token, then one captured batched step + sampler
// per token for all slots; the host reads the slots' counters every `check_every` steps and stops once every slot is done.
// Draws: exp_noise [B][max_new][V], or (exp_noise null) generated in the sampler from seeds HOST [B].
static int ar_generate_batch(svc_ar_t* m, int B, const float* x_prefill, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos,
                             const float* exp_noise, const uint64_t* seeds, int max_new, int min_tokens_before_eos, float temperature,
                             float top_p, float repetition_penalty, int check_every, int32_t* tokens_out, int32_t* n_tokens, void* stream) {
    SVC_REQUIRE(m, "null argument");
    SVC_REQUIRE(B >= 1 && B <= m->max_batch, "AR: batch outside 1 .. max_batch (svc_ar_set_max_batch)");
    SVC_REQUIRE(x_prefill && S && input_pos && kv_pos && (exp_noise || seeds) && tokens_out && n_tokens && max_new >= 1, "bad argument");
    SVC_REQUIRE(m->emb, "svc_ar_generate_batch needs model.embeddings.weight in the state dict given to svc_ar_create");
    long rows = 0;
    for (int b = 0; b < B; ++b) {
        SVC_REQUIRE(S[b] >= 1, "bad argument");
        for (int s = 0; s < S[b]; ++s)
            SVC_REQUIRE(input_pos[rows + s] >= 0 && input_pos[rows + s] < m->Lmax && kv_pos[rows + s] >= 0 && kv_pos[rows + s] < m->Lmax,
                        "position out of range");
        rows += S[b];
    }
    hipStream_t st = (hipStream_t)stream;
    const int V = m->V, eos = V - 1;
    if (check_every < 1) check_every = 16;
    if (m->ensure_batch_ws(st)) return 1;
    m->bpos_n = 0;
    // per slot: prefill + first token (EOS suppressed, no previous tokens: ar.py:399-401)
    std::vector<GenSlot> slots(B);
    int pos[2 * MAXB] = {};
    rows = 0;
    for (int b = 0; b < B; ++b) {
        const float* noise = exp_noise ? exp_noise + (size_t)b * max_new * V : nullptr;
        const unsigned long long seed = exp_noise ? 0ull : (unsigned long long)seeds[b];
        int32_t* toks = tokens_out + (size_t)b * max_new;
        if (m->prefill_slot(b, x_prefill + rows * m->D, S[b], input_pos + rows, kv_pos + rows, m->blogits + (size_t)b * V, st)) return 1;
        if (m->sample(m->blogits + (size_t)b * V, nullptr, 0, eos, temperature, top_p, repetition_penalty, noise, toks, nullptr, nullptr, st,
                      false, seed, 0))
            return 1;
        rows += S[b];
        GenSlot& g = slots[b];
        g.noise = noise; g.seed = seed; g.toks = toks; g.cnt = 1; g.min_before_eos = min_tokens_before_eos; g.eos = eos;
        g.temperature = temperature; g.top_p = top_p; g.rep_pen = repetition_penalty; g.max_new = max_new;
        const int ip = (int)input_pos[rows - 1] + 1, kp = (int)kv_pos[rows - 1] + 1;
        g.done = max_new <= 1 || ip >= m->Lmax || kp >= m->Lmax;       // a finished slot keeps valid positions
        pos[b] = g.done ? ip - 1 : ip;
        pos[MAXB + b] = g.done ? kp - 1 : kp;
    }
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_slots, slots.data(), (size_t)B * sizeof(GenSlot), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_bpos, pos, sizeof(pos), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ar_embed_batch_kernel, dim3(B), dim3(256), 0, st, m->emb, m->d_slots, m->bh, m->D);     // input of the first step
    SVC_CHECK_HIP(hipGetLastError());
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    const int Bp = (int)round_up(B, 16);
    if (m->set_nb(B, st) || m->ensure_batch_graph(Bp, true)) return 1;
    auto all_done = [&]() {
        for (const GenSlot& g : slots) if (!g.done) return false;
        return true;
    };
    for (int t = 1; t < max_new && !all_done();) {
        const int t_end = std::min(max_new, t + check_every);
        for (; t < t_end; ++t) SVC_CHECK_HIP(hipGraphLaunch(m->bgen_graph[Bp / 16 - 1], st));
        SVC_CHECK_HIP(hipMemcpyAsync(slots.data(), m->d_slots, (size_t)B * sizeof(GenSlot), hipMemcpyDeviceToHost, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
    }
    for (int b = 0; b < B; ++b) n_tokens[b] = slots[b].cnt;
    return 0;
}

int svc_ar_generate_batch(svc_ar_t* m, int B, const float* x_prefill, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos,
                          const float* exp_noise, int max_new, int min_tokens_before_eos, float temperature, float top_p,
                          float repetition_penalty, int check_every, int32_t* tokens_out, int32_t* n_tokens, void* stream) {
    SVC_REQUIRE(exp_noise, "bad argument");
    return ar_generate_batch(m, B, x_prefill, S, input_pos, kv_pos, exp_noise, nullptr, max_new, min_tokens_before_eos, temperature, top_p,
                             repetition_penalty, check_every, tokens_out, n_tokens, stream);
}

int svc_ar_generate_batch_seeded(svc_ar_t* m, int B, const float* x_prefill, const int32_t* S, const int64_t* input_pos,
                                 const int64_t* kv_pos, const uint64_t* seeds, int max_new, int min_tokens_before_eos, float temperature,
                                 float top_p, float repetition_penalty, int check_every, int32_t* tokens_out, int32_t* n_tokens,
                                 void* stream) {
    SVC_REQUIRE(seeds, "bad argument");
    return ar_generate_batch(m, B, x_prefill, S, input_pos, kv_pos, nullptr, seeds, max_new, min_tokens_before_eos, temperature, top_p,
                             repetition_penalty, check_every, tokens_out, n_tokens, stream);
}

int svc_ar_exp_draws(svc_ar_t* m, uint64_t seed, int step0, int n_steps, float* out, void* stream) {
    SVC_REQUIRE(m && out && step0 >= 0 && n_steps >= 1 && n_steps <= 65535, "bad argument");
    hipLaunchKernelGGL(ar_exp_draws_kernel, dim3(cdiv(cdiv(m->V, 4), 256), n_steps), dim3(256), 0, (hipStream_t)stream,
                       (unsigned long long)seed, step0, m->V, out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int svc_ar_sample(svc_ar_t* m, const float* logits, const int32_t* prev_tokens, int n_prev, int suppress_token, float temperature,
                  float top_p, float repetition_penalty, const float* exp_noise, int32_t* idx_out, float* probs_out, void* stream) {
    SVC_REQUIRE(m && logits && exp_noise && idx_out && n_prev >= 0 && (n_prev == 0 || prev_tokens), "bad argument");
    if (m->reserve(1, (hipStream_t)stream)) return 1;
    return m->sample(logits, prev_tokens, n_prev, suppress_token, temperature, top_p, repetition_penalty, exp_noise, idx_out, probs_out,
                     nullptr, (hipStream_t)stream);
}

}  // extern "C"
