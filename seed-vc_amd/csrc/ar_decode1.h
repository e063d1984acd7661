// The S = 1 decode step of the AR model (B = 1, slot 0): its kernels, one launch function per kernel and the size
// dispatch that selects their instances.  Included by ar.hip only.
#pragma once
#include "ar_common.h"

namespace {

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
// prefix [0, kv_pos] -- up to max_seq_len (<= 8192) x 64 fp32 keys and values, read from L2 / Infinity Cache -- and applies 1 / DEC_NS of the
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

// The dec_* kernels are instantiated for the ar_base sizes (KD = dim 768, KI = intermediate 2304: reduction lengths known
// at compile time, dead chunks pruned) and for runtime sizes (KD = KI = 0); dec_ffn13 adds NP = 12 head partials from
// registers (NP = 0: a runtime count).  Calls f(KD, KI, NP) with the instance for this shape, as compile-time constants.
template <class F>
int with_dec_sizes(int D, int I, int H, F&& f) {
    return with_ar_sizes(D, I, [&](auto KD, auto KI) { return H == 12 ? f(KD, KI, IntC<12>()) : f(KD, KI, IntC<0>()); });
}

// One launch function per kernel, on the constants with_dec_sizes hands out.
template <int KD>
int dec_qkvraw_launch(const float* h, const half_t* Wq, int K, int N, float* out, hipStream_t st) {
    hipLaunchKernelGGL((dec_qkvraw_kernel<KD>), dim3(cdiv(N, 2)), dim3(64), 0, st, h, Wq, K, N, out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int KD, int KI>
int dec_w2qkv_launch(const half_t* ff, const float* h_mid, const half_t* W2, const half_t* Wc, int I, int D, int N, float* h_out,
                     float* qkv_out, hipStream_t st) {
    hipLaunchKernelGGL((dec_w2qkv_kernel<KD, KI>), dim3(cdiv(D + N, 2)), dim3(64), 0, st, ff, h_mid, W2, Wc, I, D, N, h_out, qkv_out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// Contract (held by tests/test_gpu_ar_step.py, Lmax up to 8192): part [H][D] is written whole; cache row kv_pos of every KV head
// is written and nothing else; what that row held before never reaches the result (position kv_pos is served from registers);
// rows ABOVE kv_pos may be read (by position, clamped to Lmax - 1) and must be finite -- they enter as 0 x value; D <= 1024.
int dec_attn2_launch(const float* hres, const float* qkv_raw, float eps, const float* rope, float* kc, float* vc, const half_t* wo,
                     float* part, const int* pos, int H, int Hkv, int Lmax, hipStream_t st) {
    hipLaunchKernelGGL(dec_attn2_kernel, dim3(DEC_NS, H), dim3(512), 0, st, hres, qkv_raw, eps, rope, kc, vc, wo, part, pos, H, Hkv, Lmax);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int NP, int KD>
int dec_ffn13_launch(const float* h_in, const float* part, int n_part, float* h_out, const float* gamma, float eps, const half_t* W, int K,
                     int N, half_t* ff, hipStream_t st) {
    hipLaunchKernelGGL((dec_ffn13_kernel<NP, KD>), dim3(cdiv(N, 16)), dim3(256), 0, st, h_in, part, n_part, h_out, gamma, eps, W, K, N, ff);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int KI>
int dec_w2_launch(const half_t* x, const half_t* W, int K, int N, const float* res, float* out, hipStream_t st) {
    hipLaunchKernelGGL((dec_w2_kernel<KI>), dim3(cdiv(N, 2)), dim3(64), 0, st, x, W, K, N, res, out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int KD>
int dec_head_launch(const float* h, const float* gamma, float eps, const half_t* W, int K, int N, float* logits, hipStream_t st) {
    hipLaunchKernelGGL((dec_head_kernel<KD>), dim3(cdiv(N, 16)), dim3(256), 0, st, h, gamma, eps, W, K, N, logits);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int advance_pos_launch(int* pos, hipStream_t st) {
    hipLaunchKernelGGL(advance_pos_kernel, dim3(1), dim3(64), 0, st, pos, (int*)nullptr);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace
