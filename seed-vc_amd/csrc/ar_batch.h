// The batched AR decode step (B <= 64 sequences, one slot each): skinny MFMA GEMM, one-token attention over every slot's
// cache, position advance, and their launch functions.  Included by ar.hip only.
#pragma once
#include "ar_common.h"

namespace {

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
    // the linear itself; everything else (norm, residual, outputs, QKV) starts out null / 0
    BGemmArgs(const void* x_, long ldx_, const half_t* W_, long ldw_, int N_, int K_)
        : x(x_), ldx(ldx_), gamma(nullptr), eps(0.f), W(W_), ldw(ldw_), res(nullptr), out32(nullptr), out16(nullptr), ldo(0), N(N_), K(K_),
          q_out(nullptr), kc(nullptr), vc(nullptr), rope(nullptr), pos(nullptr), nb(nullptr), H(0), Hkv(0), Lmax(0) {}
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

// Contract (held by tests/test_gpu_ar_step.py): K a multiple of 32; rows [0, N rounded up to 16 NT) of W are read; all Bp rows of
// x are read and may hold anything in the padding rows (NaN included): a column of the MFMA never meets another.  PLAIN and GLU
// store all Bp rows of the output; QKV stores q_out and cache rows of slots b < *nb only and never dereferences the table above.
// `res` may be `out32` (a lane reads its four residuals before it stores the same four elements).
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

// Bp rows (live slots + padding of the M tile); GT = 3, 2 or 1 query heads per workgroup, whichever divides H / Hkv first.
// Contract: rows b >= *nb of y keep their bits and their table entries (NULL in the model) are loaded but never dereferenced;
// slot b addresses cache rows 0 .. kv_pos[b] only; pos holds 2 MAXB entries whatever Bp is.
int battn_launch(const float* q, float* const* kc_tab, float* const* vc_tab, half_t* y, const int* pos, const int* nb, int Bp, int H,
                 int Hkv, int Lmax, hipStream_t st) {
    const int G = H / Hkv;
    const int GT = G % 3 == 0 ? 3 : G % 2 == 0 ? 2 : 1;
    const dim3 grid(Hkv * (G / GT), Bp), block(512);
    switch (GT) {
        case 3: hipLaunchKernelGGL(battn_kernel<3>, grid, block, 0, st, q, kc_tab, vc_tab, y, pos, nb, H, Hkv, Lmax); break;
        case 2: hipLaunchKernelGGL(battn_kernel<2>, grid, block, 0, st, q, kc_tab, vc_tab, y, pos, nb, H, Hkv, Lmax); break;
        default: hipLaunchKernelGGL(battn_kernel<1>, grid, block, 0, st, q, kc_tab, vc_tab, y, pos, nb, H, Hkv, Lmax); break;
    }
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ void advance_pos_batch_kernel(int* __restrict__ pos, const int* __restrict__ nb) {
    const int b = threadIdx.x;
    if (b < *nb) { pos[b] += 1; pos[MAXB + b] += 1; }
}

int advance_pos_batch_launch(int* pos, const int* nb, hipStream_t st) {
    hipLaunchKernelGGL(advance_pos_batch_kernel, dim3(1), dim3(MAXB), 0, st, pos, nb);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace
