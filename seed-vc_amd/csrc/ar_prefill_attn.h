// The ragged AR prefill (svc_ar_prefill_batch, svc_ar_admit): n sequences, concatenated row after row, go through the
// layers in one pass, each into the cache of its own slot.  The linears and norms are the tap-GEMM and RMSNorm launches of
// the one-sequence prefill over all rows; this header holds what is ragged: RoPE + cache scatter through a row -> slot
// table, the causal GQA attention over every slot's cache, and the gather of each sequence's last row for the head.
// Included by ar.hip only; nothing here is used by the one-sequence prefill or by the decode steps.
#pragma once
#include "ar_common.h"

namespace {

constexpr int PA_ROWS = 16;          // query rows of one attention tile: rows of ONE sequence, counted from its first row
constexpr int PA_KT = 32;            // keys staged per step
constexpr int PA_LD = 68;            // LDS row stride in floats: 16-byte aligned, and row r starts at bank 4 r (mod 64)

// Per-pass tables, one upload (device ints): input_pos [R] | kv_pos [R] | slot of the row [R] | tiles [T][3] = (first row,
// rows, slot) | last row of every sequence [n].
struct PrefillTabs {
    const int* ipos;
    const int* kpos;
    const int* rslot;
    const int* tiles;
    const int* last;
};

// ar_rope_cache_kernel with the cache found per row: RoPE (bf16-rounded table) on q and k, k / v scattered into row kv_pos of
// the row's slot.  qkv [R][D + 2 kvd] fp32.
__global__ void ar_rope_cache_ragged_kernel(const float* __restrict__ qkv, long ldq, float* __restrict__ q_out,
                                            float* const* __restrict__ kc_tab, float* const* __restrict__ vc_tab,
                                            const float* __restrict__ rope, const PrefillTabs tb, int H, int Hkv, int Lmax) {
    const int s = blockIdx.x;
    const int D = H * 64, kvd = Hkv * 64;
    const float* row = qkv + (long)s * ldq;
    const int ip = tb.ipos[s], kp = tb.kpos[s], slot = tb.rslot[s];
    float* kc = kc_tab[slot];
    float* vc = vc_tab[slot];
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

int ar_rope_cache_ragged_launch(const float* qkv, long ldq, float* q_out, float* const* kc_tab, float* const* vc_tab, const float* rope,
                                const PrefillTabs& tb, int R, int H, int Hkv, int Lmax, hipStream_t st) {
    hipLaunchKernelGGL(ar_rope_cache_ragged_kernel, dim3(R), dim3(256), 0, st, qkv, ldq, q_out, kc_tab, vc_tab, rope, tb, H, Hkv, Lmax);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// Causal prefill attention on the fp32 MFMA (v_mfma_f32_16x16x4_f32: an fp32 fmaf chain, no new precision mode).
// Workgroup = (tile of PA_ROWS query rows of one sequence, GW query heads of one KV head), one wave per head: the K / V
// rows of the KV head are staged in LDS once per workgroup, PA_KT keys at a time, and every wave reads them from there
// (GQA: for ar_base six heads x 16 rows against one 64-wide K / V stream).  The next chunk's global loads are issued
// before the MFMAs of the current one and land in LDS behind them.
//
// A wave computes the TRANSPOSED scores, S^T = K Q^T (A = K rows from LDS, B = q from registers, pre-scaled by 1/8):
// lane (g = lane >> 4, c = lane & 15) then holds S^T[key 4 g + r][row c], r = 0 .. 3 -- every value of a lane belongs to
// query row c.  So the running maximum, the running sum and the rescale factor of a row live in the lanes of its column
// (the maximum over the four lane groups is two lane exchanges), the causal mask is a compare with the lane's own
// kv_pos, and the probabilities are, as they stand, the B operand of O^T = V^T P^T (k index g of MFMA r = key 4 g + r; the A
// operand V^T is read from LDS in the same key order): no transposition, no LDS round trip for P.  O^T[d][row c] ends up
// as four consecutive d per register quad: one 8-byte fp16 store per quad.
//
// Row s attends to rows 0 .. kv_pos[s] of its own slot.  The key loop runs to the tile's largest kv_pos; a key above a row's
// own kv_pos gets the score -1e30 and the probability 0 by SELECT (never by arithmetic on what was loaded), and the
// address of a key above the tile's largest kv_pos is clamped onto that row.  So no cache row above the tile's prefix is
// ever read: whatever an earlier sequence left there -- Inf and NaN included -- cannot reach the result, not even as
// 0 x value.  (A key between a row's own kv_pos and the tile's largest is a row of this very sequence.)
// No atomics; a row's sums run over its keys in an order fixed by the model shape and its own kv_pos: chunks that lie
// wholly above a row's kv_pos leave its maximum, sum and output bit for bit as they were.
template <int GW>
__global__ __launch_bounds__(GW * 64) void ar_prefill_attn_kernel(const float* __restrict__ q, float* const* __restrict__ kc_tab,
                                                                  float* const* __restrict__ vc_tab, half_t* __restrict__ y,
                                                                  const PrefillTabs tb, int H, int Hkv, int Lmax) {
    constexpr int NT = GW * 64;
    constexpr int NL = (PA_KT * 16 + NT - 1) / NT;      // 16-byte pieces of a K (or V) chunk per thread
    __shared__ __attribute__((aligned(16))) float ks[PA_KT * PA_LD];
    __shared__ __attribute__((aligned(16))) float vs[PA_KT * PA_LD];
    const int row0 = tb.tiles[3 * blockIdx.x], nrows = tb.tiles[3 * blockIdx.x + 1], slot = tb.tiles[3 * blockIdx.x + 2];
    const int G = H / Hkv, ngrp = G / GW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int hk = blockIdx.y / ngrp, h = hk * G + (blockIdx.y % ngrp) * GW + wave;
    const int D = H * 64;
    // lane column c = query row c of the tile; the columns past a short tile repeat its last row and are not stored
    const int row = row0 + (c < nrows ? c : nrows - 1);
    const int kv = tb.kpos[row];
    int kmax = kv;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) { const int u = __shfl_xor(kmax, o); kmax = u > kmax ? u : kmax; }
    kmax = __builtin_amdgcn_readfirstlane(kmax);        // the same in every wave: they hold the same rows
    float4v qf[4];                                      // q[row c][16 i + 4 g .. + 3] / 8 (exact)
#pragma unroll
    for (int i = 0; i < 4; ++i) qf[i] = *reinterpret_cast<const float4v*>(q + (long)row * D + h * 64 + 16 * i + 4 * g) * 0.125f;
    const float* kb = kc_tab[slot] + (long)hk * Lmax * 64;
    const float* vb = vc_tab[slot] + (long)hk * Lmax * 64;
    float4v kreg[NL], vreg[NL];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            if (NL * NT == PA_KT * 16 || idx < PA_KT * 16) {
                const int j = k0 + (idx >> 4);
                const long o = (long)(j < kmax ? j : kmax) * 64 + 4 * (idx & 15);
                kreg[i] = *reinterpret_cast<const float4v*>(kb + o);
                vreg[i] = *reinterpret_cast<const float4v*>(vb + o);
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * NT;
            if (NL * NT == PA_KT * 16 || idx < PA_KT * 16) {
                *reinterpret_cast<float4v*>(&ks[(idx >> 4) * PA_LD + 4 * (idx & 15)]) = kreg[i];
                *reinterpret_cast<float4v*>(&vs[(idx >> 4) * PA_LD + 4 * (idx & 15)]) = vreg[i];
            }
        }
    };
    float4v o[4];                                       // O^T[d = 16 i + 4 g + r][row c]
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (float4v){0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;                  // l_run: this lane's keys only, the four groups meet at the end
    fetch(0);
    stage();
    __syncthreads();
    for (int k0 = 0; k0 <= kmax; k0 += PA_KT) {
        const bool more = k0 + PA_KT <= kmax;
        if (more) fetch(k0 + PA_KT);
        float4v s[PA_KT / 16];
#pragma unroll
        for (int u = 0; u < PA_KT / 16; ++u) {
            s[u] = (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4v kf = *reinterpret_cast<const float4v*>(&ks[(16 * u + c) * PA_LD + 16 * i + 4 * g]);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[i][e], s[u], 0, 0, 0);
            }
        }
        float mx = -1e30f;
#pragma unroll
        for (int u = 0; u < PA_KT / 16; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = k0 + 16 * u + 4 * g + r <= kv;
                s[u][r] = valid ? s[u][r] : -1e30f;
                mx = fmaxf(mx, s[u][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float scale = __expf(m_run - m_new);
        m_run = m_new;
        float ls = 0.f;
#pragma unroll
        for (int u = 0; u < PA_KT / 16; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = k0 + 16 * u + 4 * g + r <= kv;
                const float p = valid ? __expf(s[u][r] - m_new) : 0.f;
                s[u][r] = p;
                ls += p;
            }
        l_run = l_run * scale + ls;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] *= scale;
#pragma unroll
        for (int u = 0; u < PA_KT / 16; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    o[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(vs[(16 * u + 4 * g + r) * PA_LD + 16 * i + c], s[u][r], o[i], 0, 0, 0);
        __syncthreads();                                // every wave is done with this chunk
        if (more) {
            stage();
            __syncthreads();
        }
    }
    float l = l_run;
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (c < nrows) {
        const float inv = 1.0f / l;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            half4 out;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[r] = (half_t)(o[i][r] * inv);
            *reinterpret_cast<half4*>(y + (long)row * D + h * 64 + 16 * i + 4 * g) = out;
        }
    }
}

// GW = the largest divisor of H / Hkv that is at most 8 (ar_base: 6).  Contract (held by tests/test_gpu_ar_step.py): a tile
// addresses cache rows 0 .. its largest kv_pos of its own slot only; a row's output does not depend on the later rows of its tile.
int ar_prefill_attn_launch(const float* q, float* const* kc_tab, float* const* vc_tab, half_t* y, const PrefillTabs& tb, int n_tiles, int H,
                           int Hkv, int Lmax, hipStream_t st) {
    const int G = H / Hkv;
    int GW = 8;
    while (G % GW) --GW;
    const dim3 grid(n_tiles, Hkv * (G / GW)), block(GW * 64);
#define SVC_PA_CASE(N) \
    case N: hipLaunchKernelGGL(ar_prefill_attn_kernel<N>, grid, block, 0, st, q, kc_tab, vc_tab, y, tb, H, Hkv, Lmax); break;
    switch (GW) {
        SVC_PA_CASE(1) SVC_PA_CASE(2) SVC_PA_CASE(3) SVC_PA_CASE(4) SVC_PA_CASE(5) SVC_PA_CASE(6) SVC_PA_CASE(7) SVC_PA_CASE(8)
    }
#undef SVC_PA_CASE
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// out[i] = x[last[i]]: the last row of every sequence, packed for the head
__global__ void ar_gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ last, float* __restrict__ out, int D) {
    const float* src = x + (long)last[blockIdx.x] * D;
    for (int cc = threadIdx.x; cc < D; cc += blockDim.x) out[(long)blockIdx.x * D + cc] = src[cc];
}

int ar_gather_rows_launch(const float* x, const int* last, float* out, int D, int n, hipStream_t st) {
    hipLaunchKernelGGL(ar_gather_rows_kernel, dim3(n), dim3(256), 0, st, x, last, out, D);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// Admission of n requests into a running session: request i's loop state goes to d_slots[slot], its positions to d_bpos and
// the embedding of its first token (sampled just before, on the same stream) to the slot's row of the step input.  Only
// these slots are written.
struct AdmitRec {
    GenSlot g;
    int slot, ip, kp;
};

__global__ void ar_admit_kernel(const AdmitRec* __restrict__ recs, GenSlot* __restrict__ slots, int* __restrict__ pos,
                                const float* __restrict__ emb, float* __restrict__ x, int D) {
    const AdmitRec* r = recs + blockIdx.x;
    const int b = r->slot;
    const long t = r->g.toks[r->g.cnt - 1];
    for (int cc = threadIdx.x; cc < D; cc += blockDim.x) x[(long)b * D + cc] = emb[t * D + cc];
    if (threadIdx.x == 0) {
        slots[b] = r->g;
        pos[b] = r->ip;
        pos[MAXB + b] = r->kp;
    }
}

// Slots b0 .. b0 + n - 1 become free: finished slots with valid positions that record nothing (GenSlot by value).
__global__ void ar_idle_slots_kernel(GenSlot* __restrict__ slots, int* __restrict__ pos, const GenSlot idle, int b0, int n) {
    const int b = b0 + threadIdx.x;
    if ((int)threadIdx.x < n) {
        slots[b] = idle;
        pos[b] = 0;
        pos[MAXB + b] = 0;
    }
}

int ar_idle_slots_launch(GenSlot* slots, int* pos, const GenSlot& idle, int b0, int n, hipStream_t st) {
    hipLaunchKernelGGL(ar_idle_slots_kernel, dim3(1), dim3(MAXB), 0, st, slots, pos, idle, b0, n);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int ar_admit_launch(const AdmitRec* recs, int n, GenSlot* slots, int* pos, const float* emb, float* x, int D, hipStream_t st) {
    hipLaunchKernelGGL(ar_admit_kernel, dim3(n), dim3(256), 0, st, recs, slots, pos, emb, x, D);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace
