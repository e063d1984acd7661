// The AR sampler (repetition penalty, top-p, temperature, exponential race; explicit or Philox-seeded draws) for one
// sequence and for the slots of a batch, the embedding kernels that feed a drawn token back, and their launch functions.
// Included by ar.hip only.
#pragma once
#include "ar_common.h"
#include "philox.h"

namespace {

// x = embeddings[previous token]  (embed_base of the token sampled by the previous step, ar.py:188-193,414)
__global__ void ar_embed_kernel(const float* __restrict__ emb, const GenState* __restrict__ gs, float* __restrict__ x, int D) {
    const long t = gs->toks[gs->cnt - 1];
    for (int c = threadIdx.x; c < D; c += blockDim.x) x[c] = emb[t * D + c];
}

// ---- sampler: one block, vocab <= 4096.  reference: ar.py:731-763 + :723-727

// Seeded Exp(1) draws: Philox4x32-10 (philox.h), key = (seed low word, seed high word), counter =
// (v / 4, token step, 0, 0); output word j of the call is the draw of vocabulary entry 4 (v / 4) + j.  A draw is a pure
// function of (seed, step, v): nothing about the slot, the batch or the other sequences enters it.
// u = ((word >> 8) + 1) * 2^-24 lies in (0, 1] and is exact in fp32, so q = -log(u) is finite (<= 16.64) and >= 0.
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

int ar_embed_launch(const float* emb, const GenState* gs, float* x, int D, hipStream_t st) {
    hipLaunchKernelGGL(ar_embed_kernel, dim3(1), dim3(256), 0, st, emb, gs, x, D);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int ar_embed_batch_launch(const float* emb, const GenSlot* slots, float* x, int D, int B, hipStream_t st) {
    hipLaunchKernelGGL(ar_embed_batch_kernel, dim3(B), dim3(256), 0, st, emb, slots, x, D);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int ar_exp_draws_launch(unsigned long long seed, int step0, int n_steps, int V, float* out, hipStream_t st) {
    hipLaunchKernelGGL(ar_exp_draws_kernel, dim3(cdiv(cdiv(V, 4), 256), n_steps), dim3(256), 0, st, seed, step0, V, out);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// Both sampler stages for one sequence; skey / sidx / lgp [SORT_N] carry stage 1's result to stage 2.  gs null: the
// explicit arguments; gs set: the generate loop's state, and with emb / next_x / pos it also prepares the next step.
int ar_sampler_launch(const float* logits, int V, const int* prev, int n_prev, int suppress, float rep_pen, float temperature, float top_p,
                      const float* exp_noise, unsigned long long seed, int step, int* idx_out, float* probs_out, GenState* gs,
                      const float* emb, float* next_x, int D, int* pos, float* skey, int* sidx, float* lgp, hipStream_t st) {
    hipLaunchKernelGGL(ar_rank_kernel, dim3(cdiv(V, 16)), dim3(256), 0, st, logits, V, prev, n_prev, suppress, rep_pen, gs, skey, sidx, lgp);
    hipLaunchKernelGGL(ar_sample_kernel, dim3(1), dim3(1024), 0, st, lgp, V, skey, sidx, temperature, top_p, exp_noise, seed, step, idx_out,
                       probs_out, gs, emb, next_x, D, pos);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

// Both stages for the live slots among Bp rows; skey / sidx / lgp [MAXB][SORT_N].
int ar_sampler_batch_launch(const float* logits, int V, GenSlot* slots, const int* nb, float* skey, int* sidx, float* lgp, const float* emb,
                            float* next_x, int D, int* pos, int Lmax, int Bp, hipStream_t st) {
    hipLaunchKernelGGL(ar_rank_batch_kernel, dim3(cdiv(V, 16), Bp), dim3(256), 0, st, logits, V, slots, nb, skey, sidx, lgp);
    hipLaunchKernelGGL(ar_sample_batch_kernel, dim3(Bp), dim3(1024), 0, st, lgp, V, skey, sidx, slots, nb, emb, next_x, D, pos, Lmax);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace
