// v2 AR model (NaiveTransformer, GQA 12q/2kv, KV cache): the handle, the host control flow and the C ABI of
// `forward_generate` (prefill and one-token decode step), the generate loops and the top-p / repetition-penalty /
// exponential-race sampler.  Every kernel and its launch function lives in a header that only this file includes:
//   ar_common.h   generate-loop state (GenState, GenSlot), MAXB, SORT_N, cross-lane sums, the ar_base size dispatch
//   ar_prefill.h  GEMV-pair linears (S <= 8 rows), RoPE + cache scatter, prefill attention
//   ar_prefill_attn.h  the ragged prefill of n sequences in one pass (RoPE / scatter per row's slot, MFMA attention), admission
//   ar_decode1.h  the S = 1 decode step, three launches per layer
//   ar_batch.h    the batched decode step: skinny MFMA GEMM, one-token attention per slot
//   ar_sampler.h  Philox draws, rank / sample kernels (one sequence and per slot), token embedding
//
// A forward takes one of three forms, by the number of rows S:
//   * S = 1 on slot 0, on a shape the one-token kernels hold (`dec_step`, decided once in svc_ar_create): the decode step;
//   * S <= 8 (and S = 1 on other shapes or slots): GEMV-pair layers, five launches per layer;
//   * S > 8 (prefill): the MFMA tap-GEMM on the same packed weights.
// The decode step is HBM-bound (every weight byte is read once per token), so its linears are wave-per-output-row GEMV
// kernels streaming fp16 weights with 16-byte loads.  The whole step (38 kernels for ar_base) is captured once into a
// hipGraph and replayed per token (the reference's answer to launch overhead is torch.compile "reduce-overhead",
// modules/v2/vc_wrapper.py:105-114); positions live in device memory and are advanced inside the graph, so a replay
// needs no host-side argument update.
//
// Up to 64 sequences decode together: each in its own slot (KV cache, positions), the linears as skinny MFMA GEMMs that
// read every weight byte once per step for all slots, one captured graph per padded batch, and the generate loop's state
// per slot (svc_ar_set_max_batch / _prefill_slot / _decode_step_batch / _generate_batch).  The B = 1 entry points work on
// slot 0, which exists from svc_ar_create on.
//
// Sessions (svc_ar_admit / _run / _retire) keep that batch open: sequences enter free slots while others are in
// mid-sequence (one ragged prefill for all newcomers, svc_ar_prefill_batch), the captured batched step runs over slots
// 0 .. highest occupied one, and a finished sequence frees its slot for the next.  Free slots sit in the batch as finished
// slots.  While a session is active the closed-batch entry points and svc_ar_set_max_batch are refused (they share the
// slot state), and so are the B = 1 calls while slot 0 is occupied.
//
// reference: modules/v2/ar.py:239-267 (forward_generate), :75-93 (KVCache.update), :503-567 (Attention),
//            :600-651 (RMSNorm, bf16 RoPE table), :712-763 (sample / logits_to_probs / exponential race).
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ar_common.h"
#include "ar_prefill.h"
#include "ar_prefill_attn.h"
#include "ar_decode1.h"
#include "ar_batch.h"
#include "ar_sampler.h"

namespace {
// Owns one instantiated graph.
struct GraphExec {
    hipGraphExec_t exec = nullptr;
    GraphExec() = default;
    GraphExec(GraphExec&& o) noexcept : exec(o.exec) { o.exec = nullptr; }
    GraphExec& operator=(GraphExec&& o) noexcept { std::swap(exec, o.exec); return *this; }
    ~GraphExec() { reset(); }
    void reset() {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
    }
};
}  // namespace

struct svc_ar {
    svc_ar_config_t cfg;
    int D, H, Hkv, L, I, V, Lmax, kvd, Nqkv;
    Arena wts, ws;
    struct Layer {
        half_t *wqkv, *wo, *w13, *w2;
        half_t* wc = nullptr;     // decode step (dec_step only): layer 0 [Nqkv][D] = wqkv diag(gamma); layers >= 1 [Nqkv][I + D] = [Wq' w2_prev | Wq']
        float *g_attn, *g_ffn;
    };
    std::vector<Layer> layers;
    float* g_final;
    half_t* w_out;
    float* rope;
    int cap_S = 0;
    float *h32, *qkv32, *q32, *logits;
    float *h32b, *part;           // S = 1 step: second residual buffer, per-head wo partials
    half_t *n16, *y16, *ff16, *x16;
    int* d_pos;                   // [2 S] input_pos then kv_pos of the rows in h32
    // Host mirror of the device positions {input_pos, kv_pos} that svc_ar_decode_step replays advance: valid from a set_pos call
    // until anything else rewrites d_pos (a prefill, svc_ar_generate, a reallocation), so a replay is checked against the cache
    // BEFORE it is launched -- the step itself writes cache row kv_pos and reads RoPE row input_pos unchecked.
    int h_pos[2] = {0, 0};
    bool pos_valid = false;
    GenState* d_gen = nullptr;    // generate-loop state (device)
    float *d_skey = nullptr, *d_lgp = nullptr;   // sampler stage 1 -> stage 2
    int* d_sidx = nullptr;
    int sample(const float* lg, const int* prev, int n_prev, int suppress, float temperature, float top_p, float rep_pen,
               const float* exp_noise, int* idx_out, float* probs_out, GenState* gs, hipStream_t st, bool prepare_next = false,
               unsigned long long seed = 0, int step = 0);      // exp_noise null (and gs null): the draws of (seed, step)
    // decode graphs; both capture `ws` pointers, so reserve() resets them when it reallocates
    GraphExec graph;              // step -> advance
    GraphExec gen_graph;          // step -> rank -> sample (+ next embedding, advance), driven by d_gen
    float* gx = nullptr;          // staged input of the captured step
    float* emb = nullptr;         // model.embeddings.weight [V][D] fp32 (generate loop only)
    int ensure_graph();
    int ensure_gen_graph();
    bool dec_step = false;        // S = 1 on slot 0 runs the decode step (the shape fits the dec_* kernels; `wc` is composed)

    // The KV cache of every slot: slot 0 comes from `wts` in svc_ar_create, slots 1 .. max_batch - 1 from `slot_mem` in
    // svc_ar_set_max_batch (one block per slot).
    int max_batch = 1;
    std::vector<float*> cache;         // [max_batch][L][2]: keys, values, cache_elems() floats each
    size_t cache_elems() const { return (size_t)Hkv * Lmax * 64; }
    float* kc(int slot, int layer) const { return cache[((size_t)slot * L + layer) * 2]; }
    float* vc(int slot, int layer) const { return cache[((size_t)slot * L + layer) * 2 + 1]; }

    // Rows of a forward must stay inside the cache and the RoPE table.
    bool rows_in_cache(const int64_t* input_pos, const int64_t* kv_pos, long n) const {
        for (long s = 0; s < n; ++s)
            if (input_pos[s] < 0 || input_pos[s] >= Lmax || kv_pos[s] < 0 || kv_pos[s] >= Lmax) return false;
        return true;
    }
    int reserve(int S, hipStream_t st);
    int prefill(int slot, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out, hipStream_t st,
                bool b1_step = false);
    int begin_generate(int slot, bool b1_step, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* lg,
                       const float* noise, unsigned long long seed, int32_t* toks, int min_before_eos, float temperature, float top_p,
                       float rep_pen, GenState* gs, hipStream_t st);
    int run_one(const float* x, float* logits_out, hipStream_t st);
    int run_rows(int slot, const float* x, int S, float* logits_out, hipStream_t st);
    int run_dec_step(const float* x, float* logits_out, hipStream_t st);
    int run_gemv_layers(int slot, int S, hipStream_t st);
    int run_gemm_layers(int slot, int S, hipStream_t st);
    int run_head(int S, float* logits_out, hipStream_t st);

    // ---- batch (svc_ar_set_max_batch).  The batch workspace is separate from `ws` (which reserve() may reallocate): the
    // captured batch graphs stay valid.
    Arena slot_mem, bws;
    float** d_kvtab = nullptr;         // device [L][2][MAXB] cache bases per layer (keys, values) and slot; null = no such slot
    float *bh = nullptr, *bq = nullptr, *blogits = nullptr;      // [MAXB][D] residual / q, [MAXB][V]
    half_t *by16 = nullptr, *bff16 = nullptr;                    // [MAXB][D], [MAXB][I]
    int *d_bpos = nullptr, *d_nb = nullptr;
    GenSlot* d_slots = nullptr;
    float *b_skey = nullptr, *b_lgp = nullptr;
    int* b_sidx = nullptr;
    GraphExec bstep_graph[MAXB / 16], bgen_graph[MAXB / 16];     // by padded batch: 16, 32, 48, 64 rows
    int cur_nb = 0;                    // value of *d_nb
    int bpos_n = 0;                    // slots whose device positions h_bpos mirrors (0: svc_ar_decode_step_batch needs set_pos)
    int h_bpos[2 * MAXB] = {};
    int ensure_batch_ws(hipStream_t st);
    int upload_kvtab(hipStream_t st);
    int set_nb(int B, hipStream_t st);
    int run_batch_step(int Bp, hipStream_t st);
    int ensure_batch_graph(int Bp, bool gen);

    // ---- ragged prefill (svc_ar_prefill_batch, svc_ar_admit).  A pass takes at most `prows_max` rows (PREFILL_ROWS unless
    // svc_ar_set_prefill_rows lowers it; never less than max_seq_len, so a sequence always fits); a call with more rows runs
    // as several passes of whole sequences.  The workspace is apart from `ws` and `bws`: no captured graph holds a pointer
    // into it, so it grows with the largest pass seen.
    static constexpr int PREFILL_ROWS = 8192;
    Arena pws;
    int pcap = 0, prows_max = PREFILL_ROWS, last_passes = 0;
    float *ph32 = nullptr, *pqkv32 = nullptr, *pq32 = nullptr;
    half_t *pn16 = nullptr, *py16 = nullptr, *pff16 = nullptr;
    int* d_ptab = nullptr;             // the pass's tables (PrefillTabs)
    float *plast = nullptr, *plogits = nullptr;      // [MAXB][D] last rows, [MAXB][V] first-token logits of an admission (in bws)
    AdmitRec* d_admit = nullptr;       // [MAXB] (in bws)
    int* d_idle_tok = nullptr;         // the one token (0) a free slot "has generated" (in bws)
    int reserve_prefill(int rows, hipStream_t st);
    int check_prefill_args(int n, const int* slots, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos) const;
    int prefill_batch(int n, const int* slots, const float* x, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos,
                      float* logits_out, hipStream_t st);
    int prefill_pass(int n, const int* slots, const float* x, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos,
                     float* logits_out, hipStream_t st);

    // ---- session: which slots hold an admitted sequence.  Active = n_occupied > 0.
    bool occupied[MAXB] = {};
    int n_occupied = 0;
    GenSlot idle_slot() const {
        GenSlot g;
        memset(&g, 0, sizeof(g));
        g.toks = d_idle_tok; g.cnt = 1; g.eos = V - 1; g.temperature = 1.f; g.top_p = 1.f; g.rep_pen = 1.f;
        g.done = 1; g.max_new = 1;
        return g;
    }
};

#define SVC_AR_NO_SESSION(m) SVC_REQUIRE(!(m)->n_occupied, "AR: a session is active (svc_ar_admit): retire every slot first")
#define SVC_AR_SLOT0_FREE(m) SVC_REQUIRE(!(m)->occupied[0], "AR: a session is active and holds slot 0, the cache of the B = 1 calls")

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
    pos_valid = false;
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
    graph.reset();
    gen_graph.reset();
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// forward_generate on one slot's cache: rows x [S][D] at (input_pos, kv_pos) -> logits of the last row.  Every slot, slot 0
// included, takes the GEMV-pair (S <= 8) or tap-GEMM layers, so a sequence computes the same thing whichever slot it is
// given -- unless the caller asks for the B = 1 decode step on a one-row call (b1_step; slot 0 only).
int svc_ar::prefill(int slot, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out, hipStream_t st,
                    bool b1_step) {
    if (reserve(S, st)) return 1;
    SVC_REQUIRE(rows_in_cache(input_pos, kv_pos, S), "position out of range");
    pos_valid = false;            // d_pos is rewritten below
    std::vector<int> pos(2 * S);
    for (int s = 0; s < S; ++s) {
        pos[s] = (int)input_pos[s];
        pos[S + s] = (int)kv_pos[s];
    }
    SVC_CHECK_HIP(hipMemcpyAsync(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return S == 1 && b1_step ? run_one(x, logits_out, st) : run_rows(slot, x, S, logits_out, st);
}

// One row on slot 0 at the positions in d_pos: what svc_ar_forward_generate runs for S = 1 and the B = 1 graphs replay.
int svc_ar::run_one(const float* x, float* logits_out, hipStream_t st) {
    return dec_step ? run_dec_step(x, logits_out, st) : run_rows(0, x, 1, logits_out, st);
}

int svc_ar::run_rows(int slot, const float* x, int S, float* logits_out, hipStream_t st) {
    if (x != h32) SVC_CHECK_HIP(hipMemcpyAsync(h32, x, (size_t)S * D * 4, hipMemcpyDeviceToDevice, st));
    if (S <= 8 ? run_gemv_layers(slot, S, st) : run_gemm_layers(slot, S, st)) return 1;
    return run_head(S, logits_out, st);
}

// S = 1 decode step: three launches per layer (dec_qkvraw | dec_w2qkv, dec_attn2, dec_ffn13) + the last w2 + head.
int svc_ar::run_dec_step(const float* x, float* logits_out, hipStream_t st) {
    if (x != h32) SVC_CHECK_HIP(hipMemcpyAsync(h32, x, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
    return with_dec_sizes(D, I, H, [&](auto KD, auto KI, auto NP) {
        for (int i = 0; i < L; ++i) {
            const Layer& ly = layers[i];
            if (i == 0 ? dec_qkvraw_launch<KD>(h32, ly.wc, D, Nqkv, qkv32, st)
                       : dec_w2qkv_launch<KD, KI>(ff16, h32b, layers[i - 1].w2, ly.wc, I, D, Nqkv, h32, qkv32, st))
                return 1;
            if (dec_attn2_launch(h32, qkv32, cfg.norm_eps, rope, kc(0, i), vc(0, i), ly.wo, part, d_pos, H, Hkv, Lmax, st)) return 1;
            if (dec_ffn13_launch<NP, KD>(h32, part, H, h32b, ly.g_ffn, cfg.norm_eps, ly.w13, D, 2 * I, ff16, st)) return 1;
        }
        if (dec_w2_launch<KI>(ff16, layers[L - 1].w2, I, D, h32b, h32, st)) return 1;
        return dec_head_launch<KD>(h32, g_final, cfg.norm_eps, w_out, D, V, logits_out, st);
    });
}

// S <= 8: five launches per layer; the norms, RoPE and the cache scatter live in the GEMVs.
int svc_ar::run_gemv_layers(int slot, int S, hipStream_t st) {
    for (int i = 0; i < L; ++i) {
        const Layer& ly = layers[i];
        GemvArgs qkv(h32, D, ly.wqkv, D, S, Nqkv, D);
        qkv.gamma = ly.g_attn; qkv.eps = cfg.norm_eps;
        qkv.q_out = q32; qkv.kc = kc(slot, i); qkv.vc = vc(slot, i); qkv.rope = rope; qkv.pos = d_pos;
        qkv.H = H; qkv.Hkv = Hkv; qkv.Lmax = Lmax;
        if (gemv_pair_launch<true, GV_QKV>(qkv, st)) return 1;
        if (ar_attn_launch(q32, kc(slot, i), vc(slot, i), y16, d_pos, S, H, Hkv, Lmax, st)) return 1;
        GemvArgs wo(y16, D, ly.wo, D, S, D, D);
        wo.res = h32; wo.ldres = D; wo.out32 = h32; wo.ldo = D;
        if (gemv_pair_launch<false, GV_PLAIN>(wo, st)) return 1;
        GemvArgs w13(h32, D, ly.w13, D, S, 2 * I, D);
        w13.gamma = ly.g_ffn; w13.eps = cfg.norm_eps; w13.out16 = ff16; w13.ldo = I;
        if (gemv_pair_launch<true, GV_GLU>(w13, st)) return 1;
        GemvArgs w2(ff16, I, ly.w2, I, S, D, I);
        w2.res = h32; w2.ldres = D; w2.out32 = h32; w2.ldo = D;
        if (gemv_pair_launch<false, GV_PLAIN>(w2, st)) return 1;
    }
    return 0;
}

// S > 8 (prefill): RMSNorm, tap-GEMM linears, RoPE + cache scatter, attention.
int svc_ar::run_gemm_layers(int slot, int S, hipStream_t st) {
    for (int i = 0; i < L; ++i) {
        const Layer& ly = layers[i];
        if (rmsnorm_mod_launch(h32, D, n16, D, ly.g_attn, nullptr, nullptr, 0, 0, S, D, S, cfg.norm_eps, st)) return 1;
        if (lin(n16, ly.wqkv, D, nullptr, qkv32, nullptr, Nqkv, S, Nqkv, D, false, st)) return 1;
        if (ar_rope_cache_launch(qkv32, Nqkv, q32, kc(slot, i), vc(slot, i), rope, d_pos, S, H, Hkv, Lmax, st)) return 1;
        if (ar_attn_launch(q32, kc(slot, i), vc(slot, i), y16, d_pos, S, H, Hkv, Lmax, st)) return 1;
        if (lin(y16, ly.wo, D, h32, h32, nullptr, D, S, D, D, false, st)) return 1;
        if (rmsnorm_mod_launch(h32, D, n16, D, ly.g_ffn, nullptr, nullptr, 0, 0, S, D, S, cfg.norm_eps, st)) return 1;
        if (lin(n16, ly.w13, D, nullptr, nullptr, ff16, I, S, 2 * I, D, true, st)) return 1;
        if (lin(ff16, ly.w2, I, h32, h32, nullptr, D, S, D, I, false, st)) return 1;
    }
    return 0;
}

// last token only (ar.py:255-259): final RMSNorm fused into the output GEMV
int svc_ar::run_head(int S, float* logits_out, hipStream_t st) {
    GemvArgs a(h32 + (long)(S - 1) * D, D, w_out, D, 1, V, D);
    a.gamma = g_final; a.eps = cfg.norm_eps; a.out32 = logits_out; a.ldo = V;
    return gemv_pair_launch<true, GV_PLAIN>(a, st);
}

// ---- ragged prefill ------------------------------------------------------------------------------------------------
int svc_ar::reserve_prefill(int rows, hipStream_t st) {
    if (rows <= pcap) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    pws.release();
    pcap = 0;
    const long R = rows;
    ph32 = pws.alloc_n<float>(R * D, st);
    pqkv32 = pws.alloc_n<float>(R * Nqkv, st);
    pq32 = pws.alloc_n<float>(R * D, st);
    pn16 = pws.alloc_n<half_t>(R * D, st);
    py16 = pws.alloc_n<half_t>(R * D, st);
    pff16 = pws.alloc_n<half_t>(R * I, st);
    d_ptab = pws.alloc_n<int>(3 * R + 3 * (R / PA_ROWS + MAXB) + MAXB, st);
    if (!ph32 || !pqkv32 || !pq32 || !pn16 || !py16 || !pff16 || !d_ptab) {
        pws.release();
        return 1;
    }
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    pcap = rows;
    return 0;
}

// Everything a ragged prefill needs from its arguments, before anything is launched.
int svc_ar::check_prefill_args(int n, const int* slots, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos) const {
    SVC_REQUIRE(n >= 1 && n <= max_batch, "AR: n outside 1 .. max_batch (svc_ar_set_max_batch)");
    bool seen[MAXB] = {};
    long rows = 0;
    for (int i = 0; i < n; ++i) {
        SVC_REQUIRE(slots[i] >= 0 && slots[i] < max_batch, "AR: slot outside 0 .. max_batch - 1 (svc_ar_set_max_batch)");
        SVC_REQUIRE(!seen[slots[i]], "AR: duplicate slot");
        SVC_REQUIRE(!occupied[slots[i]], "AR: slot is occupied by a session (svc_ar_retire)");
        seen[slots[i]] = true;
        SVC_REQUIRE(S[i] >= 1 && S[i] <= prows_max, "AR: S outside 1 .. rows of a prefill pass");
        SVC_REQUIRE(rows_in_cache(input_pos + rows, kv_pos + rows, S[i]), "position out of range");
        rows += S[i];
    }
    return 0;
}

// One pass: n whole sequences, R <= prows_max rows, through every layer; logits of each sequence's last row.
int svc_ar::prefill_pass(int n, const int* slots, const float* x, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos,
                         float* logits_out, hipStream_t st) {
    long R = 0;
    int T = 0;
    for (int i = 0; i < n; ++i) { R += S[i]; T += cdiv(S[i], PA_ROWS); }
    if (reserve_prefill((int)R, st)) return 1;
    std::vector<int> tab(3 * R + 3 * T + n);
    int *ip = tab.data(), *kp = ip + R, *rs = kp + R, *tiles = rs + R, *last = tiles + 3 * T;
    long r = 0;
    for (int i = 0; i < n; ++i) {
        for (int s0 = 0; s0 < S[i]; s0 += PA_ROWS) {
            *tiles++ = (int)r + s0;
            *tiles++ = std::min(PA_ROWS, S[i] - s0);
            *tiles++ = slots[i];
        }
        for (int s = 0; s < S[i]; ++s, ++r) {
            ip[r] = (int)input_pos[r];
            kp[r] = (int)kv_pos[r];
            rs[r] = slots[i];
        }
        last[i] = (int)r - 1;
    }
    SVC_CHECK_HIP(hipMemcpyAsync(d_ptab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    const PrefillTabs tb{d_ptab, d_ptab + R, d_ptab + 2 * R, d_ptab + 3 * R, d_ptab + 3 * R + 3 * T};
    SVC_CHECK_HIP(hipMemcpyAsync(ph32, x, (size_t)R * D * 4, hipMemcpyDeviceToDevice, st));
    const int Rr = (int)R;
    for (int i = 0; i < L; ++i) {
        const Layer& ly = layers[i];
        float* const* kct = d_kvtab + ((size_t)i * 2) * MAXB;
        float* const* vct = d_kvtab + ((size_t)i * 2 + 1) * MAXB;
        if (rmsnorm_mod_launch(ph32, D, pn16, D, ly.g_attn, nullptr, nullptr, 0, 0, Rr, D, Rr, cfg.norm_eps, st)) return 1;
        if (lin(pn16, ly.wqkv, D, nullptr, pqkv32, nullptr, Nqkv, Rr, Nqkv, D, false, st)) return 1;
        if (ar_rope_cache_ragged_launch(pqkv32, Nqkv, pq32, kct, vct, rope, tb, Rr, H, Hkv, Lmax, st)) return 1;
        if (ar_prefill_attn_launch(pq32, kct, vct, py16, tb, T, H, Hkv, Lmax, st)) return 1;
        if (lin(py16, ly.wo, D, ph32, ph32, nullptr, D, Rr, D, D, false, st)) return 1;
        if (rmsnorm_mod_launch(ph32, D, pn16, D, ly.g_ffn, nullptr, nullptr, 0, 0, Rr, D, Rr, cfg.norm_eps, st)) return 1;
        if (lin(pn16, ly.w13, D, nullptr, nullptr, pff16, I, Rr, 2 * I, D, true, st)) return 1;
        if (lin(pff16, ly.w2, I, ph32, ph32, nullptr, D, Rr, D, I, false, st)) return 1;
    }
    // head: final RMSNorm fused into the output GEMV, on the last row of every sequence, eight rows per launch
    if (ar_gather_rows_launch(ph32, tb.last, plast, D, n, st)) return 1;
    for (int j0 = 0; j0 < n; j0 += 8) {
        GemvArgs a(plast + (long)j0 * D, D, w_out, D, std::min(8, n - j0), V, D);
        a.gamma = g_final; a.eps = cfg.norm_eps; a.out32 = logits_out + (long)j0 * V; a.ldo = V;
        if (gemv_pair_launch<true, GV_PLAIN>(a, st)) return 1;
    }
    return 0;
}

// svc_ar_prefill_slot for n sequences at once (arguments checked by the caller): passes of whole sequences, greedily.
int svc_ar::prefill_batch(int n, const int* slots, const float* x, const int32_t* S, const int64_t* input_pos, const int64_t* kv_pos,
                          float* logits_out, hipStream_t st) {
    if (ensure_batch_ws(st)) return 1;
    last_passes = 0;
    long row0 = 0;
    for (int i0 = 0; i0 < n;) {
        int i1 = i0;
        long R = 0;
        while (i1 < n && R + S[i1] <= prows_max) R += S[i1++];
        if (prefill_pass(i1 - i0, slots + i0, x + row0 * D, S + i0, input_pos + row0, kv_pos + row0, logits_out + (long)i0 * V, st)) return 1;
        ++last_passes;
        row0 += R;
        i0 = i1;
    }
    return 0;
}

namespace {
// Captures the launches `body` issues on a fresh stream into `exec`.
template <class F>
int capture_graph(GraphExec& exec, F&& body) {
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
    SVC_CHECK_HIP(hipGraphInstantiate(&exec.exec, g, nullptr, nullptr, 0));
    (void)hipGraphDestroy(g);
    (void)hipStreamDestroy(cs);
    return 0;
}
}  // namespace

int svc_ar::ensure_graph() {
    if (graph.exec) return 0;
    return capture_graph(graph, [&](hipStream_t cs) {
        if (run_one(gx, logits, cs)) return 1;
        return advance_pos_launch(d_pos, cs);
    });
}

int svc_ar::sample(const float* lg, const int* prev, int n_prev, int suppress, float temperature, float top_p, float rep_pen,
                   const float* exp_noise, int* idx_out, float* probs_out, GenState* gs, hipStream_t st, bool prepare_next,
                   unsigned long long seed, int step) {
    return ar_sampler_launch(lg, V, prev, n_prev, suppress, rep_pen, temperature, top_p, exp_noise, seed, step, idx_out, probs_out, gs,
                             prepare_next ? emb : nullptr, prepare_next ? h32 : nullptr, D, d_pos, d_skey, d_sidx, d_lgp, st);
}

int svc_ar::ensure_gen_graph() {
    if (gen_graph.exec) return 0;
    // the step runs in place on h32, which holds the embedding of the previous token (written by svc_ar_generate for the
    // first step and by the sampler of every step for the next one)
    return capture_graph(gen_graph, [&](hipStream_t cs) {
        if (run_one(h32, logits, cs)) return 1;
        return sample(logits, nullptr, 0, -1, 1.f, 1.f, 1.f, nullptr, nullptr, nullptr, d_gen, cs, true);
    });
}

// Prefill + first token of one sequence (EOS suppressed, no previous tokens: ar.py:399-401) on `slot`, logits through `lg`,
// and in *gs the loop state from which the captured per-token graphs go on.
int svc_ar::begin_generate(int slot, bool b1_step, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* lg,
                           const float* noise, unsigned long long seed, int32_t* toks, int min_before_eos, float temperature, float top_p,
                           float rep_pen, GenState* gs, hipStream_t st) {
    const int eos = V - 1;
    if (prefill(slot, x, S, input_pos, kv_pos, lg, st, b1_step)) return 1;
    if (sample(lg, nullptr, 0, eos, temperature, top_p, rep_pen, noise, toks, nullptr, nullptr, st, false, seed, 0)) return 1;
    gs->noise = noise; gs->seed = seed; gs->toks = toks; gs->cnt = 1; gs->min_before_eos = min_before_eos; gs->eos = eos;
    gs->temperature = temperature; gs->top_p = top_p; gs->rep_pen = rep_pen;
    return 0;
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
    plast = bws.alloc_n<float>((size_t)MAXB * D, st);
    plogits = bws.alloc_n<float>((size_t)MAXB * V, st);
    d_admit = reinterpret_cast<AdmitRec*>(bws.alloc(MAXB * sizeof(AdmitRec), st));
    d_idle_tok = bws.alloc_n<int>(1, st);
    int* nb = bws.alloc_n<int>(1, st);
    if (!plast || !plogits || !d_admit || !d_idle_tok || !bh || !bq || !blogits || !by16 || !bff16 || !d_bpos || !d_slots || !b_skey || !b_sidx || !b_lgp || !d_kvtab || !nb) {
        bws.release();
        return 1;
    }
    d_nb = nb;
    cur_nb = 0;
    return upload_kvtab(st);
}

int svc_ar::upload_kvtab(hipStream_t st) {
    std::vector<float*> tab((size_t)L * 2 * MAXB, nullptr);
    for (int i = 0; i < L; ++i)
        for (int b = 0; b < max_batch; ++b) {
            tab[((size_t)i * 2) * MAXB + b] = kc(b, i);
            tab[((size_t)i * 2 + 1) * MAXB + b] = vc(b, i);
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

// The batched step on bh [Bp][D] (in place) -> blogits [Bp][V]; positions from d_bpos, live slots from d_nb.
int svc_ar::run_batch_step(int Bp, hipStream_t st) {
    return with_ar_sizes(D, I, [&](auto KD, auto KI) {
        for (int i = 0; i < L; ++i) {
            const Layer& ly = layers[i];
            float* const* kct = d_kvtab + ((size_t)i * 2) * MAXB;
            float* const* vct = d_kvtab + ((size_t)i * 2 + 1) * MAXB;
            BGemmArgs qkv(bh, D, ly.wqkv, D, Nqkv, D);
            qkv.gamma = ly.g_attn; qkv.eps = cfg.norm_eps;
            qkv.q_out = bq; qkv.kc = kct; qkv.vc = vct; qkv.rope = rope; qkv.pos = d_bpos; qkv.nb = d_nb;
            qkv.H = H; qkv.Hkv = Hkv; qkv.Lmax = Lmax;
            if (bgemm_launch<true, BG_QKV, 1, KD>(qkv, Bp, st)) return 1;
            if (battn_launch(bq, kct, vct, by16, d_bpos, d_nb, Bp, H, Hkv, Lmax, st)) return 1;
            BGemmArgs wo(by16, D, ly.wo, D, D, D);
            wo.res = bh; wo.out32 = bh; wo.ldo = D;
            if (bgemm_launch<false, BG_PLAIN, 1, KD>(wo, Bp, st)) return 1;
            BGemmArgs w13(bh, D, ly.w13, D, 2 * I, D);
            w13.gamma = ly.g_ffn; w13.eps = cfg.norm_eps; w13.out16 = bff16; w13.ldo = I;
            if (bgemm_launch<true, BG_GLU, 2, KD>(w13, Bp, st)) return 1;
            BGemmArgs w2(bff16, I, ly.w2, I, D, I);
            w2.res = bh; w2.out32 = bh; w2.ldo = D;
            if (bgemm_launch<false, BG_PLAIN, 1, KI>(w2, Bp, st)) return 1;
        }
        BGemmArgs head(bh, D, w_out, D, V, D);
        head.gamma = g_final; head.eps = cfg.norm_eps; head.out32 = blogits; head.ldo = V;
        return bgemm_launch<true, BG_PLAIN, 1, KD>(head, Bp, st);
    });
}

// One captured chain per padded batch: the step, then either the position advance (svc_ar_decode_step_batch) or the
// sampler over the live rows with the next embedding and the loop state (svc_ar_generate_batch).
int svc_ar::ensure_batch_graph(int Bp, bool gen) {
    GraphExec& ge = (gen ? bgen_graph : bstep_graph)[Bp / 16 - 1];
    if (ge.exec) return 0;
    return capture_graph(ge, [&](hipStream_t cs) {
        if (run_batch_step(Bp, cs)) return 1;
        return gen ? ar_sampler_batch_launch(blogits, V, d_slots, d_nb, b_skey, b_sidx, b_lgp, emb, bh, D, d_bpos, Lmax, Bp, cs)
                   : advance_pos_batch_launch(d_bpos, d_nb, cs);
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
        for (int kv = 0; kv < 2; ++kv) m->cache.push_back(m->wts.alloc_n<float>(m->cache_elems(), st));       // slot 0
        if (!ly.wqkv || !ly.wo || !ly.w13 || !ly.w2 || !m->kc(0, i) || !m->vc(0, i)) return fail();
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

void svc_ar_destroy(svc_ar_t* m) { delete m; }

int svc_ar_reset(svc_ar_t* m, void* stream) {
    SVC_REQUIRE(m, "null argument");
    SVC_AR_SLOT0_FREE(m);
    for (int i = 0; i < 2 * m->L; ++i)          // slot 0 only
        SVC_CHECK_HIP(hipMemsetAsync(m->cache[i], 0, m->cache_elems() * 4, (hipStream_t)stream));
    return 0;
}

int svc_ar_forward_generate(svc_ar_t* m, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out,
                            void* stream) {
    SVC_REQUIRE(m && x && input_pos && kv_pos && logits_out && S >= 1, "bad argument");
    SVC_AR_SLOT0_FREE(m);
    return m->prefill(0, x, S, input_pos, kv_pos, logits_out, (hipStream_t)stream, true);      // one row: the decode step
}

// One-token decode step replayed from a hipGraph.  The first call (or a call with set_pos != 0) sets the device
// positions {input_pos, kv_pos}; every replay advances both by one, as NaiveWrapper.generate does (ar.py:402-403).
int svc_ar_decode_step(svc_ar_t* m, const float* x, int set_pos, int64_t input_pos, int64_t kv_pos, float* logits_out, void* stream) {
    SVC_REQUIRE(m && x && logits_out, "bad argument");
    SVC_AR_SLOT0_FREE(m);
    hipStream_t st = (hipStream_t)stream;
    if (m->reserve(1, st)) return 1;
    if (set_pos) {
        SVC_REQUIRE(input_pos >= 0 && input_pos < m->Lmax && kv_pos >= 0 && kv_pos < m->Lmax, "position out of range");
        const int pos[2] = {(int)input_pos, (int)kv_pos};
        SVC_CHECK_HIP(hipMemcpyAsync(m->d_pos, pos, 8, hipMemcpyHostToDevice, st));
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        m->h_pos[0] = pos[0]; m->h_pos[1] = pos[1];
        m->pos_valid = true;
    } else {
        // every replay advanced both positions by one: the next one must still lie inside the cache and the RoPE table
        SVC_REQUIRE(m->pos_valid, "AR: svc_ar_decode_step needs set_pos on its first step and after any other B = 1 call");
        SVC_REQUIRE(m->h_pos[0] < m->Lmax && m->h_pos[1] < m->Lmax, "position out of range");
    }
    if (m->ensure_graph()) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(m->gx, x, (size_t)m->D * 4, hipMemcpyDeviceToDevice, st));
    SVC_CHECK_HIP(hipGraphLaunch(m->graph.exec, st));
    m->h_pos[0] += 1; m->h_pos[1] += 1;
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
    SVC_AR_SLOT0_FREE(m);
    hipStream_t st = (hipStream_t)stream;
    const int V = m->V, eos = V - 1;
    if (check_every < 1) check_every = 16;
    // prefill + first token, in svc_ar_forward_generate's form: a one-row prompt takes the decode-step kernels
    if (m->reserve(S, st)) return 1;       // m->logits exists from here on
    GenState gs;
    if (m->begin_generate(0, true, x_prefill, S, input_pos, kv_pos, m->logits, exp_noise, 0, tokens_out, min_tokens_before_eos, temperature,
                          top_p, repetition_penalty, &gs, st))
        return 1;
    const int pos[2] = {(int)input_pos[S - 1] + 1, (int)kv_pos[S - 1] + 1};
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_pos, pos, 8, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_gen, &gs, sizeof(gs), hipMemcpyHostToDevice, st));
    if (ar_embed_launch(m->emb, m->d_gen, m->h32, m->D, st)) return 1;      // input of the first step
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    if (m->ensure_gen_graph()) return 1;
    std::vector<int32_t> host(max_new);
    int n = 1, checked = 1, t = 1;
    bool done = false;
    while (!done) {
        const int t_end = std::min(max_new, t + check_every);
        for (; t < t_end; ++t) {
            if (pos[0] + (t - 1) >= m->Lmax || pos[1] + (t - 1) >= m->Lmax) { done = true; break; }   // cache / RoPE table exhausted
            SVC_CHECK_HIP(hipGraphLaunch(m->gen_graph.exec, st));     // decode step on embed(token t-1) -> sample token t, embed it, advance
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
    SVC_AR_NO_SESSION(m);
    hipStream_t st = (hipStream_t)stream;
    if (m->ensure_batch_ws(st)) return 1;
    if (max_batch == m->max_batch) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    m->slot_mem.release();
    m->cache.resize(2 * m->L);         // slot 0 stays
    m->max_batch = 1;
    m->bpos_n = 0;
    for (int b = 1; b < max_batch; ++b) {
        float* p = m->slot_mem.alloc_n<float>((size_t)m->L * 2 * m->cache_elems(), st);
        if (!p) {
            m->slot_mem.release();
            m->cache.resize(2 * m->L);
            (void)m->upload_kvtab(st);
            return 1;
        }
        for (int i = 0; i < 2 * m->L; ++i) m->cache.push_back(p + i * m->cache_elems());
    }
    m->max_batch = max_batch;
    return m->upload_kvtab(st);
}

int svc_ar_prefill_slot(svc_ar_t* m, int slot, const float* x, int S, const int64_t* input_pos, const int64_t* kv_pos, float* logits_out,
                        void* stream) {
    SVC_REQUIRE(m && x && input_pos && kv_pos && logits_out && S >= 1, "bad argument");
    SVC_REQUIRE(slot >= 0 && slot < m->max_batch, "AR: slot outside max_batch (svc_ar_set_max_batch)");
    SVC_REQUIRE(!m->occupied[slot], "AR: slot is occupied by a session (svc_ar_retire)");
    hipStream_t st = (hipStream_t)stream;
    if (m->ensure_batch_ws(st)) return 1;
    return m->prefill(slot, x, S, input_pos, kv_pos, logits_out, st);
}

int svc_ar_decode_step_batch(svc_ar_t* m, int B, const float* x, int set_pos, const int64_t* input_pos, const int64_t* kv_pos,
                             float* logits_out, void* stream) {
    SVC_REQUIRE(m, "null argument");
    SVC_AR_NO_SESSION(m);
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
    SVC_CHECK_HIP(hipGraphLaunch(m->bstep_graph[Bp / 16 - 1].exec, st));
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
    SVC_AR_NO_SESSION(m);
    SVC_REQUIRE(B >= 1 && B <= m->max_batch, "AR: batch outside 1 .. max_batch (svc_ar_set_max_batch)");
    SVC_REQUIRE(x_prefill && S && input_pos && kv_pos && (exp_noise || seeds) && tokens_out && n_tokens && max_new >= 1, "bad argument");
    SVC_REQUIRE(m->emb, "svc_ar_generate_batch needs model.embeddings.weight in the state dict given to svc_ar_create");
    long rows = 0;
    for (int b = 0; b < B; ++b) {
        SVC_REQUIRE(S[b] >= 1, "bad argument");
        SVC_REQUIRE(m->rows_in_cache(input_pos + rows, kv_pos + rows, S[b]), "position out of range");
        rows += S[b];
    }
    hipStream_t st = (hipStream_t)stream;
    const int V = m->V;
    if (check_every < 1) check_every = 16;
    if (m->ensure_batch_ws(st)) return 1;
    m->bpos_n = 0;
    // per slot: prefill (never the B = 1 decode step, see svc_ar::prefill) + first token
    std::vector<GenSlot> slots(B);
    int pos[2 * MAXB] = {};
    rows = 0;
    for (int b = 0; b < B; ++b) {
        GenSlot& g = slots[b];
        if (m->begin_generate(b, false, x_prefill + rows * m->D, S[b], input_pos + rows, kv_pos + rows, m->blogits + (size_t)b * V,
                              exp_noise ? exp_noise + (size_t)b * max_new * V : nullptr, exp_noise ? 0ull : (unsigned long long)seeds[b],
                              tokens_out + (size_t)b * max_new, min_tokens_before_eos, temperature, top_p, repetition_penalty, &g, st))
            return 1;
        rows += S[b];
        g.max_new = max_new;
        const int ip = (int)input_pos[rows - 1] + 1, kp = (int)kv_pos[rows - 1] + 1;
        g.done = max_new <= 1 || ip >= m->Lmax || kp >= m->Lmax;       // a finished slot keeps valid positions
        pos[b] = g.done ? ip - 1 : ip;
        pos[MAXB + b] = g.done ? kp - 1 : kp;
    }
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_slots, slots.data(), (size_t)B * sizeof(GenSlot), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_bpos, pos, sizeof(pos), hipMemcpyHostToDevice, st));
    if (ar_embed_batch_launch(m->emb, m->d_slots, m->bh, m->D, B, st)) return 1;       // input of the first step
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    const int Bp = (int)round_up(B, 16);
    if (m->set_nb(B, st) || m->ensure_batch_graph(Bp, true)) return 1;
    auto all_done = [&]() {
        for (const GenSlot& g : slots) if (!g.done) return false;
        return true;
    };
    for (int t = 1; t < max_new && !all_done();) {
        const int t_end = std::min(max_new, t + check_every);
        for (; t < t_end; ++t) SVC_CHECK_HIP(hipGraphLaunch(m->bgen_graph[Bp / 16 - 1].exec, st));
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

int svc_ar_set_prefill_rows(svc_ar_t* m, int rows) {
    SVC_REQUIRE(m, "null argument");
    SVC_REQUIRE(rows >= m->Lmax && rows <= svc_ar::PREFILL_ROWS, "AR: rows of a prefill pass must be max_seq_len .. 8192");
    m->prows_max = rows;
    return 0;
}

int svc_ar_prefill_passes(svc_ar_t* m) { return m ? m->last_passes : -1; }

int svc_ar_prefill_batch(svc_ar_t* m, int n, const int32_t* slots, const float* x, const int32_t* S, const int64_t* input_pos,
                         const int64_t* kv_pos, float* logits_out, void* stream) {
    SVC_REQUIRE(m && slots && x && S && input_pos && kv_pos && logits_out, "bad argument");
    if (m->check_prefill_args(n, slots, S, input_pos, kv_pos)) return 1;
    return m->prefill_batch(n, slots, x, S, input_pos, kv_pos, logits_out, (hipStream_t)stream);
}

int svc_ar_admit(svc_ar_t* m, int n, const svc_ar_request_t* requests, const float* x_prefill, const int64_t* input_pos,
                 const int64_t* kv_pos, void* stream) {
    SVC_REQUIRE(m && requests && x_prefill && input_pos && kv_pos, "bad argument");
    SVC_REQUIRE(n >= 1 && n <= m->max_batch, "AR: n outside 1 .. max_batch (svc_ar_set_max_batch)");
    SVC_REQUIRE(m->emb, "svc_ar_admit needs model.embeddings.weight in the state dict given to svc_ar_create");
    int slots[MAXB];
    int32_t S[MAXB];
    for (int i = 0; i < n; ++i) {
        SVC_REQUIRE(requests[i].max_new >= 1 && requests[i].tokens_out, "bad argument: max_new / tokens_out of a request");
        slots[i] = requests[i].slot;
        S[i] = requests[i].S;
    }
    if (m->check_prefill_args(n, slots, S, input_pos, kv_pos)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int V = m->V, eos = V - 1;
    if (m->ensure_batch_ws(st) || m->reserve(1, st)) return 1;       // reserve: the first token's sampler scratch
    if (!m->n_occupied) {
        // a session begins: every slot a finished one with valid positions, a zero row as its step input
        if (ar_idle_slots_launch(m->d_slots, m->d_bpos, m->idle_slot(), 0, MAXB, st)) return 1;
        SVC_CHECK_HIP(hipMemsetAsync(m->bh, 0, (size_t)MAXB * m->D * 4, st));
        m->bpos_n = 0;
    }
    if (m->prefill_batch(n, slots, x_prefill, S, input_pos, kv_pos, m->plogits, st)) return 1;
    std::vector<AdmitRec> recs(n);
    long rows = 0;
    for (int i = 0; i < n; ++i) {
        const svc_ar_request_t& q = requests[i];
        AdmitRec& a = recs[i];
        memset(&a, 0, sizeof(a));
        // first token: EOS suppressed, no previous tokens (ar.py:399-401), as begin_generate samples it
        if (m->sample(m->plogits + (size_t)i * V, nullptr, 0, eos, q.temperature, q.top_p, q.repetition_penalty, q.exp_noise, q.tokens_out,
                      nullptr, nullptr, st, false, (unsigned long long)q.seed, 0))
            return 1;
        rows += S[i];
        GenSlot& g = a.g;
        g.noise = q.exp_noise; g.seed = q.exp_noise ? 0ull : (unsigned long long)q.seed; g.toks = q.tokens_out; g.cnt = 1;
        g.min_before_eos = q.min_tokens_before_eos; g.eos = eos;
        g.temperature = q.temperature; g.top_p = q.top_p; g.rep_pen = q.repetition_penalty;
        g.max_new = q.max_new;
        const int ip = (int)input_pos[rows - 1] + 1, kp = (int)kv_pos[rows - 1] + 1;
        g.done = q.max_new <= 1 || ip >= m->Lmax || kp >= m->Lmax;      // admitted as finished: it keeps valid positions
        a.slot = q.slot;
        a.ip = g.done ? ip - 1 : ip;
        a.kp = g.done ? kp - 1 : kp;
    }
    SVC_CHECK_HIP(hipMemcpyAsync(m->d_admit, recs.data(), (size_t)n * sizeof(AdmitRec), hipMemcpyHostToDevice, st));
    if (ar_admit_launch(m->d_admit, n, m->d_slots, m->d_bpos, m->emb, m->bh, m->D, st)) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));        // `recs` may go
    for (int i = 0; i < n; ++i) m->occupied[slots[i]] = true;
    m->n_occupied += n;
    return 0;
}

int svc_ar_run(svc_ar_t* m, int n_steps, int32_t* n_tokens, int32_t* done, void* stream) {
    SVC_REQUIRE(m && n_tokens && done && n_steps >= 0, "bad argument");
    SVC_REQUIRE(m->n_occupied > 0, "AR: no session is active (svc_ar_admit)");
    hipStream_t st = (hipStream_t)stream;
    int B = 0;
    for (int b = 0; b < m->max_batch; ++b) if (m->occupied[b]) B = b + 1;
    const int Bp = (int)round_up(B, 16);
    if (m->set_nb(B, st) || m->ensure_batch_graph(Bp, true)) return 1;
    for (int t = 0; t < n_steps; ++t) SVC_CHECK_HIP(hipGraphLaunch(m->bgen_graph[Bp / 16 - 1].exec, st));
    std::vector<GenSlot> slots(B);
    SVC_CHECK_HIP(hipMemcpyAsync(slots.data(), m->d_slots, (size_t)B * sizeof(GenSlot), hipMemcpyDeviceToHost, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < m->max_batch; ++b) {
        const bool occ = b < B && m->occupied[b];
        n_tokens[b] = occ ? slots[b].cnt : 0;
        done[b] = occ ? slots[b].done : 1;
    }
    return 0;
}

int svc_ar_retire(svc_ar_t* m, int slot, void* stream) {
    SVC_REQUIRE(m, "null argument");
    SVC_REQUIRE(slot >= 0 && slot < m->max_batch && m->occupied[slot], "AR: slot is not occupied (svc_ar_admit)");
    // the slot becomes a finished one that records nothing, also when its sequence was still running
    if (ar_idle_slots_launch(m->d_slots, m->d_bpos, m->idle_slot(), slot, 1, (hipStream_t)stream)) return 1;
    m->occupied[slot] = false;
    m->n_occupied -= 1;
    return 0;
}

int svc_ar_session_active(svc_ar_t* m) { return m ? m->n_occupied : 0; }

int svc_ar_exp_draws(svc_ar_t* m, uint64_t seed, int step0, int n_steps, float* out, void* stream) {
    SVC_REQUIRE(m && out && step0 >= 0 && n_steps >= 1 && n_steps <= 65535, "bad argument");
    return ar_exp_draws_launch(seed, step0, n_steps, m->V, out, (hipStream_t)stream);
}

int svc_ar_sample(svc_ar_t* m, const float* logits, const int32_t* prev_tokens, int n_prev, int suppress_token, float temperature,
                  float top_p, float repetition_penalty, const float* exp_noise, int32_t* idx_out, float* probs_out, void* stream) {
    SVC_REQUIRE(m && logits && exp_noise && idx_out && n_prev >= 0 && (n_prev == 0 || prev_tokens), "bad argument");
    SVC_REQUIRE(suppress_token < m->V, "AR: suppress_token is a vocabulary index (negative: none)");      // it indexes the rank kernel's LDS
    if (m->reserve(1, (hipStream_t)stream)) return 1;
    return m->sample(logits, prev_tokens, n_prev, suppress_token, temperature, top_p, repetition_penalty, exp_noise, idx_out, probs_out,
                     nullptr, (hipStream_t)stream);
}

// Test aid: ONE call of the sampler launch the model makes (ar_sampler_launch without or with a GenState, or
// ar_sampler_batch_launch over the slots), on buffers of its own; see include/seedvc_hip.h.
int svc_op_ar_sampler(const svc_ar_sampler_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    SVC_REQUIRE(e, "svc_op_ar_sampler: null argument");
    SVC_REQUIRE(e->form >= 0 && e->form <= 2, "svc_op_ar_sampler: form is 0 .. 2");
    const int form = e->form, V = e->V, D = e->D;
    SVC_REQUIRE(V >= 1 && V <= SORT_N, "svc_op_ar_sampler: V is 1 .. 4096");
    SVC_REQUIRE(e->logits, "svc_op_ar_sampler: logits are required");
    const int B = form == 2 ? e->B : 1;
    if (form == 0) {
        SVC_REQUIRE(e->idx_out, "svc_op_ar_sampler: form 0 writes idx_out");
        SVC_REQUIRE(e->n_prev >= 0 && (e->n_prev == 0 || e->prev), "svc_op_ar_sampler: n_prev tokens need prev");
        SVC_REQUIRE(e->suppress < V, "svc_op_ar_sampler: suppress is a vocabulary index (negative: none)");
        SVC_REQUIRE(e->rep_pen >= 0.f, "svc_op_ar_sampler: rep_pen is a number >= 0");       // false for NaN
        SVC_REQUIRE(e->step >= 0, "svc_op_ar_sampler: step >= 0");
    } else {
        SVC_REQUIRE(form == 1 || (B >= 1 && B <= MAXB), "svc_op_ar_sampler: B is 1 .. 64");
        SVC_REQUIRE(e->max_new >= 1 && D >= 1, "svc_op_ar_sampler: max_new and D are positive");
        SVC_REQUIRE(e->emb && e->next_x && e->toks && e->pos, "svc_op_ar_sampler: the loop forms need emb, next_x, toks and pos");
        SVC_REQUIRE(e->s_cnt && e->s_min_before_eos && e->s_eos && e->s_temperature && e->s_top_p && e->s_rep_pen && e->s_seed,
                    "svc_op_ar_sampler: the loop forms need the per-slot arrays");
        SVC_REQUIRE(form == 1 || (e->s_done && e->s_max_new && e->s_has_noise), "svc_op_ar_sampler: form 2 needs done, max_new and has_noise per slot");
        SVC_REQUIRE(form == 1 || e->Lmax >= 1, "svc_op_ar_sampler: Lmax is positive");
        for (int b = 0; b < B; ++b) {
            const int mn = form == 2 ? e->s_max_new[b] : e->max_new;
            SVC_REQUIRE(mn >= 1 && mn <= e->max_new, "svc_op_ar_sampler: a slot's max_new is 1 .. max_new");
            SVC_REQUIRE(e->s_cnt[b] >= 1, "svc_op_ar_sampler: cnt >= 1");
            // token cnt is written at toks[cnt]: only a finished slot (which records nothing) may sit at cnt == max_new
            SVC_REQUIRE(e->s_cnt[b] < mn || (form == 2 && e->s_cnt[b] == mn && e->s_done[b]),
                        "svc_op_ar_sampler: cnt < max_new (form 2: cnt == max_new for a finished slot)");
            SVC_REQUIRE(e->s_eos[b] >= 0 && e->s_eos[b] < V, "svc_op_ar_sampler: eos is a vocabulary index");
            SVC_REQUIRE(e->s_rep_pen[b] >= 0.f, "svc_op_ar_sampler: rep_pen is a number >= 0");
            SVC_REQUIRE(form == 1 || !e->s_has_noise[b] || e->noise, "svc_op_ar_sampler: a slot with noise needs the noise buffer");
            if (form == 2)
                SVC_REQUIRE(e->pos[b] >= 0 && e->pos[b] < e->Lmax && e->pos[B + b] >= 0 && e->pos[B + b] < e->Lmax,
                            "svc_op_ar_sampler: positions lie in [0, Lmax)");
        }
    }
    Arena ar;
    const int rows = form == 2 ? MAXB : 1;
    float* skey = ar.alloc_n<float>((size_t)rows * SORT_N, st);
    int* sidx = ar.alloc_n<int>((size_t)rows * SORT_N, st);
    float* lgp = ar.alloc_n<float>((size_t)rows * SORT_N, st);
    if (!skey || !sidx || !lgp) return 1;
    if (form == 0) {
        if (ar_sampler_launch(e->logits, V, e->prev, e->n_prev, e->suppress, e->rep_pen, e->temperature, e->top_p, e->exp_noise, e->seed,
                              e->step, e->idx_out, e->probs_out, nullptr, nullptr, nullptr, 0, nullptr, skey, sidx, lgp, st)) return 1;
        SVC_CHECK_HIP(hipStreamSynchronize(st));
        return 0;
    }
    std::vector<GenSlot> slots(B);
    for (int b = 0; b < B; ++b) {
        GenSlot& g = slots[b];
        const bool has_noise = form == 2 ? e->s_has_noise[b] != 0 : e->noise != nullptr;
        g.noise = has_noise ? e->noise + (size_t)b * e->max_new * V : nullptr;
        g.seed = e->s_seed[b];
        g.toks = e->toks + (size_t)b * e->max_new;
        g.cnt = e->s_cnt[b];
        g.min_before_eos = e->s_min_before_eos[b];
        g.eos = e->s_eos[b];
        g.temperature = e->s_temperature[b];
        g.top_p = e->s_top_p[b];
        g.rep_pen = e->s_rep_pen[b];
        g.done = form == 2 ? e->s_done[b] : 0;
        g.max_new = form == 2 ? e->s_max_new[b] : e->max_new;
    }
    std::vector<int> pos(form == 2 ? 2 * MAXB : 2, 0);
    for (int b = 0; b < B; ++b) {
        pos[b] = e->pos[b];
        pos[(form == 2 ? MAXB : 1) + b] = e->pos[B + b];
    }
    GenSlot* d_slots = ar.alloc_n<GenSlot>(form == 2 ? MAXB : 1, st);
    int* d_pos = ar.alloc_n<int>(pos.size(), st);
    int* d_nb = ar.alloc_n<int>(1, st);
    if (!d_slots || !d_pos || !d_nb) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(d_slots, slots.data(), (size_t)B * sizeof(GenSlot), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(d_pos, pos.data(), pos.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(d_nb, &B, sizeof(int), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));            // the host arrays are pageable
    if (form == 1) {
        // a GenSlot begins with its GenState
        if (ar_sampler_launch(e->logits, V, nullptr, 0, -1, 1.f, 0.f, 0.f, nullptr, 0, 0, nullptr, e->probs_out, d_slots, e->emb, e->next_x, D,
                              d_pos, skey, sidx, lgp, st)) return 1;
    } else {
        if (ar_sampler_batch_launch(e->logits, V, d_slots, d_nb, skey, sidx, lgp, e->emb, e->next_x, D, d_pos, e->Lmax,
                                    (int)round_up(B, 16), st)) return 1;
    }
    SVC_CHECK_HIP(hipMemcpyAsync(slots.data(), d_slots, (size_t)B * sizeof(GenSlot), hipMemcpyDeviceToHost, st));
    SVC_CHECK_HIP(hipMemcpyAsync(pos.data(), d_pos, pos.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) {
        e->s_cnt[b] = slots[b].cnt;
        if (form == 2) e->s_done[b] = slots[b].done;
        e->pos[b] = pos[b];
        e->pos[B + b] = pos[(form == 2 ? MAXB : 1) + b];
    }
    return 0;
}

}  // extern "C"

namespace {
// What the cache-touching test aids share: the slots named by the caller, checked, and the device cache table over them.
int op_check_slots(const int32_t* slots, int n, int n_slots, bool distinct, const char* who) {
    bool seen[MAXB] = {};
    for (int i = 0; i < n; ++i) {
        SVC_REQUIRE(slots[i] >= 0 && slots[i] < n_slots, std::string(who) + ": a slot lies in [0, n_slots)");
        SVC_REQUIRE(!distinct || !seen[slots[i]], std::string(who) + ": a slot is named twice");
        seen[slots[i]] = true;
    }
    return 0;
}
int op_check_pos(const int32_t* pos, long R, int Lmax, const char* who) {
    for (long i = 0; i < 2 * R; ++i) SVC_REQUIRE(pos[i] >= 0 && pos[i] < Lmax, std::string(who) + ": positions lie in [0, Lmax)");
    return 0;
}
// device [2][MAXB] cache bases: entry b = the cache of slot tab_slots[b] for b < n, NULL above
int op_kvtab(Arena& ar, float* kc, float* vc, size_t slot_elems, const int32_t* tab_slots, int n, float*** out, hipStream_t st) {
    std::vector<float*> tab(2 * MAXB, nullptr);
    for (int b = 0; b < n; ++b) {
        tab[b] = kc + (size_t)tab_slots[b] * slot_elems;
        tab[MAXB + b] = vc + (size_t)tab_slots[b] * slot_elems;
    }
    float** d = reinterpret_cast<float**>(ar.alloc(tab.size() * sizeof(float*), st));
    if (!d) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(float*), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    *out = d;
    return 0;
}
int op_upload_ints(Arena& ar, const std::vector<int>& v, int** out, hipStream_t st) {
    int* d = ar.alloc_n<int>(v.size(), st);
    if (!d) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));            // the host vector is pageable
    *out = d;
    return 0;
}
}  // namespace

extern "C" {

// Test aid: ONE call of the launch function of a cache-touching AR kernel, on buffers of the caller; see include/seedvc_hip.h.
int svc_op_ar_attn(const svc_ar_attn_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const char* who = "svc_op_ar_attn";
    SVC_REQUIRE(e, "svc_op_ar_attn: null argument");
    const int kind = e->kind, H = e->H, Hkv = e->Hkv, Lmax = e->Lmax, n = e->n;
    SVC_REQUIRE(kind >= 0 && kind <= 5, "svc_op_ar_attn: kind is 0 .. 5");
    SVC_REQUIRE(H >= 1 && H <= 64 && Hkv >= 1, "svc_op_ar_attn: H is 1 .. 64, Hkv >= 1");
    SVC_REQUIRE(H % Hkv == 0, "svc_op_ar_attn: H % Hkv == 0");
    SVC_REQUIRE(Lmax >= 8 && Lmax <= 8192, "svc_op_ar_attn: Lmax is 8 .. 8192");
    SVC_REQUIRE(e->n_slots >= 1 && e->n_slots <= MAXB, "svc_op_ar_attn: n_slots is 1 .. 64");
    SVC_REQUIRE(e->x && e->kc && e->vc && e->slots && e->pos, "svc_op_ar_attn: x, kc, vc, slots and pos are required");
    const int D = H * 64, kvd = Hkv * 64;
    const bool ragged = kind == 3 || kind == 5;
    if (kind != 1) SVC_REQUIRE(n >= 1 && n <= (kind == 0 || kind == 4 ? 8192 : MAXB), "svc_op_ar_attn: n is 1 .. 8192 rows (kinds 0, 4) or 1 .. 64 slots or sequences");
    const int n_named = kind == 2 || ragged ? n : 1;
    if (op_check_slots(e->slots, n_named, e->n_slots, n_named > 1, who)) return 1;
    long R = kind == 1 ? 1 : n;
    int T = 0;
    if (ragged) {
        SVC_REQUIRE(e->seq_S, "svc_op_ar_attn: kinds 3 and 5 need seq_S");
        R = 0;
        for (int i = 0; i < n; ++i) {
            SVC_REQUIRE(e->seq_S[i] >= 1 && e->seq_S[i] <= 8192, "svc_op_ar_attn: S[i] is 1 .. 8192");
            R += e->seq_S[i];
            T += cdiv(e->seq_S[i], PA_ROWS);
        }
        SVC_REQUIRE(R <= 8192, "svc_op_ar_attn: at most 8192 rows");
    }
    if (op_check_pos(e->pos, R, Lmax, who)) return 1;
    if (kind == 0 || kind == 2 || kind == 3) SVC_REQUIRE(e->y16, "svc_op_ar_attn: kinds 0, 2 and 3 write y16");
    if (kind == 1 || kind >= 4) SVC_REQUIRE(e->rope, "svc_op_ar_attn: kinds 1, 4 and 5 need rope");
    if (kind >= 4) SVC_REQUIRE(e->q_out && e->ldq >= D + 2 * kvd, "svc_op_ar_attn: kinds 4 and 5 write q_out; ldq >= D + 2 kvd");
    if (kind == 1) {
        SVC_REQUIRE(e->hres && e->wo && e->part, "svc_op_ar_attn: kind 1 needs hres, wo and part");
        SVC_REQUIRE(D <= 64 * DA_WO * DEC_NS, "svc_op_ar_attn: kind 1 holds D <= 1024 (svc_ar_create clears the decode step above)");
    }
    const size_t slot_elems = (size_t)Hkv * Lmax * 64;
    float* kc0 = e->kc + (size_t)e->slots[0] * slot_elems;
    float* vc0 = e->vc + (size_t)e->slots[0] * slot_elems;
    half_t* y16 = reinterpret_cast<half_t*>(e->y16);
    Arena ar;
    int rc = 1;
    if (kind == 0 || kind == 1 || kind == 4) {
        int* d_pos;
        if (op_upload_ints(ar, std::vector<int>(e->pos, e->pos + 2 * R), &d_pos, st)) return 1;
        if (kind == 0) rc = ar_attn_launch(e->x, kc0, vc0, y16, d_pos, n, H, Hkv, Lmax, st);
        else if (kind == 1) rc = dec_attn2_launch(e->hres, e->x, e->eps, e->rope, kc0, vc0, reinterpret_cast<const half_t*>(e->wo), e->part, d_pos, H, Hkv, Lmax, st);
        else rc = ar_rope_cache_launch(e->x, e->ldq, e->q_out, kc0, vc0, e->rope, d_pos, n, H, Hkv, Lmax, st);
    } else if (kind == 2) {
        std::vector<int> pos(2 * MAXB + 1, 0);
        for (int b = 0; b < n; ++b) { pos[b] = e->pos[b]; pos[MAXB + b] = e->pos[n + b]; }
        pos[2 * MAXB] = n;
        int* d_pos;
        float** tab;
        if (op_upload_ints(ar, pos, &d_pos, st) || op_kvtab(ar, e->kc, e->vc, slot_elems, e->slots, n, &tab, st)) return 1;
        rc = battn_launch(e->x, tab, tab + MAXB, y16, d_pos, d_pos + 2 * MAXB, (int)round_up(n, 16), H, Hkv, Lmax, st);
    } else {
        // the tables of one ragged pass, as svc_ar::prefill_pass builds them; the cache table is indexed by slot
        std::vector<int> tab(3 * R + 3 * T + n), ident(e->n_slots);
        for (int i = 0; i < e->n_slots; ++i) ident[i] = i;
        int *ip = tab.data(), *kp = ip + R, *rs = kp + R, *tiles = rs + R, *last = tiles + 3 * T;
        long r = 0;
        for (int i = 0; i < n; ++i) {
            for (int s0 = 0; s0 < e->seq_S[i]; s0 += PA_ROWS) {
                *tiles++ = (int)r + s0;
                *tiles++ = std::min(PA_ROWS, e->seq_S[i] - s0);
                *tiles++ = e->slots[i];
            }
            for (int s = 0; s < e->seq_S[i]; ++s, ++r) { ip[r] = e->pos[r]; kp[r] = e->pos[R + r]; rs[r] = e->slots[i]; }
            last[i] = (int)r - 1;
        }
        int* d;
        float** kvt;
        if (op_upload_ints(ar, tab, &d, st) || op_kvtab(ar, e->kc, e->vc, slot_elems, ident.data(), e->n_slots, &kvt, st)) return 1;
        const PrefillTabs tb{d, d + R, d + 2 * R, d + 3 * R, d + 3 * R + 3 * T};
        rc = kind == 3 ? ar_prefill_attn_launch(e->x, kvt, kvt + MAXB, y16, tb, T, H, Hkv, Lmax, st)
                       : ar_rope_cache_ragged_launch(e->x, e->ldq, e->q_out, kvt, kvt + MAXB, e->rope, tb, (int)R, H, Hkv, Lmax, st);
    }
    if (rc) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

// Test aid: ONE call of the launch function of a skinny AR linear, in the instance the model selects; see include/seedvc_hip.h.
int svc_op_ar_linear(const svc_ar_linear_t* e, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const char* who = "svc_op_ar_linear";
    SVC_REQUIRE(e, "svc_op_ar_linear: null argument");
    const int path = e->path, role = e->role, D = e->D, I = e->I, H = e->H, Hkv = e->Hkv, V = e->V, rows = e->rows;
    SVC_REQUIRE(path >= 0 && path <= 2, "svc_op_ar_linear: path is 0 .. 2");
    SVC_REQUIRE(role >= 0 && role <= 4, "svc_op_ar_linear: role is 0 .. 4");
    SVC_REQUIRE(H >= 1 && Hkv >= 1 && H % Hkv == 0, "svc_op_ar_linear: H % Hkv == 0");
    SVC_REQUIRE(D >= 64 && D <= 8192 && D % 64 == 0 && I >= 64 && I <= 8192 && I % 64 == 0, "svc_op_ar_linear: D and I are multiples of 64, at most 8192");
    SVC_REQUIRE(D == H * 64, "svc_op_ar_linear: D == 64 H");
    SVC_REQUIRE(V >= 1 && V <= SORT_N, "svc_op_ar_linear: V is 1 .. 4096");
    if (path == 0) SVC_REQUIRE(rows >= 1 && rows <= 8, "svc_op_ar_linear: path 0 holds S = 1 .. 8 rows");
    if (path == 1) SVC_REQUIRE(rows >= 1 && rows <= MAXB, "svc_op_ar_linear: path 1 holds B = 1 .. 64 rows");
    if (path == 2)
        SVC_REQUIRE(D <= 64 * DA_WO * DEC_NS && D <= 64 * 8 * DEC_MAXC && I <= 64 * 8 * DEC_MAXC,
                    "svc_op_ar_linear: path 2 holds D <= 1024 and I <= 2560 (svc_ar_create clears the decode step above)");
    SVC_REQUIRE(e->x && e->W, "svc_op_ar_linear: x and W are required");
    const bool norm = role == 0 || role == 2 || role == 4;
    const bool cache = role == 0 && path != 2;
    if (norm && !(path == 2 && role == 0)) SVC_REQUIRE(e->gamma, "svc_op_ar_linear: the role needs gamma");
    if (role == 1 || role == 3) SVC_REQUIRE(e->res, "svc_op_ar_linear: wo and w2 need res");
    if (role == 2) SVC_REQUIRE(e->out16, "svc_op_ar_linear: w13 writes out16");
    if (role != 2 && !cache) SVC_REQUIRE(e->out32, "svc_op_ar_linear: the role writes out32");
    if (path == 2 && role == 1) SVC_REQUIRE(e->W2 && e->out2, "svc_op_ar_linear: dec_w2qkv needs W2 and out2");
    if (path == 2 && role == 2) SVC_REQUIRE(e->part && e->out2, "svc_op_ar_linear: dec_ffn13 needs part and out2");
    const int kvd = Hkv * 64, Nqkv = D + 2 * kvd;
    if (cache) {
        SVC_REQUIRE(e->q_out && e->kc && e->vc && e->rope && e->slots && e->pos, "svc_op_ar_linear: the qkv role needs q_out, kc, vc, rope, slots and pos");
        SVC_REQUIRE(e->Lmax >= 8 && e->Lmax <= 8192, "svc_op_ar_linear: Lmax is 8 .. 8192");
        SVC_REQUIRE(e->n_slots >= 1 && e->n_slots <= MAXB, "svc_op_ar_linear: n_slots is 1 .. 64");
        if (op_check_slots(e->slots, path == 1 ? rows : 1, e->n_slots, path == 1, who)) return 1;
        if (op_check_pos(e->pos, rows, e->Lmax, who)) return 1;
    }
    const half_t* W = reinterpret_cast<const half_t*>(e->W);
    half_t* out16 = reinterpret_cast<half_t*>(e->out16);
    const size_t slot_elems = (size_t)Hkv * e->Lmax * 64;
    Arena ar;
    int rc = 1;
    if (path == 0) {
        const int S = rows;
        if (role == 0) {
            int* d_pos;
            if (op_upload_ints(ar, std::vector<int>(e->pos, e->pos + 2 * S), &d_pos, st)) return 1;
            GemvArgs a(e->x, D, W, D, S, Nqkv, D);
            a.gamma = e->gamma; a.eps = e->eps;
            a.q_out = e->q_out; a.kc = e->kc + (size_t)e->slots[0] * slot_elems; a.vc = e->vc + (size_t)e->slots[0] * slot_elems;
            a.rope = e->rope; a.pos = d_pos; a.H = H; a.Hkv = Hkv; a.Lmax = e->Lmax;
            rc = gemv_pair_launch<true, GV_QKV>(a, st);
        } else if (role == 1 || role == 3) {
            const int K = role == 1 ? D : I;
            GemvArgs a(e->x, K, W, K, S, D, K);
            a.res = e->res; a.ldres = D; a.out32 = e->out32; a.ldo = D;
            rc = gemv_pair_launch<false, GV_PLAIN>(a, st);
        } else if (role == 2) {
            GemvArgs a(e->x, D, W, D, S, 2 * I, D);
            a.gamma = e->gamma; a.eps = e->eps; a.out16 = out16; a.ldo = I;
            rc = gemv_pair_launch<true, GV_GLU>(a, st);
        } else {
            GemvArgs a(e->x, D, W, D, S, V, D);
            a.gamma = e->gamma; a.eps = e->eps; a.out32 = e->out32; a.ldo = V;
            rc = gemv_pair_launch<true, GV_PLAIN>(a, st);
        }
    } else if (path == 1) {
        const int B = rows, Bp = (int)round_up(B, 16);
        int* d_pos = nullptr;
        float** tab = nullptr;
        if (role == 0) {
            std::vector<int> pos(2 * MAXB + 1, 0);
            for (int b = 0; b < B; ++b) { pos[b] = e->pos[b]; pos[MAXB + b] = e->pos[B + b]; }
            pos[2 * MAXB] = B;
            if (op_upload_ints(ar, pos, &d_pos, st) || op_kvtab(ar, e->kc, e->vc, slot_elems, e->slots, B, &tab, st)) return 1;
        }
        rc = with_ar_sizes(D, I, [&](auto KD, auto KI) {
            if (role == 0) {
                BGemmArgs a(e->x, D, W, D, Nqkv, D);
                a.gamma = e->gamma; a.eps = e->eps;
                a.q_out = e->q_out; a.kc = tab; a.vc = tab + MAXB; a.rope = e->rope; a.pos = d_pos; a.nb = d_pos + 2 * MAXB;
                a.H = H; a.Hkv = Hkv; a.Lmax = e->Lmax;
                return bgemm_launch<true, BG_QKV, 1, KD>(a, Bp, st);
            }
            if (role == 1) {
                BGemmArgs a(e->x, D, W, D, D, D);
                a.res = e->res; a.out32 = e->out32; a.ldo = D;
                return bgemm_launch<false, BG_PLAIN, 1, KD>(a, Bp, st);
            }
            if (role == 2) {
                BGemmArgs a(e->x, D, W, D, 2 * I, D);
                a.gamma = e->gamma; a.eps = e->eps; a.out16 = out16; a.ldo = I;
                return bgemm_launch<true, BG_GLU, 2, KD>(a, Bp, st);
            }
            if (role == 3) {
                BGemmArgs a(e->x, I, W, I, D, I);
                a.res = e->res; a.out32 = e->out32; a.ldo = D;
                return bgemm_launch<false, BG_PLAIN, 1, KI>(a, Bp, st);
            }
            BGemmArgs a(e->x, D, W, D, V, D);
            a.gamma = e->gamma; a.eps = e->eps; a.out32 = e->out32; a.ldo = V;
            return bgemm_launch<true, BG_PLAIN, 1, KD>(a, Bp, st);
        });
    } else {
        const float* xf = reinterpret_cast<const float*>(e->x);
        const half_t* xh = reinterpret_cast<const half_t*>(e->x);
        rc = with_dec_sizes(D, I, H, [&](auto KD, auto KI, auto NP) {
            switch (role) {
                case 0: return dec_qkvraw_launch<KD>(xf, W, D, Nqkv, e->out32, st);
                case 1: return dec_w2qkv_launch<KD, KI>(xh, e->res, reinterpret_cast<const half_t*>(e->W2), W, I, D, Nqkv, e->out32, e->out2, st);
                case 2: return dec_ffn13_launch<NP, KD>(xf, e->part, H, e->out2, e->gamma, e->eps, W, D, 2 * I, out16, st);
                case 3: return dec_w2_launch<KI>(xh, W, I, D, e->res, e->out32, st);
                default: return dec_head_launch<KD>(xf, e->gamma, e->eps, W, D, V, e->out32, st);
            }
        });
    }
    if (rc) return 1;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
