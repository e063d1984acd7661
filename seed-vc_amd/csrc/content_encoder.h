// What the 16 kHz content encoders (whisper.hip, wav2vec2.hip and, through the latter, astral.hip) share: the window table and plan of long clips, the LayerNorm
// row kernel, the V transpose, the packed linears and the pre-LN transformer stack (kernels and launchers in
// content_encoder.hip).  A model file supplies its stem, its "rows of a window of ns samples" rule and its key names.
// StageTimer and copy_f32 also serve rmvpe.hip.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "model_util.h"

namespace svc {

constexpr int MAX_WIN = 64;                       // windows computed side by side, at most
constexpr int SAMPLES_PER_ROW = 320;              // 16 kHz samples per content row (50 rows/s)

struct WinTab {                                   // one group of windows as a kernel argument
    int clip[MAX_WIN], start[MAX_WIN], n[MAX_WIN];                    // source clip, first sample, samples
    int dst0[MAX_WIN], drop[MAX_WIN], keep[MAX_WIN];                  // assemble: rows [drop, keep) go to out[clip][dst0 ...]
    int zero_from[MAX_WIN];                                           // last window of its clip: the clip's row count; else -1
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// affine LayerNorm (then erf-GELU when `gelu`) of a row held by one wave (v[i] = channel lane + 64 i): mean, then the
// variance about it (two passes), fp32
template <int NMAX>
__device__ __forceinline__ void row_norm(float (&v)[NMAX], int n, int D, float eps, const float* __restrict__ gamma, const float* __restrict__ beta,
                                         int lane, bool gelu) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) s += v[i];
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) { const float d = v[i] - mean; q = fmaf(d, d, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
    for (int i = 0; i < NMAX; ++i)
        if (i < n) {
            const int c = lane + 64 * i;
            const float o = (v[i] - mean) * rstd * gamma[c] + beta[c];
            v[i] = gelu ? gelu_erf(o) : o;
        }
}

// the drivers' window plan of a clip of n samples, window W and overlap O samples: number of windows (>= 1)
inline long window_count(long W, long O, long n) { return n <= W ? 1 : 1 + (n - W + (W - O) - 1) / (W - O); }

struct Win { int clip, start, n, dst0, drop, keep, zero_from; };

// Appends the computed windows of clip `clip` (n samples) to the call's plan and returns the clip's content rows.  rows_of(ns)
// is the model's rows of a window of ns samples.  A later window whose rows do not exceed the overlap contributes nothing and
// is skipped; the clip's last computed window zeroes the output rows above the clip's count.  (Whisper's rule ns / 320 + 1
// never skips: window j >= 1 exists only with more than O samples, so its rows exceed overlap_rows.)
template <class RowsOf>
int plan_clip(std::vector<Win>& wins, int clip, long n, long W, int overlap_rows, RowsOf rows_of) {
    const long O = (long)overlap_rows * SAMPLES_PER_ROW, nw = window_count(W, O, n);
    int dst = 0;
    for (long j = 0; j < nw; ++j) {
        const long s = j * (W - O), ns = std::min(W, n - s);
        const int keep = (int)rows_of(ns), drop = j ? overlap_rows : 0;
        if (keep <= drop) continue;
        wins.push_back({clip, (int)s, (int)ns, dst, drop, keep, -1});
        dst += keep - drop;
    }
    wins.back().zero_from = dst;
    return dst;
}

// windows [w0, w0 + G) of the plan as a kernel argument
WinTab win_table(const std::vector<Win>& wins, size_t w0, int G);
// enc [G][P][D] -> out [B][Rmax][D]: the kept rows of every window to their place, zeros above a clip's count
int assemble_launch(const float* enc, const WinTab& wt, int G, float* out, int P, int D, int Rmax, int block, hipStream_t st);

// Row kernel, one wave per row of D (a multiple of 64, at most 2048).  mode 0: LayerNorm; 1: LayerNorm, erf-GELU; 2: LayerNorm,
// erf-GELU, then a second LayerNorm (gamma2, beta2).  fp32 and / or fp16 out.  Rows at and above lens[row / seq_rows] are neither
// read nor written; lens may be null.
int rownorm_launch(int mode, const float* x, long ldx, float* y32, half_t* y16, long ldy, const float* gamma, const float* beta,
                   const float* gamma2, const float* beta2, long rows, int D, float eps, const int* lens, int seq_rows, hipStream_t st);

// V columns of qkv [G * P][3 D] (fp16) -> vt [G][D][vt_ld] in the attention's column order `mode`; columns at and above the
// window's rows (lens[g], or P when lens is null) are written as zeros
int vt_launch(const half_t* qkv, half_t* vt, const int* lens, int G, int P, int D, long vt_ld, int mode, hipStream_t st);

// src [G][P][D] rows below lens[g] -> dst [G][T][D]; the other rows of dst are not touched
int copy_rows_launch(const float* src, int P, float* dst, int T, const int* lens, int G, int rows, int D, hipStream_t st);

struct Lin { void* w = nullptr; float* b = nullptr; long ldw = 0; int N = 0; };
struct Layer { Lin qkv, o, fc1, fc2; float *g1 = nullptr, *b1 = nullptr, *g2 = nullptr, *b2 = nullptr; };

// n device floats copied into the arena (nullptr on failure, error set)
float* copy_f32(const float* src, long n, Arena& ar, hipStream_t st);
// nn.Linear weight [N][K] -> [Npad128][K] in the GEMM's dtype dt, rows optionally scaled; bias may be null
int pack_lin(int dt, Arena& wts, const float* w, const float* bias, int N, int K, const float* scale, Lin* out, hipStream_t st);
// the tap-GEMM's row map of plain rows: M rows in sequences of Lout, one tap
KGemmParams kgemm_rows(long M, int N, int Lout);
// c = act(a [M][K] W^T + b) (+ res): fp32 and / or fp16 out, leading dimension N
int linear_launch(int dt, const Lin& l, const void* a, long K, long M, int Lout, int act, const float* res, float* c32, half_t* c16, hipStream_t st);

struct KeyShape { std::string name; std::vector<long> shape; };

// A model's state-dict names of the stack: layer i's modules are "<layers><i>.<module>" + ".weight" / ".bias"; k_bias is
// the whole key under the layer, or null for a key projection without bias.
struct StackNames { const char *layers, *q, *k, *k_bias, *v, *o, *ln1, *fc1, *fc2, *ln2, *ln_final; };

// Transformer encoder (pre-LN; post-LN with `post_ln`), head dimension 64: per layer LayerNorm, q | k | v in one GEMM (1 / 8 and the attention's log2(e)
// folded into the q rows), fp16 rows for the attention and a small transpose for V^T, out_proj + residual, LayerNorm, GELU MLP
// + residual; then the final LayerNorm.  Residual stream, LayerNorm statistics and softmax are fp32; the linears run on the fp16
// tap-GEMM (dt 0) or the fp32 one (dt 1).  Every sequence is computed as if alone.
struct EncoderStack {
    int dt = 0, D = 0, F = 0, H = 0;
    int qt_form = 1;                 // the attention's query-tile form, pinned per handle by the model
    std::vector<Layer> layers;
    bool final_ln = true;            // internal: false ends at the residual stream after the last layer, left in x (the ASTRAL front, astral.hip)
    // post-LN order (the wav2vec 2.0 base family): ln_final on the stem's rows BEFORE the layers, each layer x = ln1(x + attention(x)),
    // x = ln2(x + mlp(x)), nothing after the last layer.  The sums go to `y`, the LayerNorms bring them back to x (needs final_ln).
    // In precision 0 the post-LN order keeps q, k, v and the softmax weights in fp32 (attn_f32_kernel on qkv32): their fp16
    // rounding alone is above the 1e-4 bound there.  The pre-LN order is what it was.
    bool post_ln = false;
    float *y = nullptr, *qkv32 = nullptr;
    float *gf = nullptr, *bf = nullptr;
    float *x = nullptr, *n32 = nullptr, *ao32 = nullptr, *ff32 = nullptr;           // x [G * P][D]: the residual stream, filled by the stem
    half_t *n16 = nullptr, *qkv16 = nullptr, *vt = nullptr, *ao16 = nullptr, *ff16 = nullptr;

    static void keys(const StackNames& nm, int n_layers, long D, long F, std::vector<KeyShape>& out, bool final_ln = true);
    int pack(const StateDict& sd, const std::string& pre, const StackNames& nm, int n_layers, Arena& wts, hipStream_t st);     // after keys()
    int reserve(Arena& ws, int G, int P, hipStream_t st);
    // x [G][P][D] -> out [G][P][D]; with lens, sequence g has lens[g] rows and the rows above are neither read nor written.
    // Without the final LayerNorm the result stays in x and `out` is not used.
    int run(int G, int P, const int* lens, float* out, hipStream_t st);
    int run_post(int G, int P, const int* lens, float* out, hipStream_t st);        // run() with post_ln
};

// measurement aid: events around the stages of the last group of the last call
struct StageTimer {
    bool on = false;
    hipEvent_t ev[5] = {};
    ~StageTimer() {
        for (auto& e : ev) if (e) (void)hipEventDestroy(e);
    }
    int mark(int i, hipStream_t st) {
        if (!on) return 0;
        if (!ev[i]) SVC_CHECK_HIP(hipEventCreate(&ev[i]));
        SVC_CHECK_HIP(hipEventRecord(ev[i], st));
        return 0;
    }
    // the four stage times in milliseconds (synchronises); `msg` is the caller's error when nothing was recorded
    int last(float* ms4, const char* msg) {
        SVC_REQUIRE(ms4 && on && ev[0] && ev[4], msg);
        SVC_CHECK_HIP(hipEventSynchronize(ev[4]));
        for (int i = 0; i < 4; ++i) SVC_CHECK_HIP(hipEventElapsedTime(&ms4[i], ev[i], ev[i + 1]));
        return 0;
    }
};

}  // namespace svc
