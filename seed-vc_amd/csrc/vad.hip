// FSMN voice activity detector for gfx950: funasr's `fsmn-vad` restated from memory -- Kaldi fbank + LFR + CMVN
// front-end, the FSMN encoder, and a causal statement of E2EVadModel's window detector -- for one-shot ragged batches
// (svc_vad_scores), for the op-level seam of the detector (svc_vad_detect) and for live streams (svc_vad_step).
//
// Front-end: vad_frames_kernel (x 32768, DC removal, pre-emphasis, Hamming, zero-pad to 512), the DFT and the mel bank as
// fp32 tap-GEMMs (kgemm_launch, as svc_kaldi_fbank runs them), vad_lfr_kernel (log, the 5-frame stack, CMVN -> [rows][400]).
// Frames and rows of all clips of a call are stored compactly, clip after clip; a clip's descriptor travels as a kernel
// argument (VadClips), which is how the host arrays of a call are consumed before it returns.
//
// Network: vad_net_kernel, grid (runs, streams).  A workgroup of 8 waves walks the rows of its run in time order in tiles of
// 16 rows; all activations stay in LDS (131 KB, one workgroup per CU).  16 rows, not 32: a tile is the N side of one
// v_mfma_f32_16x16x4_f32, and the four layers' row histories (4 x 35 x 132 floats) beside a 32-row [32][404] input tile and its
// hidden tiles would not fit the 160 KB of a CU.  The linears compute out^T = W in^T: the weight rows are the MFMA's A operand
// (pre-packed at create time as 1 KB fragments, lane (c, g) of fragment (n-tile, q) holding W[16 nt + c][16 q + 4 g + j],
// j = 0 .. 3, streamed from L2 with one 16-byte load per lane), the activation rows its B operand (one ds_read_b128 of
// in[c][16 q + 4 g ..]).  MFMA j of a 16-wide k group contracts k = j, 4 + j, 8 + j, 12 + j: kgemm_tile.h's order; the groups
// ascend.  Every accumulator starts at 0 and the bias is added last.  A lane ends with out[row c][16 nt + 4 g .. + 3]: one
// 16-byte LDS store.  Column t of an MFMA depends on column t of B alone, so a row's bits do not depend on what the other 15
// rows of its tile hold, nor on which tile column it sits in.
// Memory: y[t][c] = fl(chain + p[t][c]), chain = fmaf(w[c][k], p[t - 19 + k][c], chain) for k = 0 .. 19 from 0 ("+ p[t]" last).
// Softmax: max over the 248 logits (exact in any order), e = expf(x - max), lane l of a wave adds columns l, l + 64, l + 128,
// l + 192 in that order and the 64 partial sums are added in an xor butterfly (32, 16, .., 1), p_sil = e_0 / sum.
//
// The run split is exact.  Layer l's p rows are a row-local function of layer l - 1's output y (of the input rows for l = 1),
// and y_l[t] reads p_l[t - 19 .. t].  A run that starts at row w0 with zero histories therefore has p_1 right from w0 on
// and y_1 right from w0 + 19 on (from there on every p_1 row it reads was computed, none assumed zero); by induction y_l
// is right from w0 + 19 l on, the output from w0 + 76 on.  "Right" means the same bits, since every row runs the same
// instruction sequence on the same operands.  A run whose first row r is above 0 starts at w0 = max(0, r - 76) and drops the
// rows below r; with w0 = 0 the zero histories are the stream's true start.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "kaldi_tables.h"
#include "model_util.h"

using namespace svc;

namespace {

constexpr int VAD_MAXN = 64;
constexpr int VAD_WIN = 400, VAD_SHIFT = 160, VAD_BINS = 80, VAD_IN = 400, VAD_AFF = 140, VAD_LIN = 250, VAD_PROJ = 128,
              VAD_LORDER = 20, VAD_LAYERS = 4, VAD_OUT = 248, VAD_HIST = VAD_LORDER - 1, VAD_WARM = VAD_LAYERS * VAD_HIST;
constexpr int VAD_CACHE_FLOATS = VAD_LAYERS * VAD_HIST * VAD_PROJ;
static_assert(VAD_CACHE_FLOATS + 32 == SVC_VAD_STATE_FLOATS, "state layout");
constexpr int VAD_TM = 16, VAD_THREADS = 512, VAD_WAVES = VAD_THREADS / 64;
// LDS row strides (floats): multiples of 4 (16-byte rows), not of 32
constexpr int LD_A = 404, LD_B = 260, LD_C = 148, LD_P = 132;
constexpr int OFF_A = 0, OFF_B = OFF_A + VAD_TM * LD_A, OFF_C = OFF_B + VAD_TM * LD_B, OFF_H = OFF_C + VAD_TM * LD_C,
              OFF_Y = OFF_H + VAD_LAYERS * (VAD_HIST + VAD_TM) * LD_P, VAD_LDS_FLOATS = OFF_Y + VAD_TM * LD_P;
constexpr int ld_spec = 520, ld_pow = 288, ld_e = 96;       // round_up(2 * 257, 8), round_up(257, 32), round_up(80, 32)

// per-clip (per-stream) descriptors of one call, by value
struct VadClips {
    long wave_off[VAD_MAXN];      // element offset of the sample of frame f0 from the call's wave pointer
    int f0[VAD_MAXN], nF[VAD_MAXN], foff[VAD_MAXN];      // first frame computed (stream numbering), their count, first row in the frame scratch
    int r0[VAD_MAXN], nR[VAD_MAXN], roff[VAD_MAXN];      // first LFR row computed, their count, first row in the row scratch
    int fhi[VAD_MAXN];            // highest frame index a row may read (a final call clamps there)
    int slot[VAD_MAXN];
};
struct VadSlots { int slot[VAD_MAXN]; int n[VAD_MAXN]; };

__global__ __launch_bounds__(256) void vad_frames_kernel(const float* __restrict__ wave, float* __restrict__ frames, const VadClips cl,
                                                         const float* __restrict__ window) {
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (f >= cl.nF[b]) return;                                  // block-uniform
    const float* w = wave + cl.wave_off[b] + (long)f * VAD_SHIFT;
    float* out = frames + ((long)cl.foff[b] + f) * KALDI_NFFT;
    __shared__ float red[256];
    float s = 0.f;
    for (int i = tid; i < VAD_WIN; i += 256) s += w[i] * 32768.f;
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float mean = red[0] / (float)VAD_WIN;
    for (int i = tid; i < KALDI_NFFT; i += 256) {
        float v = 0.f;
        if (i < VAD_WIN) {
            const float cur = w[i] * 32768.f - mean, prev = w[i > 0 ? i - 1 : 0] * 32768.f - mean;
            v = (cur - 0.97f * prev) * window[i];
        }
        out[i] = v;
    }
}

// spec [n][ld_spec] = (re | im) -> power [n][ld_pow], pad columns zero
__global__ void vad_power_kernel(const float* __restrict__ spec, float* __restrict__ pw) {
    const long m = blockIdx.x;
    const int k = blockIdx.y * blockDim.x + threadIdx.x;
    if (k >= ld_pow) return;
    float v = 0.f;
    if (k < KALDI_NB) {
        const float re = spec[m * ld_spec + k], im = spec[m * ld_spec + KALDI_NB + k];
        v = re * re + im * im;
    }
    pw[m * ld_pow + k] = v;
}

// X[row i of clip b][80 j + m] = (log(max(E[frame clamp(i + j - 2)][m], eps)) + shift) * scale
__global__ __launch_bounds__(128) void vad_lfr_kernel(const float* __restrict__ e, float* __restrict__ X, const VadClips cl,
                                                      const float* __restrict__ shift, const float* __restrict__ scale) {
    const int il = blockIdx.x, b = blockIdx.y;
    if (il >= cl.nR[b]) return;
    const int i = cl.r0[b] + il;
    float* x = X + ((long)cl.roff[b] + il) * VAD_IN;
    for (int c = threadIdx.x; c < VAD_IN; c += 128) {
        const int j = c / VAD_BINS, m = c - j * VAD_BINS;
        const int f = min(max(i + j - 2, 0), cl.fhi[b]) - cl.f0[b];
        const float v = logf(fmaxf(e[((long)cl.foff[b] + f) * ld_e + m], 1.1920928955078125e-07f));
        x[c] = (v + shift[c]) * scale[c];
    }
}

// out[t][16 nt + 4 g + r] = act(sum_k in[t][k] W[16 nt + c'][k] + bias), for the 16 rows of the tile; n-tiles dealt to the waves
template <int NT, int KG, bool BIAS, bool RELU>
__device__ __forceinline__ void vad_linear(const float4v* __restrict__ wf, const float* __restrict__ bias, const float* in, int ldi,
                                           float* out, int ldo, int wave, int lane) {
    const int c = lane & 15, g = lane >> 4;
    for (int nt = wave; nt < NT; nt += VAD_WAVES) {
        float4v acc = {0.f, 0.f, 0.f, 0.f};
        const float4v* w = wf + (long)nt * KG * 64 + lane;
        const float* x = in + c * ldi + 4 * g;
#pragma unroll 8
        for (int q = 0; q < KG; ++q) {
            const float4v a = w[q * 64];
            const float4v bb = *reinterpret_cast<const float4v*>(x + 16 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bb[j], acc, 0, 0, 0);
        }
        if constexpr (BIAS) {
            const float4v bv = *reinterpret_cast<const float4v*>(bias + 16 * nt + 4 * g);
            acc += bv;
        }
        if constexpr (RELU) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = fmaxf(acc[r], 0.f);
        }
        *reinterpret_cast<float4v*>(out + c * ldo + 16 * nt + 4 * g) = acc;
    }
}

struct VadNet {                 // packed weights (device)
    const float4v *in1, *in2, *lin[VAD_LAYERS], *aff[VAD_LAYERS], *out1, *out2;
    const float *b_in1, *b_in2, *b_aff[VAD_LAYERS], *b_out1, *b_out2;
    const float* fir;           // [layer][k][128]
};
constexpr int NT_AFF = 9, KG_AFF = 9, NT_LIN = 16, KG_LIN = 16, NT_PROJ = 8, KG_PROJ = 8, KG_IN = 25, NT_OUT = 16;

// rel: p row index = row - r0 (streaming) instead of row; state: per-slot caches, read at the start and written at the end (then
// one run per stream), or null: zero histories and the warm-up described at the top
__global__ __launch_bounds__(VAD_THREADS) void vad_net_kernel(const float* __restrict__ X, const VadClips cl, const VadNet net, int seg_rows,
                                                              float* __restrict__ p_out, long ld_out, int rel, float* __restrict__ state) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r_lo = cl.r0[b], r_hi = r_lo + cl.nR[b];
    const long start_l = (long)r_lo + (long)blockIdx.x * seg_rows;
    if (start_l >= r_hi) return;                                  // block-uniform
    const int start = (int)start_l, stop = start_l + seg_rows < r_hi ? (int)(start_l + seg_rows) : r_hi;
    const int w0 = (state || start == 0) ? start : max(r_lo, max(0, start - VAD_WARM));
    float* bufA = lds + OFF_A; float* bufB = lds + OFF_B; float* bufC = lds + OFF_C; float* hist = lds + OFF_H; float* ybuf = lds + OFF_Y;
    float* st = state ? state + (long)cl.slot[b] * SVC_VAD_STATE_FLOATS : nullptr;
    for (int i = tid; i < VAD_LAYERS * VAD_HIST * VAD_PROJ; i += VAD_THREADS) {
        const int l = i / (VAD_HIST * VAD_PROJ), rc = i - l * (VAD_HIST * VAD_PROJ), r = rc >> 7, c = rc & 127;
        hist[(l * (VAD_HIST + VAD_TM) + r) * LD_P + c] = st ? st[i] : 0.f;
    }
    const float* xrows = X + ((long)cl.roff[b] - r_lo) * VAD_IN;  // row i of the stream at xrows + i * 400
    for (int t0 = w0; t0 < stop; t0 += VAD_TM) {
        const int nv = min(VAD_TM, stop - t0);
        __syncthreads();
        for (int i = tid; i < VAD_TM * (VAD_IN / 4); i += VAD_THREADS) {
            const int r = i / (VAD_IN / 4), c4 = i - r * (VAD_IN / 4);
            float4v v = {0.f, 0.f, 0.f, 0.f};
            if (r < nv) v = *reinterpret_cast<const float4v*>(xrows + (long)(t0 + r) * VAD_IN + 4 * c4);
            *reinterpret_cast<float4v*>(bufA + r * LD_A + 4 * c4) = v;
        }
        __syncthreads();
        vad_linear<NT_AFF, KG_IN, true, false>(net.in1, net.b_in1, bufA, LD_A, bufC, LD_C, wave, lane);
        __syncthreads();
        vad_linear<NT_LIN, KG_AFF, true, true>(net.in2, net.b_in2, bufC, LD_C, bufB, LD_B, wave, lane);
        __syncthreads();
        for (int l = 0; l < VAD_LAYERS; ++l) {
            float* h = hist + l * (VAD_HIST + VAD_TM) * LD_P;
            vad_linear<NT_PROJ, KG_LIN, false, false>(net.lin[l], nullptr, bufB, LD_B, h + VAD_HIST * LD_P, LD_P, wave, lane);
            __syncthreads();
            {
                const int c = tid & 127;
                const float* fw = net.fir + (long)l * VAD_LORDER * VAD_PROJ + c;
                float wk[VAD_LORDER];
#pragma unroll
                for (int k = 0; k < VAD_LORDER; ++k) wk[k] = fw[k * VAD_PROJ];
                for (int t = tid >> 7; t < VAD_TM; t += VAD_THREADS / 128) {
                    float acc = 0.f;
#pragma unroll
                    for (int k = 0; k < VAD_LORDER; ++k) acc = fmaf(wk[k], h[(t + k) * LD_P + c], acc);
                    ybuf[t * LD_P + c] = acc + h[(t + VAD_HIST) * LD_P + c];
                }
            }
            __syncthreads();
            // the last 19 rows up to the tile's last real row become the history (rows nv .. nv + 18 -> 0 .. 18)
            float keep[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int i = tid + u * VAD_THREADS;
                if (i < VAD_HIST * VAD_PROJ) keep[u] = h[((i >> 7) + nv) * LD_P + (i & 127)];
            }
            vad_linear<NT_LIN, KG_PROJ, true, true>(net.aff[l], net.b_aff[l], ybuf, LD_P, bufB, LD_B, wave, lane);
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int i = tid + u * VAD_THREADS;
                if (i < VAD_HIST * VAD_PROJ) h[(i >> 7) * LD_P + (i & 127)] = keep[u];
            }
        }
        __syncthreads();
        vad_linear<NT_AFF, KG_LIN, true, false>(net.out1, net.b_out1, bufB, LD_B, bufC, LD_C, wave, lane);
        __syncthreads();
        vad_linear<NT_OUT, KG_AFF, true, false>(net.out2, net.b_out2, bufC, LD_C, bufA, LD_A, wave, lane);
        __syncthreads();
        for (int r = wave; r < nv; r += VAD_WAVES) {
            const int row = t0 + r;
            if (row < start) continue;                            // warm-up rows: wave-uniform
            const float* x = bufA + r * LD_A;
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = (lane + 64 * u) < VAD_OUT ? x[lane + 64 * u] : -INFINITY;
            float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
            float e0 = 0.f, s = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float e = (lane + 64 * u) < VAD_OUT ? expf(v[u] - mx) : 0.f;
                if (u == 0) e0 = e;
                s += e;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
            if (lane == 0) p_out[(long)b * ld_out + (rel ? row - r_lo : row)] = e0 / s;
        }
    }
    if (st) {
        __syncthreads();
        for (int i = tid; i < VAD_LAYERS * VAD_HIST * VAD_PROJ; i += VAD_THREADS) {
            const int l = i / (VAD_HIST * VAD_PROJ), rc = i - l * (VAD_HIST * VAD_PROJ), r = rc >> 7, c = rc & 127;
            st[i] = hist[(l * (VAD_HIST + VAD_TM) + r) * LD_P + c];
        }
    }
}

// ---- detector: integers only.  The state words of a slot (int32 view of state[slot] + VAD_CACHE_FLOATS)
enum { DS_T = 0, DS_BITS = 1, DS_POS = 2, DS_SUM = 3, DS_WIN = 4, DS_INSEG = 5, DS_BEG = 6, DS_SILRUN = 7, DS_PREVEND = 8 };

__device__ void vad_detect_stream(const svc_vad_config_t cfg, const float* __restrict__ p, int n, int* __restrict__ ds,
                                  int* __restrict__ frame_speech, int* __restrict__ events, int* __restrict__ n_events,
                                  int* __restrict__ flag) {
    int t = ds[DS_T], pos = ds[DS_POS], s = ds[DS_SUM], win = ds[DS_WIN], inseg = ds[DS_INSEG], beg = ds[DS_BEG],
        silrun = ds[DS_SILRUN], prev_end = ds[DS_PREVEND];
    unsigned bits = (unsigned)ds[DS_BITS];
    int nev = 0, touched = 0;
    auto emit = [&](int kind, int frame) {
        if (events && nev < SVC_VAD_MAX_EVENTS) { events[2 * nev] = kind; events[2 * nev + 1] = 10 * frame; }
        ++nev;
    };
    for (int i = 0; i < n; ++i, ++t) {
        const int d = p[i] <= cfg.p_max ? 1 : 0;                  // NaN compares false: silence
        if (frame_speech) frame_speech[i] = d;
        s += d - (int)((bits >> pos) & 1u);
        bits = (bits & ~(1u << pos)) | ((unsigned)d << pos);
        pos = pos + 1 == cfg.win ? 0 : pos + 1;
        bool opened = false;
        if (win == 0) { if (s >= cfg.on_count) { win = 1; opened = true; } }
        else if (s <= cfg.off_count) win = 0;
        if (!inseg && opened) {
            inseg = 1; silrun = 0;
            beg = max(prev_end, t - cfg.lookback);
            emit(SVC_VAD_BEGIN, beg);
        }
        if (inseg) {
            touched = 1;
            silrun = win == 0 ? silrun + 1 : 0;
            if (silrun >= cfg.end_silence) {
                emit(SVC_VAD_END, t);
                inseg = 0; prev_end = t; silrun = 0;
            } else if (t - beg + 1 >= cfg.max_segment) {
                emit(SVC_VAD_END, t);
                inseg = 0; prev_end = t; silrun = 0;
                bits = 0; s = 0; win = 0;
            }
        }
    }
    ds[DS_T] = t; ds[DS_BITS] = (int)bits; ds[DS_POS] = pos; ds[DS_SUM] = s; ds[DS_WIN] = win; ds[DS_INSEG] = inseg; ds[DS_BEG] = beg;
    ds[DS_SILRUN] = silrun; ds[DS_PREVEND] = prev_end;
    if (n_events) *n_events = nev;
    if (n > 0) *flag = touched;
}

__global__ void vad_detect_kernel(const svc_vad_config_t cfg, const float* __restrict__ p, long ld, const VadSlots sl, int N,
                                  float* __restrict__ state, int* __restrict__ frame_speech, int* __restrict__ events,
                                  int* __restrict__ n_events, int* __restrict__ flags) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    const int slot = sl.slot[k];
    vad_detect_stream(cfg, p + (long)k * ld, sl.n[k], reinterpret_cast<int*>(state + (long)slot * SVC_VAD_STATE_FLOATS + VAD_CACHE_FLOATS),
                      frame_speech ? frame_speech + (long)k * ld : nullptr, events ? events + (long)k * SVC_VAD_MAX_EVENTS * 2 : nullptr,
                      n_events ? n_events + k : nullptr, flags + slot);
}

inline long vad_frames_of(long n) { return n < VAD_WIN ? 0 : (n - VAD_WIN) / VAD_SHIFT + 1; }

struct Range { const void* p; long long bytes; bool out; const char* name; };
// refuses a pair of buffers that overlap when at least one of them is written
int check_apart(const char* who, const std::vector<Range>& rs) {
    for (size_t i = 0; i < rs.size(); ++i)
        for (size_t j = i + 1; j < rs.size(); ++j) {
            if (!rs[i].p || !rs[j].p || !(rs[i].out || rs[j].out) || rs[i].bytes <= 0 || rs[j].bytes <= 0) continue;
            const uintptr_t a0 = (uintptr_t)rs[i].p, a1 = a0 + (uintptr_t)rs[i].bytes, b0 = (uintptr_t)rs[j].p, b1 = b0 + (uintptr_t)rs[j].bytes;
            if (!(a1 <= b0 || b1 <= a0)) {
                set_error(std::string(who) + ": " + rs[i].name + " overlaps " + rs[j].name);
                return 1;
            }
        }
    return 0;
}

int check_slots(const char* who, const int32_t* slots, int N, int max_slots) {
    std::vector<int32_t> sorted(slots, slots + N);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= max_slots) { set_error(std::string(who) + ": a slot outside 0 .. max_slots - 1"); return 1; }
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { set_error(std::string(who) + ": a slot appears twice in one call"); return 1; }
    return 0;
}

}  // namespace

struct svc_vad {
    svc_vad_config_t cfg;
    Arena wts, ws;
    VadNet net;
    float *window = nullptr, *dft = nullptr, *mel = nullptr, *shift = nullptr, *scale = nullptr;
    float* p_step = nullptr;              // [64][100]: the probabilities of a step whose caller does not ask for them
    long cap_frames = 0, cap_rows = 0;
    float *fr_frames = nullptr, *fr_spec = nullptr, *fr_pow = nullptr, *fr_e = nullptr, *rows_x = nullptr;

    int pack(const StateDict& sd, const float* shift400, const float* scale400, hipStream_t st);
    int reserve(long frames, long rows, hipStream_t st);
    int run(const float* wave, const VadClips& cl, int n, long tot_f, long tot_r, int max_f, int max_r, int seg_rows, float* p_out,
            long ld_out, int rel, float* state, hipStream_t st);
};

namespace {
// nn.Linear weight [N][K] (device) -> MFMA fragments [ceil(N / 16)][ceil(K / 16)][64 lanes][4], bias -> [16 ceil(N / 16)]
int pack_linear(const StateDict& sd, const std::string& pre, const std::string& name, int N, int K, bool bias, Arena& ar, hipStream_t st,
                const float4v** wf, const float** bf) {
    const auto* w = sd.get(pre + name + ".weight");
    if (require_shape(w, pre + name + ".weight", {N, K}, "svc_vad_create")) return 1;
    std::vector<float> h((size_t)N * K);
    SVC_CHECK_HIP(hipMemcpy(h.data(), w->data, h.size() * 4, hipMemcpyDeviceToHost));
    const int nt = cdiv(N, 16), kg = cdiv(K, 16);
    std::vector<float> f((size_t)nt * kg * 256, 0.f);
    for (int t = 0; t < nt; ++t)
        for (int q = 0; q < kg; ++q)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int n = 16 * t + (lane & 15), k = 16 * q + 4 * (lane >> 4) + j;
                    if (n < N && k < K) f[(((size_t)t * kg + q) * 64 + lane) * 4 + j] = h[(size_t)n * K + k];
                }
    float* d = ar.alloc_n<float>(f.size(), st);
    if (!d) return 1;
    SVC_CHECK_HIP(hipMemcpyAsync(d, f.data(), f.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));                 // f goes away
    *wf = reinterpret_cast<const float4v*>(d);
    if (bias) {
        const auto* b = sd.get(pre + name + ".bias");
        if (require_shape(b, pre + name + ".bias", {N}, "svc_vad_create")) return 1;
        float* db = ar.alloc_n<float>((size_t)nt * 16, st);  // zero-initialised: the pad columns get + 0
        if (!db) return 1;
        SVC_CHECK_HIP(hipMemcpyAsync(db, b->data, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
        *bf = db;
    }
    return 0;
}
}  // namespace

int svc_vad::pack(const StateDict& sd, const float* shift400, const float* scale400, hipStream_t st) {
    const std::string pre = sd.has("encoder.in_linear1.linear.weight") ? "encoder." : "";
    static_assert(NT_AFF * 16 >= VAD_AFF && KG_AFF * 16 >= VAD_AFF && NT_LIN * 16 >= VAD_LIN && KG_IN * 16 == VAD_IN && NT_OUT * 16 >= VAD_OUT &&
                  NT_PROJ * 16 == VAD_PROJ, "tile counts");
    if (pack_linear(sd, pre, "in_linear1.linear", VAD_AFF, VAD_IN, true, wts, st, &net.in1, &net.b_in1)) return 1;
    if (pack_linear(sd, pre, "in_linear2.linear", VAD_LIN, VAD_AFF, true, wts, st, &net.in2, &net.b_in2)) return 1;
    std::vector<float> fir((size_t)VAD_LAYERS * VAD_LORDER * VAD_PROJ);
    for (int l = 0; l < VAD_LAYERS; ++l) {
        const std::string p = "fsmn." + std::to_string(l);
        const float* none = nullptr;
        if (pack_linear(sd, pre, p + ".linear.linear", VAD_PROJ, VAD_LIN, false, wts, st, &net.lin[l], &none)) return 1;
        if (pack_linear(sd, pre, p + ".affine.linear", VAD_LIN, VAD_PROJ, true, wts, st, &net.aff[l], &net.b_aff[l])) return 1;
        const std::string cn = pre + p + ".fsmn_block.conv_left.weight";
        const auto* c = sd.get(cn);
        if (require_shape(c, cn, {VAD_PROJ, 1, VAD_LORDER, 1}, "svc_vad_create")) return 1;
        std::vector<float> h((size_t)VAD_PROJ * VAD_LORDER);
        SVC_CHECK_HIP(hipMemcpy(h.data(), c->data, h.size() * 4, hipMemcpyDeviceToHost));
        for (int ch = 0; ch < VAD_PROJ; ++ch)
            for (int k = 0; k < VAD_LORDER; ++k) fir[((size_t)l * VAD_LORDER + k) * VAD_PROJ + ch] = h[(size_t)ch * VAD_LORDER + k];
    }
    if (pack_linear(sd, pre, "out_linear1.linear", VAD_AFF, VAD_LIN, true, wts, st, &net.out1, &net.b_out1)) return 1;
    if (pack_linear(sd, pre, "out_linear2.linear", VAD_OUT, VAD_AFF, true, wts, st, &net.out2, &net.b_out2)) return 1;
    std::vector<float> wv(VAD_WIN);
    for (int i = 0; i < VAD_WIN; ++i) wv[i] = 0.54f - 0.46f * cosf(2.0f * (float)M_PI * (float)i / (float)(VAD_WIN - 1));
    const std::vector<float> basis = kaldi_dft_basis(), melb = kaldi_mel_bank(VAD_BINS);
    float* d_fir = wts.alloc_n<float>(fir.size(), st);
    window = wts.alloc_n<float>(VAD_WIN, st);
    dft = wts.alloc_n<float>(basis.size(), st);
    mel = wts.alloc_n<float>(melb.size(), st);
    shift = wts.alloc_n<float>(VAD_IN, st);
    scale = wts.alloc_n<float>(VAD_IN, st);
    p_step = wts.alloc_n<float>((size_t)VAD_MAXN * 100, st);
    if (!d_fir || !window || !dft || !mel || !shift || !scale || !p_step) return 1;
    net.fir = d_fir;
    SVC_CHECK_HIP(hipMemcpyAsync(d_fir, fir.data(), fir.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(window, wv.data(), wv.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(dft, basis.data(), basis.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(mel, melb.data(), melb.size() * 4, hipMemcpyHostToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(shift, shift400, VAD_IN * 4, hipMemcpyDeviceToDevice, st));
    SVC_CHECK_HIP(hipMemcpyAsync(scale, scale400, VAD_IN * 4, hipMemcpyDeviceToDevice, st));
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    SVC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(vad_net_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      VAD_LDS_FLOATS * (int)sizeof(float)));
    return 0;
}

int svc_vad::reserve(long frames, long rows, hipStream_t st) {
    if (frames <= cap_frames && rows <= cap_rows) return 0;
    SVC_CHECK_HIP(hipStreamSynchronize(st));
    ws.release();                                           // the stream is idle: nothing reads the old buffers any more
    cap_frames = std::max(frames, cap_frames); cap_rows = std::max(rows, cap_rows);
    fr_frames = ws.alloc_n<float>((size_t)cap_frames * KALDI_NFFT, st);
    fr_spec = ws.alloc_n<float>((size_t)cap_frames * ld_spec, st);
    fr_pow = ws.alloc_n<float>((size_t)cap_frames * ld_pow, st);
    fr_e = ws.alloc_n<float>((size_t)cap_frames * ld_e, st);
    rows_x = ws.alloc_n<float>((size_t)cap_rows * VAD_IN, st);
    if (!fr_frames || !fr_spec || !fr_pow || !fr_e || !rows_x) { cap_frames = cap_rows = 0; return 1; }
    return 0;
}

int svc_vad::run(const float* wave, const VadClips& cl, int n, long tot_f, long tot_r, int max_f, int max_r, int seg_rows, float* p_out,
                 long ld_out, int rel, float* state, hipStream_t st) {
    if (tot_r == 0) return 0;
    if (reserve(tot_f, tot_r, st)) return 1;
    hipLaunchKernelGGL(vad_frames_kernel, dim3(max_f, n), dim3(256), 0, st, wave, fr_frames, cl, window);
    SVC_CHECK_HIP(hipGetLastError());
    auto gemm = [&](const float* a, long lda, int K, const float* w, int N, float* c, long ldc) {
        KGemmParams p;
        memset(&p, 0, sizeof(p));
        p.M = (int)tot_f; p.N = N; p.Lout = (int)tot_f; p.a_seq_rows = (int)tot_f; p.c_seq_rows = (int)tot_f; p.a_stride = 1; p.a_len = (int)tot_f;
        p.n_taps = 1; p.a_ptr[0] = a; p.a_ld[0] = lda; p.a_ktiles[0] = K / 32;
        p.w = w; p.ldw = K; p.c32 = c; p.ldc32 = ldc; p.vec_ok = 1;
        return kgemm_launch(p, 1, KG_EPI_STORE, st);
    };
    if (gemm(fr_frames, KALDI_NFFT, KALDI_NFFT, dft, 2 * KALDI_NB, fr_spec, ld_spec)) return 1;
    hipLaunchKernelGGL(vad_power_kernel, dim3(tot_f, cdiv(ld_pow, 128)), dim3(128), 0, st, fr_spec, fr_pow);
    SVC_CHECK_HIP(hipGetLastError());
    if (gemm(fr_pow, ld_pow, ld_pow, mel, VAD_BINS, fr_e, ld_e)) return 1;
    hipLaunchKernelGGL(vad_lfr_kernel, dim3(max_r, n), dim3(128), 0, st, fr_e, rows_x, cl, shift, scale);
    SVC_CHECK_HIP(hipGetLastError());
    const int runs = state ? 1 : cdiv(max_r, seg_rows);
    hipLaunchKernelGGL(vad_net_kernel, dim3(runs, n), dim3(VAD_THREADS), VAD_LDS_FLOATS * sizeof(float), st, rows_x, cl, net,
                       state ? max_r : seg_rows, p_out, ld_out, rel, state);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" {

long svc_vad_rows(long n_samples, int final_) {
    const long f = vad_frames_of(n_samples);
    return final_ ? f : std::max(0L, f - 2);
}

long svc_vad_history(long total) { return total - (long)VAD_SHIFT * std::max(0L, svc_vad_rows(total, 0) - 2); }

long long svc_vad_state_floats(int max_slots) { return max_slots > 0 ? (long long)max_slots * SVC_VAD_STATE_FLOATS : 0; }

int svc_vad_create(const svc_vad_config_t* cfg, const svc_tensor_desc_t* weights, int n_weights, const float* shift400,
                   const float* scale400, void* stream, svc_vad_t** out) {
    SVC_REQUIRE(cfg && weights && n_weights > 0 && shift400 && scale400 && out, "svc_vad_create: null argument");
    SVC_REQUIRE(cfg->win >= 1 && cfg->win <= 32, "svc_vad_create: win outside 1 .. 32 (the ring is one 32-bit word)");
    SVC_REQUIRE(cfg->on_count >= 1 && cfg->on_count <= cfg->win && cfg->off_count >= 0 && cfg->off_count <= cfg->win,
                "svc_vad_create: on_count outside 1 .. win or off_count outside 0 .. win");
    SVC_REQUIRE(cfg->lookback >= 0 && cfg->end_silence >= 1 && cfg->max_segment >= 1, "svc_vad_create: lookback, end_silence or max_segment");
    SVC_REQUIRE(cfg->seg_rows == 0 || cfg->seg_rows >= VAD_TM, "svc_vad_create: seg_rows is neither 0 nor at least 16");
    svc_vad* m = new svc_vad();
    m->cfg = *cfg;
    if (m->cfg.seg_rows == 0) m->cfg.seg_rows = 512;
    memset(&m->net, 0, sizeof(m->net));
    StateDict sd(weights, n_weights);
    if (m->pack(sd, shift400, scale400, (hipStream_t)stream)) { delete m; return 1; }
    *out = m;
    return 0;
}

void svc_vad_destroy(svc_vad_t* vad) { delete vad; }

int svc_vad_scores(svc_vad_t* vad, const float* wave, const int32_t* lens, int B, long L, int final_, int seg_rows, float* p_sil,
                   void* stream) {
    SVC_REQUIRE(B >= 1 && B <= VAD_MAXN, "svc_vad_scores: B outside 1 .. 64");
    SVC_REQUIRE(L >= 1 && L < (1L << 31), "svc_vad_scores: L outside 1 .. 2^31 - 1");
    SVC_REQUIRE(final_ == 0 || final_ == 1, "svc_vad_scores: final is neither 0 nor 1");
    SVC_REQUIRE(seg_rows == 0 || seg_rows >= VAD_TM, "svc_vad_scores: seg_rows is neither 0 nor at least 16");
    SVC_REQUIRE(lens != nullptr, "svc_vad_scores: lens is NULL");
    const long ld = svc_vad_rows(L, final_);
    SVC_REQUIRE(wave && (p_sil || ld == 0), "svc_vad_scores: wave or p_sil is NULL");      // L gives no row: nothing to write
    SVC_REQUIRE((((uintptr_t)wave | (uintptr_t)p_sil) & 3) == 0, "svc_vad_scores: wave or p_sil is not aligned to 4 bytes");
    VadClips cl;
    memset(&cl, 0, sizeof(cl));
    long tot_f = 0, tot_r = 0;
    int max_f = 0, max_r = 0;
    for (int b = 0; b < B; ++b) {
        SVC_REQUIRE(lens[b] >= 0 && lens[b] <= L, "svc_vad_scores: lens outside 0 .. L");
        const long f = vad_frames_of(lens[b]), r = svc_vad_rows(lens[b], final_);
        cl.wave_off[b] = (long)b * L;
        cl.nF[b] = r ? (int)f : 0; cl.foff[b] = (int)tot_f; cl.nR[b] = (int)r; cl.roff[b] = (int)tot_r; cl.fhi[b] = (int)std::max(0L, f - 1);
        tot_f += cl.nF[b]; tot_r += r;
        max_f = std::max(max_f, cl.nF[b]); max_r = std::max(max_r, (int)r);
    }
    SVC_REQUIRE(tot_f < (1L << 24), "svc_vad_scores: the frames of all clips must stay below 2^24 (split the batch)");
    if (check_apart("svc_vad_scores", {{wave, (long long)B * L * 4, false, "wave"}, {p_sil, (long long)B * ld * 4, true, "p_sil"}})) return 1;
    SVC_REQUIRE(vad != nullptr, "svc_vad_scores: vad is NULL");
    return vad->run(wave, cl, B, tot_f, tot_r, max_f, max_r, seg_rows ? seg_rows : vad->cfg.seg_rows, p_sil, ld, 0, nullptr, (hipStream_t)stream);
}

int svc_vad_detect(svc_vad_t* vad, const float* p_sil, long ld, const int32_t* n_rows, int N, const int32_t* slots, int max_slots,
                   float* state, int32_t* frame_speech, int32_t* events, int32_t* n_events, int32_t* flags, void* stream) {
    SVC_REQUIRE(N >= 1 && N <= VAD_MAXN, "svc_vad_detect: N outside 1 .. 64");
    SVC_REQUIRE(max_slots >= 1, "svc_vad_detect: max_slots below 1");
    SVC_REQUIRE(ld >= 1, "svc_vad_detect: ld below 1");
    SVC_REQUIRE(n_rows && slots, "svc_vad_detect: n_rows or slots is NULL");
    SVC_REQUIRE(p_sil && state && events && n_events && flags, "svc_vad_detect: p_sil, state, events, n_events or flags is NULL");
    SVC_REQUIRE((((uintptr_t)p_sil | (uintptr_t)state | (uintptr_t)frame_speech | (uintptr_t)events | (uintptr_t)n_events | (uintptr_t)flags) & 3) == 0,
                "svc_vad_detect: a buffer is not aligned to 4 bytes");
    VadSlots sl;
    memset(&sl, 0, sizeof(sl));
    for (int k = 0; k < N; ++k) {
        SVC_REQUIRE(n_rows[k] >= 0 && n_rows[k] <= ld && n_rows[k] <= SVC_VAD_MAX_ROWS, "svc_vad_detect: n_rows outside 0 .. min(ld, 6000)");
        sl.slot[k] = slots[k]; sl.n[k] = n_rows[k];
    }
    if (check_slots("svc_vad_detect", slots, N, max_slots)) return 1;
    if (check_apart("svc_vad_detect", {{p_sil, (long long)N * ld * 4, false, "p_sil"},
                                       {state, svc_vad_state_floats(max_slots) * 4, true, "state"},
                                       {frame_speech, (long long)N * ld * 4, true, "frame_speech"},
                                       {events, (long long)N * SVC_VAD_MAX_EVENTS * 8, true, "events"},
                                       {n_events, (long long)N * 4, true, "n_events"},
                                       {flags, (long long)max_slots * 4, true, "flags"}})) return 1;
    SVC_REQUIRE(vad != nullptr, "svc_vad_detect: vad is NULL");
    hipLaunchKernelGGL(vad_detect_kernel, dim3(1), dim3(VAD_MAXN), 0, (hipStream_t)stream, vad->cfg, p_sil, ld, sl, N, state, frame_speech,
                       events, n_events, flags);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

int svc_vad_step(svc_vad_t* vad, const float* x, long long stride, long end, int n_new, const int64_t* total, int N, const int32_t* slots,
                 int max_slots, float* state, int32_t* flags, float* p_sil, int max_rows, int32_t* events, int32_t* n_events, void* stream) {
    SVC_REQUIRE(N >= 1 && N <= VAD_MAXN, "svc_vad_step: N outside 1 .. 64");
    SVC_REQUIRE(max_slots >= 1, "svc_vad_step: max_slots below 1");
    SVC_REQUIRE(n_new >= VAD_SHIFT && n_new % VAD_SHIFT == 0 && n_new <= 16000, "svc_vad_step: n_new is not a positive multiple of 160 up to 16000");
    SVC_REQUIRE(end >= n_new && end <= stride, "svc_vad_step: end outside n_new .. stride");
    SVC_REQUIRE(total && slots, "svc_vad_step: total or slots is NULL");
    SVC_REQUIRE(x && state && flags, "svc_vad_step: x, state or flags is NULL");
    SVC_REQUIRE(!p_sil || max_rows >= n_new / VAD_SHIFT, "svc_vad_step: max_rows below n_new / 160");
    SVC_REQUIRE((events == nullptr) == (n_events == nullptr), "svc_vad_step: events and n_events go together");
    SVC_REQUIRE((((uintptr_t)x | (uintptr_t)state | (uintptr_t)flags | (uintptr_t)p_sil | (uintptr_t)events | (uintptr_t)n_events) & 3) == 0,
                "svc_vad_step: a buffer is not aligned to 4 bytes");
    VadClips cl;
    VadSlots sl;
    memset(&cl, 0, sizeof(cl));
    memset(&sl, 0, sizeof(sl));
    long tot_f = 0, tot_r = 0;
    int max_f = 0, max_r = 0;
    for (int k = 0; k < N; ++k) {
        const long tot = (long)total[k];
        SVC_REQUIRE(tot >= 0 && tot % VAD_SHIFT == 0 && tot < (1L << 40), "svc_vad_step: total is not a multiple of 160 in 0 .. 2^40");
        SVC_REQUIRE(end - n_new >= svc_vad_history(tot), "svc_vad_step: end - n_new is below the history a listed stream needs (min(total, 960))");
        const long r0 = svc_vad_rows(tot, 0), r1 = svc_vad_rows(tot + n_new, 0), f0 = std::max(0L, r0 - 2), f1 = vad_frames_of(tot + n_new);
        SVC_REQUIRE(r1 < (1L << 31), "svc_vad_step: the stream is past 2^31 frames");
        cl.wave_off[k] = (long)k * stride + end - (tot + n_new) + VAD_SHIFT * f0;
        cl.f0[k] = (int)f0; cl.nF[k] = r1 > r0 ? (int)(f1 - f0) : 0; cl.foff[k] = (int)tot_f;
        cl.r0[k] = (int)r0; cl.nR[k] = (int)(r1 - r0); cl.roff[k] = (int)tot_r; cl.fhi[k] = (int)std::max(0L, f1 - 1);
        cl.slot[k] = slots[k];
        sl.slot[k] = slots[k]; sl.n[k] = cl.nR[k];
        tot_f += cl.nF[k]; tot_r += cl.nR[k];
        max_f = std::max(max_f, cl.nF[k]); max_r = std::max(max_r, cl.nR[k]);
    }
    if (check_slots("svc_vad_step", slots, N, max_slots)) return 1;
    if (check_apart("svc_vad_step", {{x, ((long long)(N - 1) * stride + end) * 4, false, "x"},
                                     {state, svc_vad_state_floats(max_slots) * 4, true, "state"},
                                     {flags, (long long)max_slots * 4, true, "flags"},
                                     {p_sil, (long long)N * max_rows * 4, true, "p_sil"},
                                     {events, (long long)N * SVC_VAD_MAX_EVENTS * 8, true, "events"},
                                     {n_events, (long long)N * 4, true, "n_events"}})) return 1;
    SVC_REQUIRE(vad != nullptr, "svc_vad_step: vad is NULL");
    float* p = p_sil ? p_sil : vad->p_step;
    const long ld = p_sil ? max_rows : 100;
    if (vad->run(x, cl, N, tot_f, tot_r, max_f, max_r, 0, p, ld, 1, state, (hipStream_t)stream)) return 1;
    hipLaunchKernelGGL(vad_detect_kernel, dim3(1), dim3(VAD_MAXN), 0, (hipStream_t)stream, vad->cfg, p, ld, sl, N, state, (int*)nullptr,
                       events, n_events, flags);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
