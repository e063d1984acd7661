// Sample-rate conversion: torchaudio's `resample` with its defaults as a polyphase dot product.
//
// With o = orig / gcd, n = new / gcd the operator is out[i n + j] = sum_k K[j][k] xpad[i o + k], a strided convolution with n dense
// kernels of 2 width + o columns.  In float32 all but a short contiguous run of every K[j] is exactly 0.0 (the Hann window meets
// the clamp), so the library takes the runs only: taps[n][ntaps] and the column first[n] where each run starts, built by the
// host mirror (audio.py: `sinc_resample_taps`).  The library knows nothing about the filter.
//
// One kernel, output-stationary.  A workgroup owns 4 G whole periods of n outputs of one clip (G chosen per rate pair so that
// the G n work items fill 256-lane passes and the input span fits the LDS budget).  It stages the input span those outputs need
// in LDS (16-byte loads, zeros outside the clip's own [0, lens[b])), then every work item (phase j, period g) computes the
// four outputs of phase j in periods g, g + G, g + 2 G, g + 3 G: one tap load (taps are stored [k][n], so adjacent lanes read
// adjacent words) feeds four FMA chains, and for each of the four the lanes of a pass store consecutive words.
// Lengths travel as kernel arguments (B <= 64): nothing is copied, nothing is synchronised.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "resample_core.h"

using namespace svc;

namespace {

constexpr int RS_MAX_B = 64;
constexpr int RS_SPAN_BUDGET = 6144;        // floats of LDS a tile's input span may take when G > 1 (24 KB: six workgroups per CU)
constexpr int RS_SPAN_LIMIT = 16000;        // floats, G = 1 (64 KB of static + dynamic LDS is what a launch gets without opting in)

struct RsLens { int32_t v[RS_MAX_B]; };

// x [B][L], out [B][Lout]; taps_kn [ntaps][n]; first [n]
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, long L, RsLens lens, RsGeom q,
                                                              const float* __restrict__ taps_kn, const int* __restrict__ first,
                                                              float* __restrict__ out, long Lout) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const int b = blockIdx.y;
    const int S = q.G * q.n;                                    // work items, and the distance between an item's outputs
    const long len = lens.v[b];
    const long nout = (len * q.n + q.o - 1) / q.o;              // outputs this clip has
    const long m0 = (long)blockIdx.x * RS_ROWS * S;             // the tile's first output; a multiple of n
    float* orow = out + (long)b * Lout;
    if (m0 >= nout) {                                           // nothing but zeros to write (uniform for the workgroup)
        const long m1 = m0 + (long)RS_ROWS * S < Lout ? m0 + (long)RS_ROWS * S : Lout;
        for (long m = m0 + threadIdx.x; m < m1; m += RS_THREADS) orow[m] = 0.f;
        return;
    }
    // ---- stage x[lo - shift, lo - shift + span) of this clip, zeros outside [0, len); shift makes the loads 16-byte aligned
    const float* xrow = x + (long)b * L;
    const long lo = (long)blockIdx.x * RS_ROWS * q.G * q.o + q.fmin - q.width;
    const int shift = (int)(((uintptr_t)(xrow + lo) >> 2) & 3);
    const long p0 = lo - shift;
    for (int v = threadIdx.x * 4; v < q.span; v += RS_THREADS * 4) {
        const long p = p0 + v;
        float4 t;
        if (p >= 0 && p + 3 < len) {
            t = *reinterpret_cast<const float4*>(xrow + p);
        } else {                                                // a clip's edge: element by element, nothing outside it is read
            t.x = (p >= 0 && p < len) ? xrow[p] : 0.f;
            t.y = (p + 1 >= 0 && p + 1 < len) ? xrow[p + 1] : 0.f;
            t.z = (p + 2 >= 0 && p + 2 < len) ? xrow[p + 2] : 0.f;
            t.w = (p + 3 >= 0 && p + 3 < len) ? xrow[p + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(xs + v) = t;
    }
    __syncthreads();
    // ---- work item w = g n + j: phase j of periods g + G r (resample_core.h: the dot product shared with svc_rt_push)
    for (int w = threadIdx.x; w < S; w += RS_THREADS) {
        float a0, a1, a2, a3;
        rs_dot4(xs, shift, q, taps_kn, first, w, a0, a1, a2, a3);
        const long m = m0 + w;
        if (m < Lout) orow[m] = m < nout ? a0 : 0.f;
        if (m + S < Lout) orow[m + S] = m + S < nout ? a1 : 0.f;
        if (m + 2L * S < Lout) orow[m + 2L * S] = m + 2L * S < nout ? a2 : 0.f;
        if (m + 3L * S < Lout) orow[m + 3L * S] = m + 3L * S < nout ? a3 : 0.f;
    }
}

}  // namespace

extern "C" {

long svc_resample_len(int o, int n, long L) {
    if (o < 1 || n < 1 || L < 0) return 0;
    return (long)(((long long)n * L + o - 1) / o);
}

int svc_resampler_create(int o, int n, int width, int ntaps, const int32_t* first, const float* taps, void* stream,
                         svc_resampler_t** out) {
    SVC_REQUIRE(out && first && taps, "svc_resampler_create: null argument");
    SVC_REQUIRE(o >= 1 && n >= 1 && width >= 0 && ntaps >= 1 && o <= (1 << 20) && n <= (1 << 20) && ntaps <= 4096,
                "svc_resampler_create: o, n >= 1 (reduced rates), width >= 0, ntaps >= 1");
    int fmin = first[0], fmax = first[0];
    for (int j = 0; j < n; ++j) {
        SVC_REQUIRE(first[j] >= 0 && first[j] < 2 * width + o, "svc_resampler_create: first[j] outside the 2 width + o columns of a phase");
        fmin = std::min(fmin, first[j]);
        fmax = std::max(fmax, first[j]);
    }
    // G: the most periods per row group whose span fits the budget, among those the one that fills its 256-lane passes best
    auto span_of = [&](long G) { return round_up((RS_ROWS * G - 1) * o + (fmax - fmin) + ntaps + 3, 4); };
    SVC_REQUIRE(span_of(1) <= RS_SPAN_LIMIT, "svc_resampler_create: o too large: the input span of four periods does not fit the LDS");
    int G = 1;
    double best = 0.0;
    for (long g = 1; g * n <= 2048 && (g == 1 || span_of(g) <= RS_SPAN_BUDGET); ++g) {
        const long S = g * n;
        const double fill = (double)S / (double)(round_up(S, RS_THREADS));
        if (fill >= best) { best = fill; G = (int)g; }
    }
    hipStream_t st = (hipStream_t)stream;
    auto* r = new svc_resampler();
    r->q = RsGeom{o, n, width, ntaps, G, fmin, (int)span_of(G)};
    auto fail = [&]() { delete r; return 1; };
    std::vector<float> kn((size_t)ntaps * n);                   // [k][n]: adjacent lanes hold adjacent phases
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < ntaps; ++k) kn[(size_t)k * n + j] = taps[(size_t)j * ntaps + k];
    r->taps_kn = r->mem.alloc_n<float>(kn.size(), st);
    r->first = r->mem.alloc_n<int>(n, st);
    if (!r->taps_kn || !r->first) return fail();
    if (hipMemcpyAsync(r->taps_kn, kn.data(), kn.size() * sizeof(float), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(r->first, first, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) {
        set_error("svc_resampler_create: table upload failed");
        return fail();
    }
    *out = r;
    return 0;
}

void svc_resampler_destroy(svc_resampler_t* r) { delete r; }

long svc_resampler_tile(const svc_resampler_t* r) { return r ? (long)RS_ROWS * r->q.G * r->q.n : 0; }

int svc_resample(svc_resampler_t* r, const float* x, const int32_t* lens, int B, long L, float* out, long Lout, void* stream) {
    SVC_REQUIRE(r != nullptr, "svc_resample: the handle is NULL");
    SVC_REQUIRE(x != nullptr, "svc_resample: x is NULL");
    SVC_REQUIRE(out != nullptr, "svc_resample: out is NULL");
    SVC_REQUIRE(B >= 1 && B <= RS_MAX_B, "svc_resample: B outside [1, 64]");
    SVC_REQUIRE(L >= 1 && L <= INT32_MAX, "svc_resample: L outside [1, 2^31 - 1]");
    RsLens hl;
    long longest = 0;
    for (int b = 0; b < B; ++b) {
        const long len = lens ? (long)lens[b] : L;
        SVC_REQUIRE(len >= 1 && len <= L, "svc_resample: lens outside [1, L]");
        hl.v[b] = (int32_t)len;
        longest = std::max(longest, len);
    }
    for (int b = B; b < RS_MAX_B; ++b) hl.v[b] = 0;
    SVC_REQUIRE(Lout >= svc_resample_len(r->q.o, r->q.n, longest), "svc_resample: Lout below svc_resample_len(o, n, max lens)");
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)B * (uintptr_t)L * 4, o0 = (uintptr_t)out,
                    o1 = o0 + (uintptr_t)B * (uintptr_t)Lout * 4;
    SVC_REQUIRE(x1 <= o0 || o1 <= x0, "svc_resample: x and out overlap");
    const long tiles = (Lout + svc_resampler_tile(r) - 1) / svc_resampler_tile(r);
    SVC_REQUIRE(tiles <= INT32_MAX, "svc_resample: Lout too large");
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, B), dim3(RS_THREADS), (size_t)r->q.span * sizeof(float), (hipStream_t)stream,
                       x, L, hl, r->q, r->taps_kn, r->first, out, Lout);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
