// Real-time sessions from audio: the per-stream audio history of the reference GUI's audio callback
// (real-time-gui.py, `audio_callback`: `input_wav` / `input_wav_res`; restated from memory) as ONE launch per call: shift
// the content-rate context, resample the new block with its 2 zc samples of history, write the dense batch the encoder
// takes and update the history.
//
// A left shift in place is a read-after-write race between workgroups, so the context of every slot lives in two planes:
// a push reads the slot's current plane and writes the other one.  Which plane is current is kept on the device, next to
// the planes: tickets[slot] counts the workgroups that ever pushed to the slot.  Every workgroup takes a ticket when it
// starts; a push of one stream is always `tiles` workgroups (a function of L16 alone), so ticket / tiles is the number of
// pushes the slot has seen, the same for all workgroups of one push, and its low bit names the plane to read.  The call
// keeps no host state, needs no handle and nothing flips a bit after the launch.
//
// Grid (tiles, N).  Workgroups 0 .. tiles - 2 move RT_TILE samples each of the kept part (16-byte accesses where the
// shift, L16 and the pointers allow).  The last workgroup of a stream owns everything that touches hist[slot]: it stages
// x = hist ‖ block tile by tile in LDS and runs the resampler's dot product (resample_core.h) on it, then writes the new
// history.  It is the only reader and the only writer of hist[slot], so one plane of history is enough.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "resample_core.h"

using namespace svc;

namespace {

constexpr int RT_MAXN = 64;
constexpr int RT_TILE = 2048;               // samples of the kept part one workgroup moves: two 16-byte accesses per lane
constexpr int RT_LDS_FLOATS = 16000;        // the staged span (as svc_resample: 64 KB per launch without opting in)

struct RtSlots { int slot[RT_MAXN]; };

struct RtArgs {
    const float* block; long stride; int Lin;
    int max_slots, zc, z16, L16, shift, n_new;
    float* hist; float* ring; unsigned long long* tickets; float* ctx;
};

// x = hist ‖ block at position p (0 <= p < 2 zc + Lin)
__device__ __forceinline__ float rt_x(const float* h, const float* blk, int two_zc, long p) {
    return p < two_zc ? h[p] : blk[p - two_zc];
}

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void rt_push_kernel(const RtArgs a, const RtSlots slots, const RsGeom q, const int resample,
                                                             const float* __restrict__ taps_kn, const int* __restrict__ first) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ unsigned plane_s;
    const int k = blockIdx.y, tid = threadIdx.x;
    const int s = slots.slot[k];
    if (tid == 0) {
        const unsigned long long t = atomicAdd(a.tickets + s, 1ULL);
        plane_s = (unsigned)((t / gridDim.x) & 1ULL);
    }
    __syncthreads();
    const unsigned plane = plane_s;
    const float* old_row = a.ring + ((long)plane * a.max_slots + s) * a.L16;
    float* new_row = a.ring + ((long)(plane ^ 1u) * a.max_slots + s) * a.L16;
    float* c_row = a.ctx + (long)k * a.L16;
    const int keep = a.L16 - a.n_new;                             // samples that only move

    if (blockIdx.x + 1 < gridDim.x) {                             // ---- the kept part: c[i] = old[shift + i]
        const float* src = old_row + a.shift;
        const int i0 = blockIdx.x * RT_TILE;
        if constexpr (VEC) {                                      // shift, z16 and L16 are multiples of 4: so is keep
            const int ia = i0 + tid * 4, ib = ia + RS_THREADS * 4;
            float4v va, vb;
            if (ia < keep) va = *reinterpret_cast<const float4v*>(src + ia);
            if (ib < keep) vb = *reinterpret_cast<const float4v*>(src + ib);
            if (ia < keep) { *reinterpret_cast<float4v*>(new_row + ia) = va; *reinterpret_cast<float4v*>(c_row + ia) = va; }
            if (ib < keep) { *reinterpret_cast<float4v*>(new_row + ib) = vb; *reinterpret_cast<float4v*>(c_row + ib) = vb; }
        } else {
#pragma unroll
            for (int u = 0; u < RT_TILE / RS_THREADS; ++u) {
                const int i = i0 + u * RS_THREADS + tid;
                if (i < keep) { const float v = src[i]; new_row[i] = v; c_row[i] = v; }
            }
        }
        return;
    }

    // ---- the new part: c[keep + t] = y[z16 + t], t < n_new, y = the resampler's output for x = hist ‖ block alone
    float* h = a.hist + (long)s * 2 * a.zc;
    const float* blk = a.block + (long)k * a.stride;
    const int two_zc = 2 * a.zc;
    const long len = (long)two_zc + a.Lin;
    if (!resample) {                                              // equal rates: y = x
        for (int t = tid; t < a.n_new; t += RS_THREADS) {
            const float v = rt_x(h, blk, two_zc, (long)a.z16 + t);
            new_row[keep + t] = v;
            c_row[keep + t] = v;
        }
    } else {
        const int S = q.G * q.n;                                  // work items of a tile, and the distance between an item's outputs
        const long m_end = (long)a.z16 + a.n_new;                 // outputs z16 .. m_end - 1 are wanted
        for (long m0 = a.z16; m0 < m_end; m0 += (long)RS_ROWS * S) {          // tiles as svc_resample cuts them, from z16 on
            // stage x[lo - sh, lo - sh + span), zeros outside [0, len); sh puts the block's samples on 16-byte addresses
            const long lo = (m0 / q.n) * q.o + q.fmin - q.width;
            const int sh = (int)((((long)(reinterpret_cast<uintptr_t>(blk) >> 2) + lo - two_zc) % 4 + 4) % 4);
            const long p0 = lo - sh;
            if (m0 != a.z16) __syncthreads();                     // the previous tile's readers are done with xs
            for (int v = tid * 4; v < q.span; v += RS_THREADS * 4) {
                const long p = p0 + v;
                float4v t;
                if (p >= two_zc && p + 3 < len) {
                    t = *reinterpret_cast<const float4v*>(blk + (p - two_zc));
                } else {                                          // the history, the seam and the ends: element by element
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = (p + e >= 0 && p + e < len) ? rt_x(h, blk, two_zc, p + e) : 0.f;
                }
                *reinterpret_cast<float4v*>(xs + v) = t;
            }
            __syncthreads();
            for (int w = tid; w < S; w += RS_THREADS) {
                float acc[RS_ROWS];
                rs_dot4(xs, sh, q, taps_kn, first, w, acc[0], acc[1], acc[2], acc[3]);
#pragma unroll
                for (int r = 0; r < RS_ROWS; ++r) {
                    const long m = m0 + w + (long)r * S;
                    if (m < m_end) {
                        const long d = keep + (m - a.z16);
                        new_row[d] = acc[r];
                        c_row[d] = acc[r];
                    }
                }
            }
        }
    }
    // ---- hist = x[-2 zc:].  Every read of the old history above has landed (its value went through LDS or a store).
    __syncthreads();
    if (a.Lin >= two_zc) {
        const float* tail = blk + (a.Lin - two_zc);
        for (int i = tid; i < two_zc; i += RS_THREADS) h[i] = tail[i];
    } else {                                                      // Lin == zc: the second half moves down, chunk by chunk
        const int moved = two_zc - a.Lin;                         // h[i] = h[i + Lin], i < moved: a chunk's writes lie below
        for (int i0 = 0; i0 < moved; i0 += RS_THREADS) {          // every later chunk's reads
            const int i = i0 + tid;
            const float v = i < moved ? h[i + a.Lin] : 0.f;
            __syncthreads();
            if (i < moved) h[i] = v;
        }
        for (int i = tid; i < a.Lin; i += RS_THREADS) h[moved + i] = blk[i];
    }
}

inline bool disjoint(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a1 <= b0 || b1 <= a0; }

}  // namespace

extern "C" {

int svc_rt_push_tiles(int L16) { return L16 >= 1 ? (L16 + RT_TILE - 1) / RT_TILE + 1 : 0; }

long long svc_rt_ring_floats(int max_slots, int L16) {
    if (max_slots < 1 || L16 < 1) return 0;
    return 2LL * max_slots * L16 + 2LL * max_slots;
}

int svc_rt_push(const svc_resampler_t* r, const float* block, long long stride, int Lin, int N, const int32_t* slots, int max_slots,
                int zc, int z16, float* hist, float* ring, int L16, float* ctx, void* stream) {
    SVC_REQUIRE(block && slots && hist && ring && ctx, "rt_push: null argument (block, slots, hist, ring, ctx)");
    SVC_REQUIRE(N >= 1 && N <= RT_MAXN, "rt_push: N outside [1, 64]");
    SVC_REQUIRE(max_slots >= 1 && zc >= 1 && z16 >= 1 && L16 >= 1, "rt_push: max_slots, zc, z16 and L16 must be at least 1");
    SVC_REQUIRE(zc <= (1 << 24) && z16 <= (1 << 24), "rt_push: zc or z16 above 2^24");
    SVC_REQUIRE(Lin >= zc && Lin % zc == 0, "rt_push: Lin is not a positive multiple of zc");
    SVC_REQUIRE(stride >= Lin, "rt_push: stride below Lin");
    const long long m = Lin / zc, shift = m * z16, n_new = shift + z16, xlen = 2LL * zc + Lin;
    SVC_REQUIRE(n_new <= L16, "rt_push: L16 below n_new = (Lin / zc + 1) z16");
    SVC_REQUIRE(xlen <= INT32_MAX, "rt_push: 2 zc + Lin above 2^31 - 1");
    const int o = r ? r->q.o : 1, n = r ? r->q.n : 1;
    SVC_REQUIRE(zc % o == 0 && z16 % n == 0, "rt_push: zc is not a multiple of o or z16 not of n (a block must start at phase 0)");
    SVC_REQUIRE(svc_resample_len(o, n, (long)xlen) >= z16 + n_new,
                "rt_push: svc_resample_len(o, n, 2 zc + Lin) below z16 + n_new: hist and block do not hold the new samples");
    std::vector<int32_t> sorted(slots, slots + N);
    std::sort(sorted.begin(), sorted.end());
    SVC_REQUIRE(sorted.front() >= 0 && sorted.back() < max_slots, "rt_push: a slot outside 0 .. max_slots - 1");
    SVC_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "rt_push: a slot appears twice in one call");
    SVC_REQUIRE((((uintptr_t)block | (uintptr_t)hist | (uintptr_t)ring | (uintptr_t)ctx) & 3) == 0 &&
                ((uintptr_t)ring & 7) == 0, "rt_push: a buffer is not aligned (floats: 4 bytes, ring: 8 bytes)");
    const long long ring_floats = svc_rt_ring_floats(max_slots, L16);
    const uintptr_t b0 = (uintptr_t)block, b1 = b0 + (uintptr_t)(((long long)(N - 1) * stride + Lin) * 4);
    const uintptr_t h0 = (uintptr_t)hist, h1 = h0 + (uintptr_t)(2LL * zc * max_slots * 4);
    const uintptr_t r0 = (uintptr_t)ring, r1 = r0 + (uintptr_t)(ring_floats * 4);
    const uintptr_t c0 = (uintptr_t)ctx, c1 = c0 + (uintptr_t)((long long)N * L16 * 4);
    SVC_REQUIRE(disjoint(b0, b1, h0, h1) && disjoint(b0, b1, r0, r1) && disjoint(b0, b1, c0, c1) && disjoint(h0, h1, r0, r1) &&
                disjoint(h0, h1, c0, c1) && disjoint(r0, r1, c0, c1), "rt_push: block, hist, ring and ctx overlap");
    if (r) SVC_REQUIRE(r->q.span <= RT_LDS_FLOATS, "rt_push: the resampler's span does not fit the LDS");

    RtArgs a;
    a.block = block; a.stride = (long)stride; a.Lin = Lin;
    a.max_slots = max_slots; a.zc = zc; a.z16 = z16; a.L16 = L16; a.shift = (int)shift; a.n_new = (int)n_new;
    a.hist = hist; a.ring = ring; a.tickets = reinterpret_cast<unsigned long long*>(ring + 2LL * max_slots * L16); a.ctx = ctx;
    RtSlots sl;
    memset(&sl, 0, sizeof(sl));
    for (int k = 0; k < N; ++k) sl.slot[k] = slots[k];
    RsGeom q;
    memset(&q, 0, sizeof(q));
    if (r) q = r->q;
    const bool vec = shift % 4 == 0 && z16 % 4 == 0 && L16 % 4 == 0 && (((uintptr_t)ring | (uintptr_t)ctx) & 15) == 0;
    const dim3 grid((unsigned)svc_rt_push_tiles(L16), (unsigned)N);
    const size_t lds = r ? (size_t)q.span * sizeof(float) : 0;
    const float* taps = r ? r->taps_kn : nullptr;
    const int* first = r ? r->first : nullptr;
    if (vec)
        hipLaunchKernelGGL(rt_push_kernel<true>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a, sl, q, r ? 1 : 0, taps, first);
    else
        hipLaunchKernelGGL(rt_push_kernel<false>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a, sl, q, r ? 1 : 0, taps, first);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
