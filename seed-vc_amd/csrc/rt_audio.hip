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
//
// The input gate (`svc_rt_push_gated`) lives in that last workgroup too: before it stages anything it sums the
// block's 20 ms frames (`rt_gate`: one wave per frame, an order that is a function of zc alone), decides from the last four
// energies which frames are muted, and from then on reads the block through `rt_blk`, which gives +0.0 for a muted frame.  Its
// only state is the three carried energies of gate_e[slot].  A stream whose gate is off is only tracked; its first workgroup
// does that beside its move, so the last one is as long as without the gate.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "resample_core.h"

using namespace svc;

namespace {

constexpr int RT_MAXN = 64;
constexpr int RT_TILE = 2048;               // samples of the kept part one workgroup moves: two 16-byte accesses per lane
constexpr int RT_LDS_FLOATS = 16000;        // the staged span (as svc_resample: 64 KB per launch without opting in)
constexpr int RT_GATE_FRAMES = 256;         // frames of a block the gate can hold in static LDS (5.12 s)

struct RtSlots { int slot[RT_MAXN]; };
struct RtGate { float pow[RT_MAXN]; };      // the threshold on the energy of 4 frames, per listed stream; 0.0f: off

struct RtArgs {
    const float* block; long stride; int Lin;
    int max_slots, zc, z16, L16, shift, n_new;
    float* hist; float* ring; unsigned long long* tickets; float* ctx;
    float* gate_e; int* gate_mask;          // NULL: svc_rt_push
};

// block sample i behind the gate: +0.0 inside a muted frame (mute == NULL: no frame is muted)
__device__ __forceinline__ float rt_blk(const float* blk, const unsigned char* mute, int zc, long i) {
    return mute && mute[i / zc] ? 0.f : blk[i];
}

// x = hist ‖ block at position p (0 <= p < 2 zc + Lin)
__device__ __forceinline__ float rt_x(const float* h, const float* blk, const unsigned char* mute, int zc, long p) {
    return p < 2 * zc ? h[p] : rt_blk(blk, mute, zc, p - 2 * zc);
}

// The gate of one stream, by one workgroup: the energies of the block's frames behind the three carried ones in ge, the
// decisions in mute_s and gate_mask, the new carried energies in gate_e[slot].  A frame is summed by one wave: a lane's four
// interleaved ascending FMA chains over i = lane, lane + 64, ... (the loads of a pass do not wait for each other), their sum
// ((e0 + e1) + (e2 + e3)), then the xor butterfly -- a function of zc alone.  -> whether a frame of this block is muted at all.
// A stream whose gate is off (pw == 0) has this done by its FIRST workgroup, which only moves samples, so that tracking the
// energies does not lengthen the last one; a stream whose gate is on needs the decisions where the block is staged.
__device__ __forceinline__ bool rt_gate(const RtArgs& a, float pw, int k, int s, const float* blk, int tid, float* ge,
                                        unsigned char* mute_s) {
    const int m = a.Lin / a.zc;
    if (!a.gate_e) {                                              // nothing to track: the mask is all zero
        if (a.gate_mask)
            for (int j = tid; j < m; j += RS_THREADS) a.gate_mask[(long)k * m + j] = 0;
        return false;
    }
    float* g = a.gate_e + (long)s * 3;
    if (tid < 3) ge[tid] = g[tid];
    const int lane = tid & 63;
    for (int j = tid >> 6; j < m; j += RS_THREADS / 64) {         // a wave per frame
        const float* f = blk + (long)j * a.zc;
        float e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
        int i = lane;
        for (; i + 192 < a.zc; i += 256) {
            const float x0 = f[i], x1 = f[i + 64], x2 = f[i + 128], x3 = f[i + 192];
            e0 = fmaf(x0, x0, e0); e1 = fmaf(x1, x1, e1); e2 = fmaf(x2, x2, e2); e3 = fmaf(x3, x3, e3);
        }
        for (; i < a.zc; i += 64) e0 = fmaf(f[i], f[i], e0);
        float e = (e0 + e1) + (e2 + e3);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) e += __shfl_xor(e, d, 64);
        if (lane == 0) ge[3 + j] = e;
    }
    __syncthreads();
    int any = 0;
    for (int j = tid; j < m; j += RS_THREADS) {
        const float E = ((ge[j] + ge[j + 1]) + ge[j + 2]) + ge[j + 3];
        const bool mu = E < pw;                                   // a NaN energy never mutes; pw == 0: nothing does
        mute_s[j] = mu ? 1 : 0;
        any |= mu ? 1 : 0;
        if (a.gate_mask) a.gate_mask[(long)k * m + j] = mu ? 1 : 0;
    }
    if (tid < 3) g[tid] = ge[m + tid];                            // the last three raw frames of the stream
    return __syncthreads_or(any) != 0;
}

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void rt_push_kernel(const RtArgs a, const RtSlots slots, const RtGate gate, const RsGeom q,
                                                             const int resample, const float* __restrict__ taps_kn,
                                                             const int* __restrict__ first) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ unsigned plane_s;
    __shared__ float ge[RT_GATE_FRAMES + 3];                      // g0, g1, g2, e_0 .. e_{m-1}
    __shared__ unsigned char mute_s[RT_GATE_FRAMES];
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

    if (blockIdx.x == 0 && (a.gate_e || a.gate_mask) && !(gate.pow[k] > 0.f))      // gate off: the energies are tracked here
        rt_gate(a, 0.f, k, s, a.block + (long)k * a.stride, tid, ge, mute_s);
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
    const unsigned char* mute = nullptr;                          // uniform: set where this stream's gate is on
    if (gate.pow[k] > 0.f && rt_gate(a, gate.pow[k], k, s, blk, tid, ge, mute_s)) mute = mute_s;
    if (!resample) {                                              // equal rates: y = x
        for (int t = tid; t < a.n_new; t += RS_THREADS) {
            const float v = rt_x(h, blk, mute, a.zc, (long)a.z16 + t);
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
                    if (mute) {                                   // four samples lie in at most two frames
                        const int f = (int)((p - two_zc) / a.zc), left = (int)((long)(f + 1) * a.zc - (p - two_zc));
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (mute[e < left ? f : f + 1]) t[e] = 0.f;
                    }
                } else {                                          // the history, the seam and the ends: element by element
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = (p + e >= 0 && p + e < len) ? rt_x(h, blk, mute, a.zc, p + e) : 0.f;
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
        for (int i = tid; i < two_zc; i += RS_THREADS) h[i] = rt_blk(tail, mute ? mute + (a.Lin - two_zc) / a.zc : nullptr, a.zc, i);
    } else {                                                      // Lin == zc: the second half moves down, chunk by chunk
        const int moved = two_zc - a.Lin;                         // h[i] = h[i + Lin], i < moved: a chunk's writes lie below
        for (int i0 = 0; i0 < moved; i0 += RS_THREADS) {          // every later chunk's reads
            const int i = i0 + tid;
            const float v = i < moved ? h[i + a.Lin] : 0.f;
            __syncthreads();
            if (i < moved) h[i] = v;
        }
        for (int i = tid; i < a.Lin; i += RS_THREADS) h[moved + i] = rt_blk(blk, mute, a.zc, i);
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
    return svc_rt_push_gated(r, block, stride, Lin, N, slots, max_slots, zc, z16, hist, ring, L16, ctx, nullptr, nullptr, nullptr, stream);
}

int svc_rt_push_gated(const svc_resampler_t* r, const float* block, long long stride, int Lin, int N, const int32_t* slots,
                      int max_slots, int zc, int z16, float* hist, float* ring, int L16, float* ctx, const float* gate_pow,
                      float* gate_e, int32_t* gate_mask, void* stream) {
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
    // ---- the gate
    SVC_REQUIRE(gate_e || !gate_pow, "rt_push: gate_pow is given but gate_e is NULL");
    RtGate gt;
    memset(&gt, 0, sizeof(gt));
    for (int k = 0; gate_pow && k < N; ++k) {
        SVC_REQUIRE(gate_pow[k] >= 0.f, "rt_push: a gate_pow entry is negative or NaN");
        gt.pow[k] = gate_pow[k];
    }
    SVC_REQUIRE(!gate_e || m <= RT_GATE_FRAMES, "rt_push: Lin / zc above 256 frames with gate_e given");
    SVC_REQUIRE((((uintptr_t)gate_e | (uintptr_t)gate_mask) & 3) == 0, "rt_push: gate_e or gate_mask is not aligned to 4 bytes");
    const uintptr_t e0 = (uintptr_t)gate_e, e1 = e0 + (uintptr_t)(3LL * max_slots * 4);
    const uintptr_t k0 = (uintptr_t)gate_mask, k1 = k0 + (uintptr_t)((long long)N * m * 4);
    for (const auto& o2 : {std::pair<uintptr_t, uintptr_t>{b0, b1}, {h0, h1}, {r0, r1}, {c0, c1}}) {
        SVC_REQUIRE(!gate_e || disjoint(e0, e1, o2.first, o2.second), "rt_push: gate_e overlaps block, hist, ring or ctx");
        SVC_REQUIRE(!gate_mask || disjoint(k0, k1, o2.first, o2.second), "rt_push: gate_mask overlaps block, hist, ring or ctx");
    }
    SVC_REQUIRE(!gate_e || !gate_mask || disjoint(e0, e1, k0, k1), "rt_push: gate_e and gate_mask overlap");

    RtArgs a;
    a.block = block; a.stride = (long)stride; a.Lin = Lin;
    a.max_slots = max_slots; a.zc = zc; a.z16 = z16; a.L16 = L16; a.shift = (int)shift; a.n_new = (int)n_new;
    a.hist = hist; a.ring = ring; a.tickets = reinterpret_cast<unsigned long long*>(ring + 2LL * max_slots * L16); a.ctx = ctx;
    a.gate_e = gate_e; a.gate_mask = gate_mask;
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
        hipLaunchKernelGGL(rt_push_kernel<true>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a, sl, gt, q, r ? 1 : 0, taps, first);
    else
        hipLaunchKernelGGL(rt_push_kernel<false>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, a, sl, gt, q, r ? 1 : 0, taps, first);
    SVC_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
