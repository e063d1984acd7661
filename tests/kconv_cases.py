"""Float64 references for the resident-tile Conv1d (csrc/kconv.hip) at op level, shared by test_host_kconv.py (which checks that
the references can tell a right kernel from a subtly wrong one) and test_gpu_kconv.py (which holds the kernel to them).  CPU only,
plain torch ops.  Everything here is channels-last, as the kernel's seam is: x (B, L, Cin), w (Cout, Cin, k), y (B, Lout, Cout).

The three operand modes round as follows (a = activation, w = weight, both fp32 values):
  f16     a_hi = half(a), w_hi = half(w);                        y = a_hi * w_hi
  f16x3   a_lo = half(a - a_hi), w_lo = half(w - w_hi);          y = a_hi w_hi + a_hi w_lo + a_lo w_hi
  p8      fp16 + fp8 corrections (common.h lo_pair_p8, kconv.hip pack_p8_kernel), restated in ref_p8 below.
"""
import math
import random

import torch
import torch.nn.functional as F

LRELU = 3       # KG_ACT_LRELU (csrc/common.h)
MODES = ("f16", "f16x3", "p8")
KCONV_MIN_ROWS = 192
F8 = torch.float8_e4m3fn


def half(t):
    """fp16 rounding of fp32-representable values, returned in float64"""
    return t.to(torch.float32).half().double()


def q8(t):
    """the kernels' fp8 conversion: clamp to +-448, round to OCP e4m3 (round to nearest even, subnormals kept)"""
    return t.to(torch.float32).clamp(-448.0, 448.0).to(F8).double()


def conv(a, w, dil, pad_left, Lout, dt=torch.float64):
    """zero-padded stride-1 conv of channels-last a (B, L, Cin) with w (Cout, Cin, k): (B, Lout, Cout), computed in dt"""
    L = a.shape[1]
    span = (w.shape[2] - 1) * dil
    right = Lout + span - pad_left - L          # negative: the conv never reaches the last rows
    ap = F.pad(a.to(dt).transpose(1, 2), (pad_left, right))
    return F.conv1d(ap, w.to(dt), dilation=dil).transpose(1, 2)


def epilogue(v, bias=None, act=0, act_slope=0.0, res=None, out_scale=0.0, res2=None):
    """the kernel's order: bias, activation, + res, * out_scale (0 means 1), + res2"""
    if bias is not None:
        v = v + bias.to(v.dtype)
    if act == LRELU:
        v = torch.where(v > 0, v, v * float(torch.tensor(act_slope, dtype=torch.float32)))
    elif act != 0:
        raise ValueError(act)
    if res is not None:
        v = v + res.to(v.dtype)
    if out_scale != 0.0:
        v = v * float(torch.tensor(out_scale, dtype=torch.float32))
    if res2 is not None:
        v = v + res2.to(v.dtype)
    return v


def w8_exp(w):
    """kconv_pack_p8: s = 2^ex, ex = floor(log2(224 / max|w|)) in fp32, clamped to +-24; an all-zero weight gives 0"""
    mx = w.to(torch.float32).abs().max()
    if mx.item() == 0.0:
        return 0
    ex = int(math.floor(torch.log2(torch.tensor(224.0, dtype=torch.float32) / mx).item()))
    return max(-24, min(24, ex))


def ref_true(x, w, dil, pad_left, Lout, **epi):
    return epilogue(conv(x.double(), w.double(), dil, pad_left, Lout), **epi)


def ref_f16(x, w, dil, pad_left, Lout, **epi):
    return epilogue(conv(half(x), half(w), dil, pad_left, Lout), **epi)


def ref_x3(x, w, dil, pad_left, Lout, **epi):
    a_hi, w_hi = half(x), half(w)
    a_lo, w_lo = half(x.double() - a_hi), half(w.double() - w_hi)
    c = lambda a, b: conv(a, b, dil, pad_left, Lout)     # noqa: E731
    return epilogue(c(a_hi, w_hi) + c(a_hi, w_lo) + c(a_lo, w_hi), **epi)


def act_planes_p8(x):
    """(hi, byte 0, byte 1) of an activation as lo_pair_p8 writes it: half(a), q8(hi), q8(2^11 (a - hi)), decoded to float64"""
    a_hi = half(x)
    return a_hi, q8(a_hi), q8(2048.0 * (x.double() - a_hi))


def ref_p8(x, w, dil, pad_left, Lout, dt=torch.float64, planes=None, drop=0, exp_off=0, swap=None, **epi):
    """The fp16 + fp8-corrections mode restated from common.h / kconv.hip:
         y = conv(a_hi, w_hi) + [conv(q8(a_hi), q8(2^11 s w_lo)) + conv(q8(2^11 a_lo), q8(s w_hi))] / (2^11 s)
       with a_lo = a - a_hi and w_lo = w - w_hi in fp32 (not rounded to fp16) and s = 2^w8_exp(w).
       planes: the activation planes (hi, byte 0, byte 1) as decoded from a producer instead of x's own.
       dt = float32 evaluates the same convs in fp32 (the reference's own summation noise).
       Sabotages, for checking that the tests can see them: drop = 1 | 2 leaves out the first | second correction product,
       exp_off = +-1 decodes with the weight scale off by a factor 2, swap = "w" | "a" swaps the two bytes on that side."""
    ex = w8_exp(w)
    s = 2.0 ** ex
    w_hi = half(w)
    wb0, wb1 = q8(2048.0 * s * (w.double() - w_hi)), q8(s * w_hi)
    a_hi, ab0, ab1 = planes if planes is not None else act_planes_p8(x)
    if swap == "w":
        wb0, wb1 = wb1, wb0
    if swap == "a":
        ab0, ab1 = ab1, ab0
    c = lambda a, b: conv(a, b, dil, pad_left, Lout, dt)     # noqa: E731
    corr = 0.0
    if drop != 1:
        corr = corr + c(ab0, wb0)
    if drop != 2:
        corr = corr + c(ab1, wb1)
    scale = torch.tensor(2.0 ** -(11 + ex + exp_off), dtype=dt)
    return epilogue((c(a_hi, w_hi) + corr * scale), **epi).double()


# ref_p8's sabotages by name: what a subtly wrong kernel or weight packing would compute
SABOTAGES = {"drop hi*w_lo": dict(drop=1), "drop lo*w_hi": dict(drop=2), "scale x2": dict(exp_off=-1), "scale /2": dict(exp_off=1),
             "weight bytes swapped": dict(swap="w"), "activation bytes swapped": dict(swap="a")}

REFS = {"f16": ref_f16, "f16x3": ref_true, "p8": ref_p8}        # what each mode is held to (f16x3 is held to the truth)
ABS_BOUND = {"f16": 3e-5, "f16x3": 1e-5}                        # test_conv1d_channels_last's bounds, times max(1, |ref|max)


def p8_numbers(x, w, dil, pad_left, Lout, floor=1.0, **epi):
    """(ref_p8, ref_true, e_p8, n32, scale): the distance of the mode's restatement from the truth and the fp32 summation noise
    of the restatement itself, both relative to scale = max(floor, |ref_true|max); floor = 1 as test_conv1d_fuzz has it, 0 for
    the cases whose outputs are tiny by construction (a bound relative to 1 would ask nothing of them)"""
    rt = ref_true(x, w, dil, pad_left, Lout, **epi)
    rp = ref_p8(x, w, dil, pad_left, Lout, **epi)
    r32 = ref_p8(x, w, dil, pad_left, Lout, dt=torch.float32, **epi)
    scale = max(floor, rt.abs().max().item())
    return rp, rt, (rp - rt).abs().max().item() / scale, (r32 - rp).abs().max().item() / scale, scale


def snake(v, a, ib, dt=torch.float64):
    v = v.to(dt)
    return v + ib.to(dt) * torch.sin(a.to(dt) * v) ** 2


def snake_err(v, a, ib):
    """the fp32 Snake's own error: 4 x |snake in float32 torch - snake in float64|max"""
    return 4.0 * (snake(v, a, ib, torch.float32).double() - snake(v, a, ib)).abs().max().item()


def f16_boundary_dist(sv):
    """distance of each float64 value from the nearest fp16 rounding boundary (the midpoint of two neighbouring fp16 values)"""
    h = half(sv)
    inf = torch.tensor(float("inf"), dtype=torch.float16)
    up = torch.nextafter(h.half(), inf).double()
    dn = torch.nextafter(h.half(), -inf).double()
    return torch.minimum(((h + up) / 2 - sv).abs(), ((h + dn) / 2 - sv).abs())


def f16_ulp_steps(a, b):
    """fp16 values a, b (int16 bit patterns of finite fp16) -> how many representable values apart they are"""
    def key(t):
        t = t.to(torch.int32) & 0xFFFF
        return torch.where(t >= 0x8000, 0x8000 - t, t)
    return (key(a) - key(b)).abs()


def make_case(seed, B, L, Cin, Cout, k, amp=1.0, w_amp=1.0):
    """randn inputs of amplitude amp, w ~ w_amp randn / sqrt(Cin k), bias ~ randn"""
    g = torch.Generator().manual_seed(seed)
    x = amp * torch.randn(B, L, Cin, generator=g)
    w = w_amp * torch.randn(Cout, Cin, k, generator=g) / (Cin * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    return x, w, b


# ---- the shapes.  (k, dil): the last two have span 64, the largest the kernel serves.
KD = [(3, 1), (7, 3), (11, 5), (5, 16), (3, 32)]
LS = [192, 193, 256, 257, 321]
CINS = [18, 64, 65, 192]
# (bm override, Cout): cout_pad 128 / 192 under each position tile (at 192 the second column tile is half empty), and the
# 64-channel form, which has one position tile only
FORMS = [(64, 72), (128, 72), (256, 72), (64, 130), (128, 130), (256, 130), (0, 64)]


def _pads(span):
    return [0, span // 2, span]


def parity_cases():
    """(mode, bm, Cout, L, B, Cin, k, dil, pad_left, Lout): the named edges first, then a seeded sample of the product"""
    out = []
    # every (mode, form) at least once, on shapes that also walk L, B, Cin, (k, dil) and the pads
    i = 0
    for mode in MODES:
        for bm, Cout in FORMS:
            k, dil = KD[i % 5]
            L = LS[(i // 2) % 5]
            span = (k - 1) * dil
            out.append((mode, bm, Cout, L, (1, 3)[i % 2], CINS[(i + 1) % 4], k, dil, _pads(span)[i % 3], L))
            i += 1
    for mode in MODES:
        # fewer weight tiles (3 in f16: one chunk, k = 3) than the 5- and 8-stage rings of the 256-row tiles have slots
        out.append((mode, 256, 72, 192, 1, 64, 3, 1, 1, 192))
        out.append((mode, 0, 64, 193, 1, 18, 3, 1, 1, 193))
        # Lin != Lout: a valid conv (no padding), span 64
        out.append((mode, 128, 130, 321, 3, 65, 5, 16, 0, 321 - 64))
        out.append((mode, 0, 64, 321, 1, 192, 3, 32, 0, 321 - 64))
        # span 64 with the whole pad on the left, across a tile edge (L = 257 is 256 + 1)
        out.append((mode, 64, 72, 257, 3, 18, 3, 32, 64, 257))
        # three chunks with the longest kernel, B = 3 (grids of 3, 6, 9, 12: below 8 and no multiples of 8)
        out.append((mode, 128, 130, 256, 3, 192, 11, 5, 25, 256))
    rng = random.Random(20240611)
    for _ in range(18):
        mode = rng.choice(MODES)
        bm, Cout = rng.choice(FORMS)
        L, B, Cin = rng.choice(LS), rng.choice([1, 3]), rng.choice(CINS)
        k, dil = rng.choice(KD)
        span = (k - 1) * dil
        pad_left = rng.choice(_pads(span))
        Lout = L - span if (pad_left == 0 and L - span >= KCONV_MIN_ROWS and rng.random() < 0.5) else L
        out.append((mode, bm, Cout, L, B, Cin, k, dil, pad_left, Lout))
    return out


def expected_form(bm, Cout, B, Lout):
    """(BM, BN) that kconv_launch runs: the override where given, else its own choice by grid size"""
    cout_pad = -(-Cout // 64) * 64
    if cout_pad <= 64:
        return 256, 64
    if bm:
        return bm, 128
    g256 = B * -(-Lout // 256) * -(-cout_pad // 128)
    return (64 if g256 <= 96 else 128), 128


# host-test cases: the (Cin, k, dil) whose reference figures DESIGN.md quotes
HOST_CASES = [(64, 3, 1), (192, 11, 5), (64, 7, 3), (100, 5, 16)]



def snake_case(seed=72, B=3, L=257, Cin=64, Cout=72, k=7):
    """(x, w, bias, a, 1/b) of the fused-Snake tests: a and 1/b of the size HiFT's Snakes have; v = 0.3 randn +- 2 per channel, so
    that |sv| stays above ~0.5 where fp16 values are far apart against the fp32 Snake's error (test_host_kconv.py checks the
    share of elements near an fp16 rounding boundary)"""
    x, w, b = make_case(seed, B, L, Cin, Cout, k, amp=0.3)
    g = torch.Generator().manual_seed(seed + 1)
    a = 0.5 + 1.5 * torch.rand(Cout, generator=g)
    ib = 0.3 + 0.9 * torch.rand(Cout, generator=g)
    return x, w, 2.0 * torch.sign(b), a, ib
