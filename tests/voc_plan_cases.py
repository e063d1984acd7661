"""Shared by test_host_voc_plan.py and test_gpu_voc_plan.py: the CPU statement of the two range censuses of the fp16p8 vocoder
mode (csrc/range_census.hip) with torch.float8_e4m3fn as the yardstick, the census inputs, and the vocoder fixtures (in-range,
quiet, channel gains) with their oracle references.  CPU only, plain torch ops.

Census of operand planes (hi fp16, lo fp16 residual; live = rows below lens[b], channels below C):
  bytes    b_hi = q8(hi), b_lo = q8(2^11 lo)          q8 = clamp to +-448, round to OCP e4m3 (common.h lo_pair_p8)
  counts   n: hi != 0;  n_hi_clamp: |hi| > 448;  n_hi_sub: 0 < |hi| < 2^-6;  n_lo_flush: lo != 0 and b_lo == 0;
           n_lo_clamp: |2^11 lo| > 448;  max_hi = max |hi|
  sums     s_hi2 = sum hi^2, s_hi_err2 = sum (hi - b_hi)^2, s_lo2 = sum lo^2, s_lo_err2 = sum (lo - 2^-11 b_lo)^2
Every term is exact in float64 (fp16 and e4m3 values, their differences and the squares of those), so the kernel and this
statement differ by summation order alone: |difference| <= 2 n 2^-53 sum (SUM_BOUND).
Weight census per output channel of w (Cout, Cin, k), s = 2^w8_exp(w) (kconv.hip pack_p8_kernel):
  w_hi = half(w), w_lo = half(w - w_hi);  b_hi = q8(s w_hi), b_lo = q8(2^11 s (w - w_hi))   (the fp32 residual feeds the byte)
  sum w_hi^2, sum (w_hi - b_hi / s)^2, sum w_lo^2, sum (w_lo - b_lo / (2^11 s))^2
"""
import torch

import cases
import kconv_cases as K
import seedvc_oracle as O
from seedvc_amd import specs, weights

COUNTS = ("n", "n_hi_clamp", "n_hi_sub", "n_lo_flush", "n_lo_clamp")
SUMS = ("s_hi2", "s_hi_err2", "s_lo2", "s_lo_err2")
TAU = 2.0 ** -6


def sum_bound(n):
    """relative bound on the difference of two float64 sums of the same n non-negative exact terms in different orders"""
    return 2.0 * n * 2.0 ** -53


def census_ref(hi, lo, C, lens=None):
    """hi, lo (B, L, ld) fp16 -> dict as ops.census_dict gives it"""
    B, L, _ = hi.shape
    lens = [L] * B if lens is None else lens
    h = torch.cat([hi[b, :lens[b], :C].reshape(-1) for b in range(B)]).double()
    l = torch.cat([lo[b, :lens[b], :C].reshape(-1) for b in range(B)]).double()
    bh, bl = K.q8(h), K.q8(l * 2048.0) / 2048.0
    d = {"n": int((h != 0).sum()), "n_hi_clamp": int((h.abs() > 448).sum()),
         "n_hi_sub": int(((h.abs() > 0) & (h.abs() < 2.0 ** -6)).sum()),
         "n_lo_flush": int(((l != 0) & (bl == 0)).sum()), "n_lo_clamp": int(((l * 2048.0).abs() > 448).sum()),
         "max_hi": float(h.abs().max()) if h.numel() else 0.0,
         "s_hi2": float((h * h).sum()), "s_hi_err2": float(((h - bh) ** 2).sum()),
         "s_lo2": float((l * l).sum()), "s_lo_err2": float(((l - bl) ** 2).sum())}
    return d


def ratios(d):
    """(rho, eta) of a census record"""
    return (d["s_lo_err2"] / d["s_lo2"] if d["s_lo2"] > 0 else 0.0, d["s_hi_err2"] / d["s_hi2"] if d["s_hi2"] > 0 else 0.0)


def weight_census_ref(w):
    """w (Cout, Cin, k) fp32 -> (sums (Cout, 4) float64, w8_exp)"""
    ex = K.w8_exp(w)
    s = 2.0 ** ex
    w_hi = K.half(w)
    res = w.double() - w_hi
    w_lo = K.half(res)
    b_hi, b_lo = K.q8(s * w_hi) / s, K.q8(2048.0 * s * res) / (2048.0 * s)
    f = lambda t: t.reshape(t.shape[0], -1).sum(1)      # noqa: E731
    return torch.stack([f(w_hi ** 2), f((w_hi - b_hi) ** 2), f(w_lo ** 2), f((w_lo - b_lo) ** 2)], 1), ex


def split_planes(v):
    """fp32 values -> (hi, lo) fp16 planes as the fp16x3 producers write them"""
    hi = v.to(torch.float32).half()
    return hi, (v.to(torch.float32) - hi.float()).half()


# ---- the census op case: 3 x 200 x 72 (ld 128), amplitudes 2^-14 .. 2^11 within one plane, exact zeros, NaN where nothing may read
CENSUS_SHAPE = (3, 200, 72, 128)
CENSUS_LENS = (200, 1, 137)


def census_planes(seed=7101):
    B, L, C, ld = CENSUS_SHAPE
    e = cases.rand("voc_plan.census.exp", seed, B, L, C) * 25.0 - 14.0
    v = cases.randn("voc_plan.census.val", seed, B, L, C) * torch.exp2(e)
    v[cases.rand("voc_plan.census.zero", seed, B, L, C) < 0.05] = 0.0
    hi, lo = split_planes(v)
    ph = torch.full((B, L, ld), float("nan"), dtype=torch.float16)
    pl = torch.full((B, L, ld), float("nan"), dtype=torch.float16)
    for b, n in enumerate(CENSUS_LENS):
        ph[b, :n, :C], pl[b, :n, :C] = hi[b, :n], lo[b, :n]
    return ph, pl


def census_weight(seed=7102):
    """[64][7][72] conv (Cout 64, Cin 72, k 7) with per-output-channel gains 2^(3 N(0,1)) and two all-zero channels"""
    w = cases.randn("voc_plan.w", seed, 64, 72, 7) * 0.05
    w = w * torch.exp2(3.0 * cases.randn("voc_plan.w.gain", seed, 64))[:, None, None]
    w[5] = 0.0
    w[40] = 0.0
    return w


# ---- the vocoder fixtures
BIG_S, BIG_B = 64, 2
HIFT_S, HIFT_B = 32, 2
VARIANTS = ("in_range", "quiet", "gains")


def bigvgan_config():
    return specs.bigvgan_config("22k", upsample_initial_channel=256, num_mels=20, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4])


def hift_config(**ov):
    return specs.hift_config(base_channels=128, f0_cond_channels=48, **ov)


def _resblock_prefixes(sd):
    return sorted({k.rsplit(".convs1.", 1)[0] for k in sd if ".convs1." in k})


def _eff_weight(sd, p):
    """the effective conv weight of prefix p (weight-normed or not)"""
    if p + ".weight" in sd:
        return sd[p + ".weight"].float()
    v, g = sd[p + ".weight_v"].float(), sd[p + ".weight_g"].float()
    return v * (g / v.reshape(v.shape[0], -1).norm(dim=1).reshape(-1, 1, 1))


def _set_weight(sd, p, w):
    if p + ".weight" in sd:
        sd[p + ".weight"] = w
    else:       # g = ||v|| makes the effective weight v itself
        sd[p + ".weight_v"] = w
        sd[p + ".weight_g"] = w.reshape(w.shape[0], -1).norm(dim=1).reshape(-1, 1, 1)


def transform(sd, variant, seed):
    """in_range: sd as it is.  quiet: conv_pre weight and bias, every ups and ResBlock bias x 2^-10, conv_post weight x 2^10 (Snake
    is near-linear at that amplitude, so the waveform level is roughly kept).  gains: each ResBlock convs1 output channel x g_c and
    the matching convs2 input channel / g_c, g_c = 2^(3 N(0,1)), seeded."""
    sd = {k: v.clone() for k, v in sd.items()}
    if variant == "in_range":
        return sd
    if variant == "quiet":
        q = 2.0 ** -10
        _set_weight(sd, "conv_pre", _eff_weight(sd, "conv_pre") * q)
        _set_weight(sd, "conv_post", _eff_weight(sd, "conv_post") / q)
        for k in sd:
            if k.endswith(".bias") and (k.startswith("ups.") or "resblocks." in k or k == "conv_pre.bias"):
                sd[k] = sd[k] * q
        return sd
    assert variant == "gains"
    for p in _resblock_prefixes(sd):
        d = 0
        while f"{p}.convs1.{d}.bias" in sd:
            c1, c2 = f"{p}.convs1.{d}", f"{p}.convs2.{d}"
            w1, w2 = _eff_weight(sd, c1), _eff_weight(sd, c2)
            g = torch.exp2(3.0 * cases.randn(f"voc_plan.gain.{p}.{d}", seed, w1.shape[0]))
            _set_weight(sd, c1, w1 * g[:, None, None])
            sd[c1 + ".bias"] = sd[c1 + ".bias"] * g
            _set_weight(sd, c2, w2 / g[None, :, None])
            d += 1
    return sd


_FIX = {}


def bigvgan_fixture(variant):
    """(h, sd, mel (B, 20, S), ref (B, 1, S * 8)): the oracle's waveform is computed once and shared"""
    key = ("bigvgan", variant)
    if key not in _FIX:
        h = bigvgan_config()
        sd = weights.make_state_dict(specs.bigvgan_state_spec(h), seed=71, prefix="bigvgan.")
        sd = transform(sd, variant, 71)
        mel = cases.logmel("voc_plan.bigvgan.mel", 71, BIG_B, h["num_mels"], BIG_S)
        _FIX[key] = (h, sd, mel, O.bigvgan_forward(sd, h, mel))
    return _FIX[key]


def hift_fixture(variant, **ov):
    """(c, sd, mel, f0, phase0, noise, ref): f0 is pinned to the oracle's predictor output (the phase integrates f0)"""
    key = ("hift", variant, tuple(sorted((k, str(v)) for k, v in ov.items())))
    if key not in _FIX:
        c = hift_config(**ov)
        sd = weights.make_state_dict(specs.hift_state_spec(c), seed=72, prefix="hift.")
        sd = transform(sd, variant, 72)
        mel = cases.logmel("voc_plan.hift.mel", 72, HIFT_B, c["in_channels"], HIFT_S)
        Lw = HIFT_S * specs.hift_total_upsample(c)
        nh = c["nb_harmonics"] + 1
        phase0 = (cases.rand("voc_plan.hift.phase", 72, HIFT_B, nh, 1) * 2 - 1) * 3.141592653589793
        noise = cases.randn("voc_plan.hift.noise", 72, HIFT_B, nh, Lw)
        f0 = O.hift_f0_predictor(sd, mel)
        _FIX[key] = (c, sd, mel, f0, phase0, noise, O.hift_forward(sd, c, mel, phase0, noise, f0=f0))
    return _FIX[key]


def rel_rms(y, ref):
    """RMS(err) / RMS(reference)"""
    y, ref = y.double().reshape(-1), ref.double().reshape(-1)
    return ((y - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
