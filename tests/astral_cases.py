"""Cases and the yardstick of the ASTRAL tokenizer tests (csrc/astral.hip, seedvc_amd/astral.py).

The yardstick is a plain-torch restatement in float64: the SSL front is w2v_cases' extractor, positional conv and layers WITHOUT
encoder.layer_norm; a head is the ConvNeXt V2 stage in 1-D (depthwise conv of 7 taps, LayerNorm eps 1e-6, pwconv1, erf-GELU, GRN over
the window's own rows, pwconv2, residual) and the binary spherical quantizer's index (project_in, strict sign, MSB first).
test_host_astral.py pins the block to transformers' `ConvNextV2Layer` and the front to `HubertModel` with the final LayerNorm
replaced by Identity.  The same code with `dtype=torch.float16` is the reference's own arithmetic: its error is the cap of precision 1.

Weights follow w2v_cases: matrices and conv kernels N(0, 1 / fan_in), biases 0.1 N(0, 1), LayerNorm weights 1 + 0.1 N(0, 1);
grn.gamma = 0.5 + 0.1 N(0, 1) so that GRN matters, grn.beta = 0.1 N(0, 1).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import w2v_cases as VC
from w2v_cases import make_wave, rms  # noqa: F401

torch.set_grad_enabled(False)

SPR = 320
HEADS_S = [dict(dim=64, intermediate_dim=192, n_blocks=3, bits=11, dw_kernel=7), dict(dim=64, intermediate_dim=192, n_blocks=3, bits=5, dw_kernel=7)]
HEADS_F = [dict(dim=512, intermediate_dim=1536, n_blocks=12, bits=11, dw_kernel=7), dict(dim=512, intermediate_dim=1536, n_blocks=12, bits=5, dw_kernel=7)]
CFG_S = dict(ssl=VC.CFG_S, heads=HEADS_S)
# F exercises the head seams only: the front is as narrow as the handle allows at d_model 1024
CFG_F = dict(ssl=dict(VC.CFG_F, n_layers=1, ffn_dim=64, conv_dim=64), heads=HEADS_F)

SEAM_T = (1, 3, 4, 7, 63, 64, 65, 129, 300)                 # both paddings overlap, shorter than the kernel, around a row tile, several GRN tiles
HEAD_T = (65, 300)
TOKEN_LENS = (400, 719, 3000, 16000)
CLIP_LENS = (20000, 32000, 32400, 57700)                     # 1 + 1 + 2 + 3 windows of 32 000 samples at an overlap of 20 rows
OV = 20

# Largest errors measured on MI355X, RMS of (device - float64) relative to max(1, RMS of the float64 values), on the
# last block's stream x and on the logits z, per configuration and precision; the asserted bound is min(cap, 4 x measured) with
# the caps of `rms_bound`.
MEASURED = {"S": {0: dict(x=6.47e-7, z=8.92e-7), 1: dict(x=9.38e-4, z=1.04e-3)}, "F": {0: dict(x=1.38e-6, z=1.53e-6), 1: dict(x=7.95e-4, z=8.36e-4)}}
# The same for ONE block (head 0 with n_blocks = 1 on the nine lengths of `seam_case`, worst clip): the block seam has its own bound.
MEASURED_BLOCK = {"S": {0: 3.98e-7, 1: 5.32e-4}, "F": {0: 9.77e-7, 1: 6.31e-4}}
# Token margin m per configuration and precision: 4 x the largest |device - float64| logit error measured on MI355X (S: audio in,
# through the SSL front, 1.04e-3 / 1.34e-2; F: head seams on given rows, 2.32e-5 / 1.13e-2).  A bit of the device index may differ
# from the float64 index only where |z64| <= m; `excluded_fraction` bounds how many bits that may be.
MARGIN = {"S": {0: 4.2e-3, 1: 5.4e-2}, "F": {0: 9.3e-5, 1: 4.6e-2}}
MAX_EXCLUDED = 0.05


def head_state_spec(c, k):
    from seedvc_amd import specs
    return specs.astral_head_state_spec(c, k)


def make_head_sd(c, k, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shp in head_state_spec(c, k).items():
        if key.endswith("grn.gamma"):
            sd[key] = 0.5 + 0.1 * torch.randn(shp, generator=g)
        elif key.endswith("grn.beta") or key.endswith("bias"):
            sd[key] = 0.1 * torch.randn(shp, generator=g)
        elif ".norm." in key:
            sd[key] = 1.0 + 0.1 * torch.randn(shp, generator=g)
        else:
            sd[key] = torch.randn(shp, generator=g) / math.sqrt(float(np.prod(shp[1:])))
    return sd


# ---------------------------------------------------------------------------------------------------- SSL front
def window_rows(c, n):
    return min(VC.frames(c["ssl"], n), n // SPR)


def ssl_layers(sd, c, x, dtype=torch.float64):
    """w2v_cases.layers without encoder.layer_norm: x (T, D) after the positional conv -> the residual stream after the last layer"""
    D, H = c["d_model"], c["n_heads"]
    w = lambda k: sd[k].to(dtype)                                   # noqa: E731
    lin = lambda t, p: F.linear(t, w(p + ".weight"), w(p + ".bias"))   # noqa: E731
    T = x.shape[0]
    heads = lambda t: t.view(T, H, 64).transpose(0, 1)              # noqa: E731
    for i in range(c["n_layers"]):
        p = f"encoder.layers.{i}."
        hN = F.layer_norm(x, (D,), w(p + "layer_norm.weight"), w(p + "layer_norm.bias"), 1e-5)
        q, k, v = heads(lin(hN, p + "attention.q_proj") * 0.125), heads(lin(hN, p + "attention.k_proj")), heads(lin(hN, p + "attention.v_proj"))
        a = (torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v).transpose(0, 1).reshape(T, D)
        x = x + lin(a, p + "attention.out_proj")
        hN = F.layer_norm(x, (D,), w(p + "final_layer_norm.weight"), w(p + "final_layer_norm.bias"), 1e-5)
        x = x + lin(F.gelu(lin(hN, p + "feed_forward.intermediate_dense")), p + "feed_forward.output_dense")
    return x


def ssl(sd, c, wave, dtype=torch.float64):
    """raw samples (n,) of ONE window -> (window_rows(n), D): normalisation, extractor, positional conv, layers, no final LayerNorm"""
    cs = c["ssl"]
    xn = VC.normalize(wave).to(dtype)
    h = VC.posconv(sd, cs, VC.extractor(sd, cs, xn, dtype), dtype)
    return ssl_layers(sd, cs, h, dtype)[:window_rows(c, wave.numel())]


# ---------------------------------------------------------------------------------------------------- head
def block(sd, i, x, dtype=torch.float64, branches=None):
    """ConvNeXt V2 block i on x (T, D): transformers' ConvNextV2Layer with the image height 1"""
    p = f"encoder.blocks.{i}."
    w = lambda k: sd[p + k].to(dtype)                               # noqa: E731
    D = x.shape[1]
    y = F.conv1d(x.T[None], w("dwconv.weight"), w("dwconv.bias"), padding=3, groups=D)[0].T
    y = F.layer_norm(y, (D,), w("norm.weight"), w("norm.bias"), 1e-6)
    y = F.gelu(F.linear(y, w("pwconv1.weight"), w("pwconv1.bias")))
    gx = y.pow(2).sum(0, keepdim=True).sqrt()
    nx = gx / (gx.mean(-1, keepdim=True) + 1e-6)
    y = w("grn.gamma").reshape(1, -1) * (y * nx) + w("grn.beta").reshape(1, -1) + y
    f = F.linear(y, w("pwconv2.weight"), w("pwconv2.bias"))
    if branches is not None:
        branches.append((f.double().pow(2).mean().sqrt().item(), x.double().pow(2).mean().sqrt().item()))
    return x + f


def convnext(sd, hc, h, dtype=torch.float64, n_blocks=None, branches=None):
    """SSL rows h (T, Din) of ONE window -> x (T, dim) after the last block"""
    x = F.linear(h.to(dtype), sd["encoder.input_projection.weight"].to(dtype).flatten(1), sd["encoder.input_projection.bias"].to(dtype))
    for i in range(hc["n_blocks"] if n_blocks is None else n_blocks):
        x = block(sd, i, x, dtype, branches)
    return x


def logits(sd, x, dtype=torch.float64):
    return F.linear(x.to(dtype), sd["quantizer.project_in.weight"].to(dtype), sd["quantizer.project_in.bias"].to(dtype))


def bsq_index(z):
    """index = sum_j [z_j > 0] 2^(bits - 1 - j): strict comparison, MSB first"""
    bits = z.shape[-1]
    idx = torch.zeros(z.shape[:-1], dtype=torch.int64)
    for j in range(bits):
        idx += (z[..., j] > 0).to(torch.int64) << (bits - 1 - j)
    return idx


def index_bits(idx, bits):
    """(...,) indices -> (..., bits) booleans, MSB first"""
    return torch.stack([(idx >> (bits - 1 - j)) & 1 for j in range(bits)], -1).bool()


def excluded_fraction(z64, m):
    """share of the bits of a case that a margin m excludes from the comparison, counted on the float64 logits alone"""
    return (z64.abs() <= m).double().mean().item()


def check_tokens(dev_idx, z64, m):
    """(bits differing where |z64| > m -- must be 0, bits differing inside the margin, share of bits inside the margin)"""
    bits = z64.shape[-1]
    diff = index_bits(dev_idx.long().cpu(), bits) != (z64 > 0)
    inside = z64.abs() <= m
    return int((diff & ~inside).sum()), int((diff & inside).sum()), inside.double().mean().item()


# ---------------------------------------------------------------------------------------------------- duration reduction, driver loop
def reduce_unfold(seq, n_gram=1):
    """the reference's formula, literally"""
    n_gram_seq = seq.unfold(0, n_gram, 1)
    mask = torch.all(n_gram_seq[1:] != n_gram_seq[:-1], dim=1)
    return torch.cat([n_gram_seq[0, :n_gram], n_gram_seq[1:, -1][mask]])


def reduce_ref(seq):
    return torch.unique_consecutive(seq)


def driver_logits(ssl_sd, head_sds, c, wave, overlap_rows):
    """the literal driver loop (30 s windows, the first `overlap_rows` rows of every later window dropped) over the float64
    yardstick: wave (L,) -> a list per head of z64 (rows, bits); every window is normalised, encoded and quantised on its own"""
    out = [[] for _ in head_sds]
    for start, n, drop in VC.driver_plan(wave.numel(), c["ssl"]["window_samples"], overlap_rows * SPR):
        h = ssl(ssl_sd, c, wave[start:start + n])
        for k, sd in enumerate(head_sds):
            out[k].append(logits(sd, convnext(sd, c["heads"][k], h))[drop:])
    return [torch.cat(v) for v in out]


# ---------------------------------------------------------------------------------------------------- bounds
def rel_rms(got, want):
    """RMS of (got - want) relative to max(1, RMS of want): the project's 1e-4 is absolute on O(1) values and relative on a larger stream"""
    want = want.double().cpu()
    return (got.double().cpu() - want).pow(2).mean().sqrt().item() / max(1.0, want.pow(2).mean().sqrt().item())


@functools.lru_cache(maxsize=None)
def cap16(name):
    """precision-1 caps: the error of this restatement run end to end in torch.float16 on the CPU, on the case's head inputs:
    dict(x, z) of the largest rel_rms over heads and lengths, and zmax = the largest |z16 - z64|"""
    k = case(name)
    ex = ez = zmax = 0.0
    for hk, sd in enumerate(k["heads"]):
        hc = k["cfg"]["heads"][hk]
        for h, x64, z64 in zip(k["h"], k["x"][hk], k["z"][hk]):
            x16 = convnext(sd, hc, h.half(), torch.float16)
            z16 = logits(sd, x16, torch.float16)
            ex, ez = max(ex, rel_rms(x16, x64)), max(ez, rel_rms(z16, z64))
            zmax = max(zmax, (z16.double() - z64).abs().max().item())
    return dict(x=ex, z=ez, zmax=zmax)


def rms_bound(name, precision, what):
    """min(cap, 4 x the largest value measured on MI355X); cap: 1e-4 (precision 0), the float16 restatement's error (precision 1)"""
    cap = 1e-4 if precision == 0 else cap16(name)[what]
    meas = MEASURED[name][precision][what]
    return cap if meas is None else min(cap, 4 * meas)


def block_bound(name, precision):
    """the block seam's bound: min(cap, 4 x measured) with the cap of ONE block: 1e-4, or the float16 restatement's error on the seam's
    own inputs"""
    cap = 1e-4 if precision == 0 else seam_case(name)["cap16"]
    return min(cap, 4 * MEASURED_BLOCK[name][precision])


# ---------------------------------------------------------------------------------------------------- shared, cached cases
@functools.lru_cache(maxsize=None)
def case(name):
    """name "S" | "F" -> dict(cfg, ssl_sd, heads [sd], T, h [list (T, Din)] head inputs, x [head][i] (T, dim), z [head][i] (T, bits)),
    float64 references computed once.  The head inputs have the scale of an SSL residual stream (RMS about 1)."""
    c = CFG_S if name == "S" else CFG_F
    ssl_sd = VC.make_state_dict(c["ssl"], seed=21 if name == "S" else 31)
    heads = [make_head_sd(c, k, seed=50 + 10 * (name == "F") + k) for k in range(2)]
    T = SEAM_T if name == "S" else HEAD_T
    g = torch.Generator().manual_seed(90 + (name == "F"))
    h = [torch.randn(t, c["ssl"]["d_model"], generator=g) for t in T]
    x = [[convnext(sd, c["heads"][k], t) for t in h] for k, sd in enumerate(heads)]
    z = [[logits(sd, t) for t in x[k]] for k, sd in enumerate(heads)]
    return dict(cfg=c, ssl_sd=ssl_sd, heads=heads, T=T, h=h, x=x, z=z)


@functools.lru_cache(maxsize=None)
def seam_case(name):
    """the block seam: head 0 of case `name` cut to ONE block on nine clips of SEAM_T rows -> dict(h [i] (T, Din), x [i] (T, dim) float64,
    cap16 = the largest rel_rms of the same block run in torch.float16 on the CPU)"""
    k = case(name)
    sd, hc = k["heads"][0], k["cfg"]["heads"][0]
    g = torch.Generator().manual_seed(11)
    h = [torch.randn(t, k["cfg"]["ssl"]["d_model"], generator=g) for t in SEAM_T]
    x = [convnext(sd, hc, t.double(), n_blocks=1) for t in h]
    cap = max(rel_rms(convnext(sd, hc, t.half(), torch.float16, n_blocks=1), w) for t, w in zip(h, x))
    return dict(h=h, x=x, cap16=cap)


@functools.lru_cache(maxsize=None)
def token_case():
    """config S through the SSL front: clips of TOKEN_LENS samples -> dict(waves, ssl [i] (rows, D), z [head][i] (rows, bits)) float64"""
    k = case("S")
    waves = [make_wave(n, 70 + i) for i, n in enumerate(TOKEN_LENS)]
    rows = [ssl(k["ssl_sd"], k["cfg"], w) for w in waves]
    z = [[logits(sd, convnext(sd, k["cfg"]["heads"][hk], r)) for r in rows] for hk, sd in enumerate(k["heads"])]
    return dict(waves=waves, ssl=rows, z=z)


@functools.lru_cache(maxsize=None)
def clip_case():
    """the four long clips of the one-call test: dict(buf (4, 60000) NaN above each end, z [clip][head] (rows, bits)) float64"""
    k = case("S")
    buf = torch.full((len(CLIP_LENS), 60000), float("nan"))
    for b, n in enumerate(CLIP_LENS):
        buf[b, :n] = make_wave(n, 20 + b)
    z = [driver_logits(k["ssl_sd"], k["heads"], k["cfg"], buf[b, :n], OV) for b, n in enumerate(CLIP_LENS)]
    return dict(buf=buf, z=z)
