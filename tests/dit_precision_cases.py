"""What the tests of the DiT's full-precision mode (precision 2, fp16x3: include/seedvc_hip.h) hold it to: the
float64 yardstick of the estimator and the sampler, the numpy statement of the split product, the float64 attention and the
committed error bounds.  Shared by test_host_dit_precision.py and test_gpu_dit_precision.py; needs no GPU.

The float64 yardstick is the oracle itself (oracle/seedvc_oracle.py), run on float64 copies of the weights and the inputs.  The
oracle casts every weight with `.float()`; `as_f64` hands it tensors whose `.float()` keeps float64, so those lines follow the
input dtype.  Two pieces of the oracle build float32 values from integers whatever the inputs are and are restated here
(`float64_oracle` swaps them in for the duration of a call and puts the oracle's own back):
  * `timestep_embed`: the sinusoid's ARGUMENT 1000 t f stays the float32 product the reference and the device form (t and the
    frequencies are float32 values; a float64 product would move the argument by 1000 x 2^-24, which is a property of the
    time grid, not of the estimator's arithmetic); cos / sin and the MLP are float64.
  * `rope_table`: the angles stay the float32 products the device's table is made from, cos / sin are taken in float64 and
    rounded once to float32 (v2: to bf16), which is how the device packs its table (csrc/dit.hip).
The time grid (`t_span_linear` / `t_span_cosine`) is float32 in the reference and on the device and is left as the oracle has it.
"""
import contextlib
import math

import numpy as np
import torch

import cases
import seedvc_oracle as O

# ---- the split product -------------------------------------------------------------------------------------------------
# v = hi + lo + r with hi = half(v), lo = half(v - hi): |lo| <= 2^-11 |v| and |r| <= 2^-11 |lo| <= 2^-22 |v| (values in fp16's normal
# range).  A product a b is taken as hi_a hi_b + lo_a hi_b + hi_a lo_b (each exact in fp32): what is missing is r_a b + a r_b (2 x
# 2^-22 |a b|) and lo_a lo_b (2^-22 |a b|).
X3_REL = 3 * 2.0 ** -22          # per-product relative error of the split, worst case
F32_EPS = 2.0 ** -24             # unit roundoff of the fp32 accumulation both share
X3_KS = (64, 512, 1536)          # reduction lengths: a head (attention), a hidden dim, an FFN width


def split_hi_lo(v):
    """float32 array -> (hi, lo) as float32 arrays holding fp16 values: hi = half(v), lo = half(v - float(hi))."""
    v = np.asarray(v, dtype=np.float32)
    hi = v.astype(np.float16).astype(np.float32)
    lo = (v - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def x3_matmul(a, b):
    """a [M][K], b [N][K] float32 -> a b^T as the device forms it: three products of fp16 planes, fp32 accumulation, the two
    correction products first."""
    ah, al = split_hi_lo(a)
    bh, bl = split_hi_lo(b)
    return ((al @ bh.T + ah @ bl.T) + ah @ bh.T).astype(np.float32)


def x3_operands(K, M=48, N=40):
    g = np.random.Generator(np.random.Philox(key=[0xD17, K]))
    return g.standard_normal((M, K)).astype(np.float32), g.standard_normal((N, K)).astype(np.float32)


# ---- float64 yardstick -------------------------------------------------------------------------------------------------
class _F64(torch.Tensor):
    """A float64 tensor whose `.float()` stays float64 (and so does everything computed from it)."""

    def float(self, *a, **k):
        return self


def as_f64(t):
    return t.detach().double().as_subclass(_F64)


def timestep_embed64(t, sd, prefix, freqs=None):
    if freqs is None:
        freqs = sd.get(prefix + ".freqs")
    if freqs is None:
        freqs = torch.exp(-math.log(10000) * torch.arange(0, 128, dtype=torch.float32) / 128)
    t32 = torch.as_tensor(t).detach().to(torch.float32).as_subclass(torch.Tensor)
    f32 = freqs.detach().to(torch.float32).as_subclass(torch.Tensor)
    args = (1000.0 * t32[:, None] * f32[None]).double()          # the float32 product, as the reference and the device form it
    emb = as_f64(torch.cat([torch.cos(args), torch.sin(args)], dim=-1))
    h = O.silu(O.linear(emb, sd, prefix + ".mlp.0"))
    return O.linear(h, sd, prefix + ".mlp.2")


def rope_table64(n_pos, head_dim=64, base=10000.0, bf16_round=False):
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2).to(torch.float32) / head_dim))
    ang = torch.outer(torch.arange(n_pos).to(torch.float32), inv).double()
    tab = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).to(torch.float32)
    if bf16_round:
        tab = tab.to(torch.bfloat16)
    return tab.double()


@contextlib.contextmanager
def float64_oracle():
    saved = O.timestep_embed, O.rope_table
    O.timestep_embed, O.rope_table = timestep_embed64, rope_table64
    try:
        yield
    finally:
        O.timestep_embed, O.rope_table = saved


def sd64(sd):
    return {k: as_f64(v) for k, v in sd.items()}


def estimator64(sd_f64, cfg, x, prompt_x, x_lens, t, style, mu):
    with float64_oracle():
        y = O.dit_forward(sd_f64, cfg, x.double(), prompt_x.double(), x_lens, t, style.double(), mu.double())
    return y.as_subclass(torch.Tensor)


def sampler64(sd_f64, cfg, z, T, prompt, mu, style, n_steps, cfg_rate, random_voice=False):
    with float64_oracle():
        y = O.cfm_sample(sd_f64, cfg, z.double(), T, prompt.double(), mu.double(), style.double(), n_steps, cfg_rate,
                         random_voice=random_voice)
    return y.as_subclass(torch.Tensor)


_ref = {}


def dit_reference(name):
    """(cfg, sd, inp, meta, est64, sample64) of `cases.dit_case(name)`: the float64 estimator output on the probe (x, t) and the
    float64 sampler output; computed once per process."""
    if name not in _ref:
        cfg, sd, inp, meta = cases.dit_case(name)
        s64 = sd64(sd)
        T, P = meta["T"], meta["P"]
        prompt_x = torch.zeros(1, cfg["C"], T)
        prompt_x[..., :P] = inp["prompt"]
        est = estimator64(s64, cfg, inp["x"], prompt_x, torch.LongTensor([T]), inp["t"], inp["style"], inp["mu"])
        smp = sampler64(s64, cfg, inp["z"], T, inp["prompt"], inp["mu"], inp["style"], meta["n_steps"], meta["cfg_rate"],
                        meta["random_voice"])
        _ref[name] = (cfg, sd, inp, meta, est, smp)
    return _ref[name]


# ---- committed bounds --------------------------------------------------------------------------------------
# Errors of precision 2 against the float64 yardstick over every case of cases.DIT_CASES.  Each bound is 4 x the worst value
# measured on the MI355X (the measured value is beside it); neither is derived from the code's output at test time.
P2_EST_MAXABS_MEASURED = 7.436e-06         # small_full (WaveNet head); precision 1 on the same case: 3.521e-03
P2_EST_MAXABS_BOUND = 4 * P2_EST_MAXABS_MEASURED
P2_SAMPLE_L1_MEASURED = 8.559e-07          # small_full; precision 1 on the same case: 3.835e-04
P2_SAMPLE_L1_BOUND = 4 * P2_SAMPLE_L1_MEASURED
# The cap: precision 2's error is at most this fraction of precision 1's on the same case.  Operand roundoff goes from 2^-11 to about
# 2^-21; the cap leaves a factor 20 for the fp32 arithmetic both share.
P2_CAP = 1.0 / 50.0
GOLDEN_MEL_L1 = 1e-3              # the existing bound against the reference's fp32 goldens (tests/test_gpu_dit.py)


# ---- attention op ------------------------------------------------------------------------------------------------------
ATTN_H, ATTN_SEQ_ROWS, ATTN_TQ = 2, 208, 200
# two launches of three sequences; between them kv_len 1, 63, 64, 65, 200 and q_start 0 and 130
ATTN_LAUNCHES = {"a": dict(kv_lens=[1, 63, 200], q_start=0), "b": dict(kv_lens=[64, 65, 200], q_start=130)}


def attention_case(name):
    """fp32 q, k, v (3, 208, 2, 64).  Logit scale differs by (sequence, head): some rows get one dominant key (scores spread
    over tens of units), some are near-uniform.  Rows at and above kv_len hold NaN in k and v."""
    spec = ATTN_LAUNCHES[name]
    n, R, H = len(spec["kv_lens"]), ATTN_SEQ_ROWS, ATTN_H
    q = cases.randn(f"attnx3.{name}.q", 7, n, R, H, 64)
    k = cases.randn(f"attnx3.{name}.k", 7, n, R, H, 64)
    v = cases.randn(f"attnx3.{name}.v", 7, n, R, H, 64)
    scale = torch.tensor([[4.0, 0.05], [1.0, 6.0], [0.02, 2.5]])[:n, :H]         # (sequence, head)
    q = q * scale[:, None, :, None]
    for s, L in enumerate(spec["kv_lens"]):
        k[s, L:] = float("nan")
        v[s, L:] = float("nan")
    return q, k, v, list(spec["kv_lens"]), spec["q_start"]


def attention_ref(q, k, v, kv_lens, dtype):
    """softmax(q k^T / 8 over keys < kv_len) v in `dtype`, every row; (n, R, H, 64)."""
    out = torch.zeros(q.shape, dtype=dtype)
    for s, L in enumerate(kv_lens):
        qs, ks, vs = (t[s, :, :, :].to(dtype).transpose(0, 1) for t in (q, k[:, :L], v[:, :L]))      # (H, rows, 64)
        p = torch.softmax(torch.matmul(qs, ks.transpose(-1, -2)) / 8.0, dim=-1)
        out[s] = torch.matmul(p, vs).transpose(0, 1)
    return out


def attention_x3_level(q, k, v, kv_lens):
    """The x3 level of the host test carried through the attention, per (sequence, head): a score moves by at most
    d = X3_REL max_keys sum_d |q_d k_d| / 8, the softmax weights by a factor within exp(+-2 d), the output by at most
    (exp(2 d) - 1) max|v|, and the PV product (P and V split) by X3_REL max|v| more."""
    lvl = torch.zeros(q.shape[0], 1, q.shape[2], 1, dtype=torch.float64)
    for s, L in enumerate(kv_lens):
        qa, ka, va = q[s].double().abs(), k[s, :L].double().abs(), v[s, :L].double().abs()
        d = X3_REL * torch.einsum("qhd,khd->hqk", qa, ka).amax(dim=(1, 2)) / 8.0          # (H,)
        vmax = va.amax(dim=(0, 2))
        lvl[s, 0, :, 0] = torch.expm1(2 * d) * vmax + X3_REL * vmax
    return lvl
