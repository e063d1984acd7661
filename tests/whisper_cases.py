"""Cases and the yardstick of the Whisper content encoder tests (csrc/whisper.hip, seedvc_amd/whisper.py).

The yardstick is a plain-torch restatement of the log-mel front-end and of the encoder, run in float64; test_host_whisper.py pins
it to transformers' `WhisperFeatureExtractor` and `WhisperEncoder`, the GPU tests use only the restatement.  The same code with
`attn16=True` rounds q, k, v and the softmax weights to fp16 (what the device's precision 0 does by design), with `gemm16=True`
every GEMM operand, and with `dtype=torch.float16` it is the reference's own arithmetic (the drivers run the encoder in float16).

Weights are not the HF initialisation (std 0.02 makes every branch negligible beside the residual and would hide attention or
FFN mistakes): matrices and conv kernels N(0, 1 / fan_in), biases 0.1 N(0, 1), LayerNorm weights 1 + 0.1 N(0, 1), and the
sinusoidal `embed_positions` HF builds.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

torch.set_grad_enabled(False)

SPR = 320
CFG_S = dict(n_mels=80, d_model=128, n_heads=2, n_layers=2, ffn_dim=512, max_source_positions=100)
CFG_F = dict(n_mels=80, d_model=768, n_heads=12, n_layers=12, ffn_dim=3072, max_source_positions=1500)

# Asserted error bounds of the encoder, RMS of (device - float64) over all outputs.  Precision 0: the project's bound
# 1e-4; precision 1: the RMS error of this restatement run end to end in torch.float16 on the CPU (test_host_whisper.py computes
# it and checks the constants below against it); in each mode the smaller of that cap and 4 x the largest value measured on MI355X.
RMS_BOUND = {0: 1.0e-4, 1: 8.5e-4}


def state_spec(c):
    from seedvc_amd import specs
    return specs.whisper_state_spec(c)


def sinusoids(length, channels, max_timescale=10000.0):
    """`transformers.models.whisper.modeling_whisper.sinusoids`, restated"""
    inc = math.log(max_timescale) / (channels // 2 - 1)
    inv = torch.exp(-inc * torch.arange(channels // 2))
    t = torch.arange(length).view(-1, 1) * inv.view(1, -1)
    return torch.cat([t.sin(), t.cos()], dim=1)


def make_state_dict(c, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shp in state_spec(c).items():
        if k == "embed_positions.weight":
            sd[k] = sinusoids(*shp).float()
        elif "layer_norm" in k:
            sd[k] = (1.0 if k.endswith("weight") else 0.0) + 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        else:
            sd[k] = torch.randn(shp, generator=g) / math.sqrt(float(np.prod(shp[1:])))
    return sd


def make_wave(n, seed):
    """a voiced-like test signal: a few drifting partials under an envelope, plus noise"""
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.arange(n, dtype=torch.float64) / 16000.0
    f0 = 110.0 * (1 + seed % 5) * (1.0 + 0.1 * torch.sin(2 * math.pi * 0.7 * t))
    ph = 2 * math.pi * torch.cumsum(f0, 0) / 16000.0
    y = sum(torch.sin(k * ph) / k for k in range(1, 6)) * (0.55 + 0.45 * torch.sin(2 * math.pi * 1.3 * t + seed))
    y = 0.2 * y + 0.02 * torch.randn(n, generator=g, dtype=torch.float64)
    return y.float()


def mel_basis64(n_mels=80):
    from seedvc_amd.audio import whisper_mel_basis
    return whisper_mel_basis(n_mels).double()


def log_mel(wave, P, basis, dtype=torch.float64):
    """wave (n <= 320 P,) -> (n_mels, 2 P): WhisperFeatureExtractor's features of the clip zero-padded to one window"""
    W = P * SPR
    x = torch.zeros(W, dtype=dtype)
    x[:wave.numel()] = wave.to(dtype)
    xp = F.pad(x.view(1, 1, -1), (200, 200), mode="reflect").view(-1)
    frames = xp.unfold(0, 400, 160) * torch.hann_window(400, periodic=True, dtype=dtype)
    spec = torch.fft.rfft(frames, dim=-1)
    power = (spec.real ** 2 + spec.imag ** 2)[:-1]                 # the last of the 2 P + 1 frames is dropped
    mel = basis.to(dtype) @ power.T
    lg = torch.log10(torch.clamp(mel, min=1e-10))
    lg = torch.maximum(lg, lg.max() - 8.0)
    return (lg + 4.0) / 4.0


def mel_power(wave, P, basis):
    """the linear mel power (n_mels, 2 P) in float64 (for the relative bound on the linear scale)"""
    W = P * SPR
    x = torch.zeros(W, dtype=torch.float64)
    x[:wave.numel()] = wave.double()
    xp = F.pad(x.view(1, 1, -1), (200, 200), mode="reflect").view(-1)
    spec = torch.fft.rfft(xp.unfold(0, 400, 160) * torch.hann_window(400, periodic=True, dtype=torch.float64), dim=-1)
    return basis.double() @ (spec.real ** 2 + spec.imag ** 2)[:-1].T


def encoder(sd, c, feats, dtype=torch.float64, attn16=False, gemm16=False, gelu="none", branches=None):
    """feats (B, n_mels, 2 P) -> (B, P, D).  attn16: q, k, v and the softmax weights rounded to fp16; gemm16: every GEMM operand
    rounded to fp16; gelu: "none" = exact erf form, "tanh" = the approximation (a deliberately wrong network for the tests);
    branches: optional list that receives (branch RMS, residual RMS) per half layer."""
    D, H = c["d_model"], c["n_heads"]
    r16 = lambda t: t.half().to(dtype)                              # noqa: E731
    ga = (lambda t: r16(t)) if gemm16 else (lambda t: t)           # noqa: E731
    w = lambda k: sd[k].to(dtype)                                   # noqa: E731
    lin = lambda x, p, bias=True: F.linear(ga(x), ga(w(p + ".weight")), w(p + ".bias") if bias else None)   # noqa: E731
    act = lambda t: F.gelu(t, approximate=gelu)                     # noqa: E731
    x = act(F.conv1d(ga(feats.to(dtype)), ga(w("conv1.weight")), w("conv1.bias"), padding=1))
    x = act(F.conv1d(ga(x), ga(w("conv2.weight")), w("conv2.bias"), stride=2, padding=1))
    x = x.permute(0, 2, 1) + w("embed_positions.weight")
    B, P, _ = x.shape
    heads = lambda t: t.view(B, P, H, 64).transpose(1, 2)           # noqa: E731
    for i in range(c["n_layers"]):
        p = f"layers.{i}."
        h = F.layer_norm(x, (D,), w(p + "self_attn_layer_norm.weight"), w(p + "self_attn_layer_norm.bias"), 1e-5)
        q, k, v = heads(lin(h, p + "self_attn.q_proj") * 0.125), heads(lin(h, p + "self_attn.k_proj", False)), heads(lin(h, p + "self_attn.v_proj"))
        if attn16 or gemm16:
            q, k, v = r16(q), r16(k), r16(v)
        s = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
        if attn16 or gemm16:
            s = r16(s)
        a = lin((s @ v).transpose(1, 2).reshape(B, P, D), p + "self_attn.out_proj")
        if branches is not None:
            branches.append((a.double().pow(2).mean().sqrt().item(), x.double().pow(2).mean().sqrt().item()))
        x = x + a
        h = F.layer_norm(x, (D,), w(p + "final_layer_norm.weight"), w(p + "final_layer_norm.bias"), 1e-5)
        f = lin(act(lin(h, p + "fc1")), p + "fc2")
        if branches is not None:
            branches.append((f.double().pow(2).mean().sqrt().item(), x.double().pow(2).mean().sqrt().item()))
        x = x + f
    return F.layer_norm(x, (D,), w("layer_norm.weight"), w("layer_norm.bias"), 1e-5)


def rms(a, b):
    return (a.double().cpu() - b.double().cpu()).pow(2).mean().sqrt().item()


def driver_plan(L, W, O):
    """The drivers' loop over the windows of a long clip, literally (inference.py: `if waves_16k.size(-1) <= 16000 * 30` ... else
    `while traversed_time < waves_16k.size(-1)`): a list of (start, samples, rows dropped at the front)."""
    if L <= W:
        return [(0, L, 0)]
    plan, traversed, first = [], 0, True
    while traversed < L:
        if first:
            start, n, drop = 0, min(W, L), 0
            traversed += W
            first = False
        else:
            start = traversed - O
            n, drop = min(L, traversed + W - O) - start, O // SPR
            traversed += n - O
        plan.append((start, n, drop))
    return plan


def driver_content(sd, c, wave, overlap_rows, basis):
    """the literal driver loop over the float64 restatement: wave (L,) -> (rows, D)"""
    P = c["max_source_positions"]
    out = []
    for start, n, drop in driver_plan(wave.numel(), P * SPR, overlap_rows * SPR):
        e = encoder(sd, c, log_mel(wave[start:start + n], P, basis)[None])[0]
        out.append(e[drop:n // SPR + 1])
    return torch.cat(out)


# ---- shared, cached cases (computed once per process, never modified)
S_LENS = (20000, 32000, 513)                       # the mel seam's three clips


@functools.lru_cache(maxsize=None)
def case(name):
    """name "S" | "F" -> dict(cfg, sd, waves [list], feats (B, n_mels, 2 P) float64, ref (B, P, D) float64)"""
    c = CFG_S if name == "S" else CFG_F
    P = c["max_source_positions"]
    sd = make_state_dict(c, seed=11 if name == "S" else 12)
    basis = mel_basis64(c["n_mels"])
    lens = S_LENS if name == "S" else (301234,)
    waves = [make_wave(n, i) for i, n in enumerate(lens)]
    feats = torch.stack([log_mel(w, P, basis) for w in waves])
    return dict(cfg=c, sd=sd, waves=waves, lens=lens, feats=feats, ref=encoder(sd, c, feats), basis=basis)
