"""Inputs shared by the v2 chain tests (test_host_v2_chain.py, test_gpu_v2_chain.py): reduced models of every link
(AR = ar_batch_cases.model(), both v2 length regulators, the v2_r DiT, the bigvgan_r2 vocoder), ragged utterances, the
oracle chain, a numpy Philox4x32-10 and the Kolmogorov-Smirnov statistic the seeded-sampling tests use.

The AR prompts of the chain come out of the AR length regulator, not out of ar_batch_cases.prompt, so they are qualified
here the way that module qualifies its own: oracle tokens first, the winners' draws divided by BOOST, then the CPU probe
(fp16-rounded matrices + uniform logit noise of LOGIT_TOL x mean |logit|, 10 trials) must reproduce the oracle's tokens.
CANDIDATES is a fixed list; `qualified()` keeps those that pass the probe, in list order."""
import functools

import numpy as np
import torch

import ar_batch_cases as A
import cases
import seedvc_oracle as O
from seedvc_amd import specs, weights
from seedvc_amd.pipeline import v2_ar_prompt, v2_target_frames

N_STEPS = 3
CFG_RATES = (0.7, 0.7)
# k -> (target narrow tokens Nn, source narrow tokens Ns, target prompt tokens Np, prompt frames P, frames per token)
CANDIDATES = {
    0: (5, 9, 4, 14, 1.37),
    1: (3, 6, 2, 9, 0.81),
    2: (7, 12, 6, 17, 1.9),
    3: (4, 8, 2, 11, 1.12),
    4: (6, 5, 5, 13, 0.55),
    5: (2, 11, 3, 16, 1.61),
    6: (8, 7, 1, 10, 2.2),
    7: (5, 10, 7, 12, 0.93),
}


@functools.lru_cache(maxsize=None)
def models():
    """dict of (config, state dict) for ar, ar_lr, cfm_lr, dit, voc."""
    c, sd = A.model()
    dcfg, dsd, _, _ = cases.dit_case("v2_r")
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")
    assert h["num_mels"] == dcfg["C"]
    alc = specs.lr_config("v2_ar", channels=c["dim"], codebook_size=32)
    alsd = weights.make_state_dict(specs.lr_state_spec(alc), seed=191, prefix="lr.")
    clc = specs.lr_config("v2_cfm", channels=64, codebook_size=32, out_channels=dcfg["Dc"])
    clsd = weights.make_state_dict(specs.lr_state_spec(clc), seed=192, prefix="lr.")
    return dict(ar=(c, sd), ar_lr=(alc, alsd), cfm_lr=(clc, clsd), dit=(dcfg, dsd), voc=(h, vsd))


def _tokens(tag, seed, n, codebook=32):
    return (cases.rand(tag, seed, 1, n) * codebook).long().clamp(max=codebook - 1)


@functools.lru_cache(maxsize=None)
def utterance(k):
    """Inputs of candidate k and its oracle AR run: plain and boosted draws, reference tokens, ylen."""
    M = models()
    c, sd = M["ar"]
    dcfg = M["dit"][0]
    Nn, Ns, Np, P, fpt = CANDIDATES[k]
    seed = 400 + k
    u = dict(k=k, P=P, frames_per_token=fpt,
             target_narrow=_tokens(f"v2c.{k}.tn", seed, Nn), src_narrow=_tokens(f"v2c.{k}.sn", seed, Ns),
             target_tokens=_tokens(f"v2c.{k}.tt", seed, Np), target_mel=cases.logmel(f"v2c.{k}.mel", seed, 1, dcfg["C"], P),
             style=cases.randn(f"v2c.{k}.style", seed, 1, dcfg["style_dim"]))
    narrow = v2_ar_prompt(u["target_narrow"], u["src_narrow"])
    u["ar_cond"] = O.lr_forward(M["ar_lr"][1], M["ar_lr"][0], narrow, narrow.size(1))
    noise = -torch.log(cases.rand(f"v2c.{k}.expn", seed, A.MAX_NEW + 1, c["vocab_size"]).clamp_min(1e-9))
    u["noise_plain"] = noise
    u["ref_tokens"] = A.oracle_tokens(sd, u["ar_cond"], u["target_tokens"], noise)
    u["noise"] = A.boost(noise, u["ref_tokens"])
    u["ylen"] = v2_target_frames(fpt, u["ref_tokens"].shape[1])
    u["z"] = cases.randn(f"v2c.{k}.z", seed, 1, dcfg["C"], P + u["ylen"])
    return u


def probe(k, trials=10):
    """The probe of test_host_ar_batch.py on candidate k: True when every noisy fp16 trial reproduces the oracle tokens."""
    c, sd = models()["ar"]
    u = utterance(k)
    if not torch.equal(A.oracle_tokens(sd, u["ar_cond"], u["target_tokens"], u["noise"]), u["ref_tokens"]):
        return False
    sd16 = {n: (v.half().float() if v.dim() == 2 and ("layers." in n or n == "model.output.weight") else v) for n, v in sd.items()}
    plain_forward = O.ar_forward_generate
    gen = torch.Generator().manual_seed(2000 + k)

    def noisy_forward(*args, **kw):
        lg = plain_forward(*args, **kw)
        amp = A.LOGIT_TOL * max(lg.abs().mean().item(), 1.0)
        return lg + (torch.rand(lg.shape, generator=gen) * 2 - 1) * amp

    O.ar_forward_generate = noisy_forward
    try:
        for _ in range(trials):
            got = A.oracle_tokens(sd16, u["ar_cond"], u["target_tokens"], u["noise"])
            if got.shape != u["ref_tokens"].shape or not torch.equal(got, u["ref_tokens"]):
                return False
    finally:
        O.ar_forward_generate = plain_forward
    return True


@functools.lru_cache(maxsize=None)
def qualified():
    return tuple(k for k in CANDIDATES if probe(k))


@functools.lru_cache(maxsize=None)
def oracle_chain(k):
    """Reference of utterance k: O.lr_forward -> O.ar_generate -> O.lr_forward -> O.cfm_sample -> O.bigvgan_forward.
    -> (tokens (1, n), ylen, mel (1, C, ylen))."""
    M = models()
    u = utterance(k)
    toks, ylen, P = u["ref_tokens"], u["ylen"], u["P"]
    clc, clsd = M["cfm_lr"]
    dcfg, dsd = M["dit"]
    pc = O.lr_forward(clsd, clc, u["target_tokens"], P)
    cond = O.lr_forward(clsd, clc, toks, ylen)
    mu = torch.cat([pc, cond], dim=1)
    mel = O.cfm_sample(dsd, dcfg, u["z"], P + ylen, u["target_mel"], mu, u["style"], N_STEPS, list(CFG_RATES))[:, :, P:]
    return toks, ylen, mel


# ---------------------------------------------------------------------------------------------- seeded draws: references
def philox4x32_10(counter, key):
    """counter (..., 4), key (2,) uint32 -> (..., 4) uint32 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3")."""
    c = np.asarray(counter, dtype=np.uint64) & 0xFFFFFFFF
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def reference_uniforms(seed, step0, n_steps, vocab):
    """u (n_steps, vocab) float64 of the layout DESIGN.md documents: key = (seed low, seed high), counter = (v // 4, step, 0, 0),
    word v % 4, u = ((word >> 8) + 1) / 2^24."""
    n4 = (vocab + 3) // 4
    ctr = np.zeros((n_steps, n4, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(n4)[None, :]
    ctr[..., 1] = (step0 + np.arange(n_steps))[:, None]
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(n_steps, n4 * 4)[:, :vocab]
    return ((w >> 8).astype(np.float64) + 1.0) / 2.0 ** 24


def ks_exp1(q):
    """Kolmogorov-Smirnov statistic of the sample q against Exp(1), cdf 1 - exp(-q)."""
    x = np.sort(np.asarray(q, dtype=np.float64).reshape(-1))
    n = x.size
    cdf = 1.0 - np.exp(-x)
    i = np.arange(1, n + 1)
    return float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()))


def ks_critical(n):
    """0.1 % critical value of the KS statistic for large n: 1.95 / sqrt(n)."""
    return 1.95 / np.sqrt(n)
