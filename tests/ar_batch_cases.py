"""Inputs shared by the batched-AR tests (test_host_ar_batch.py, test_gpu_ar_batch.py).

A free-running token comparison between the fp16-weight HIP model and the fp32 oracle only means something on sequences
whose every sampling decision survives the logit error the kernels are allowed (LOGIT_TOL x mean |logit|).  The sequences
below were chosen with the CPU probe that test_host_ar_batch.py keeps as a test: oracle weights rounded to fp16 plus
uniform noise of +- LOGIT_TOL x mean |logit| on every logit vector reproduces the oracle's tokens.  The winner's Exp(1)
draw of every step (and the EOS entry of the row that ends a sequence) is divided by BOOST, as cases.ar_gen_full_case
does; boosting a winner cannot change the oracle's trajectory.  Candidate b = 3 (5, 2) failed the probe and is left out."""
import functools

import torch

import cases
import seedvc_oracle as O
from seedvc_amd import specs, weights

LOGIT_TOL = 5e-3          # the bound tests/test_gpu_ar.py holds the logits to
SEED = 181
MAX_NEW = 40
BOOST = cases.AR_GEN_FULL_BOOST
CFG = dict(dim=128, n_head=2, n_local_heads=1, n_layer=3, intermediate_size=256, vocab_size=33, max_seq_len=160)
# b -> (condition frames, prompt tokens)
SEQS = {0: (7, 5), 1: (3, 0), 2: (9, 6), 4: (8, 1), 5: (4, 4), 6: (6, 3)}
# b -> tokens the oracle generates; fewer than MAX_NEW = the sequence ends by EOS
N_TOKENS = {0: 15, 1: 13, 2: 40, 4: 17, 5: 40, 6: 17}
ORDER = sorted(SEQS)


@functools.lru_cache(maxsize=None)
def model():
    c = specs.ar_config(**CFG)
    sd = weights.make_state_dict(specs.ar_state_spec(c), seed=SEED, prefix="ar.")
    return c, sd


def prompt(b, tt=None, tp=None):
    """(text (1, tt, dim), target (1, tp), plain Exp(1) draws (MAX_NEW + 1, vocab)) of sequence b."""
    c, _ = model()
    tt, tp = (tt, tp) if tt is not None else SEQS[b]
    text = cases.randn(f"arb.{b}.text", SEED + b, 1, tt, c["dim"])
    target = (cases.rand(f"arb.{b}.tgt", SEED + b, 1, tp) * (c["vocab_size"] - 1)).floor().long()
    noise = -torch.log(cases.rand(f"arb.{b}.expn", SEED + b, MAX_NEW + 1, c["vocab_size"]).clamp_min(1e-9))
    return text, target, noise


def oracle_tokens(sd, text, target, noise):
    c, _ = model()
    return O.ar_generate(sd, c, text, target, noise, max_iters=MAX_NEW - 1)


def boost(noise, tokens):
    """Divides the draw of every generated token, and of EOS in the row that ends the sequence, by BOOST."""
    c, _ = model()
    q = noise.clone()
    w = tokens.reshape(-1).long()
    q[torch.arange(w.numel()), w] /= BOOST
    if w.numel() < MAX_NEW:
        q[w.numel(), c["vocab_size"] - 1] /= BOOST
    return q


@functools.lru_cache(maxsize=None)
def sequence(b):
    """(text, target, boosted draws, reference tokens (1, n)) of qualified sequence b."""
    _, sd = model()
    text, target, noise = prompt(b)
    ref = oracle_tokens(sd, text, target, noise)
    return text, target, boost(noise, ref), ref
