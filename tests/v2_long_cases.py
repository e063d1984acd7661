"""Inputs shared by the whole-file v2 tests (test_host_v2_long.py, test_gpu_v2_long.py): files on the reduced models of
v2_chain_cases (AR with 160 positions, MAX_NEW 40, hop 8), cut into AR chunks by `pipeline.v2_chunk_plan`, the oracle
chain restated per chunk, and the host statements of the seam rule.

Every chunk's AR prompt is qualified the way v2_chain_cases qualifies an utterance: oracle tokens first, the winners'
draws divided by BOOST, then the CPU probe (fp16-rounded matrices + uniform logit noise of LOGIT_TOL x mean |logit|, 10
trials, generator seed 3000 + 10 f + j for chunk j of file f) must reproduce the oracle's tokens.  A file is used only if
all its chunks qualify; `qualified()` keeps those files, in table order."""
import functools

import numpy as np
import torch

import ar_batch_cases as A
import cases
import long_batch_cases as LB
import seedvc_oracle as O
import v2_chain_cases as V
from seedvc_amd.pipeline import stream_wave_chunks, v2_ar_prompt, v2_chunk_plan, v2_seam_plan, v2_target_frames

HOP = 8
N_STEPS = V.N_STEPS
CFG_RATES = V.CFG_RATES
# f -> (target narrow tokens Nn, source narrow tokens Ns, target prompt tokens Np, chunk_tokens, frames per token)
FILES = {
    0: (5, 23, 4, 9, 1.37),
    1: (3, 20, 2, 7, 0.81),
    2: (7, 31, 6, 12, 1.9),
    3: (4, 16, 3, 8, 1.12),
    4: (6, 27, 5, 9, 0.9),
    5: (2, 18, 3, 6, 1.6),
}
PROMPT_FRAMES = {f: 10 + f for f in FILES}                      # P: frames of the target mel
WIDE_TOKENS = {f: FILES[f][1] + 5 + f for f in FILES}           # Nw: wide source tokens (the timbre branch)
models = V.models


def _exp_draws(f, j):
    vocab = V.models()["ar"][0]["vocab_size"]
    return -torch.log(cases.rand(f"v2l.{f}.{j}.expn", 700 + f, A.MAX_NEW + 1, vocab).clamp_min(1e-9))


def _probe(ar_cond, target_tokens, noise, ref, gen_seed, trials=10):
    """The probe of v2_chain_cases.probe on one AR prompt: True when every noisy fp16 trial reproduces the oracle tokens."""
    c, sd = V.models()["ar"]
    if not torch.equal(A.oracle_tokens(sd, ar_cond, target_tokens, noise), ref):
        return False
    sd16 = {n: (v.half().float() if v.dim() == 2 and ("layers." in n or n == "model.output.weight") else v) for n, v in sd.items()}
    plain_forward = O.ar_forward_generate
    gen = torch.Generator().manual_seed(gen_seed)

    def noisy_forward(*args, **kw):
        lg = plain_forward(*args, **kw)
        amp = A.LOGIT_TOL * max(lg.abs().mean().item(), 1.0)
        return lg + (torch.rand(lg.shape, generator=gen) * 2 - 1) * amp

    O.ar_forward_generate = noisy_forward
    try:
        for _ in range(trials):
            got = A.oracle_tokens(sd16, ar_cond, target_tokens, noise)
            if got.shape != ref.shape or not torch.equal(got, ref):
                return False
    finally:
        O.ar_forward_generate = plain_forward
    return True


def _chunk(f, j, narrow, target_tokens, fpt, P, gen_seed):
    """One AR prompt and its oracle run: condition, boosted draws, reference tokens, ylen, sampler noise, probe verdict."""
    M = models()
    _, sd = M["ar"]
    ar_cond = O.lr_forward(M["ar_lr"][1], M["ar_lr"][0], narrow, narrow.size(1))
    plain = _exp_draws(f, j)
    ref = A.oracle_tokens(sd, ar_cond, target_tokens, plain)
    noise = A.boost(plain, ref)
    ylen = v2_target_frames(fpt, ref.shape[1])
    return dict(ar_cond=ar_cond, noise=noise, ref_tokens=ref, ylen=ylen,
                z=cases.randn(f"v2l.{f}.{j}.z", 700 + f, 1, M["dit"][0]["C"], P + ylen),
                ok=_probe(ar_cond, target_tokens, noise, ref, gen_seed))


@functools.lru_cache(maxsize=None)
def file_inputs(f):
    """Tokens, target mel and style of file f (no oracle run)."""
    dcfg = models()["dit"][0]
    Nn, Ns, Np, chunk_tokens, fpt = FILES[f]
    seed, P = 700 + f, PROMPT_FRAMES[f]
    return dict(f=f, P=P, chunk_tokens=chunk_tokens, frames_per_token=fpt,
                target_narrow=V._tokens(f"v2l.{f}.tn", seed, Nn), src_narrow=V._tokens(f"v2l.{f}.sn", seed, Ns),
                target_tokens=V._tokens(f"v2l.{f}.tt", seed, Np), src_tokens=V._tokens(f"v2l.{f}.sw", seed, WIDE_TOKENS[f]),
                target_mel=cases.logmel(f"v2l.{f}.mel", seed, 1, dcfg["C"], P), style=cases.randn(f"v2l.{f}.style", seed, 1, dcfg["style_dim"]))


@functools.lru_cache(maxsize=None)
def file_case(f):
    """file_inputs(f) plus `chunks`: the oracle AR run of every chunk of `v2_chunk_plan(Ns, chunk_tokens)`."""
    u = dict(file_inputs(f))
    u["chunks"] = [_chunk(f, j, v2_ar_prompt(u["target_narrow"], u["src_narrow"][:, p0:p0 + n]), u["target_tokens"],
                          u["frames_per_token"], u["P"], 3000 + 10 * f + j)
                   for j, (p0, n, _) in enumerate(v2_chunk_plan(u["src_narrow"].size(1), u["chunk_tokens"]))]
    return u


@functools.lru_cache(maxsize=None)
def qualified():
    return tuple(f for f in FILES if all(c["ok"] for c in file_case(f)["chunks"]))


@functools.lru_cache(maxsize=None)
def anonymized_case():
    """The first qualified file whose chunks also qualify as prompts WITHOUT target tokens (condition = the range alone,
    empty prompt target; probe seeds 3500 + 10 f + j): (file_inputs, chunks), or None."""
    none = torch.zeros(1, 0, dtype=torch.int64)
    for f in qualified():
        u = file_inputs(f)
        chunks = []
        for j, (p0, n, _) in enumerate(v2_chunk_plan(u["src_narrow"].size(1), u["chunk_tokens"])):
            chunks.append(_chunk(f, j, u["src_narrow"][:, p0:p0 + n], none, u["frames_per_token"], u["P"], 3500 + 10 * f + j))
            if not chunks[-1]["ok"]:
                break
        if all(c["ok"] for c in chunks):
            return u, chunks
    return None


@functools.lru_cache(maxsize=None)
def oracle_chunk(f, j, anonymized=False):
    """`v2_chain_cases.oracle_chain` for chunk j of file f: O.lr_forward -> O.cfm_sample on the oracle's tokens.
    -> (tokens (1, n), ylen, mel (1, C, ylen)); the wave reference is the oracle vocoder on the mel under test, as there."""
    M = models()
    u = file_inputs(f)
    c = (anonymized_case()[1] if anonymized else file_case(f)["chunks"])[j]
    clc, clsd = M["cfm_lr"]
    dcfg, dsd = M["dit"]
    P, ylen = u["P"], c["ylen"]
    pc = O.lr_forward(clsd, clc, u["target_tokens"], P)
    cond = O.lr_forward(clsd, clc, c["ref_tokens"], ylen)
    mel = O.cfm_sample(dsd, dcfg, c["z"], P + ylen, u["target_mel"], torch.cat([pc, cond], dim=1), u["style"], N_STEPS,
                       list(CFG_RATES))[:, :, P:]
    return c["ref_tokens"], ylen, mel


# ------------------------------------------------------------------------------------------- the seam rule, on the host
def stream_reference(waves, overlap_frame_len, hop):
    """`pipeline.stream_wave_chunks` run in order over the chunk waves of ONE file (1-D float32 arrays, each frames x hop
    samples), the last of them flagged last -> the file's samples.  The inputs are copied: `crossfade` works in place."""
    chunks, previous, processed = [], None, 0
    for i, w in enumerate(waves):
        processed, previous, _ = stream_wave_chunks(torch.from_numpy(np.array(w, dtype=np.float32))[None], processed, len(w) // hop,
                                                    overlap_frame_len * hop, overlap_frame_len, chunks, previous, i == len(waves) - 1)
    return np.concatenate(chunks).astype(np.float32) if chunks else np.zeros(0, np.float32)


def seam_model(waves, chunk_files, is_last, ov, n_files):
    """The numpy statement of what the style branch assembles: `v2_seam_plan`'s flags, then the `svc_chunks_assemble`
    formula (long_batch_cases.assemble_model) over the kept chunks.  waves: 1-D float32 arrays, file-major.
    -> (list of one array per file, the plan)."""
    lens = [len(w) for w in waves]
    plan = v2_seam_plan(chunk_files, lens, is_last, ov, n_files)
    kept = [k for k in range(len(waves)) if plan["kept"][k]]
    flat = np.zeros(0, np.float32)
    if kept:
        flat = LB.assemble_model(LB.padded_rows([waves[k] for k in kept], max(lens) + 3), [lens[k] for k in kept],
                                 [plan["first"][k] for k in kept], [plan["last"][k] for k in kept], ov)
    offs = np.cumsum([0] + plan["out_lens"])
    assert offs[-1] == len(flat)
    return [flat[offs[u]:offs[u + 1]] for u in range(n_files)], plan
