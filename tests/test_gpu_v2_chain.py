"""GPU tests of the v2 chain: seeded on-device sampling (`svc_ar_generate_batch_seeded`, `svc_ar_exp_draws`), the ragged
assembly calls (`svc_v2_assemble_cond`, `svc_mel_strip_prompt`) and `pipeline.V2HotPath` (tokens in, audio out) against
the oracle chain.  The seeded path is reduced to the explicit-noise path, which tests/test_gpu_ar_batch.py pins: the
draws of a seed, handed back as `exp_noise`, must give the same tokens bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import ar_batch_cases as A
import cases
import seedvc_oracle as O
import v2_chain_cases as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SPREAD_40 = (0, 9, 17, 26, 33, 39)
SEEDS = {b: 0x9E3779B97F4A7C15 * (b + 1) % 2 ** 64 for b in A.ORDER}      # high and low words both in use


def _ar(c, sd, max_batch):
    from seedvc_amd.ar import ARModel
    m = ARModel(c, sd, "cuda:0")
    m.setup_caches(max_batch_size=max_batch)
    return m


def _seeded(m, order, seeds=SEEDS, check_every=16, max_new=A.MAX_NEW):
    seqs = [A.sequence(b) for b in order]
    out = m.generate_batch([s[0].cuda() for s in seqs], [s[1].cuda() for s in seqs], seeds=[seeds[b] for b in order],
                           max_new=max_new, check_every=check_every)
    return [t.cpu() for t in out]


# --------------------------------------------------------------------------------------------------- 1. seeded == explicit
def test_seeded_equals_explicit_draws():
    c, sd = A.model()
    m = _ar(c, sd, len(A.ORDER))
    seqs = [A.sequence(b) for b in A.ORDER]
    got = _seeded(m, A.ORDER)
    draws = [m.exp_draws(SEEDS[b], 0, A.MAX_NEW) for b in A.ORDER]
    want = m.generate_batch([s[0].cuda() for s in seqs], [s[1].cuda() for s in seqs], exp_noise=draws, max_new=A.MAX_NEW)
    for b, g, w in zip(A.ORDER, got, want):
        print(f"sequence {b}: {g.shape[1]} tokens seeded, {w.shape[1]} explicit")
        assert g.shape[1] >= 10 and torch.equal(g, w.cpu()), f"sequence {b}: {g.tolist()} vs {w.tolist()}"
    # the draws as one (B, max_new, vocab) tensor, the layout of the C call, are taken as they are
    stacked = m.generate_batch([s[0].cuda() for s in seqs], [s[1].cuda() for s in seqs], exp_noise=torch.stack(draws), max_new=A.MAX_NEW)
    assert all(torch.equal(g, w.cpu()) for g, w in zip(got, stacked))
    # step0: rows of a later window are the same draws
    assert torch.equal(m.exp_draws(SEEDS[0], 7, 5), draws[0][7:12])


def test_seeded_equals_explicit_draws_full_size():
    c, sd, text, target, _ = cases.ar_gen_full_case()
    m = _ar(c, sd, 2)
    n = cases.AR_GEN_FULL_TOKENS
    seeds = [1234, 2 ** 63 + 5]
    got = m.generate_batch([text.cuda()] * 2, [target.cuda()] * 2, seeds=seeds, max_new=n)
    want = m.generate_batch([text.cuda()] * 2, [target.cuda()] * 2, exp_noise=[m.exp_draws(s, 0, n) for s in seeds], max_new=n)
    for g, w in zip(got, want):
        print(f"ar_gen_full, seeded: {g.shape[1]} tokens")
        assert 10 <= g.shape[1] <= n and g.shape == w.shape and torch.equal(g, w)
    assert got[0].shape != got[1].shape or not torch.equal(got[0], got[1])
    one = m.generate(text.cuda(), target.cuda(), seed=seeds[1], max_new=n)          # B = 1 is slot 0 of the same call
    assert torch.equal(one, got[1])


# ------------------------------------------------------------------------------------------------ 2. invariance with seeds
def test_seeded_invariance():
    c, sd = A.model()
    m = _ar(c, sd, 40)
    base = _seeded(m, A.ORDER)
    perm = [A.ORDER[i] for i in (3, 0, 5, 1, 4, 2)]
    for b, t in zip(perm, _seeded(m, perm)):
        assert torch.equal(t, base[A.ORDER.index(b)]), f"permuted: sequence {b}"
    order40 = [A.ORDER[j % len(A.ORDER)] for j in range(40)]
    for slot, b in zip(SPREAD_40, A.ORDER):
        order40[slot] = b
    in40 = _seeded(m, order40)
    for k, b in enumerate(A.ORDER):
        alone = _seeded(m, [b])[0]
        assert torch.equal(alone, base[k]) and torch.equal(alone, in40[SPREAD_40[k]]), f"sequence {b}"
    for a, b in zip(base, _seeded(m, A.ORDER, check_every=1)):
        assert torch.equal(a, b)
    for a, b in zip(base, _seeded(m, A.ORDER)):
        assert torch.equal(a, b)
    other = _seeded(m, A.ORDER, seeds={b: s + 1 for b, s in SEEDS.items()})
    assert any(not torch.equal(a, b) for a, b in zip(base, other))


def test_unseeded_generation_follows_torch_manual_seed():
    c, sd = A.model()
    m = _ar(c, sd, 2)
    text, target = A.sequence(0)[0].cuda(), A.sequence(0)[1].cuda()
    torch.manual_seed(5)
    a = m.generate_batch([text] * 2, [target] * 2, max_new=A.MAX_NEW)
    torch.manual_seed(5)
    b = m.generate_batch([text] * 2, [target] * 2, max_new=A.MAX_NEW)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], a[1])          # two sequences of one call get different seeds


# ---------------------------------------------------------------------------------------------------- 3. the draws are Exp(1)
def test_draws_are_exponential():
    from seedvc_amd import specs, weights
    c = specs.ar_config(dim=128, n_head=2, n_local_heads=1, n_layer=1, intermediate_size=256, vocab_size=2049, max_seq_len=64)
    m = _ar(c, weights.make_state_dict(specs.ar_state_spec(c), seed=7, prefix="ar."), 1)
    seed, steps, Vv = 0xC0FFEE1234567890, 64, 2049
    q = m.exp_draws(seed, 0, steps).cpu().numpy().astype(np.float64)
    q2 = m.exp_draws(seed + 1, 0, steps).cpu().numpy().astype(np.float64)
    n = q.size
    assert q.shape == (steps, Vv) and n == 131136
    assert np.isfinite(q).all() and (q >= 0).all()
    d = V.ks_exp1(q)
    r_seed = abs(np.corrcoef(q.reshape(-1), q2.reshape(-1))[0, 1])
    r_step = abs(np.corrcoef(q[:-1].reshape(-1), q[1:].reshape(-1))[0, 1])
    print(f"KS {d:.5f} (bound {V.ks_critical(n):.5f}); |corr| seeds {r_seed:.5f}, adjacent steps {r_step:.5f} (bound {4 / np.sqrt(n):.5f})")
    assert d < V.ks_critical(n)
    assert r_seed < 4 / np.sqrt(n) and r_step < 4 / np.sqrt(n)
    u = V.reference_uniforms(seed, 0, steps, Vv)
    rel = np.abs(np.exp(-q) - u) / u
    print(f"exp(-q) vs numpy Philox4x32-10: max relative error {rel.max():.2e}")
    assert rel.max() < 1e-6
    u5 = V.reference_uniforms(seed, 5, 2, Vv)
    q5 = m.exp_draws(seed, 5, 2).cpu().numpy().astype(np.float64)
    assert (np.abs(np.exp(-q5) - u5) / u5).max() < 1e-6


# --------------------------------------------------------------------------------------------------------- 4. no noise tensor
def test_seeded_generation_allocates_no_noise_tensor():
    c, sd, text, target, _ = cases.ar_gen_case("ar_gen_r")
    B = 8
    m = _ar(c, sd, B)
    texts, targets = [text.cuda()] * B, [target.cuda()] * B
    S = text.size(1) + 2 + target.size(1)
    max_new = min(4001, c["max_seq_len"] - S + 1)
    noise_bytes = B * max_new * c["vocab_size"] * 4
    m.generate_batch(texts, targets, seeds=list(range(B)))          # workspaces and graphs exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = m.generate_batch(texts, targets, seeds=list(range(B)))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"seeded generate_batch: peak rise {rise} B; the explicit path's noise tensor alone is {noise_bytes} B")
    assert rise < noise_bytes
    assert all(t.shape[1] >= 1 for t in out)


# ------------------------------------------------------------------------------------------------------------ ragged kernels
def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


@pytest.mark.parametrize("Dc", [512, 6, 13])
def test_assemble_cond_matches_indexing(Dc):
    from seedvc_amd import _lib
    B, Pmax, Smax = 5, 9, 11
    P, S = [0, 1, 9, 5, 3], [11, 0, 7, 1, 0]
    T = max(p + s for p, s in zip(P, S)) + 2
    pc, cd = cases.randn("asm.pc", Dc, B, Pmax, Dc), cases.randn("asm.cd", Dc, B, Smax, Dc)
    out = torch.full((B, T, Dc), float("nan"), device="cuda")
    pcd, cdd = pc.cuda(), cd.cuda()
    _lib.check(_lib.lib().svc_v2_assemble_cond(_lib.ptr(pcd), _i32(P), _lib.ptr(cdd), _i32(S), B, Pmax, Smax, Dc, T, _lib.ptr(out),
                                               _lib.stream_ptr()))
    want = torch.zeros(B, T, Dc)
    for b in range(B):
        want[b, :P[b] + S[b]] = torch.cat([pc[b, :P[b]], cd[b, :S[b]]])
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("Cm,Smax", [(80, 12), (80, 11), (7, 12), (5, 9)])
def test_strip_prompt_matches_indexing(Cm, Smax):
    from seedvc_amd import _lib
    B, T = 5, 23
    P = [0, 1, 11, 5, 4]
    n = [Smax, 0, 7, 1, 3]                       # frames kept: full, none, odd, one
    x_lens = [p + k for p, k in zip(P, n)]
    x_lens[1] = 0                                # x_len below the prompt length: nothing kept
    assert max(x_lens) <= T
    mel = cases.randn("strip.mel", Cm * 100 + Smax, B, Cm, T)
    out = torch.full((B, Cm, Smax), float("nan"), device="cuda")
    md = mel.cuda()
    pad = -11.5
    _lib.check(_lib.lib().svc_mel_strip_prompt(_lib.ptr(md), _i32(P), _i32(x_lens), B, Cm, T, Smax, C.c_float(pad), _lib.ptr(out),
                                               _lib.stream_ptr()))
    want = torch.full((B, Cm, Smax), pad)
    for b in range(B):
        if n[b] and x_lens[b] > P[b]:
            want[b, :, :n[b]] = mel[b, :, P[b]:x_lens[b]]
    assert torch.equal(out.cpu(), want)


# --------------------------------------------------------------------------------------------------------------------- chain
def _hotpath(max_batch=4):
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath
    from seedvc_amd.vocoder import BigVGAN
    M = V.models()
    ar = _ar(*M["ar"], max_batch)
    return V2HotPath(ar, InterpolateRegulator(*M["ar_lr"], "cuda:0"), InterpolateRegulator(*M["cfm_lr"], "cuda:0"),
                     CFM(*M["dit"], "cuda:0"), BigVGAN(*M["voc"], "cuda:0"))


def _convert(hp, ks, **kw):
    us = [V.utterance(k) for k in ks]
    targets = [hp.prepare_target(u["target_narrow"], u["target_tokens"], u["target_mel"], u["style"]) for u in us]
    args = dict(exp_noise=[u["noise"].cuda() for u in us], z=[u["z"].cuda() for u in us], max_new=A.MAX_NEW)
    args.update(kw)
    out = hp.convert_batch([u["src_narrow"].cuda() for u in us], targets, [u["frames_per_token"] for u in us], V.N_STEPS,
                           cfg_rates=V.CFG_RATES, **args)
    torch.cuda.synchronize()
    return out


def _check_against(out, ks, refs, what):
    """tokens equal; ylen equal; mel mean abs error < 1e-3; wave RMS < 1e-4 (refs: (tokens, ylen, mel, wave_fn))."""
    hop = 8
    for o, k, (toks, ylen, mel, wave_fn) in zip(out, ks, refs):
        assert torch.equal(o["tokens"].cpu(), toks), f"{what}, utterance {k}: {o['tokens'].tolist()} vs {toks.tolist()}"
        assert o["mel"].shape == (1, mel.shape[1], ylen) and o["wave"].shape == (1, ylen * hop)
        e_mel = (o["mel"].cpu() - mel).abs().mean().item()
        e_wav = (o["wave"].cpu() - wave_fn(o["mel"].cpu())).pow(2).mean().sqrt().item()
        print(f"{what}, utterance {k}: {toks.shape[1]} tokens, {ylen} frames, mel mean abs err {e_mel:.3e}, wave RMS {e_wav:.3e}")
        assert e_mel < 1e-3 and e_wav < 1e-4


def _oracle_refs(ks):
    h, vsd = V.models()["voc"]
    return [V.oracle_chain(k) + (lambda m: O.bigvgan_forward(vsd, h, m).reshape(1, -1),) for k in ks]


def test_chain_matches_oracle_chain_ragged():
    ks = V.qualified()[:3]
    assert len(ks) == 3
    out = _convert(_hotpath(), ks)
    assert len({V.utterance(k)["ylen"] for k in ks}) == 3          # three vocoder groups
    _check_against(out, ks, _oracle_refs(ks), "chain vs oracle")


def test_batch_equals_alone():
    """Tokens bit for bit; mels to the bound of the oracle comparison (the DiT's kernel paths agree to fp16 rounding only);
    the wave of the run alone against the oracle vocoder on its own mel, as in the oracle comparison."""
    ks = V.qualified()[:3]
    hp = _hotpath()
    batch = _convert(hp, ks)
    alone = [_convert(hp, [k])[0] for k in ks]
    for k, a, b in zip(ks, alone, batch):
        assert torch.equal(a["tokens"], b["tokens"]), f"utterance {k}"
        assert a["mel"].shape == b["mel"].shape and a["wave"].shape == b["wave"].shape
        e_mel = (a["mel"] - b["mel"]).abs().mean().item()
        e_wav = (a["wave"] - b["wave"]).pow(2).mean().sqrt().item()
        print(f"utterance {k}: alone vs batched mel mean abs err {e_mel:.3e}, wave RMS {e_wav:.3e}")
        assert e_mel < 1e-3
        if torch.equal(a["mel"], b["mel"]):
            assert e_wav < 1e-4
    _check_against(alone, ks, _oracle_refs(ks), "alone vs oracle")


def test_padding_never_leaks():
    ks = V.qualified()[:3]
    hp = _hotpath()
    first = _convert(hp, ks)
    first = [{n: t.cpu() for n, t in o.items()} for o in first]
    junk = torch.full((64 << 20,), float("nan"), device="cuda")     # 256 MB of NaN handed back to the caching allocator
    torch.cuda.synchronize()
    del junk
    second = _convert(hp, ks)
    for a, b in zip(first, second):
        for n in ("tokens", "mel", "wave"):
            assert torch.isfinite(b[n].float()).all()
            assert torch.equal(a[n], b[n].cpu()), n


def test_chain_edges_and_errors():
    ks = V.qualified()[:3]
    hp = _hotpath(max_batch=3)
    us = [V.utterance(k) for k in ks]
    targets = [hp.prepare_target(u["target_narrow"], u["target_tokens"], u["target_mel"], u["style"]) for u in us]
    src = [u["src_narrow"].cuda() for u in us]
    fpt = [u["frames_per_token"] for u in us]
    noise = [u["noise"].cuda() for u in us]
    with pytest.raises(ValueError):
        hp.convert_batch(src, targets[:2], fpt, V.N_STEPS)
    with pytest.raises(ValueError):
        hp.convert_batch(src, targets, fpt[:1], V.N_STEPS)
    with pytest.raises(ValueError):
        hp.convert_batch(src, targets, fpt, V.N_STEPS, seeds=[1, 2, 3], exp_noise=noise)
    with pytest.raises(RuntimeError, match="max_batch"):
        hp.convert_batch(src + src[:1], targets + targets[:1], fpt + fpt[:1], V.N_STEPS, seeds=[1, 2, 3, 4], max_new=A.MAX_NEW)
    # ylen = 0 for the middle utterance: empty mel and wave, the others as in the full batch
    z = [u["z"].cuda() for u in us]
    out = hp.convert_batch(src, targets, [fpt[0], 0.01, fpt[2]], V.N_STEPS, cfg_rates=V.CFG_RATES, exp_noise=noise, z=z, max_new=A.MAX_NEW)
    assert out[1]["mel"].shape == (1, 80, 0) and out[1]["wave"].shape == (1, 0)
    assert torch.equal(out[1]["tokens"].cpu(), us[1]["ref_tokens"])
    refs = _oracle_refs(ks)
    _check_against([out[0], out[2]], [ks[0], ks[2]], [refs[0], refs[2]], "with an empty neighbour")
    none = hp.convert_batch(src[:1], targets[:1], [0.0], V.N_STEPS, seeds=[3], max_new=A.MAX_NEW)
    assert none[0]["mel"].shape[2] == 0 and none[0]["tokens"].shape[1] >= 1
    # the object still converts afterwards, seeded too
    _check_against(_convert(hp, ks), ks, refs, "after the refusals")
    a = _convert(hp, ks, exp_noise=None, seeds=[5, 6, 7], z=None)
    b = _convert(hp, ks, exp_noise=None, seeds=[5, 6, 7], z=None)
    for x, y in zip(a, b):
        assert x["tokens"].shape[1] >= 1 and torch.equal(x["tokens"], y["tokens"])
        assert x["mel"].shape == y["mel"].shape and torch.isfinite(x["wave"]).all()


# ----------------------------------------------------------------------------------------------------------------- full size
def test_chain_full_size(golden):
    """ar_base + full-size v2 length regulators, DiT (fs_v2 weights, fused D = 512 path) and BigVGAN 22k: ar_gen_full in
    slots 0 and 2 of B = 3 gives the committed 160 tokens, the lengths are as computed and the output is finite.  The AR
    length regulator is embedding-only, so an embedding table holding the case's 120 condition frames and the narrow
    tokens 0 .. 119 make the chain build exactly the case's AR prompt."""
    from seedvc_amd import specs, weights
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath, v2_target_frames
    from seedvc_amd.vocoder import BigVGAN
    ref = torch.from_numpy(golden["ar_gen_full.codes"])
    c, sd, text, target, boosted = cases.ar_gen_full_case(winners=ref)
    plain = cases.ar_gen_full_case()[4]
    n_new = cases.AR_GEN_FULL_TOKENS
    alc = specs.lr_config("v2_ar", codebook_size=text.size(1))
    alsd = weights.make_state_dict(specs.lr_state_spec(alc), seed=5, prefix="lr.")
    assert alsd["embedding.weight"].shape == text[0].shape
    alsd["embedding.weight"] = text[0].clone()
    clc = specs.lr_config("v2_cfm")
    clsd = weights.make_state_dict(specs.lr_state_spec(clc), seed=6, prefix="lr.")
    dcfg, dsd, _, _ = cases.fullsize_cfm_case("fs_v2")
    h, vsd, _ = cases.fullsize_voc_case("fs_bigvgan22k")
    ar = _ar(c, sd, 3)
    cfm = CFM(dcfg, dsd, "cuda:0")
    assert cfm.estimator.fused_available
    cfm.estimator.set_fused_min_rows(0)
    hp = V2HotPath(ar, InterpolateRegulator(alc, alsd, "cuda:0"), InterpolateRegulator(clc, clsd, "cuda:0"), cfm, BigVGAN(h, vsd, "cuda:0"))
    narrow = torch.arange(text.size(1))[None]
    Ps, fpt, keep = [100, 61, 140], [1.5, 1.1, 1.5], [200, 150, 200]
    targets = [hp.prepare_target(narrow[:, :40], target[:, :keep[b]], cases.logmel(f"fsc.mel{b}", 9, 1, dcfg["C"], Ps[b]),
                                 cases.randn(f"fsc.style{b}", 9, 1, dcfg["style_dim"])) for b in range(3)]
    out = hp.convert_batch([narrow[:, 40:]] * 3, targets, fpt, 4, cfg_rates=(0.7, 0.7), max_new=n_new,
                           exp_noise=[boosted.cuda(), plain.cuda(), boosted.cuda()])
    torch.cuda.synchronize()
    hop = specs.bigvgan_total_upsample(h)
    for b in range(3):
        toks = out[b]["tokens"].cpu()
        ylen = v2_target_frames(fpt[b], toks.shape[1])
        print(f"slot {b}: {toks.shape[1]} tokens, {ylen} frames, {out[b]['wave'].shape[1]} samples")
        if b != 1:
            assert toks.shape == ref.shape and torch.equal(toks, ref)
            assert ylen == 240
        assert out[b]["mel"].shape == (1, dcfg["C"], ylen) and out[b]["wave"].shape == (1, ylen * hop)
        assert torch.isfinite(out[b]["mel"]).all() and torch.isfinite(out[b]["wave"]).all()
        assert out[b]["wave"].abs().max().item() <= 1.0
