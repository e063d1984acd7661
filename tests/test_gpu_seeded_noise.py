"""GPU tests of per-utterance noise seeds: the exporters against the numpy restatement of the draw layout
(seeded_noise_cases.py), the seeded sampler and HiFT calls against their explicit forms fed the exported draws, and every
pipeline entry point against its own explicit form.  The one claim is "seeds mean these tensors", so the comparisons are
`torch.equal`; where two sides run different kernels (a ragged against a plain HiFT call, another micro-batch size of the
sampler) the project's bounds for that difference apply (mel mean-abs < 1e-3, wave RMS < 1e-4).

Measured, exporters against the float64 restatement (bound 1e-5 = ~20 fp32 ulps at |n| = 5.77; phase0 bound 1e-6): printed
by test_exporters_equal_the_restatement and recorded in DESIGN.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import hift_ragged_cases as HR
import seeded_noise_cases as SN
import v2_chain_cases as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
MEL_L1, WAVE_RMS = 1e-3, 1e-4          # test_gpu_dit.py's and the vocoder tests' bounds
_cache = {}


def _cfm(name):
    from seedvc_amd.cfm import CFM
    if ("cfm", name) not in _cache:
        cfg, sd, inp, meta = cases.dit_case(name)
        _cache[("cfm", name)] = (CFM(cfg, sd, DEV), cfg, meta)
    return _cache[("cfm", name)]


def _hift():
    from seedvc_amd.vocoder import HiFT
    if "hift" not in _cache:
        c, sd, _, _, _, _ = cases.hift_case(HR.MODEL)
        _cache["hift"] = (HiFT(c, sd, DEV), c, sd)
    return _cache["hift"]


def _bigvgan():
    from seedvc_amd.vocoder import BigVGAN
    if "bigvgan" not in _cache:
        h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")       # 80 mels, upsample rates [4, 2]: hop 8
        _cache["bigvgan"] = BigVGAN(h, vsd, DEV)
    return _cache["bigvgan"]


def _rms(a, b):
    return (a.double() - b.double()).pow(2).mean().sqrt().item()


def _z_draws(cfm, seeds, T):
    return torch.cat([cfm.noise_draws(s, T) for s in seeds])


def _hift_draws(voc, seeds, S):
    d = [voc.noise_draws(s, S) for s in seeds]
    return dict(phase0=torch.cat([p for p, _ in d]), noise=torch.cat([n for _, n in d]))


# ---------------------------------------------------------------------------------------------------------- 1. exporters
def _export_z(seed, Cc, T):
    from seedvc_amd import _lib
    z = torch.full((Cc, T), float("nan"), device=DEV)
    _lib.check(_lib.lib().svc_cfm_noise_draws(seed, Cc, T, _lib.ptr(z), _lib.stream_ptr()))
    return z.cpu().numpy()


def _export_hift(seed, NH, n):
    from seedvc_amd import _lib
    ph, x = torch.full((NH,), float("nan"), device=DEV), torch.full((NH, n), float("nan"), device=DEV)
    _lib.check(_lib.lib().svc_hift_noise_draws(seed, NH, n, _lib.ptr(ph), _lib.ptr(x), _lib.stream_ptr()))
    return ph.cpu().numpy(), x.cpu().numpy()


@pytest.mark.parametrize("seed", SN.SEEDS)
def test_exporters_equal_the_restatement(seed):
    z = _export_z(seed, 80, 67)
    ph, x = _export_hift(seed, 9, 1027)
    assert z.dtype == np.float32 and z.shape == (80, 67) and x.shape == (9, 1027) and ph.shape == (9,)
    ez = np.abs(z.astype(np.float64) - SN.reference_normals(seed, SN.DOMAIN_Z, 80, 67)).max()
    ex = np.abs(x.astype(np.float64) - SN.reference_normals(seed, SN.DOMAIN_HIFT_NOISE, 9, 1027)).max()
    ep = np.abs(ph.astype(np.float64) - SN.reference_phase0(seed, 9)).max()
    print(f"seed {seed}: max |device - float64 restatement|: z (80 x 67) {ez:.3e}, HiFT noise (9 x 1027) {ex:.3e}, phase0 {ep:.3e}")
    assert ez < 1e-5 and ex < 1e-5
    assert ep < 1e-6
    # the prefix property on the device: fewer rows / positions give a sub-array, bit for bit
    assert np.array_equal(_export_z(seed, 77, 33), z[:77, :33])
    ph5, x5 = _export_hift(seed, 5, 259)
    assert np.array_equal(x5, x[:5, :259]) and np.array_equal(ph5, ph[:5])
    assert not np.array_equal(_export_z(seed + 1, 80, 67), z) and not np.array_equal(z[:9], x[:, :67])


@pytest.mark.parametrize("seed", SN.STAT_SEEDS)
def test_exported_draws_are_standard_normal(seed):
    SN.check_statistics(_export_z(seed, 80, 512).astype(np.float64), f"device z, seed {seed}")
    ph, x = _export_hift(seed, 9, 4096)
    SN.check_statistics(x.astype(np.float64), f"device HiFT noise, seed {seed}")
    assert np.abs(ph).max() <= np.pi + 1e-6


# ------------------------------------------------------------------------------------------------------------- 2. sampler
def _ragged_inputs(cfg, meta):
    """The inputs of test_gpu_dit.py::test_batched_ragged_equals_independent_runs."""
    T, P = meta["T"], meta["P"]
    lens, plens = [T, T - 9, T - 17], [P, P - 4, 3]
    B = len(lens)
    mu = torch.cat([cases.randn(f"rag.mu{b}", 1, 1, T, cfg["Dc"]) for b in range(B)]).to(DEV)
    prompt = torch.cat([cases.logmel(f"rag.p{b}", 1, 1, cfg["C"], P) for b in range(B)]).to(DEV)
    style = torch.cat([cases.randn(f"rag.s{b}", 1, 1, cfg["style_dim"]) for b in range(B)]).to(DEV)
    return T, lens, plens, mu, prompt, style


@pytest.mark.parametrize("name", ["small_r", "tiny_r"])
def test_seeded_sampler_equals_the_explicit_call(name):
    cfm, cfg, meta = _cfm(name)
    T, lens, plens, mu, prompt, style = _ragged_inputs(cfg, meta)
    seeds = [1234, 2 ** 63 + 5, 77]
    run = lambda **kw: cfm.inference(mu, torch.LongTensor(lens), prompt, style, None, 2, temperature=0.8, inference_cfg_rate=0.7,   # noqa: E731
                                     prompt_lens=plens, **kw)
    cfm.estimator.set_microbatch(2)             # the second group starts at seeds + 2
    try:
        got = run(seeds=seeds)
        want = run(z=_z_draws(cfm, seeds, T))
        again = run(seeds=seeds)
        other = run(seeds=[1234, 2 ** 63 + 5, 78])
    finally:
        cfm.estimator.set_microbatch(0)
    one = cfm.inference(mu, torch.LongTensor(lens), prompt, style, None, 2, temperature=0.8, inference_cfg_rate=0.7, prompt_lens=plens,
                        seeds=seeds)            # one group of three
    assert got.shape == (3, cfg["C"], T) and torch.isfinite(got).all()
    assert torch.equal(got, want), f"{name}: seeded differs from explicit, max {(got - want).abs().max().item():.3e}"
    assert torch.equal(got, again) and torch.equal(got, one)
    assert torch.equal(got[:2], other[:2]) and not torch.equal(got[2], other[2])
    for b in range(3):
        assert float(got[b, :, :plens[b]].abs().max()) == 0.0


def test_seeded_sampler_three_way_cfg_v2():
    cfm, cfg, meta = _cfm("v2_r")
    T, lens, plens, mu, prompt, style = _ragged_inputs(cfg, meta)
    seeds = [5, 2 ** 64 - 1, 1234]
    run = lambda **kw: cfm.inference(mu, lens, prompt, style, None, 2, inference_cfg_rate=[0.7, 0.7], prompt_lens=plens, **kw)   # noqa: E731
    got = run(seeds=seeds)
    assert torch.equal(got, run(z=_z_draws(cfm, seeds, T))) and torch.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------- 3. HiFT
def test_seeded_hift_equals_the_explicit_call():
    voc, c, sd = _hift()
    B, S, up = 3, 13, HR.total_up(c)
    mel = cases.logmel("sn.hift.mel", 7, B, c["in_channels"], S).to(DEV)
    f0 = (120.0 + 80.0 * cases.rand("sn.hift.f0", 7, B, S)).to(DEV)
    seeds = [1234, 2 ** 63 + 5, 77]
    voc.set_microbatch(2)
    try:
        for f0_arg in (f0, None):
            got, f0_got = voc(mel, f0=f0_arg, seeds=seeds, return_f0=True)
            want, f0_want = voc(mel, f0=f0_arg, return_f0=True, **_hift_draws(voc, seeds, S))
            assert got.shape == (B, S * up) and torch.isfinite(got).all()
            assert torch.equal(got, want) and torch.equal(f0_got, f0_want)
            assert torch.equal(got, voc(mel, f0=f0_arg, seeds=seeds))
            other = voc(mel, f0=f0_arg, seeds=[1234, 2 ** 63 + 5, 78])
            assert torch.equal(got[:2], other[:2]) and not torch.equal(got[2], other[2])
    finally:
        voc.set_microbatch(0)


def test_seeded_ragged_hift_equals_each_utterance_alone_and_needs_no_noise_tensor():
    voc, c, sd = _hift()
    lens = [7, 3, 12, 0]
    B, S, up, nh = len(lens), max(lens), HR.total_up(c), c["nb_harmonics"] + 1
    bt = HR.batch(c, sd, lens, tag="sn.hr")              # NaN in every padding frame and f0 slot
    mel, f0 = bt["mel"].to(DEV), bt["f0"].to(DEV)
    seeds = [1234, 2 ** 63 + 5, 77, 9]
    voc.set_microbatch(2)
    try:
        got = voc(mel, f0=f0, lens=lens, seeds=seeds)
        explicit = voc(mel, f0=f0, lens=lens, **_hift_draws(voc, seeds, S))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        again = voc(mel, f0=f0, lens=lens, seeds=seeds)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    finally:
        voc.set_microbatch(0)
    noise_bytes = B * nh * S * up * 4
    print(f"seeded ragged HiFT call: peak rise {rise} B; the explicit call's noise tensor alone is {noise_bytes} B")
    assert rise < noise_bytes
    assert torch.equal(got, explicit) and torch.equal(got, again)
    for b, n in enumerate(lens):
        assert (got[b, n * up:] == 0).all(), f"utterance {b}: the tail is not zero"
        if n:
            alone = voc(mel[b:b + 1, :, :n].contiguous(), f0=f0[b:b + 1, :n].contiguous(), seeds=[seeds[b]])
            assert torch.isfinite(alone).all() and torch.equal(got[b, :n * up], alone[0]), f"utterance {b} ({n} frames)"


# ---------------------------------------------------------------------------------------------------------- 4. pipelines
@pytest.mark.parametrize("which", ["hift", "bigvgan"])
def test_convert_batch_ragged_with_seeds(which):
    from seedvc_amd.pipeline import HotPath
    cfm, cfg, _ = _cfm("tiny_r" if which == "hift" else "small_r")
    voc = _hift()[0] if which == "hift" else _bigvgan()
    hp = HotPath(cfm, voc)
    x_lens, P = [60, 41, 52], [16, 9, 3]
    B, T, Pmax, Smax = 3, max(x_lens), max(P), max(t - p for t, p in zip(x_lens, P))
    mu = torch.cat([cases.randn(f"sn.cbr.mu{b}", 6, 1, T, cfg["Dc"]) for b in range(B)]).to(DEV)
    prompt = torch.cat([cases.logmel(f"sn.cbr.p{b}", 6, 1, cfg["C"], Pmax) for b in range(B)]).to(DEV)
    style = torch.cat([cases.randn(f"sn.cbr.s{b}", 6, 1, cfg["style_dim"]) for b in range(B)]).to(DEV)
    seeds = [1234, 2 ** 63 + 5, 77]
    got = hp.convert_batch_ragged_seeded(mu, prompt, style, x_lens, P, 2, 0.7, seeds)
    want = hp.convert_batch_ragged(mu, prompt, style, x_lens, P, 2, 0.7, z=_z_draws(cfm, seeds, T),
                                   vocoder_kwargs=_hift_draws(voc, seeds, Smax) if which == "hift" else None)
    for b in range(B):
        assert got[b][0].shape == (1, cfg["C"], x_lens[b] - P[b]) and got[b][1].shape[1] % (x_lens[b] - P[b]) == 0
        assert torch.equal(got[b][0], want[b][0]) and torch.equal(got[b][1], want[b][1]), f"{which}: utterance {b}"
        assert torch.isfinite(got[b][1]).all()
    # the plain entry point, one length
    m1, w1 = hp.convert_batch(mu[:2, :41], prompt[:2, :, :9].contiguous(), style[:2], 2, 0.7, seeds=seeds[:2])
    m2, w2 = hp.convert_batch(mu[:2, :41], prompt[:2, :, :9].contiguous(), style[:2], 2, 0.7, z=_z_draws(cfm, seeds[:2], 41),
                              vocoder_kwargs=_hift_draws(voc, seeds[:2], 32) if which == "hift" else None)
    assert torch.equal(m1, m2) and torch.equal(w1, w2)


def test_realtime_step_with_seeds():
    from seedvc_amd import specs, weights
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import RealtimeEngine, derive_seed
    cfm, cfg, _ = _cfm("tiny_r")
    voc, c, _ = _hift()
    preset, ov, tin, _, _, seed = cases.LR_CASES["lr_tiny_r"]
    lcfg = specs.lr_config(preset, **ov, out_channels=cfg["Dc"])
    lr = InterpolateRegulator(lcfg, weights.make_state_dict(specs.lr_state_spec(lcfg), seed=seed, prefix="lr."), DEV)
    hop, S, prompts = HR.total_up(c), 10, (16, 11)
    q = hop // 4
    geo = dict(S=S, hop=hop, block=4 * q, sola_buffer=2 * q, sola_search=q, tail=q // 2, max_streams=3)
    engines = [RealtimeEngine(lr, cfm, voc, **geo) for _ in range(2)]
    refs = [(cases.randn(f"sn.rt.pc{i}", 143, 1, P, cfg["Dc"]), cases.logmel(f"sn.rt.mel{i}", 143, 1, cfg["C"], P),
             cases.randn(f"sn.rt.style{i}", 143, 1, cfg["style_dim"])) for i, P in enumerate(prompts)]
    slots = [[eng.open(*r) for r in refs] for eng in engines]
    assert slots[0] == slots[1] == [0, 1]
    stream_seeds = [1234, 2 ** 63 + 5]
    for k in range(2):
        x = cases.randn(f"sn.rt.x{k}", 143, 2, tin, lcfg["in_channels"]).to(DEV)
        seeds = [derive_seed(s, k) for s in stream_seeds]
        out_s, parts_s = engines[0].step_seeded(slots[0], x, 2, 0.7, seeds, return_parts=True)
        out_e, parts_e = engines[1].step(slots[1], x, 2, 0.7, z=_z_draws(cfm, seeds, max(prompts) + S),
                                         vocoder_kwargs=_hift_draws(voc, seeds, S), return_parts=True)
        assert torch.equal(out_s, out_e) and torch.isfinite(out_s).all(), f"block {k}"
        assert torch.equal(parts_s["offsets"], parts_e["offsets"]) and torch.equal(parts_s["mel"], parts_e["mel"])
        assert torch.equal(engines[0].state, engines[1].state) and engines[0].state[:2].any()
    assert len({derive_seed(s, k) for s in stream_seeds for k in range(2)}) == 4


def test_v2_chain_with_noise_seeds():
    import ar_batch_cases as A
    from seedvc_amd.ar import ARModel
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath
    from seedvc_amd.vocoder import BigVGAN
    M = V.models()
    ks = V.qualified()[:2]
    assert len(ks) == 2
    ar = ARModel(*M["ar"], DEV)
    ar.setup_caches(max_batch_size=2)
    hp = V2HotPath(ar, InterpolateRegulator(*M["ar_lr"], DEV), InterpolateRegulator(*M["cfm_lr"], DEV), CFM(*M["dit"], DEV),
                   BigVGAN(*M["voc"], DEV))
    us = [V.utterance(k) for k in ks]
    targets = [hp.prepare_target(u["target_narrow"], u["target_tokens"], u["target_mel"], u["style"]) for u in us]
    run = lambda **kw: hp.convert_batch([u["src_narrow"].to(DEV) for u in us], targets, [u["frames_per_token"] for u in us], V.N_STEPS,   # noqa: E731
                                        cfg_rates=V.CFG_RATES, max_new=A.MAX_NEW, seeds=[5, 6], **kw)
    noise_seeds = [1234, 2 ** 63 + 5]
    got = run(noise_seeds=noise_seeds)
    # explicit: the draws of each utterance, longer than it needs (the first frames of a row do not depend on the length)
    want = run(z=[hp.cfm.noise_draws(s, 400) for s in noise_seeds])
    other = run(noise_seeds=[1234, 2 ** 63 + 6])
    for b in range(2):
        assert got[b]["tokens"].shape[1] >= 1 and got[b]["mel"].shape[2] >= 1
        for n in ("tokens", "mel", "wave"):
            assert torch.equal(got[b][n], want[b][n]), (b, n)
        assert torch.equal(got[b]["tokens"], other[b]["tokens"])          # `seeds` alone decides the tokens
    assert torch.equal(got[0]["mel"], other[0]["mel"]) and not torch.equal(got[1]["mel"], other[1]["mel"])


# ------------------------------------------------------------------------------------------------------ convert_long_batch
HOP, WINDOW, OVERLAP, STEPS = 8, 40, 4, 2
FILES = [(60, 16), (20, 11)]                 # source frames, prompt frames: chunks of 24 24 20 frames and one of 20
FILE_SEEDS = [1234, 2 ** 63 + 5]


def _files(cfg):
    return [(cases.randn(f"sn.lb.cond{S}", 3, 1, S, cfg["Dc"]).to(DEV), cases.randn(f"sn.lb.pc{P}", 3, 1, P, cfg["Dc"]).to(DEV),
             cases.logmel(f"sn.lb.mel{P}", 3, 1, cfg["C"], P).to(DEV), cases.randn(f"sn.lb.style{P}", 3, 1, cfg["style_dim"]).to(DEV))
            for S, P in FILES]


def _chunk_seeds():
    from seedvc_amd.pipeline import derive_seed, long_batch_plan
    plan = long_batch_plan([f[0] for f in FILES], [f[1] for f in FILES], WINDOW, OVERLAP, HOP)
    assert [c[0] for c in plan["chunks"]] == [0, 0, 0, 1]
    return [derive_seed(FILE_SEEDS[0], k) for k in range(3)] + [derive_seed(FILE_SEEDS[1], 0)]


class _InOrder:
    """The per-chunk functions of the explicit form: call j (plan order) returns the exported draws of chunk j's seed."""

    def __init__(self, seeds, fn):
        self.seeds, self.fn, self.calls = seeds, fn, 0

    def __call__(self, n):
        self.calls += 1
        return self.fn(self.seeds[self.calls - 1], n)


def test_long_batch_with_seeds_bigvgan():
    from seedvc_amd.pipeline import HotPath
    cfm, cfg, _ = _cfm("tiny_r")
    hp = HotPath(cfm, _bigvgan())
    utts, cs = _files(cfg), _chunk_seeds()
    got = hp.convert_long_batch(utts, STEPS, 0.7, HOP, WINDOW, overlap_frame_len=OVERLAP, seeds=FILE_SEEDS, ragged_vocoder=False)
    noise_fn, kw_fn = _InOrder(cs, cfm.noise_draws), _InOrder(cs, lambda s, n: {})
    want = hp.convert_long_batch(utts, STEPS, 0.7, HOP, WINDOW, overlap_frame_len=OVERLAP, noise_fn=noise_fn, vocoder_kwargs_fn=kw_fn,
                                 ragged_vocoder=False)
    assert noise_fn.calls == kw_fn.calls == 4
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.shape == (1, FILES[u][0] * HOP) and torch.isfinite(g).all()
        assert torch.equal(g, w), f"file {u}: RMS {_rms(g, w):.3e}"
    # a file alone gives the same draws: its chunks' seeds do not depend on the pool (the sampler's kernels may)
    alone = hp.convert_long_batch(utts[1:], STEPS, 0.7, HOP, WINDOW, overlap_frame_len=OVERLAP, seeds=FILE_SEEDS[1:], ragged_vocoder=False)
    e = _rms(alone[0], got[1])
    print(f"file 1 alone vs in the pool: wave RMS {e:.3e}, equal {torch.equal(alone[0], got[1])}")
    assert e < WAVE_RMS

    # micro-batches of two chunks against one of four: identical draws, possibly other sampler kernels
    class Recorder:
        def __init__(self, voc):
            self.voc, self.mels = voc, []

        def __call__(self, mel, lens=None):
            self.mels += [mel[i, :, :(mel.size(2) if lens is None else lens[i])].clone() for i in range(mel.size(0))]
            return self.voc(mel) if lens is None else self.voc(mel, lens=lens)
    runs = []
    for max_chunks in (2, 64):
        rec = Recorder(_bigvgan())
        out = HotPath(cfm, rec).convert_long_batch(utts, STEPS, 0.7, HOP, WINDOW, overlap_frame_len=OVERLAP, seeds=FILE_SEEDS,
                                                   max_chunks=max_chunks, ragged_vocoder=True)
        runs.append((rec.mels, out))
    (mels2, out2), (mels64, out64) = runs
    assert [m.shape[1] for m in mels2] == [m.shape[1] for m in mels64] == [24, 24, 20, 20]
    for k, (a, b) in enumerate(zip(mels2, mels64)):
        l1 = (a - b).abs().mean().item()
        print(f"chunk {k}: max_chunks 2 vs 64: mel mean abs difference {l1:.3e}, equal {torch.equal(a, b)}")
        assert l1 < MEL_L1
    for u, (a, b) in enumerate(zip(out2, out64)):
        e = _rms(a, b)
        print(f"file {u}: max_chunks 2 vs 64: wave RMS {e:.3e}")
        assert e < WAVE_RMS


def test_long_batch_with_seeds_ragged_hift():
    """The ragged HiFT call on the seeded side, one plain call per chunk length fed the exported draws on the explicit side:
    the same mels and draws through HiFT calls of other batch shapes -- the project's vocoder bound, RMS < 1e-4."""
    from seedvc_amd.pipeline import HotPath
    cfm, cfg, _ = _cfm("tiny_r")
    voc = _hift()[0]
    hop = HR.total_up(_hift()[1])
    hp = HotPath(cfm, voc)
    utts, cs = _files(cfg), _chunk_seeds()
    calls = []
    hp._vocoder_seeds = lambda seeds, _f=hp._vocoder_seeds: calls.append(seeds) or _f(seeds)
    got = hp.convert_long_batch(utts, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP, seeds=FILE_SEEDS, ragged_vocoder=True)
    assert calls == [cs]                        # ONE vocoder call, the four chunk seeds in plan order
    del hp._vocoder_seeds
    noise_fn = _InOrder(cs, cfm.noise_draws)
    kw_fn = _InOrder(cs, lambda s, n: dict(zip(("phase0", "noise"), voc.noise_draws(s, n))))
    want = hp.convert_long_batch(utts, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP, noise_fn=noise_fn, vocoder_kwargs_fn=kw_fn,
                                 ragged_vocoder=False)
    grouped = hp.convert_long_batch(utts, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP, seeds=FILE_SEEDS, ragged_vocoder=False)
    for u, (g, w, gr) in enumerate(zip(got, want, grouped)):
        e = _rms(g, w)
        print(f"file {u}: seeded ragged HiFT vs explicit grouped: wave RMS {e:.3e} (signal RMS {w.pow(2).mean().sqrt().item():.3e}), "
              f"equal {torch.equal(g, w)}")
        assert g.shape == w.shape == (1, FILES[u][0] * hop) and torch.isfinite(g).all()
        assert e < WAVE_RMS
        assert torch.equal(gr, w), f"file {u}: the grouped seeded call runs the explicit side's own vocoder calls"


# ------------------------------------------------------------------------------------------------------ 5. argument checks
def _cfm_args(cfm, cfg, B, T, P, keep):
    from seedvc_amd import _lib
    mu, prompt = torch.zeros(max(B, 1), T, cfg["Dc"], device=DEV), torch.zeros(max(B, 1), cfg["C"], P, device=DEV)
    style, out = torch.zeros(max(B, 1), cfg["style_dim"], device=DEV), torch.full((max(B, 1), cfg["C"], T), 7.5, device=DEV)
    a = _lib.CfmArgs()
    a.B, a.T, a.P = B, T, P
    a.mu, a.prompt, a.style, a.out, a.z = mu.data_ptr(), prompt.data_ptr(), style.data_ptr(), out.data_ptr(), None
    a.n_timesteps, a.temperature = 2, 1.0
    a.cfg_rate[0] = a.cfg_rate[1] = 0.7
    keep += [mu, prompt, style]
    return a, out


def test_seeded_calls_check_their_arguments_before_anything_is_launched():
    from seedvc_amd import _lib
    l = _lib.lib()
    cfm, cfg, _ = _cfm("tiny_r")
    voc, c, _ = _hift()
    keep, one_seed = [], (C.c_uint64 * 1)(1234)
    a, out = _cfm_args(cfm, cfg, 1, 20, 4, keep)
    assert l.svc_cfm_sample_seeded(cfm.estimator._h, C.byref(a), None, _lib.stream_ptr()) != 0
    assert b"seeds" in l.svc_last_error()
    a0, out0 = _cfm_args(cfm, cfg, 0, 20, 4, keep)
    assert l.svc_cfm_sample_seeded(cfm.estimator._h, C.byref(a0), one_seed, _lib.stream_ptr()) != 0
    assert l.svc_last_error()
    S, up = 5, HR.total_up(c)
    mel = torch.zeros(1, c["in_channels"], S, device=DEV)
    wave = torch.full((1, S * up), 7.5, device=DEV)
    assert l.svc_hift_forward_seeded(voc._h, _lib.ptr(mel), None, None, None, 1, S, _lib.ptr(wave), None, _lib.stream_ptr()) != 0
    assert b"seeds" in l.svc_last_error()
    assert l.svc_hift_forward_seeded(voc._h, _lib.ptr(mel), None, None, one_seed, 0, S, _lib.ptr(wave), None, _lib.stream_ptr()) != 0
    assert l.svc_hift_forward_seeded(voc._h, _lib.ptr(mel), (C.c_int32 * 1)(S + 1), None, one_seed, 1, S, _lib.ptr(wave), None,
                                     _lib.stream_ptr()) != 0
    assert b"lens" in l.svc_last_error()
    if torch.cuda.device_count() > 1:           # a handle of another device
        with torch.cuda.device(1):
            assert l.svc_cfm_sample_seeded(cfm.estimator._h, C.byref(a), one_seed, _lib.stream_ptr()) != 0
            assert b"another device" in l.svc_last_error()
            assert l.svc_hift_forward_seeded(voc._h, _lib.ptr(mel), None, None, one_seed, 1, S, _lib.ptr(wave), None,
                                             _lib.stream_ptr()) != 0
            assert b"another device" in l.svc_last_error()
    torch.cuda.synchronize()
    assert (out == 7.5).all() and (out0 == 7.5).all() and (wave == 7.5).all()
    # the same arguments with seeds are accepted
    assert l.svc_cfm_sample_seeded(cfm.estimator._h, C.byref(a), one_seed, _lib.stream_ptr()) == 0
    assert l.svc_hift_forward_seeded(voc._h, _lib.ptr(mel), None, None, one_seed, 1, S, _lib.ptr(wave), None, _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not (out == 7.5).all() and torch.isfinite(wave).all() and not (wave == 7.5).all()
