"""Per-utterance sampler settings on the device (`svc_cfm_sample_rows` behind `CFM.inference_rows`, `RealtimeEngine.set_sampler`,
`sampler=` of `convert_long_batch`).  The contract of include/seedvc_hip.h: (a) rows that carry one setting are the existing
call bit for bit, (b) the call is bit for bit the existing call on each class's members stacked in batch order, (c) every row
is a B = 1 run of the reference sampler with its own settings, held to the oracle at the project's mel L1 bound."""
import pytest
import torch

import cases
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEL_L1 = 1e-3
torch.set_grad_enabled(False)
_cache = {}


def _model(name):
    if name not in _cache:
        from seedvc_amd.cfm import CFM
        cfg, sd, _, meta = cases.dit_case(name)
        _cache[name] = (CFM(cfg, sd, DEV), cfg, sd, meta)
    return _cache[name]


def _batch(tag, cfg, B, T, P):
    """mu, prompt, style, z of B utterances (host tensors)."""
    return (cases.randn(tag + ".mu", 5, B, T, cfg["Dc"]), cases.logmel(tag + ".prompt", 5, B, cfg["C"], P),
            cases.randn(tag + ".style", 5, B, cfg["style_dim"]), cases.randn(tag + ".z", 5, B, cfg["C"], T))


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _oracle_row(sd, cfg, batch, b, x_len, p_len, setting):
    """Row b alone through the reference sampler with its own settings -> (1, C, x_len)."""
    mu, prompt, style, z = batch
    steps, rate, temperature, random_voice = tuple(setting) + (1.0, False)[len(setting) - 2:]
    return O.cfm_sample(sd, cfg, z[b:b + 1, :, :x_len], x_len, prompt[b:b + 1, :, :p_len], mu[b:b + 1, :x_len], style[b:b + 1], steps,
                        list(rate) if isinstance(rate, tuple) else rate, temperature=temperature, random_voice=random_voice)


def _check_rows_against_oracle(tag, out, sd, cfg, batch, x_lens, p_lens, settings):
    for b, setting in enumerate(settings):
        ref = _oracle_row(sd, cfg, batch, b, x_lens[b], p_lens[b], setting)
        l1 = (out[b:b + 1, :, :x_lens[b]] - ref).abs().mean().item()
        print(f"{tag} row {b} {setting}: mel L1 vs oracle {l1:.3e}")
        assert l1 < MEL_L1, (tag, b, l1)
        assert not out[b, :, :p_lens[b]].any(), (tag, b)                 # prompt frames are exactly 0


# ------------------------------------------------------------------------------------------ 1: uniform rows = the existing call
@pytest.mark.parametrize("name,B,setting", [("tiny_r", 5, (3, 0.7, 0.8)), ("v2_r", 3, (3, (0.7, 0.3), 0.8))])
def test_uniform_rows_equal_the_existing_call_bit_for_bit(name, B, setting):
    cfm, cfg, sd, meta = _model(name)
    T, P = meta["T"], meta["P"]
    mu, prompt, style, z = _dev(*_batch(f"rows.uniform.{name}", cfg, B, T, P))
    x_lens, p_lens = [T - 3 * b for b in range(B)], [P - 2 * b for b in range(B)]
    steps, rate, temperature = setting
    for draws in (dict(z=z), dict(seeds=[77 + b for b in range(B)])):
        want = cfm.inference(mu, x_lens, prompt, style, None, steps, temperature=temperature,
                             inference_cfg_rate=list(rate) if isinstance(rate, tuple) else rate, prompt_lens=p_lens, **draws)
        got = cfm.inference_rows(mu, x_lens, prompt, style, [setting] * B, prompt_lens=p_lens, **draws)
        assert torch.equal(got, want), (name, list(draws))
        as_dicts = [dict(n_timesteps=steps, inference_cfg_rate=rate, temperature=temperature)] * B
        assert torch.equal(cfm.inference_rows(mu, x_lens, prompt, style, as_dicts, prompt_lens=p_lens, **draws), want)


# ------------------------------------------------------------------------------------------ 2: mixed rates in one class
def test_mixed_rates_and_temperatures_share_one_class():
    cfm, cfg, sd, meta = _model("tiny_r")
    T, P, B = meta["T"], meta["P"], 4
    settings = [(3, r, t) for r, t in zip([.3, .7, 1., .7], [1., .5, .8, 1.])]
    assert cfm.rows_plan(settings) == ([0] * B, [2])
    batch = _batch("rows.mixed", cfg, B, T, P)
    mu, prompt, style, z = _dev(*batch)
    out = cfm.inference_rows(mu, [T] * B, prompt, style, settings, z=z)
    for b, (steps, rate, temperature) in enumerate(settings):
        alone = cfm.inference(mu[b:b + 1], [T], prompt[b:b + 1], style[b:b + 1], None, steps, temperature=temperature,
                              inference_cfg_rate=rate, z=z[b:b + 1])
        assert torch.equal(out[b:b + 1], alone), b
    _check_rows_against_oracle("mixed", out.cpu(), sd, cfg, batch, [T] * B, [P] * B, settings)
    # the rows really ran with their own settings: rows 1 and 3 share the rate, not the temperature
    same = cfm.inference_rows(mu, [T] * B, prompt, style, [settings[3]] * B, z=z)
    assert torch.equal(same[3], out[3]) and not torch.equal(same[1], out[1]) and not torch.equal(same[0], out[0])


# ------------------------------------------------------------------------------------------ 3: interleaved classes
def test_interleaved_classes_with_non_adjacent_members():
    cfm, cfg, sd, meta = _model("small_r")
    T, P, B = meta["T"], meta["P"], 5
    x_lens, p_lens = [T, T - 5, T - 1, T - 9, T - 2], [P, P - 3, P - 1, P, P - 5]
    settings = [(4, .7), (2, .7), (4, .7), (4, 0.), (4, .7)]
    assert cfm.rows_plan(settings) == ([0, 1, 0, 2, 0], [2, 2, 1])
    batch = _batch("rows.interleaved", cfg, B, T, P)
    mu, prompt, style, z = _dev(*batch)
    for draws in ("z", "seeds"):
        seeds = [1000 + b for b in range(B)]
        kw = (lambda rows: dict(z=z[rows])) if draws == "z" else (lambda rows: dict(seeds=[seeds[b] for b in rows]))
        out = cfm.inference_rows(mu, x_lens, prompt, style, settings, prompt_lens=p_lens, **kw(list(range(B))))
        for rows, (steps, rate) in (([0, 2, 4], (4, .7)), ([1], (2, .7)), ([3], (4, 0.))):
            want = cfm.inference(mu[rows], [x_lens[b] for b in rows], prompt[rows], style[rows], None, steps, inference_cfg_rate=rate,
                                 prompt_lens=[p_lens[b] for b in rows], **kw(rows))
            for i, b in enumerate(rows):       # frames past a row's length are not part of the result
                assert torch.equal(out[b, :, :x_lens[b]], want[i, :, :x_lens[b]]), (draws, b)
        if draws == "z":
            _check_rows_against_oracle("interleaved", out.cpu(), sd, cfg, batch, x_lens, p_lens, settings)


# ------------------------------------------------------------------------------------------ 4: v2, every guidance structure
def test_v2_one_row_per_guidance_structure():
    cfm, cfg, sd, meta = _model("v2_r")
    T, P = meta["T"], meta["P"]
    settings = [(3, (.7, .7), 1.0, True), (3, (0., 0.), .8), (3, (0., .7), 1.0), (3, (.7, 0.), .5), (3, (.7, .7), 1.0), (3, (.4, .9), .8)]
    B = len(settings)
    assert cfm.rows_plan(settings) == ([0, 1, 2, 3, 4, 4], [2, 1, 2, 2, 3])
    x_lens, p_lens = [T, T - 2, T - 7, T, T - 1, T - 4], [P, P - 1, P, P - 4, P - 2, P]
    batch = _batch("rows.v2", cfg, B, T, P)
    mu, prompt, style, z = _dev(*batch)
    out = cfm.inference_rows(mu, x_lens, prompt, style, settings, z=z, prompt_lens=p_lens)
    _check_rows_against_oracle("v2", out.cpu(), sd, cfg, batch, x_lens, p_lens, settings)


# ------------------------------------------------------------------------------------------ 5: the fused row-panel path
def test_fused_panels_feed_the_per_row_update():
    cfm, cfg, sd, meta = _model("tiny_full")
    assert cfm.estimator.fused_available                                 # D = 384: the row-panel kernel exists for this width
    T, P, B = meta["T"], meta["P"], 3
    settings = [(2, r) for r in (.7, .3, 1.)]
    batch = _batch("rows.fused", cfg, B, T, P)
    mu, prompt, style, z = _dev(*batch)
    x_lens, p_lens = [T, T - 7, T - 1], [P, P - 3, P]
    cfm.estimator.set_fused_min_rows(0)
    try:
        out = cfm.inference_rows(mu, x_lens, prompt, style, settings, z=z, prompt_lens=p_lens)
        want = cfm.inference(mu, x_lens, prompt, style, None, 2, inference_cfg_rate=.3, z=z, prompt_lens=p_lens)
        got = cfm.inference_rows(mu, x_lens, prompt, style, [(2, .3)] * B, z=z, prompt_lens=p_lens)
    finally:
        cfm.estimator.set_fused_min_rows(-1)
    assert torch.equal(got, want)
    assert torch.equal(out[1, :, :x_lens[1]], want[1, :, :x_lens[1]]) and not torch.equal(out[0], want[0])
    _check_rows_against_oracle("fused", out.cpu(), sd, cfg, batch, x_lens, p_lens, settings)


# ------------------------------------------------------------------------------------------ 6: graph replay reads the table
def test_graph_replay_uses_the_rates_of_its_own_call():
    cfm, cfg, sd, meta = _model("tiny_r")
    T, P, B = meta["T"], meta["P"], 3
    mu, prompt, style, z = _dev(*_batch("rows.graph", cfg, B, T, P))
    lists = [[(3, r, t) for r, t in zip(rates, temps)]
             for rates, temps in (([.3, .7, 1.], [1., .5, .8]), ([.7, .7, .3], [.8, 1., 1.]), ([1., .3, .7], [.5, .8, 1.]))]
    run = lambda settings: cfm.inference_rows(mu, [T, T - 4, T - 1], prompt, style, settings, z=z, prompt_lens=[P, P - 2, P])  # noqa: E731
    eager = [run(s) for s in lists]
    cfm.estimator.set_graphs(True)
    try:
        replayed = [run(s) for s in lists]             # eager, capture + replay, replay
    finally:
        cfm.estimator.set_graphs(False)
    for k in range(3):
        assert torch.equal(replayed[k], eager[k]), k
    assert not torch.equal(replayed[2], replayed[0])


# ------------------------------------------------------------------------------------------ 7: the engine
def test_engine_slot_override_is_the_stream_alone_with_those_arguments():
    from seedvc_amd import specs, weights
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import RealtimeEngine
    from seedvc_amd.vocoder import BigVGAN
    cfm, cfg, sd, _ = _model("tiny_r")
    preset, ov, tin, _, _, seed = cases.LR_CASES["lr_tiny_r"]
    lcfg = specs.lr_config(preset, **ov, out_channels=cfg["Dc"])
    lr = InterpolateRegulator(lcfg, weights.make_state_dict(specs.lr_state_spec(lcfg), seed=seed, prefix="lr."), DEV)
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")                      # upsample rates [4, 2]: hop 8
    eng = RealtimeEngine(lr, cfm, BigVGAN(h, vsd, DEV), 40, 8, 96, 32, 16, tail=8, max_streams=3)
    P = 16
    for i in range(3):
        assert eng.open(cases.randn(f"rows.rt.pc{i}", 9, 1, P, cfg["Dc"]), cases.logmel(f"rows.rt.mel{i}", 9, 1, cfg["C"], P),
                        cases.randn(f"rows.rt.style{i}", 9, 1, cfg["style_dim"])) == i
    x = cases.randn("rows.rt.x", 9, 3, tin, lcfg["in_channels"]).to(DEV)
    seeds = [31, 32, 33]
    mel = lambda slots, steps, rate: eng.step_seeded(slots, x[slots], steps, rate, [seeds[s] for s in slots],  # noqa: E731
                                                     return_parts=True)[1]["mel"]
    plain = mel([0, 1, 2], 3, 0.7)
    eng.set_sampler(1, n_timesteps=2, inference_cfg_rate=0.0)
    got = mel([0, 1, 2], 3, 0.7)
    eng.set_sampler(1)
    assert torch.equal(got[1:2], mel([1], 2, 0.0))
    assert torch.equal(got[[0, 2]], mel([0, 2], 3, 0.7))
    assert not torch.equal(got[1], plain[1])
    assert torch.equal(mel([0, 1, 2], 3, 0.7), plain)                    # the override is gone: the plain three-stream step


# ------------------------------------------------------------------------------------------ 8: the chunk pool
class _KeepMels:
    """The real sampler, keeping the mel of every call (the pool returns waves only)."""

    def __init__(self, cfm):
        self.cfm, self.device, self.in_channels, self.mels = cfm, cfm.device, cfm.in_channels, []

    def inference(self, *a, **kw):
        self.mels.append(self.cfm.inference(*a, **kw))
        return self.mels[-1]

    def inference_rows(self, *a, **kw):
        self.mels.append(self.cfm.inference_rows(*a, **kw))
        return self.mels[-1]


def test_pool_files_with_their_own_settings():
    """Two files, the first with its own (2 steps, 0.3), seeded.  Per chunk the mel is within MEL_L1 of the file converted alone
    with its settings as call arguments; a file whose mels are all bit-identical has a bit-identical wave (the vocoder and the
    seams see nothing else)."""
    from seedvc_amd.pipeline import HotPath, long_batch_plan
    from seedvc_amd.vocoder import BigVGAN
    cfm, cfg, sd, _ = _model("tiny_r")
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")
    HOP, WINDOW, OVERLAP, STEPS, RATE = 8, 40, 4, 3, 0.7
    keep = _KeepMels(cfm)
    hp = HotPath(keep, BigVGAN(h, vsd, DEV))
    sizes = [(70, 16), (45, 11)]                                          # (source frames, prompt frames): 3 and 2 chunks
    utts = [_dev(cases.randn(f"rows.pool.cond{u}", 3, 1, S, cfg["Dc"]), cases.randn(f"rows.pool.pc{u}", 3, 1, P, cfg["Dc"]),
                 cases.logmel(f"rows.pool.mel{u}", 3, 1, cfg["C"], P), cases.randn(f"rows.pool.style{u}", 3, 1, cfg["style_dim"]))
            for u, (S, P) in enumerate(sizes)]
    seeds = [501, 502]

    def run(us, steps, rate, **kw):
        """-> (waves, the mels of the sampler calls)"""
        waves = hp.convert_long_batch([utts[u] for u in us], steps, rate, HOP, WINDOW, overlap_frame_len=OVERLAP,
                                      seeds=[seeds[u] for u in us], **kw)
        mels, keep.mels = keep.mels, []
        return [w.clone() for w in waves], mels

    plan = long_batch_plan([s for s, _ in sizes], [p for _, p in sizes], WINDOW, OVERLAP, HOP, 64)
    chunks, file_of = plan["chunks"], [c[0] for c in plan["chunks"]]
    assert len(plan["micro_batches"]) == 1 and file_of.count(0) >= 2 and file_of.count(1) == 2
    waves, (mels,) = run([0, 1], STEPS, RATE, sampler=[(2, 0.3), None])
    for u, (steps, rate) in enumerate([(2, 0.3), (STEPS, RATE)]):
        (wave,), (alone,) = run([u], steps, rate)
        rows = [k for k, f in enumerate(file_of) if f == u]
        identical = True
        for i, k in enumerate(rows):
            n = sizes[u][1] + chunks[k][2]                                # prompt + the chunk's frames
            l1 = (mels[k, :, :n] - alone[i, :, :n]).abs().mean().item()
            same = torch.equal(mels[k, :, :n], alone[i, :, :n])
            identical &= same
            print(f"pool file {u} chunk {i}: mel L1 vs the file alone {l1:.3e}, bit-identical: {same}")
            assert l1 < MEL_L1
        assert waves[u].shape == wave.shape
        if identical:
            assert torch.equal(waves[u], wave)
    # sampler=None is the call without the keyword; entries that are all None are the call's arguments on every file
    today, _ = run([0, 1], STEPS, RATE)
    none, _ = run([0, 1], STEPS, RATE, sampler=None)
    nones, _ = run([0, 1], STEPS, RATE, sampler=[None, None])
    for a, b, c in zip(today, none, nones):
        assert torch.equal(a, b) and torch.equal(a, c)


# ------------------------------------------------------------------------------------------ 9: the v2 pools, both branches
def test_v2_pools_use_each_files_entry_in_both_branches():
    """`V2HotPath.convert_long_batch(sampler=)` on the reduced chain of v2_long_cases.py, two files, seeded, one of them with
    its own steps and rates.  Style branch: per chunk the tokens equal those of the file alone with its settings as call
    arguments and the mel is within MEL_L1 of it.  Timbre branch (`_long_pool`): the same per chunk on the sampler's mels.
    Waves: the vocoder call of the pool holds the chunks of both files, that of a file alone its own, and which kernel form
    a vocoder launch takes depends on its row count, so equal mels give waves inside the project's vocoder bound (RMS 1e-4,
    as test_gpu_long_batch.py applies it to another batch size), not necessarily equal bits."""
    WAVE_RMS = 1e-4
    rms = lambda a, b: (a - b).pow(2).mean().sqrt().item()  # noqa: E731
    import ar_batch_cases as A
    import v2_long_cases as L
    from seedvc_amd.ar import ARModel
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath, long_batch_plan
    from seedvc_amd.vocoder import BigVGAN
    M = L.models()
    ar = ARModel(*M["ar"], DEV)
    ar.setup_caches(max_batch_size=4)
    keep = _KeepMels(CFM(*M["dit"], DEV))
    hp = V2HotPath(ar, InterpolateRegulator(*M["ar_lr"], DEV), InterpolateRegulator(*M["cfm_lr"], DEV), keep, BigVGAN(*M["voc"], DEV))
    fs = L.qualified()[:2]
    recs = []
    for f in fs:
        u = L.file_inputs(f)
        target = hp.prepare_target(u["target_narrow"], u["target_tokens"], u["target_mel"], u["style"])
        recs.append(dict(target=target, src_narrow=u["src_narrow"].to(DEV), src_tokens=u["src_tokens"].to(DEV),
                         frames_per_token=u["frames_per_token"], source_frames=0))
    seeds, ov = [41, 42], 2
    own = (2, (0.3, 0.0))                                                  # file 0: other steps, intelligibility guidance only
    call = (L.N_STEPS, tuple(L.CFG_RATES))
    assert keep.cfm.rows_plan([own, call])[0] == [0, 1]                    # two classes in every micro-batch that mixes them

    # ---- style branch
    def style(us, steps, rates, **kw):
        out = hp.convert_long_batch([recs[u] for u in us], steps, rates, max_context_window=64, hop=L.HOP, max_new=A.MAX_NEW,
                                    return_parts=True, ar_chunk_tokens=9, overlap_frame_len=ov, seeds=[seeds[u] for u in us], **kw)
        keep.mels = []
        return out

    waves, parts = style([0, 1], *call, sampler=[own, None])
    plain_w, plain_p = style([0, 1], *call)
    assert len(parts[0]) >= 2 and len(parts[1]) >= 2
    for u, (steps, rates) in enumerate([own, call]):
        alone_w, alone_p = style([u], steps, rates)
        same = True
        for j, (a, b) in enumerate(zip(alone_p[0], parts[u])):
            assert torch.equal(a["tokens"], b["tokens"]) and a["ylen"] == b["ylen"] and a["kept"] == b["kept"]
            l1, eq = (a["mel"] - b["mel"]).abs().mean().item(), torch.equal(a["mel"], b["mel"])
            print(f"v2 style file {u} chunk {j}: alone vs pool mel L1 {l1:.3e}, identical {eq}")
            assert l1 < MEL_L1
            if eq:
                assert rms(a["wave"], b["wave"]) < WAVE_RMS
            same = same and eq
        assert alone_w[0].shape == waves[u].shape
        if same:
            assert rms(alone_w[0], waves[u]) < WAVE_RMS
    assert not torch.equal(parts[0][0]["mel"], plain_p[0][0]["mel"])        # file 0 really ran with its own entry
    for a, b in zip(parts[1], plain_p[1]):                                 # file 1 ran with the call's arguments
        assert (a["mel"] - b["mel"]).abs().mean().item() < MEL_L1

    # ---- timbre branch
    frames = [30, 9]
    trecs = [dict(r, source_frames=n) for r, n in zip(recs, frames)]
    P = [r["target"]["P"] for r in trecs]
    window = P[0] + 12
    plan = long_batch_plan(frames, P, window, ov, L.HOP)
    file_of = [c[0] for c in plan["chunks"]]
    assert file_of == [0, 0, 0, 1] and len(plan["micro_batches"]) == 1

    def timbre(us, steps, rates, **kw):
        w = hp.convert_long_batch([trecs[u] for u in us], steps, rates, convert_style=False, max_context_window=window, hop=L.HOP,
                                  overlap_frame_len=ov, seeds=[seeds[u] for u in us], **kw)
        mels, keep.mels = keep.mels, []
        return [x.clone() for x in w], mels

    waves, (mels,) = timbre([0, 1], *call, sampler=[None, own])
    for u, (steps, rates) in enumerate([call, own]):
        (wave,), (alone,) = timbre([u], steps, rates)
        same = True
        for i, k in enumerate([k for k, f in enumerate(file_of) if f == u]):
            n = P[u] + plan["chunks"][k][2]
            l1, eq = (mels[k, :, :n] - alone[i, :, :n]).abs().mean().item(), torch.equal(mels[k, :, :n], alone[i, :, :n])
            print(f"v2 timbre file {u} chunk {i}: alone vs pool mel L1 {l1:.3e}, identical {eq}")
            assert l1 < MEL_L1
            same = same and eq
        assert wave.shape == waves[u].shape
        if same:
            assert rms(wave, waves[u]) < WAVE_RMS
    today, _ = timbre([0, 1], *call)
    none, _ = timbre([0, 1], *call, sampler=None)
    assert all(torch.equal(a, b) for a, b in zip(today, none))
