"""GPU side of v2 real-time sessions.  Op level: `svc_astral_tokens_heads` for every mask against the plane of one
`svc_astral_tokens` call bit for bit, with a sentinel plane behind the selected ones, the duration reduction of a selected head,
`tokens_fn` against `tokens_batch`, and every refusal with the output untouched.  Engine: a token-mode `RealtimeEngine` with the
exact stand-ins of rt_v2_cases.py against the numpy session bit for bit and without a host synchronisation; and with reduced real
models (ASTRAL CFG_S, the `v2_cfm` regulator, the v2_r DiT, BigVGAN) `step_audio` against `step_tokens`, the oracle chain on the
engine's own tokens within the project's bounds for it (mel L1 < 1e-3, `infer` RMS < 1e-4: DESIGN.md 8c), per-slot rate pairs and
`random_voice`, and the audio-side features (output rate, mute).  Every figure is printed before it is asserted."""
import warnings

import numpy as np
import pytest
import torch

import astral_cases as AC
import cases
import long_batch_cases as LB
import realtime_cases as RT
import resample_cases as RC
import rt_audio_cases as RA
import rt_v2_cases as V
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
OV_S = AC.OV * 320 / 16000
CLIP_LENS = (20000, 32400, 57700)                            # 1, 2 and 3 windows of 32 000 samples at an overlap of 20 rows
SENTINEL = -7777
_resamplers = {}


def _resample(pair):
    from seedvc_amd.audio import Resample
    if pair not in _resamplers:
        _resamplers[pair] = Resample(*pair, device=DEV)
    return _resamplers[pair]


@pytest.fixture(scope="module")
def small():
    from seedvc_amd.astral import AstralTokenizer
    k = AC.case("S")
    return {p: AstralTokenizer(k["ssl_sd"], k["heads"], cfg=k["cfg"], device=DEV, precision=p) for p in (0, 1)}


@pytest.fixture(scope="module")
def clips():
    buf = torch.full((len(CLIP_LENS), 60000), float("nan"))
    for b, n in enumerate(CLIP_LENS):
        buf[b, :n] = AC.make_wave(n, 20 + b)
    return buf.to(DEV)


def _heads_call(m, w, lens, mask, out, R, reduce_head=-1, red=None, cnt=None, ov=AC.OV, B=None, L=None, handle=True):
    """The raw call on device tensors -> its return code."""
    from seedvc_amd import _lib
    return _lib.lib().svc_astral_tokens_heads(m._h if handle else None, _lib.ptr(w), None if lens is None else _lib.i32_host(list(lens)),
                                              w.size(0) if B is None else B, w.size(1) if L is None else L, ov, mask, _lib.ptr(out), R,
                                              reduce_head, _lib.ptr(red), _lib.ptr(cnt), _lib.stream_ptr())


# ------------------------------------------------------------------------------------------------ 1. a subset of the heads
@pytest.mark.parametrize("precision", [0, 1])
def test_selected_planes_equal_the_full_call(small, clips, precision):
    """Masks 0b01, 0b10, 0b11 on clips of 1, 2 and 3 windows: each selected plane is the plane of ONE `svc_astral_tokens` call on the
    same input; the buffer is one plane too long and that plane keeps its sentinel; with reduce_head = 1 under mask 0b10 the
    reduction equals the full call's."""
    from seedvc_amd import _lib
    m = small[precision]
    full, rows, red, cnt = m.tokens_batch(clips, CLIP_LENS, overlap_s=OV_S, reduce_head=1)
    assert rows == [62, 100, 178] and full.shape == (2, 3, 178)
    B, R = 3, max(rows)
    for mask in (0b01, 0b10, 0b11):
        sel = [k for k in range(2) if mask >> k & 1]
        out = torch.full((len(sel) + 1, B, R), SENTINEL, dtype=torch.int32, device=DEV)
        _lib.check(_heads_call(m, clips, CLIP_LENS, mask, out, R))
        for p, k in enumerate(sel):
            assert torch.equal(out[p], full[k]), f"mask {mask:#b}: plane {p} is not head {k}'s"
        assert bool((out[len(sel)] == SENTINEL).all()), f"mask {mask:#b}: the plane behind the selected ones was written"
    assert not torch.equal(full[0], full[1])                 # the two heads differ: a plane cannot pass for the other
    out = torch.full((2, B, R), SENTINEL, dtype=torch.int32, device=DEV)
    red1 = torch.full((B, R), SENTINEL, dtype=torch.int32, device=DEV)
    cnt1 = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    _lib.check(_heads_call(m, clips, CLIP_LENS, 0b10, out, R, reduce_head=1, red=red1, cnt=cnt1))
    assert torch.equal(out[0], full[1]) and bool((out[1] == SENTINEL).all())
    assert torch.equal(red1, red) and torch.equal(cnt1, cnt) and int(cnt.min()) > 0
    # the mirror's heads= is the same call
    t1, r1, red2, cnt2 = m.tokens_batch(clips, CLIP_LENS, overlap_s=OV_S, reduce_head=1, heads=(1,))
    assert t1.shape == (1, B, R) and r1 == rows and torch.equal(t1[0], full[1]) and torch.equal(red2, red) and torch.equal(cnt2, cnt)
    t2, _ = m.tokens_batch(clips, CLIP_LENS, overlap_s=OV_S, heads=(1, 0))
    assert torch.equal(t2, full)                             # ascending head order whatever the order given


@pytest.mark.parametrize("precision", [0, 1])
def test_tokens_fn_is_one_head_of_the_context(small, precision):
    m = small[precision]
    ctx = torch.stack([AC.make_wave(12 * 320, 31 + b) for b in range(2)]).to(DEV)
    both, rows = m.tokens_batch(ctx, overlap_s=0)
    assert rows == [11, 11]
    m.set_timing(True)
    for head in (0, 1):
        got = m.tokens_fn(ctx, head)
        assert got.dtype == torch.int32 and got.shape == (2, 11) and torch.equal(got, both[head])
        assert int(got.min()) >= 0 and int(got.max()) < m.codebook_size(head)
        t = m.last_timing()                                  # the four stages stay
        assert list(t) == ["ssl", "convnext", "bsq", "assemble"] and all(np.isfinite(v) and v >= 0 for v in t.values())
    m.set_timing(False)


def test_every_library_refusal_leaves_the_output_untouched(small, clips):
    """The good call's arguments with one thing wrong each: non-zero, a message under the entry point's name, and tokens, reduced and
    counts keep every bit."""
    from seedvc_amd import _lib
    m = small[1]
    B, R = 3, 178
    out = torch.full((3, B, R), SENTINEL, dtype=torch.int32, device=DEV)
    red = torch.full((B, R), SENTINEL, dtype=torch.int32, device=DEV)
    cnt = torch.full((B,), SENTINEL, dtype=torch.int32, device=DEV)
    good = dict(lens=CLIP_LENS, mask=0b11, R=R, reduce_head=1, red=red, cnt=cnt)
    bad = dict(mask_zero=dict(mask=0), mask_above=dict(mask=0b100), mask_with_a_bit_above=dict(mask=0b111), mask_all_ones=dict(mask=0xffffffff),
               reduce_head_not_selected=dict(mask=0b01), reduce_head_above=dict(reduce_head=2), reduce_without_reduced=dict(red=None),
               reduce_without_counts=dict(cnt=None), reduced_on_the_selected_planes=dict(red=out[1]), null_handle=dict(handle=False),
               B_zero=dict(B=0), B_65=dict(B=65), lens_above_L=dict(lens=(20000, 32400, 60001)), lens_zero=dict(lens=(20000, 0, 57700)),
               lens_below_the_field=dict(lens=(20000, 300, 57700)), overlap_negative=dict(ov=-1), overlap_a_window=dict(ov=100),
               Rmax_small=dict(R=177), Rmax_zero=dict(R=0))
    for name, kw in bad.items():
        rc = _heads_call(m, clips, **{**good, **kw}, out=out)
        assert rc != 0, name
        assert _lib.lib().svc_last_error().startswith(b"svc_astral_tokens_heads:"), (name, _lib.lib().svc_last_error())
    for name, w, o in (("null_wave", None, out), ("null_tokens", clips, None)):
        rc = _lib.lib().svc_astral_tokens_heads(m._h, _lib.ptr(w), _lib.i32_host(list(CLIP_LENS)), B, 60000, AC.OV, 0b11, _lib.ptr(o), R, 1,
                                                _lib.ptr(red), _lib.ptr(cnt), _lib.stream_ptr())
        assert rc != 0 and b"null wave or tokens" in _lib.lib().svc_last_error(), name
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((red == SENTINEL).all()) and bool((cnt == SENTINEL).all())
    # reduced behind the two selected planes of a mask with one bit is no overlap: the compacted size counts
    _lib.check(_heads_call(m, clips, CLIP_LENS, 0b10, out, R, reduce_head=1, red=out[1], cnt=cnt))
    # and the good call is good
    _lib.check(_heads_call(m, clips, **good, out=out))
    torch.cuda.synchronize()
    assert bool((out[:2] != SENTINEL).all()) and bool((out[2] == SENTINEL).all()) and bool((cnt > 0).all())


# ------------------------------------------------------------------------------------ 2. the engine with the exact stand-ins
def _fake_refs():
    return [(cases.randn(f"rt.pc{s}", 142, 1, P, cases.CHUNK_DC).to(DEV), cases.logmel(f"rt.mel{s}", 142, 1, cases.CHUNK_C, P).to(DEV),
             cases.randn(f"rt.style{s}", 142, 1, 3).to(DEV)) for s, P in enumerate(RT.FAKE_PROMPTS)]


def _fake_engine(max_streams=4):
    from seedvc_amd.pipeline import RealtimeEngine
    cfm, voc, tok = LB.BatchedFakeCFM(DEV), RT.FakeVocoder(), V.FakeTokenizer()
    eng = RealtimeEngine(V.FakeTokenLR(DEV), cfm, voc, max_streams=max_streams, **RT.FAKE_GEOMETRY)
    assert eng.token_mode
    eng.attach_audio(tok, _resample(V.FAKE_PAIR), V.FAKE_M * 441, V.FAKE_L16, V.FAKE_CE)
    return eng, cfm, voc, tok


def _audio(sess, streams, k):
    return torch.from_numpy(np.stack([sess["audio"][s][k] for s in streams])).to(DEV)


def _check_step(sess, eng, slots, streams, k, out, parts):
    assert "content" not in parts and parts["tokens"].shape == (len(streams), 6) and not parts["tokens"].is_floating_point()
    for row, s in enumerate(streams):
        want_out, want_new, want_o, scores, before = sess["models"][s][k]
        assert np.array_equal(parts["ctx"][row].cpu().numpy(), sess["ctx"][s][k]), (s, k)
        assert np.array_equal(parts["tokens"][row].cpu().numpy(), sess["tokens"][s][k]), (s, k)
        assert int(parts["offsets"][row]) == want_o, (s, k, RT.score_gap(scores))
        assert np.array_equal(out[row].cpu().numpy(), want_out), (s, k)
        assert np.array_equal(eng.state[slots[s]].cpu().numpy(), want_new), (s, k)
        assert np.array_equal(eng.audio_context(slots[s]).cpu().numpy(), sess["ctx"][s][k]), (s, k)


def test_three_token_streams_from_audio_equal_the_numpy_session():
    sess = V.sessions()
    eng, cfm, voc, tok = _fake_engine()
    slots = [eng.open(*r) for r in _fake_refs()]
    for k in range(V.N_BLOCKS):
        order = [0, 1, 2] if k < 3 else [2, 0, 1]
        out, parts = eng.step_audio([slots[s] for s in order], _audio(sess, order, k), 10, (0.7, 0.7), return_parts=True)
        assert out.shape == (3, RT.FAKE_GEOMETRY["block"]) and parts["ctx"].shape == (3, V.FAKE_L16)
        _check_step(sess, eng, slots, order, k, out, parts)
    assert cfm.batch_sizes == [3] * 5 and voc.calls == [(3, 12)] * 5 and tok.calls == [(3, V.FAKE_L16, 0)] * 5
    a = eng._audio
    assert not a["planes"][:, 3].any() and not a["hist"][3].any() and not eng.state[3].any()        # the unused slot
    assert sess["min_gap"] > 1e-4                            # no block is decided by a near tie


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_each_token_stream_alone_equals_the_numpy_session(stream):
    sess = V.sessions()
    eng, _, _, _ = _fake_engine(max_streams=1)
    slot = eng.open(*_fake_refs()[stream])
    for k in range(V.N_BLOCKS):
        out, parts = eng.step_audio([slot], _audio(sess, [stream], k), 10, 0.7, return_parts=True)
        _check_step(sess, eng, {stream: slot}, [stream], k, out, parts)


def test_step_tokens_is_the_step_from_audio():
    """The numpy session's tokens through `step_tokens` (int32 and int64 alike) give the session's blocks; seeds are taken."""
    sess = V.sessions()
    eng, _, _, _ = _fake_engine()
    slots = [eng.open(*r) for r in _fake_refs()]
    for k in range(3):
        tokens = torch.from_numpy(np.stack([sess["tokens"][s][k] for s in range(3)])).to(DEV)
        if k == 1:
            out = eng.step_tokens(slots, tokens.long(), 10, (0.7, 0.5), seeds=[5, 6, 7])
        else:
            out = eng.step_tokens(slots, tokens, 10, 0.7)
        for s in range(3):
            assert np.array_equal(out[s].cpu().numpy(), sess["models"][s][k][0]), (s, k)
            assert np.array_equal(eng.state[slots[s]].cpu().numpy(), sess["models"][s][k][1]), (s, k)


def test_reset_and_a_reopened_token_slot_start_from_an_empty_context():
    sess = V.sessions()
    eng, _, _, _ = _fake_engine()
    refs = _fake_refs()
    slots = [eng.open(*r) for r in refs]
    for k in range(3):                                       # an odd number of pushes: the slots' current plane is 1
        eng.step_audio(slots, _audio(sess, [0, 1, 2], k), 10, 0.7)
    eng.close(1)
    assert eng.open(*refs[2]) == 1
    eng.reset(0)
    out, parts = eng.step_audio([0, 1], _audio(sess, [0, 2], 0), 10, 0.7, return_parts=True)
    _check_step(sess, eng, {0: 0, 2: 1}, [0, 2], 0, out, parts)


def test_a_token_step_from_audio_does_not_synchronise():
    watch = hasattr(torch.cuda, "set_sync_debug_mode")
    sess = V.sessions()
    eng, _, _, _ = _fake_engine()
    slots = [eng.open(*r) for r in _fake_refs()]
    xs = [_audio(sess, [0, 1, 2], k) for k in range(3)]
    eng.step_audio(slots, xs[0], 10, 0.7)                    # the first step stacks the prompts
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode() if watch else None
    if watch:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            torch.cuda.set_sync_debug_mode("error")
    try:
        out1 = eng.step_audio(slots, xs[1], 10, (0.7, 0.7))
        out2, parts = eng.step_audio(slots, xs[2], 10, (0.7, 0.7), return_parts=True)
    finally:
        if watch:
            torch.cuda.set_sync_debug_mode(before)
    for s in range(3):
        assert np.array_equal(out1[s].cpu().numpy(), sess["models"][s][1][0])
    _check_step(sess, eng, slots, [0, 1, 2], 2, out2, parts)


# ------------------------------------------------------------------------------------------------ 3. reduced real models
PAIR, S_REAL, CE_DIT, CE, STEPS, RATES, PROMPTS, SLOTS = (22050, 16000), 40, 0.04, 2, 3, (0.7, 0.5), (16, 11), [1, 0]
GEOMETRY = dict(S=S_REAL, hop=8, block=96, sola_buffer=32, sola_search=16, tail=8, max_streams=3)
# for `attach_output` at the model rate 22050 the splice lengths are multiples of zc = 441 samples: a step of 168 frames
GEOMETRY_OUT = dict(S=168, hop=8, block=441, sola_buffer=441, sola_search=441, tail=8, max_streams=3)
LIN, L16 = 2 * 441, 12 * 320                                 # 11 rows, 9 tokens after ce = 2
MEL_L1, INFER_RMS = 1e-3, 1e-4                               # the project's bounds for this chain


@pytest.fixture(scope="module")
def real():
    from seedvc_amd import specs, weights
    from seedvc_amd.astral import AstralTokenizer
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.vocoder import BigVGAN
    cfg, sd, _, _ = cases.dit_case("v2_r")
    lcfg = specs.lr_config("v2_cfm", channels=64, codebook_size=2048, out_channels=cfg["Dc"])
    lsd = weights.make_state_dict(specs.lr_state_spec(lcfg), seed=193, prefix="lr.")
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")
    k = AC.case("S")
    refs = [(cases.randn(f"rt_v2.real.pc{i}", 147, 1, P, cfg["Dc"]), cases.logmel(f"rt_v2.real.mel{i}", 147, 1, cfg["C"], P),
             cases.randn(f"rt_v2.real.style{i}", 147, 1, cfg["style_dim"])) for i, P in enumerate(PROMPTS)]
    return dict(cfg=cfg, sd=sd, lcfg=lcfg, lsd=lsd, h=h, vsd=vsd, refs=refs, cfm=CFM(cfg, sd, DEV), lr=InterpolateRegulator(lcfg, lsd, DEV),
                voc=BigVGAN(h, vsd, DEV),
                astral={p: AstralTokenizer(k["ssl_sd"], k["heads"], cfg=k["cfg"], device=DEV, precision=p) for p in (0, 1)})


def _real_engine(m, precision=None, geometry=GEOMETRY):
    from seedvc_amd.pipeline import RealtimeEngine
    eng = RealtimeEngine(m["lr"], m["cfm"], m["voc"], **geometry)
    assert eng.token_mode
    if precision is not None:
        eng.attach_audio(m["astral"][precision], _resample(PAIR), LIN, L16, CE_DIT)
    return eng


def _open(m, eng):
    assert [eng.open(*m["refs"][0]), eng.open(*m["refs"][1])] == [0, 1]


def _block(k, S=S_REAL):
    """(audio (2, Lin), z (2, C, Pmax + S)) of block k"""
    return (RC.noise(f"rt_v2.real.audio{k}", 147, 2, LIN) * 0.3).to(DEV), cases.randn(f"rt_v2.real.z{k}", 147, 2, 80, max(PROMPTS) + S).to(DEV)


def _oracle_mel(m, tokens, z, row, rates, random_voice=False, S=S_REAL):
    """The oracle chain of row `row` (stream SLOTS[row]) on the engine's own tokens -> mel (1, C, S)"""
    pc, mel2, style = m["refs"][SLOTS[row]]
    P = PROMPTS[SLOTS[row]]
    cond = O.lr_forward(m["lsd"], m["lcfg"], tokens[row:row + 1].long().cpu(), S)
    return O.cfm_sample(m["sd"], m["cfg"], z[row:row + 1, :, :P + S].cpu(), P + S, mel2, torch.cat([pc, cond], 1), style, STEPS, list(rates),
                        random_voice=random_voice)[:, :, P:]


@pytest.mark.parametrize("precision", [0, 1])
def test_step_audio_equals_step_tokens_and_the_oracle_chain(real, precision):
    """2 streams on slots [1, 0], 3 blocks of 2 zc samples, a context of 12 rows.  Engine A steps from audio; engine B is given
    `tokens_fn(ctx)[:, 2:]` of A's context and the same z: blocks and SOLA buffers are equal bit for bit.  Per block and row the mel
    against O.lr_forward -> O.cfm_sample on the engine's own tokens and `infer` against the oracle vocoder on the engine's own mel."""
    m = real
    a, b = _real_engine(m, precision), _real_engine(m)
    _open(m, a)
    _open(m, b)
    start, n_inf = a.start, a.n_inf
    seen = set()
    for k in range(3):
        audio, z = _block(k)
        out_a, parts = a.step_audio(SLOTS, audio, STEPS, RATES, z=z, return_parts=True)
        tokens = m["astral"][precision].tokens_fn(parts["ctx"])[:, CE:]
        assert parts["ctx"].shape == (2, L16) and tokens.shape == (2, 9) and "content" not in parts
        assert torch.equal(parts["tokens"], tokens)
        out_b = b.step_tokens(SLOTS, tokens, STEPS, RATES, z=z)
        assert torch.equal(out_a, out_b) and torch.equal(a.state, b.state), k
        assert bool(torch.isfinite(out_a).all()) and bool(out_a.abs().max() > 0)
        assert int(tokens.min()) >= 0 and int(tokens.max()) < 2048
        seen |= set(tokens.reshape(-1).tolist())
        mel, infer = parts["mel"].cpu(), parts["infer"].cpu()
        for row in range(2):
            l1 = (mel[row:row + 1] - _oracle_mel(m, tokens, z, row, RATES)).abs().mean().item()
            wave = O.bigvgan_forward(m["vsd"], m["h"], mel[row:row + 1]).reshape(-1)
            rms = (infer[row] - wave[start:start + n_inf]).pow(2).mean().sqrt().item()
            print(f"v2 real-time precision {precision} block {k} row {row}: mel L1 vs oracle {l1:.3e} (bound {MEL_L1:.0e}); infer RMS vs oracle "
                  f"vocoder {rms:.3e} (bound {INFER_RMS:.0e}; signal RMS {wave.pow(2).mean().sqrt().item():.3e})")
            assert l1 < MEL_L1
            assert rms < INFER_RMS
    assert len(seen) > 9 and not a.state[2].any()            # the tokens vary; the unused slot's buffer stays zero


def test_per_slot_pair_and_random_voice(real):
    """`set_sampler` with the v2 sampler's pair and with random_voice: one `inference_rows` call with two classes; each row within
    the mel bound of the oracle run with that row's own settings; the row without an override keeps its block bit for bit
    (contract (b) of DESIGN.md 8p); clearing the override gives back the uniform call's blocks."""
    m = real
    cfm = m["cfm"]
    calls = []

    class Recording:
        device, in_channels, cfg = cfm.device, cfm.in_channels, cfm.cfg

        def inference(self, *a, **kw):
            calls.append("inference")
            return cfm.inference(*a, **kw)

        def inference_rows(self, mu, x_lens, prompt, style, settings, **kw):
            calls.append(("inference_rows", list(settings)))
            return cfm.inference_rows(mu, x_lens, prompt, style, settings, **kw)

    from seedvc_amd.pipeline import RealtimeEngine
    audio, z = _block(0)

    def run(setup):
        """One block from a fresh engine -> (out, mel, tokens)"""
        eng = RealtimeEngine(m["lr"], Recording(), m["voc"], **GEOMETRY)
        eng.attach_audio(m["astral"][1], _resample(PAIR), LIN, L16, CE_DIT)
        _open(m, eng)
        setup(eng)
        out, parts = eng.step_audio(SLOTS, audio, STEPS, RATES, z=z, return_parts=True)
        return out, parts["mel"].cpu(), parts["tokens"]

    uniform, mel_u, tokens = run(lambda e: None)
    assert calls == ["inference"]
    # a pair on the slot of row 0
    pair = (0.7, 0.0)
    out_p, mel_p, tok_p = run(lambda e: e.set_sampler(SLOTS[0], inference_cfg_rate=pair))
    assert calls[1][0] == "inference_rows" and len(calls) == 2 and torch.equal(tok_p, tokens)
    settings = calls[1][1]
    class_of, n_streams = cfm.rows_plan(settings)
    assert len(set(class_of)) == 2 and class_of[0] != class_of[1], (settings, class_of, n_streams)
    for row, rates in enumerate((pair, RATES)):
        l1 = (mel_p[row:row + 1] - _oracle_mel(m, tokens, z, row, rates)).abs().mean().item()
        print(f"per-slot pair: row {row} with rates {rates}: mel L1 vs the oracle with its own pair {l1:.3e} (bound {MEL_L1:.0e})")
        assert l1 < MEL_L1
    assert not torch.equal(mel_p[0], mel_u[0])

    def set_then_clear(e):
        e.set_sampler(SLOTS[0], inference_cfg_rate=pair)
        e.set_sampler(SLOTS[0])
    out_c, _, _ = run(set_then_clear)
    assert calls[2] == "inference" and torch.equal(out_c, uniform)
    # random_voice on the slot of row 0: its own class, the other row untouched
    out_r, mel_r, _ = run(lambda e: e.set_sampler(SLOTS[0], random_voice=True))
    class_of, n_streams = cfm.rows_plan(calls[3][1])
    assert calls[3][0] == "inference_rows" and class_of[0] != class_of[1], (calls[3][1], class_of, n_streams)
    assert torch.equal(out_r[1], uniform[1]) and torch.equal(mel_r[1], mel_u[1])
    assert not torch.equal(mel_r[0], mel_u[0])
    l1 = (mel_r[0:1] - _oracle_mel(m, tokens, z, 0, RATES, random_voice=True)).abs().mean().item()
    print(f"random_voice: row 0: mel L1 vs the oracle with random_voice {l1:.3e} (bound {MEL_L1:.0e})")
    assert l1 < MEL_L1


def test_output_rate_and_mute_do_not_care_about_the_mode(real):
    """`attach_output(Resample(22050, 48000))` on a token engine, the slot of row 1 muted by `set_speech`: the muted row is the SOLA
    of zeros (from a zero buffer: zeros, offset 0) and the other row equals the run without the mute.  One block."""
    m = real
    audio, z = _block(0, GEOMETRY_OUT["S"])
    res = []
    for mute in (False, True):
        eng = _real_engine(m, geometry=GEOMETRY_OUT)
        eng.attach_output(_resample((22050, 48000)))
        eng.attach_audio(m["astral"][1], _resample(PAIR), LIN, L16, CE_DIT)
        _open(m, eng)
        if mute:
            eng.set_speech(SLOTS[1], False)
        out, parts = eng.step_audio(SLOTS, audio, STEPS, RATES, z=z, return_parts=True)
        assert out.shape == (2, 960) and parts["infer"].shape == (2, 3 * 960) and eng.state.shape == (3, 960)
        res.append((out, parts, eng.state.clone()))
    (out_u, parts_u, state_u), (out_m, parts_m, state_m) = res
    assert torch.equal(out_m[0], out_u[0]) and torch.equal(state_m[SLOTS[0]], state_u[SLOTS[0]])
    assert torch.equal(parts_m["tokens"], parts_u["tokens"]) and torch.equal(parts_m["mel"], parts_u["mel"])      # the model still runs
    assert not out_m[1].any() and not parts_m["infer"][1].any() and int(parts_m["offsets"][1]) == 0 and not state_m[SLOTS[1]].any()
    assert bool(out_u.abs().max(dim=1).values.min() > 0) and bool(torch.isfinite(out_u).all())
