"""GPU side of audio-in real-time sessions: `svc_rt_push` bit for bit against `audio.Resample` on hist ‖ block and within the
project's fp32 bound of the float64 push model (rt_audio_cases.py; test_host_rt_audio.py pins that to the reference GUI's own
lines); a stream pushed block by block against the one-shot conversion of the whole stream; `RealtimeEngine.step_audio` bit for
bit against the numpy session with exactly rounded stand-ins, without a host synchronisation, and against `step` on the returned
context with a real wav2vec 2.0 encoder; and every refusal of the C ABI with the state untouched."""
import warnings

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB
import realtime_cases as RT
import resample_cases as RC
import rt_audio_cases as RA
import w2v_cases as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
EQUAL = (16000, 16000)                                       # r = NULL: zc = z16 = 320
KERNEL_PAIRS = RA.PAIRS + [EQUAL]
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)      # noqa: E731  (NaN payloads compare as integers)
_resamplers = {}


def _resample(pair):
    from seedvc_amd.audio import Resample
    if pair not in _resamplers:
        _resamplers[pair] = Resample(*pair, device=DEV)
    return _resamplers[pair]


def _push(pair, block, slots, max_slots, hist, ring, L16, ctx, zc=None, z16=None, Lin=None, stride=None, N=None):
    """The raw call on device tensors -> its return code."""
    from seedvc_amd import _lib
    u = RA.units(*pair)
    return _lib.lib().svc_rt_push(_resample(pair)._h, _lib.ptr(block), block.stride(0) if stride is None else stride,
                                  block.size(1) if Lin is None else Lin, len(slots) if N is None else N, _lib.i32_host([int(s) for s in slots]),
                                  max_slots, u[0] if zc is None else zc, u[1] if z16 is None else z16, _lib.ptr(hist), _lib.ptr(ring), L16,
                                  _lib.ptr(ctx), _lib.stream_ptr())


class _Rig:
    """Device state of `svc_rt_push` for max_slots streams beside its expectation on the host.  Rows of `live` slots start from
    noise (both planes: different noise, the current one is plane 0), every other row of hist and of both planes is NaN."""

    def __init__(self, pair, Lin, L16, max_slots, live, seed):
        from seedvc_amd import _lib
        self.pair, self.Lin, self.L16, self.ms = pair, Lin, L16, max_slots
        self.zc, self.z16, _, _ = RA.units(*pair)
        self.tiles = int(_lib.lib().svc_rt_push_tiles(L16))
        n_ring = int(_lib.lib().svc_rt_ring_floats(max_slots, L16))
        rng = np.random.default_rng(seed)
        ring = np.zeros(n_ring, np.float32)
        planes, _ = RA.ring_planes(ring, max_slots, L16)
        planes[:] = np.nan
        planes[:, live] = rng.uniform(-1, 1, (2, len(live), L16)).astype(np.float32)
        self.hist = np.full((max_slots, 2 * self.zc), np.nan, np.float32)
        self.hist[live] = rng.uniform(-1, 1, (len(live), 2 * self.zc)).astype(np.float32)
        self.ring = ring                                     # the whole buffer as the device must hold it: planes + tickets
        self.cur = planes[0].copy()                          # expected context of every slot
        self.d_hist, self.d_ring = torch.from_numpy(self.hist.copy()).to(DEV), torch.from_numpy(ring.copy()).to(DEV)
        self.rng = rng

    def push(self, slots):
        """One push of fresh noise for `slots`; checks ctx, ring, hist and the rows of every other slot; -> (x, ctx) numpy."""
        from seedvc_amd import _lib
        n, zc, z16, L16, Lin = len(slots), self.zc, self.z16, self.L16, self.Lin
        shift, n_new = (Lin // zc) * z16, (Lin // zc + 1) * z16
        block = self.rng.uniform(-1, 1, (n, Lin)).astype(np.float32)
        d_block = torch.from_numpy(block).to(DEV)
        ctx = torch.full((n, L16), float("nan"), device=DEV)
        _lib.check(_push(self.pair, d_block, slots, self.ms, self.d_hist, self.d_ring, L16, ctx))
        x = np.concatenate([self.hist[slots], block], axis=1)
        y = _resample(self.pair)(torch.from_numpy(x).to(DEV)).cpu().numpy()       # svc_resample on x alone
        want = np.concatenate([self.cur[slots][:, shift:L16 - z16], y[:, z16:z16 + n_new]], axis=1)
        assert want.shape == (n, L16)
        ctx, ring, hist = ctx.cpu().numpy(), self.d_ring.cpu().numpy(), self.d_hist.cpu().numpy()
        planes, tickets = RA.ring_planes(ring, self.ms, L16)
        old_planes, old_tickets = RA.ring_planes(self.ring, self.ms, L16)
        assert np.array_equal(tickets[slots], old_tickets[slots] + np.uint64(self.tiles))
        plane = RA.current_plane(tickets, self.tiles)
        assert np.array_equal(bits(ctx), bits(want)), "ctx"
        assert np.array_equal(bits(planes[plane[slots], slots]), bits(want)), "ring"
        assert np.array_equal(bits(hist[slots]), bits(x[:, -2 * zc:])), "hist"
        rest = np.setdiff1d(np.arange(self.ms), slots)
        assert np.array_equal(bits(hist[rest]), bits(self.hist[rest])) and np.array_equal(bits(planes[:, rest]), bits(old_planes[:, rest]))
        assert np.array_equal(tickets[rest], old_tickets[rest])
        self.cur[slots], self.hist, self.ring = want, hist, ring
        return x, ctx


def _l16(kind, Lin, zc, z16):
    n_new = (Lin // zc + 1) * z16
    return {"exact": n_new, "plus1": n_new + 1, "x40": 40 * z16}[kind]


@pytest.mark.parametrize("kind", ["exact", "plus1", "x40"])
@pytest.mark.parametrize("m", [1, 9])
@pytest.mark.parametrize("pair", KERNEL_PAIRS, ids=[f"{a}_{b}" for a, b in KERNEL_PAIRS])
def test_push_equals_resample_bit_for_bit(pair, m, kind):
    """Five consecutive pushes of 64 permuted slots of 70; L16 = n_new (nothing to shift), n_new + 1 (4-byte accesses) and
    40 z16 (16-byte accesses where z16 is a multiple of 4)."""
    zc, z16, _, _ = RA.units(*pair)
    Lin = m * zc
    L16 = _l16(kind, Lin, zc, z16)
    rng = np.random.default_rng(pair[0] + 7 * m + len(kind))
    slots = rng.permutation(70)[:64]
    rig = _Rig(pair, Lin, L16, 70, slots, seed=pair[0] * 3 + m)
    for k in range(5):
        rig.push(rng.permutation(slots))


@pytest.mark.parametrize("pair", [(250, 150), (22050, 16000), EQUAL], ids=["250_150", "22050_16000", "equal"])
def test_streams_that_advance_at_different_times(pair):
    """N = 1 and N = 3 with another subset of 6 live slots per push: every slot keeps its own plane."""
    zc, z16, _, _ = RA.units(*pair)
    live = np.array([5, 0, 8, 3, 9, 6])
    rig = _Rig(pair, 2 * zc, 9 * z16 + (1 if pair == EQUAL else 0), 10, live, seed=11)
    rng = np.random.default_rng(12)
    counts = np.zeros(10, int)
    for k in range(10):
        slots = rng.permutation(live)[:1 if k % 2 else 3]
        rig.push(slots)
        counts[slots] += 1
    _, tickets = RA.ring_planes(rig.ring, 10, rig.L16)
    assert np.array_equal(RA.current_plane(tickets, rig.tiles), counts & 1) and len(set(counts[live].tolist())) > 1


@pytest.mark.parametrize("pair", RA.PAIRS, ids=[f"{a}_{b}" for a, b in RA.PAIRS])
def test_new_samples_against_float64(pair):
    """The new samples of a push within `resample_cases.fp32_bound` of `push_model`; the kept ones are the old ring's."""
    zc, z16, _, _ = RA.units(*pair)
    Lin, L16 = 9 * zc, 14 * z16
    slots = np.array([2, 0, 3])
    rig = _Rig(pair, Lin, L16, 4, slots, seed=21)
    before, hist = rig.cur.copy(), rig.hist.copy()
    x, ctx = rig.push(slots)
    for k, s in enumerate(slots):
        c, h = RA.push_model(hist[s], before[s], x[k, 2 * zc:], *pair, zc, z16)
        bound = RA.push_bound(hist[s], np.zeros(L16), x[k, 2 * zc:], *pair, zc, z16)
        err = np.abs(ctx[k] - c)
        print(f"{pair}: stream {k}: max |device - float64| {err.max():.3e}, bound there {bound[err.argmax()]:.3e}")
        assert (err <= bound).all() and err[:L16 - 10 * z16].max() == 0 and bound[L16 - 10 * z16:].min() > 0
        assert np.array_equal(RA.push_model_fp32(hist[s], before[s], x[k, 2 * zc:], *pair, zc, z16)[0], ctx[k])     # the numpy FMA chain


@pytest.mark.parametrize("pair", [(22050, 16000), (250, 150)], ids=["22050_16000", "250_150"])
def test_streamed_equals_one_shot(pair):
    """Six blocks of one signal from an empty state: at the supported positions (rt_audio_cases.supported) the final context is
    `audio.Resample` of the whole signal, bit for bit.  (250, 150): width 11 > zc 5, so samples near a block's seams are excluded
    too; most of a 9 zc block is supported."""
    from seedvc_amd import _lib
    zc, z16, _, _ = RA.units(*pair)
    Lin, L16, pushes = 9 * zc, 40 * z16, 6
    signal = RC.noise(f"rt_audio.gpu.stream.{pair[0]}", 6, 2, pushes * Lin).to(DEV)
    hist = torch.zeros(3, 2 * zc, device=DEV)
    ring = torch.zeros(int(_lib.lib().svc_rt_ring_floats(3, L16)), device=DEV)
    ctx = torch.empty(2, L16, device=DEV)
    for b in range(pushes):
        _lib.check(_push(pair, signal[:, b * Lin:(b + 1) * Lin].contiguous(), [2, 0], 3, hist, ring, L16, ctx))
    Y = _resample(pair)(signal).cpu().numpy()
    M, ok = RA.supported(*pair, Lin, L16, pushes)
    planes, tickets = RA.ring_planes(ring.cpu().numpy(), 3, L16)
    plane = RA.current_plane(tickets, int(_lib.lib().svc_rt_push_tiles(L16)))
    assert plane.tolist() == [0, 0, 0] and ok.sum() > L16 // 2
    for k, s in enumerate([2, 0]):
        got = planes[plane[s], s]
        assert np.array_equal(bits(got), bits(ctx[k].cpu().numpy()))
        assert np.array_equal(bits(got[ok]), bits(Y[k][M[ok]])), s
    if pair == (22050, 16000):                               # width <= zc: only the end of the context is excluded
        assert np.flatnonzero(~ok & (M >= 0)).min() >= L16 - RA.excluded_cap(*pair)


# ------------------------------------------------------------------------------------ the engine with the exact stand-ins
FAKE_PAIR, FAKE_M, FAKE_L16, FAKE_CE = (22050, 16000), 2, 8 * 320, 0.04          # blocks of 2 zc; 8 content rows, 2 dropped


def _fake_refs():
    return [(cases.randn(f"rt.pc{s}", 142, 1, P, cases.CHUNK_DC).to(DEV), cases.logmel(f"rt.mel{s}", 142, 1, cases.CHUNK_C, P).to(DEV),
             cases.randn(f"rt.style{s}", 142, 1, 3).to(DEV)) for s, P in enumerate(RT.FAKE_PROMPTS)]


def _fake_engine(max_streams=4):
    from seedvc_amd.pipeline import RealtimeEngine
    cfm, voc = LB.BatchedFakeCFM(DEV), RT.FakeVocoder()
    eng = RealtimeEngine(RT.FakeLR(), cfm, voc, max_streams=max_streams, **RT.FAKE_GEOMETRY)
    eng.attach_audio(RA.FakeContent(), _resample(FAKE_PAIR), FAKE_M * 441, FAKE_L16, FAKE_CE)
    return eng, cfm, voc


_session_cache = {}


def _sessions():
    """Per stream: the audio blocks and the numpy session (push_model_fp32 -> fake_content -> realtime_cases.session_model);
    computed once."""
    if not _session_cache:
        fi, fo = RT.gui_windows(RT.FAKE_GEOMETRY["sola_buffer"])
        zc, z16, _, _ = RA.units(*FAKE_PAIR)
        audio, ctxs, contents, models = [], [], [], []
        for s in range(3):
            blocks = (RC.noise(f"rt_audio.session{s}", 31, 5, FAKE_M * zc) * 0.5).numpy()
            hist, ring = np.zeros(2 * zc, np.float32), np.zeros(FAKE_L16, np.float32)
            cs, xs = [], []
            for k in range(5):
                ring, hist = RA.push_model_fp32(hist, ring, blocks[k], *FAKE_PAIR, zc, z16)
                cs.append(ring)
                xs.append(RA.fake_content(ring)[int(FAKE_CE * 50):])
            audio.append(blocks)
            ctxs.append(cs)
            contents.append(xs)
            models.append(RT.session_model(xs, fi, fo))
        _session_cache.update(audio=audio, ctx=ctxs, content=contents, models=models)
    return _session_cache


def _audio(sess, streams, k):
    return torch.from_numpy(np.stack([sess["audio"][s][k] for s in streams])).to(DEV)


def _check_step(sess, eng, slots, streams, k, out, parts):
    for row, s in enumerate(streams):
        want_out, want_new, want_o, scores, before = sess["models"][s][k]
        assert np.array_equal(parts["ctx"][row].cpu().numpy(), sess["ctx"][s][k]), (s, k)
        assert np.array_equal(parts["content"][row].cpu().numpy(), sess["content"][s][k]), (s, k)
        assert int(parts["offsets"][row]) == want_o, (s, k, RT.score_gap(scores))
        assert np.array_equal(out[row].cpu().numpy(), want_out), (s, k)
        assert np.array_equal(eng.state[slots[s]].cpu().numpy(), want_new), (s, k)
        assert np.array_equal(eng.audio_context(slots[s]).cpu().numpy(), sess["ctx"][s][k]), (s, k)


def test_three_streams_from_audio_equal_the_numpy_session():
    sess = _sessions()
    eng, cfm, voc = _fake_engine()
    slots = [eng.open(*r) for r in _fake_refs()]
    for k in range(5):
        order = [0, 1, 2] if k < 3 else [2, 0, 1]
        out, parts = eng.step_audio([slots[s] for s in order], _audio(sess, order, k), 10, 0.7, return_parts=True)
        assert out.shape == (3, RT.FAKE_GEOMETRY["block"]) and parts["ctx"].shape == (3, FAKE_L16)
        assert parts["content"].shape == (3, 6, cases.CHUNK_DC)
        _check_step(sess, eng, slots, order, k, out, parts)
    assert cfm.batch_sizes == [3] * 5 and voc.calls == [(3, 12)] * 5
    a = eng._audio
    assert not a["planes"][:, 3].any() and not a["hist"][3].any() and not eng.state[3].any()
    assert all(RT.score_gap(m[3]) > 1e-4 for ms in sess["models"] for m in ms[1:])      # no block is decided by a near tie


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_each_stream_alone_from_audio_equals_the_numpy_session(stream):
    sess = _sessions()
    eng, _, _ = _fake_engine(max_streams=1)
    slot = eng.open(*_fake_refs()[stream])
    slots = {stream: slot}
    for k in range(5):
        out, parts = eng.step_audio([slot], _audio(sess, [stream], k), 10, 0.7, return_parts=True)
        _check_step(sess, eng, slots, [stream], k, out, parts)


def test_reset_and_a_reopened_slot_start_from_an_empty_context():
    sess = _sessions()
    eng, _, _ = _fake_engine()
    refs = _fake_refs()
    slots = [eng.open(*r) for r in refs]
    for k in range(3):                                       # an odd number of pushes: the slots' current plane is 1
        eng.step_audio(slots, _audio(sess, [0, 1, 2], k), 10, 0.7)
    eng.close(1)
    assert eng.open(*refs[2]) == 1
    eng.reset(0)
    out, parts = eng.step_audio([0, 1], _audio(sess, [0, 2], 0), 10, 0.7, return_parts=True)
    _check_step(sess, eng, {0: 0, 2: 1}, [0, 2], 0, out, parts)


def test_a_step_from_audio_does_not_synchronise():
    watch = hasattr(torch.cuda, "set_sync_debug_mode")
    sess = _sessions()
    eng, _, _ = _fake_engine()
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
        out1 = eng.step_audio(slots, xs[1], 10, 0.7)
        out2, parts = eng.step_audio(slots, xs[2], 10, 0.7, return_parts=True)
    finally:
        if watch:
            torch.cuda.set_sync_debug_mode(before)
    for s in range(3):
        assert np.array_equal(out1[s].cpu().numpy(), sess["models"][s][1][0])
    _check_step(sess, eng, slots, [0, 1, 2], 2, out2, parts)


# ------------------------------------------------------------------------------------------------------- a real encoder
@pytest.mark.parametrize("precision", [0, 1])
def test_step_audio_equals_step_on_the_returned_context(precision):
    """W.CFG_S behind the tiny_r DiT, a regulator as wide as the encoder and BigVGAN (hop 8); 2 streams, 3 blocks of 2 zc samples,
    a context of 12 rows.  Engine A steps from audio; engine B is given `semantic_fn(ctx)[:, ce:]` of A's context and the same
    z: the blocks and the SOLA buffers are equal bit for bit.  A's context against the float64 push model within the fp32 bound
    every sample carries."""
    from seedvc_amd import specs, weights
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import RealtimeEngine
    from seedvc_amd.vocoder import BigVGAN
    from seedvc_amd.wav2vec2 import Wav2Vec2Content
    pair, S, ce_dit = (22050, 16000), 40, 0.04
    zc, z16, _, _ = RA.units(*pair)
    Lin, L16, ce = 2 * zc, 12 * z16, 2
    cfg, sd, _, _ = cases.dit_case("tiny_r")
    lcfg = specs.lr_config("tiny", channels=64, in_channels=W.CFG_S["d_model"], out_channels=cfg["Dc"])
    lr = InterpolateRegulator(lcfg, weights.make_state_dict(specs.lr_state_spec(lcfg), seed=75, prefix="lr."), DEV)
    cfm = CFM(cfg, sd, DEV)
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")
    voc = BigVGAN(h, vsd, DEV)
    w2v = Wav2Vec2Content(W.make_state_dict(W.CFG_S, seed=21), W.CFG_S, device=DEV, precision=precision)
    engines = [RealtimeEngine(lr, cfm, voc, S, 8, 96, 32, 16, tail=8, max_streams=3) for _ in range(2)]
    engines[0].attach_audio(w2v, _resample(pair), Lin, L16, ce_dit)
    prompts = (16, 11)
    refs = [(cases.randn(f"rt_audio.real.pc{i}", 145, 1, P, cfg["Dc"]), cases.logmel(f"rt_audio.real.mel{i}", 145, 1, cfg["C"], P),
             cases.randn(f"rt_audio.real.style{i}", 145, 1, cfg["style_dim"])) for i, P in enumerate(prompts)]
    for e in engines:
        assert [e.open(*refs[0]), e.open(*refs[1])] == [0, 1]
    slots = [1, 0]
    hist = np.zeros((2, 2 * zc), np.float32)
    ring, bound = np.zeros((2, L16)), np.zeros((2, L16))
    for k in range(3):
        audio = RC.noise(f"rt_audio.real.audio{k}", 145, 2, Lin) * 0.3
        z = cases.randn(f"rt_audio.real.z{k}", 145, 2, cfg["C"], max(prompts) + S).to(DEV)
        out_a, parts = engines[0].step_audio(slots, audio.to(DEV), 3, 0.7, z=z, return_parts=True)
        ctx = parts["ctx"]
        content = w2v.semantic_fn(ctx)[:, ce:]
        assert ctx.shape == (2, L16) and content.shape == (2, W.frames(W.CFG_S, L16) - ce, W.CFG_S["d_model"])
        assert torch.equal(parts["content"], content)
        out_b = engines[1].step(slots, content, 3, 0.7, z=z)
        assert torch.equal(out_a, out_b) and torch.equal(engines[0].state, engines[1].state), k
        assert bool(torch.isfinite(out_a).all()) and bool(out_a.abs().max() > 0)
        for row in range(2):
            bound[row] = RA.push_bound(hist[row], bound[row], audio[row].numpy(), *pair, zc, z16)
            ring[row], hist[row] = RA.push_model(hist[row], ring[row], audio[row].numpy(), *pair, zc, z16)
        err = np.abs(ctx.cpu().numpy() - ring)
        print(f"precision {precision}, block {k}: max |ctx - float64 model| {err.max():.3e}")
        assert (err <= bound).all(), k


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_every_refusal_leaves_the_state_untouched():
    """(250, 150): o 5, n 3, zc 5, z16 3.  The good call's arguments with one thing wrong each: non-zero, a message, and hist,
    ring and ctx keep every bit."""
    from seedvc_amd import _lib
    pair, ms, L16, Lin = (250, 150), 4, 40, 10
    rng = np.random.default_rng(3)
    hist0 = rng.uniform(-1, 1, (ms, 10)).astype(np.float32)
    n_ring = int(_lib.lib().svc_rt_ring_floats(ms, L16))
    ring0 = rng.uniform(-1, 1, n_ring).astype(np.float32)
    ring0[2 * ms * L16:] = 0
    ctx0 = rng.uniform(-1, 1, (2, L16)).astype(np.float32)
    hist, ring, ctx = (torch.from_numpy(a.copy()).to(DEV) for a in (hist0, ring0, ctx0))
    block = torch.from_numpy(rng.uniform(-1, 1, (2, 12)).astype(np.float32)).to(DEV)
    big = torch.zeros(65, 12, device=DEV)
    bad = dict(Lin_zero=dict(Lin=0), Lin_off_the_grid=dict(Lin=12), L16_below_n_new=dict(L16=8),
               zc_not_a_multiple_of_o=dict(zc=4, Lin=8), z16_not_a_multiple_of_n=dict(z16=4),
               x_too_short=dict(z16=6), N_zero=dict(slots=[]), N_65=dict(block=big, slots=list(range(65)), max_slots=70),
               slot_above=dict(slots=[0, 4]), slot_negative=dict(slots=[-1, 0]), slot_twice=dict(slots=[1, 1]),
               stride_below_Lin=dict(stride=9), null_block=dict(block=None), null_hist=dict(hist=None), null_ring=dict(ring=None),
               null_ctx=dict(ctx=None), ctx_in_ring=dict(ctx=ring[8:]), hist_in_ring=dict(hist=ring[2 * L16:]),
               block_is_hist=dict(block=hist[:2]), ctx_is_block=dict(ctx=block))
    for name, kw in bad.items():
        a = dict(block=block, slots=[3, 1], max_slots=ms, hist=hist, ring=ring, L16=L16, ctx=ctx, zc=5, z16=3, Lin=Lin, stride=12)
        a.update(kw)
        blk = a.pop("block")
        if blk is None:
            rc = _lib.lib().svc_rt_push(_resample(pair)._h, None, 12, Lin, 2, _lib.i32_host([3, 1]), ms, 5, 3, _lib.ptr(hist), _lib.ptr(ring),
                                        L16, _lib.ptr(ctx), _lib.stream_ptr())
        else:
            rc = _push(pair, blk, a.pop("slots"), a.pop("max_slots"), a.pop("hist"), a.pop("ring"), a.pop("L16"), a.pop("ctx"), **a)
        assert rc != 0, name
        assert b"rt_push" in _lib.lib().svc_last_error(), name
    torch.cuda.synchronize()
    assert np.array_equal(bits(hist.cpu().numpy()), bits(hist0)) and np.array_equal(bits(ring.cpu().numpy()), bits(ring0))
    assert np.array_equal(bits(ctx.cpu().numpy()), bits(ctx0))
    # and the good call is good
    _lib.check(_push(pair, block, [3, 1], ms, hist, ring, L16, ctx, Lin=Lin, stride=12))
    torch.cuda.synchronize()
    assert not np.array_equal(ctx.cpu().numpy(), ctx0)
