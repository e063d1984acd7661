"""GPU side of the live block step.  `svc_rt_out` bit for bit against `svc_resample` followed by `svc_sola_step`,
its mute, and within the fp32 bounds of the float64 statement (rt_live_cases.py); `svc_sola_step` as the form of that kernel
without the prologue; `svc_rt_push_gated` against the float64 gate decisions and, on the host-gated audio, bit for bit against
`svc_rt_push`; `RealtimeEngine.attach_output` / `set_speech` / `set_gate` against the numpy sessions with exactly rounded
stand-ins; an engine that uses none of them against the calls it made before; and every refusal with the state untouched.

Where the issue's wording of the mute test ("its new state is zeros") and the contract (the splice runs on a row of +0.0)
differ, the contract holds: with block < Lb the first Lb - block samples of the new buffer are the faded old buffer,
fl(b fade_out), and only the rest is zero (`_muted_expectation`); with block >= Lb the buffer is all zero."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB
import realtime_cases as RT
import resample_cases as RC
import rt_audio_cases as RA
import rt_live_cases as LV

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
i32 = lambda v: (C.c_int32 * len(v))(*[int(x) for x in v])      # noqa: E731
f32 = lambda v: (C.c_float * len(v))(*[float(x) for x in v])    # noqa: E731
bits = lambda t: t.contiguous().view(torch.int32)                # noqa: E731  (NaN rows and signed zeros compare as integers)
same = lambda a, b: a.shape == b.shape and torch.equal(bits(a), bits(b))      # noqa: E731
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)             # noqa: E731
OUT_IDS = [f"{a}_{b}" for a, b in LV.OUT_PAIRS]
GATE_IDS = [f"{a}_{b}" for a, b in LV.GATE_PAIRS]
START, EXTRA = 3, 2
_resamplers = {}


def _resample(pair):
    from seedvc_amd.audio import Resample
    if pair not in _resamplers:
        _resamplers[pair] = Resample(*pair, device=DEV)
    return _resamplers[pair]


def _handle(pair):
    return None if pair[0] == pair[1] else _resample(pair)._h


# =========================================================================================================== svc_rt_out
class _Out:
    """The arguments of one output case on the device: geometry, windows and a state of MAX_SLOTS rows."""

    def __init__(self, pair, Lb_units, state):
        self.pair = pair
        self.zc_m, self.zc_o, self.gm, self.go = LV.out_units(pair, Lb_units)
        self.n_in = self.gm["block"] + self.gm["Lb"] + self.gm["Ls"]
        self.fi, self.fo = (dev(w) for w in RT.gui_windows(self.go["Lb"]))
        self.state = dev(state)

    def fresh(self, n=3):
        g = self.go
        return (torch.full((n, g["n_inf"]), float("nan"), device=DEV), torch.full((n, g["block"]), float("nan"), device=DEV),
                torch.full((n,), -1, dtype=torch.int32, device=DEV))

    def rt_out(self, w, speech=None, sl=LV.SLOTS, **over):
        """One svc_rt_out on this state -> (rc, infer, out, offsets)."""
        from seedvc_amd import _lib
        g = self.go
        infer, out, offs = self.fresh(len(sl))
        a = dict(r=_handle(self.pair), wave=_lib.ptr(w), stride=w.stride(0), start=START, n_in=self.n_in, N=len(sl),
                 state=_lib.ptr(self.state), max_slots=LV.MAX_SLOTS, slots=i32(sl), speech=None if speech is None else i32(speech),
                 fi=_lib.ptr(self.fi), fo=_lib.ptr(self.fo), block=g["block"], Lb=g["Lb"], Ls=g["Ls"], infer=_lib.ptr(infer),
                 out=_lib.ptr(out), offs=_lib.ptr(offs))
        a.update(over)
        rc = _lib.lib().svc_rt_out(a["r"], a["wave"], a["stride"], a["start"], a["n_in"], a["N"], a["state"], a["max_slots"], a["slots"],
                                   a["speech"], a["fi"], a["fo"], a["block"], a["Lb"], a["Ls"], a["infer"], a["out"], a["offs"],
                                   _lib.stream_ptr())
        return rc, infer, out, offs

    def composed(self, wave, zero_rows=()):
        """svc_resample on the slice (rows in zero_rows replaced by +0.0), then svc_sola_step -> (infer, out, offsets)."""
        from seedvc_amd import _lib
        g = self.go
        seg = wave[:, START:START + self.n_in].contiguous()
        y = _resample(self.pair)(seg).clone()                         # out of inference mode: rows are zeroed below
        assert y.shape == (3, g["n_inf"])
        for k in zero_rows:
            y[k] = 0.0
        _, out, offs = self.fresh()
        _lib.check(_lib.lib().svc_sola_step(_lib.ptr(y), g["n_inf"], 0, 3, _lib.ptr(self.state), LV.MAX_SLOTS, i32(LV.SLOTS),
                                            _lib.ptr(self.fi), _lib.ptr(self.fo), g["block"], g["Lb"], g["Ls"], _lib.ptr(out),
                                            _lib.ptr(offs), _lib.stream_ptr()))
        return y, out, offs


@pytest.mark.parametrize("Lb_units", [1, 4])
@pytest.mark.parametrize("pair", LV.OUT_PAIRS, ids=OUT_IDS)
def test_rt_out_equals_resample_then_sola_step(pair, Lb_units):
    """Three consecutive steps of 3 streams in slots (4, 0, 2) of 5 from a noise buffer: out, state (every row, the NaN rows of
    the other slots included), offsets and infer are those of the two-call composition, bit for bit."""
    from seedvc_amd import _lib
    wave, state = LV.out_waves(pair, Lb_units, START, EXTRA)
    a, b = _Out(pair, Lb_units, state), _Out(pair, Lb_units, state)
    for t in range(3):
        w = dev(wave[t])
        rc, infer, out, offs = a.rt_out(w)
        _lib.check(rc)
        infer2, out2, offs2 = b.composed(w)
        assert same(infer, infer2) and same(out, out2) and torch.equal(offs, offs2) and same(a.state, b.state), (pair, Lb_units, t)
        assert bool(torch.isfinite(out).all()) and bool(((offs >= 0) & (offs <= a.go["Ls"])).all())
    assert not same(a.state, dev(state))


SOLA_FORMS = [("x4_aligned", 64, 16, 12, 8, 8), ("block_lt_Lb_scalar", 7, 30, 9, 2, 3), ("gui_scalar", 3969, 882, 441, 10907, 441)]


@pytest.mark.parametrize("name,block,Lb,Ls,start,extra", SOLA_FORMS, ids=[c[0] for c in SOLA_FORMS])
def test_sola_step_is_rt_out_without_the_prologue(name, block, Lb, Ls, start, extra):
    """70 streams (two launches) on permuted slots: `svc_sola_step` and `svc_rt_out(r = NULL, speech = NULL)` give the same out,
    state and offsets, and infer is the slice."""
    from seedvc_amd import _lib
    rng = np.random.default_rng(len(name) + block)
    N, ms, n_inf = 70, 80, block + Lb + Ls
    stride = start + n_inf + extra
    slots = rng.permutation(ms)[:N]
    wave = dev(rng.standard_normal((N, stride)).astype(np.float32))
    state0 = rng.standard_normal((ms, Lb)).astype(np.float32)
    fi, fo = (dev(w) for w in RT.gui_windows(Lb))
    res = []
    for live in (False, True):
        st, out = dev(state0), torch.full((N, block), float("nan"), device=DEV)
        offs, infer = torch.full((N,), -1, dtype=torch.int32, device=DEV), torch.full((N, n_inf), float("nan"), device=DEV)
        if live:
            _lib.check(_lib.lib().svc_rt_out(None, _lib.ptr(wave), stride, start, n_inf, N, _lib.ptr(st), ms, i32(slots), None, _lib.ptr(fi),
                                             _lib.ptr(fo), block, Lb, Ls, _lib.ptr(infer), _lib.ptr(out), _lib.ptr(offs), _lib.stream_ptr()))
            assert same(infer, wave[:, start:start + n_inf])
        else:
            _lib.check(_lib.lib().svc_sola_step(_lib.ptr(wave), stride, start, N, _lib.ptr(st), ms, i32(slots), _lib.ptr(fi), _lib.ptr(fo),
                                                block, Lb, Ls, _lib.ptr(out), _lib.ptr(offs), _lib.stream_ptr()))
        res.append((st, out, offs))
    assert same(res[0][0], res[1][0]) and same(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert len(set(res[0][2].tolist())) > 1


def _muted_expectation(before, fo, block):
    """A row of +0.0 spliced onto the buffer b: the offset is 0, y[:Lb] = fl(fl(0 fade_in) + fl(b fade_out)) = fl(b fade_out),
    y[Lb:] = 0 -> (out (block,), new buffer (Lb,))."""
    Lb = before.numel()
    y = torch.cat([before * fo, torch.zeros(block, device=DEV)])
    return y[:block], y[block:block + Lb]


@pytest.mark.parametrize("Lb_units", [1, 4])
@pytest.mark.parametrize("pair", LV.OUT_PAIRS, ids=OUT_IDS)
def test_rt_out_mutes_a_stream_without_speech(pair, Lb_units):
    """Step 2 of the middle stream with speech = 0: its infer row is +0.0, its offset 0, its output the old buffer's fade-out and
    then zeros, its new buffer what the splice of zeros leaves (all zero where block >= Lb); the other two streams are those of
    the run without a mute, bit for bit; step 3 of the muted stream is a step from the buffer the mute left."""
    from seedvc_amd import _lib
    wave, state = LV.out_waves(pair, Lb_units, START, EXTRA)
    a, b, c = (_Out(pair, Lb_units, state) for _ in range(3))       # a: with the mute, b: without, c: the composition with a zero row
    block, Lb = a.go["block"], a.go["Lb"]
    for t in range(3):
        w = dev(wave[t])
        before = a.state[LV.SLOTS[1]].clone()
        rc, infer, out, offs = a.rt_out(w, speech=[1, 0, 1] if t == 1 else ([1, 1, 1] if t == 0 else None))
        _lib.check(rc)
        rc_b, infer_b, out_b, offs_b = b.rt_out(w)
        _lib.check(rc_b)
        infer_c, out_c, offs_c = c.composed(w, zero_rows=(1,) if t == 1 else ())
        assert same(infer, infer_c) and same(out, out_c) and torch.equal(offs, offs_c) and same(a.state, c.state), t
        for k in (0, 2):                                              # the other streams never notice
            s = LV.SLOTS[k]
            assert same(infer[k], infer_b[k]) and same(out[k], out_b[k]) and int(offs[k]) == int(offs_b[k]) and same(a.state[s], b.state[s])
        if t == 0:
            assert same(a.state, b.state)
        if t == 1:
            want_out, want_new = _muted_expectation(before, a.fo, block)
            assert same(infer[1], torch.zeros(a.go["n_inf"], device=DEV))                    # +0.0, bit for bit
            assert int(offs[1]) == 0
            assert torch.equal(out[1], want_out) and torch.equal(a.state[LV.SLOTS[1]], want_new)
            assert not out[1, Lb:].any() and not a.state[LV.SLOTS[1], max(Lb - block, 0):].any()
            if block >= Lb:
                assert not a.state[LV.SLOTS[1]].any()
            assert bool(out[1, :min(Lb, block)].abs().max() > 0)
            assert not same(out[1], out_b[1])
        if t == 2:                                                    # a step from the buffer the mute left
            d = _Out(pair, Lb_units, state)
            d.state[LV.SLOTS[1]] = _muted_expectation(before_mute, a.fo, block)[1]
            _, out_d, offs_d = d.composed(w)
            assert same(out[1], out_d[1]) and int(offs[1]) == int(offs_d[1]) and same(a.state[LV.SLOTS[1]], d.state[LV.SLOTS[1]])
        if t == 1:
            before_mute = before


@pytest.mark.parametrize("Lb_units", [1, 4])
@pytest.mark.parametrize("pair", LV.OUT_PAIRS, ids=OUT_IDS)
def test_rt_out_against_float64(pair, Lb_units):
    """`resample_dense` followed by the float64 splice, per step from the device's own buffer before it.  Precondition (asserted
    on the host, not a skip): every case's float64 score gap is at least 1e-3, so the offsets must be equal.  The samples are
    within `resample_cases.fp32_bound` of the row, scaled by the window where they are faded, plus three fp32 roundings of the
    fade terms, (|y fi| + |b fo|) 2^-23 1.5."""
    from seedvc_amd import _lib
    wave, state = LV.out_waves(pair, Lb_units, START, EXTRA)
    a = _Out(pair, Lb_units, state)
    g = a.go
    fi, fo = RT.gui_windows(g["Lb"])
    worst = 0.0
    for t in range(3):
        before = a.state.cpu().numpy()
        rc, infer, out, offs = a.rt_out(dev(wave[t]))
        _lib.check(rc)
        infer, out, offs, after = infer.cpu().numpy(), out.cpu().numpy(), offs.cpu().numpy(), a.state.cpu().numpy()
        for k, s in enumerate(LV.SLOTS):
            seg = wave[t, k, START:START + a.n_in]
            y64, yb = LV.resample64(pair, seg), LV.resample_bound(pair, seg)
            want_out, want_new, o, scores, fade = LV.splice64(y64, before[s], fi, fo, g["block"], g["Ls"])
            assert RT.score_gap(scores) >= LV.GAP, (pair, Lb_units, t, k, RT.score_gap(scores))       # the precondition
            assert int(offs[k]) == o, (t, k, int(offs[k]), o)
            assert (np.abs(infer[k] - y64) <= yb).all(), (t, k)
            bound = yb[o:o + g["block"] + g["Lb"]].copy()
            bound[:g["Lb"]] = bound[:g["Lb"]] * np.abs(fi.astype(np.float64)) + fade[:g["Lb"]]
            bound += np.abs(np.concatenate([want_out, want_new])) * 2.0 ** -52                      # the float64 statement's own rounding
            err = np.abs(np.concatenate([out[k], after[s]]) - np.concatenate([want_out, want_new]))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if bound.max() > 0 else 0.0)
            assert (err <= bound).all(), (t, k, float(err.max()))
    print(f"{pair}, Lb {Lb_units}: worst |device - float64| / bound = {worst:.3f}")


def test_rt_out_refusals_leave_everything_untouched():
    """(150, 250), block 2, Lb 1, Ls 1 units: the good call's arguments with one thing wrong each."""
    from seedvc_amd import _lib
    pair = (150, 250)
    wave, state = LV.out_waves(pair, 1, START, EXTRA)
    a = _Out(pair, 1, state)
    w = dev(wave[0])
    g = a.go
    state0 = a.state.clone()
    other = _resample((22050, 48000))._h                              # n_in 12 -> 27 samples, not block + Lb + Ls = 20
    big = torch.zeros(20000, device=DEV)
    bad = dict(n_in_short=dict(n_in=a.n_in - 1), n_in_long=dict(n_in=a.n_in + 1, stride=100), wrong_rates=dict(r=other),
               equal_rates_but_lengths_differ=dict(r=None), past_the_row=dict(stride=START + a.n_in - 1), start_past=dict(start=START + EXTRA + 1),
               infer_null=dict(infer=None), speech_2=dict(speech=i32([1, 2, 0])), speech_minus_1=dict(speech=i32([-1, 1, 1])),
               slot_twice=dict(slots=i32([4, 4, 2])), slot_above=dict(slots=i32([4, 0, 5])), slot_negative=dict(slots=i32([-1, 0, 2])),
               block_zero=dict(block=0), Lb_zero=dict(Lb=0), Ls_negative=dict(Ls=-1), block_plus_one=dict(block=g["block"] + 1),
               search_above_the_lds=dict(Lb=8000, Ls=200, block=20, n_in=4932, r=_handle(pair), wave=_lib.ptr(big), stride=6000),
               null_wave=dict(wave=None), null_state=dict(state=None), null_fade=dict(fi=None), negative_start=dict(start=-1))
    outs = []
    for name, kw in bad.items():
        rc, infer, out, offs = a.rt_out(w, **kw)
        assert rc != 0, name
        assert b"rt_out" in _lib.lib().svc_last_error(), name
        outs.append((name, infer, out, offs))
    for name, over in (("infer_is_out", "out"), ("infer_is_state", "state"), ("infer_is_fade_in", "fi"), ("infer_in_wave", "wave")):
        tgt = dict(out=None, state=a.state, fi=a.fi, wave=w)[over]
        if tgt is None:
            infer, out, offs = a.fresh()
            rc = a.rt_out(w, infer=_lib.ptr(out), out=_lib.ptr(out))[0]
        else:
            rc = a.rt_out(w, infer=_lib.ptr(tgt))[0]
        assert rc != 0 and b"rt_out" in _lib.lib().svc_last_error(), name
    torch.cuda.synchronize()
    assert same(a.state, state0) and same(w, dev(wave[0]))
    for name, infer, out, offs in outs:
        assert bool(torch.isnan(infer).all()) and bool(torch.isnan(out).all()) and bool((offs == -1).all()), name
    rc, infer, out, offs = a.rt_out(w)                                # and the good call is good
    _lib.check(rc)
    assert bool(torch.isfinite(out).all()) and not same(a.state, state0)


# ==================================================================================================== svc_rt_push_gated
class _Push:
    """Device state of the push calls for MAX_SLOTS streams: the rows of SLOTS are a fresh stream (zeros), every other row of
    hist, of both planes and of gate_e holds a sentinel that must keep its bits (NaN; 7.0 in gate_e)."""

    def __init__(self, pair, m, L16=None):
        from seedvc_amd import _lib
        self.pair, self.m = pair, m
        self.zc, self.z16, _, _ = RA.units(*pair)
        self.Lin = m * self.zc
        self.L16 = (m + 5) * self.z16 if L16 is None else L16
        ms = LV.MAX_SLOTS
        self.n_planes = 2 * ms * self.L16
        ring = np.zeros(int(_lib.lib().svc_rt_ring_floats(ms, self.L16)), np.float32)
        planes, _ = RA.ring_planes(ring, ms, self.L16)
        rest = [s for s in range(ms) if s not in LV.SLOTS]
        planes[:, rest] = np.nan
        hist = np.zeros((ms, 2 * self.zc), np.float32)
        hist[rest] = np.nan
        ge = np.zeros((ms, 3), np.float32)
        ge[rest] = 7.0
        self.ring, self.hist, self.ge = dev(ring), dev(hist), dev(ge)

    def push(self, sl, blocks, pows="plain", mask=True, **over):
        """blocks (n, Lin) numpy; pows: "plain" = svc_rt_push, None = the gated entry with gate_pow NULL, else n thresholds
        -> (rc, ctx, gate_mask | None)."""
        from seedvc_amd import _lib
        n = len(sl)
        d_block = dev(blocks)
        ctx = torch.full((n, self.L16), float("nan"), device=DEV)
        a = dict(block=_lib.ptr(d_block), stride=d_block.stride(0), Lin=self.Lin, N=n, slots=i32(sl), max_slots=LV.MAX_SLOTS, zc=self.zc,
                 z16=self.z16, hist=_lib.ptr(self.hist), ring=_lib.ptr(self.ring), L16=self.L16, ctx=_lib.ptr(ctx))
        if isinstance(pows, str):
            a.update(over)
            rc = _lib.lib().svc_rt_push(_handle(self.pair), a["block"], a["stride"], a["Lin"], a["N"], a["slots"], a["max_slots"], a["zc"],
                                        a["z16"], a["hist"], a["ring"], a["L16"], a["ctx"], _lib.stream_ptr())
            return rc, ctx, None
        gm = torch.full((n, self.m), -1, dtype=torch.int32, device=DEV) if mask else None
        a.update(pow=None if pows is None else f32(pows), ge=_lib.ptr(self.ge), gm=_lib.ptr(gm))
        a.update(over)
        rc = _lib.lib().svc_rt_push_gated(_handle(self.pair), a["block"], a["stride"], a["Lin"], a["N"], a["slots"], a["max_slots"], a["zc"],
                                          a["z16"], a["hist"], a["ring"], a["L16"], a["ctx"], a["pow"], a["ge"], a["gm"], _lib.stream_ptr())
        return rc, ctx, gm

    def snapshot(self):
        return self.hist.clone(), self.ring.clone(), self.ge.clone()


def _assert_twins(a, b, ctx_a, ctx_b, tag):
    """ctx, hist and the whole ring buffer (both planes and the tickets) of a gated rig and of the plain one."""
    assert same(ctx_a, ctx_b), ("ctx", tag)
    assert same(a.hist, b.hist), ("hist", tag)
    assert same(a.ring[:a.n_planes], b.ring[:b.n_planes]), ("ring planes", tag)
    assert same(a.ring[a.n_planes:], b.ring[b.n_planes:]), ("tickets", tag)


def _streams(pair, m):
    zc = pair[0] // 50
    return [LV.gate_audio(loud, 6 * m, zc, seed=100 * m + s).reshape(6, m * zc) for s, loud in enumerate(LV.LOUD_FRAMES[m])]


@pytest.mark.parametrize("m", [1, 9])
@pytest.mark.parametrize("pair", LV.GATE_PAIRS, ids=GATE_IDS)
def test_gated_push_mutes_the_frames_of_the_float64_gate(pair, m):
    """Six pushes of three streams at -40 dB: gate_mask is the float64 decision for every frame (all of them are at least 25
    times off the threshold: none is excluded), and ctx, hist, both ring planes and the tickets are those of a plain
    `svc_rt_push` fed the host-masked audio, bit for bit.  With m = 1 every decision uses the carried energies."""
    from seedvc_amd import _lib
    a, b = _Push(pair, m), _Push(pair, m)
    audio = _streams(pair, m)
    power = LV.gate_power(LV.GATE_DB, a.zc)
    carry = [(0.0, 0.0, 0.0)] * 3
    seen = []
    for t in range(6):
        order = [0, 1, 2] if t % 2 == 0 else [2, 0, 1]
        slots = [LV.SLOTS[s] for s in order]
        raw = np.stack([audio[s][t] for s in order])
        gated, want = [], []
        for s in order:
            y, muted, carry[s] = LV.gate_block(audio[s][t], a.zc, power, carry[s])
            gated.append(y)
            want.append(muted)
        rc, ctx_a, gm = a.push(slots, raw, [power] * 3)
        _lib.check(rc)
        rc, ctx_b, _ = b.push(slots, np.stack(gated))
        _lib.check(rc)
        assert torch.equal(gm.cpu(), torch.from_numpy(np.stack(want).astype(np.int32))), (t, gm.cpu().tolist())
        _assert_twins(a, b, ctx_a, ctx_b, t)
        seen.append(np.stack(want))
        for row, s in enumerate(order):                               # the state holds the last three RAW energies
            e = LV.frame_energies(np.concatenate([x for x in audio[s][:t + 1]]), a.zc)
            e = np.concatenate([np.zeros(3), e])[-3:]
            assert np.allclose(a.ge[LV.SLOTS[s]].cpu().numpy(), e, rtol=1e-5, atol=0), (t, s)
    seen = np.concatenate(seen, axis=1)
    assert seen.any() and not seen.all()
    rest = [s for s in range(LV.MAX_SLOTS) if s not in LV.SLOTS]
    assert bool((a.ge[rest] == 7.0).all()) and bool(torch.isnan(a.hist[rest]).all())


@pytest.mark.parametrize("m", [1, 9])
@pytest.mark.parametrize("pair", [(250, 150), (48000, 16000)], ids=["250_150", "48000_16000"])
def test_gate_off_is_the_plain_push_and_still_tracks_energies(pair, m):
    """gate_pow NULL and 0.0f are `svc_rt_push` bit for bit with an all-zero mask; a gate switched on at push 4 decides from the
    energies tracked during pushes 1 - 3 (the float64 decisions of the whole stream)."""
    from seedvc_amd import _lib
    null, zero, plain = _Push(pair, m), _Push(pair, m), _Push(pair, m)
    audio = _streams(pair, m)
    power = LV.gate_power(LV.GATE_DB, null.zc)
    carry = [(0.0, 0.0, 0.0)] * 3
    differs = False
    for t in range(6):
        raw = np.stack([audio[s][t] for s in range(3)])
        on = t >= 3
        gated, want, cold = [], [], []
        for s in range(3):
            y, muted, c = LV.gate_block(audio[s][t], null.zc, power, carry[s])
            cold.append(LV.gate_block(audio[s][t], null.zc, power, (0.0, 0.0, 0.0))[1])
            carry[s] = c
            gated.append(y if on else audio[s][t])
            want.append(muted if on else np.zeros(m, bool))
        rc, ctx_n, gm_n = null.push(LV.SLOTS, raw, [power] * 3 if on else None)
        _lib.check(rc)
        rc, ctx_z, gm_z = zero.push(LV.SLOTS, raw, [power] * 3 if on else [0.0] * 3)
        _lib.check(rc)
        rc, ctx_p, _ = plain.push(LV.SLOTS, np.stack(gated))
        _lib.check(rc)
        want = torch.from_numpy(np.stack(want).astype(np.int32))
        assert torch.equal(gm_n.cpu(), want) and torch.equal(gm_z.cpu(), want), t
        _assert_twins(null, plain, ctx_n, ctx_p, t)
        _assert_twins(zero, plain, ctx_z, ctx_p, t)
        if t == 3:
            differs = not np.array_equal(np.stack(cold), want.numpy().astype(bool))
    assert differs                                                    # at push 4 a gate without the tracked energies decides otherwise
    assert same(null.ge, zero.ge)


def test_gated_streams_that_advance_at_different_times_with_different_thresholds():
    """(22050, 16000), m = 2, eight pushes of changing subsets; slot 4 at -40 dB, slot 0 off, slot 2 at -10 dB (above the loud
    frames' -20 dB: everything is muted).  Every stream follows its own float64 gate; slots that are not listed keep every bit
    of gate_e, hist and the ring."""
    from seedvc_amd import _lib
    pair, m = (22050, 16000), 2
    a, b = _Push(pair, m), _Push(pair, m)
    zc = a.zc
    powers = [LV.gate_power(LV.GATE_DB, zc), np.float32(0.0), LV.gate_power(-10.0, zc)]
    audio = [LV.gate_audio(loud, 16, zc, seed=50 + s).reshape(8, m * zc) for s, loud in enumerate(({0, 9}, {3, 4}, {1, 2, 12}))]
    carry, nxt = [(0.0, 0.0, 0.0)] * 3, [0, 0, 0]
    subsets = ([0, 1, 2], [1], [2, 0], [0], [1, 2], [2], [0, 1], [2, 1, 0], [0])
    masks = [[], [], []]
    for t, order in enumerate(subsets):
        slots = [LV.SLOTS[s] for s in order]
        raw, gated, want = [], [], []
        for s in order:
            x = audio[s][nxt[s]]
            nxt[s] += 1
            y, muted, carry[s] = LV.gate_block(x, zc, powers[s], carry[s])
            raw.append(x), gated.append(y), want.append(muted), masks[s].append(muted)
        before = a.snapshot()
        rc, ctx_a, gm = a.push(slots, np.stack(raw), [powers[s] for s in order])
        _lib.check(rc)
        rc, ctx_b, _ = b.push(slots, np.stack(gated))
        _lib.check(rc)
        assert torch.equal(gm.cpu(), torch.from_numpy(np.stack(want).astype(np.int32))), t
        _assert_twins(a, b, ctx_a, ctx_b, t)
        rest = [s for s in range(LV.MAX_SLOTS) if s not in slots]
        planes0, planes1 = before[1][:a.n_planes].view(2, LV.MAX_SLOTS, a.L16), a.ring[:a.n_planes].view(2, LV.MAX_SLOTS, a.L16)
        assert same(a.ge[rest], before[2][rest]) and same(a.hist[rest], before[0][rest]) and same(planes1[:, rest], planes0[:, rest]), t
        tk0, tk1 = before[1][a.n_planes:].view(torch.int64), a.ring[a.n_planes:].view(torch.int64)
        assert torch.equal(tk1[rest], tk0[rest]) and bool((tk1[slots] > tk0[slots]).all())
    masks = [np.concatenate(v) for v in masks]
    assert masks[0].any() and not masks[0].all() and not masks[1].any() and masks[2].all() and len(set(nxt)) > 1


def test_gated_push_refusals_leave_the_state_untouched():
    """(250, 150): zc 5, z16 3, m = 2.  The good call's arguments with one thing wrong each: non-zero, a message, and hist, ring,
    gate_e, ctx and gate_mask keep every bit."""
    from seedvc_amd import _lib
    a = _Push((250, 150), 2)
    blocks = _streams((250, 150), 1)[0].reshape(3, 10)
    rc, _, _ = a.push(LV.SLOTS, blocks, [0.1, 0.0, 0.2])                 # a used state
    _lib.check(rc)
    before = a.snapshot()
    spare = torch.zeros(64, device=DEV)
    bad = dict(gate_e_null=dict(ge=None), pow_negative=dict(pow=f32([0.1, -0.1, 0.0])), pow_nan=dict(pow=f32([float("nan"), 0.0, 0.0])),
               pow_minus_inf=dict(pow=f32([0.0, 0.0, float("-inf")])), gate_e_is_hist=dict(ge=_lib.ptr(a.hist)),
               gate_e_in_ring=dict(ge=_lib.ptr(a.ring[8:])), mask_is_gate_e=dict(gm=_lib.ptr(a.ge)), mask_in_ring=dict(gm=_lib.ptr(a.ring[16:])),
               mask_is_hist=dict(gm=_lib.ptr(a.hist)), gate_e_off_4_bytes=dict(ge=C.c_void_p(spare.data_ptr() + 2)),
               Lin_off_the_grid=dict(Lin=9), L16_below_n_new=dict(L16=8), slot_twice=dict(slots=i32([4, 4, 2])), slot_above=dict(slots=i32([4, 0, 5])),
               N_zero=dict(N=0), null_hist=dict(hist=None), null_ctx=dict(ctx=None), z16_not_a_multiple_of_n=dict(z16=4))
    kept = []
    for name, kw in bad.items():
        rc, ctx, gm = a.push(LV.SLOTS, blocks, [0.1, 0.0, 0.2], **kw)
        assert rc != 0, name
        assert b"rt_push" in _lib.lib().svc_last_error(), name
        kept.append((name, ctx, gm))
    rc, ctx, gm = a.push(LV.SLOTS, blocks, [0.1, 0.0, 0.2], gm=_lib.ptr(spare), ctx=_lib.ptr(spare))     # the mask on ctx
    assert rc != 0 and b"rt_push" in _lib.lib().svc_last_error()
    torch.cuda.synchronize()
    for x, y in zip(a.snapshot(), before):
        assert same(x, y)
    for name, ctx, gm in kept:
        assert bool(torch.isnan(ctx).all()) and bool((gm == -1).all()), name
    assert not spare.any()
    rc, ctx, gm = a.push(LV.SLOTS, blocks, [0.1, 0.0, 0.2])              # and the good call is good
    _lib.check(rc)
    assert bool(torch.isfinite(ctx).all()) and bool(((gm == 0) | (gm == 1)).all()) and not same(a.ge, before[2])


# ============================================================================================================ the engine
FAKE_PAIR, FAKE_M, FAKE_L16, FAKE_CE = (22050, 16000), 2, 8 * 320, 0.04
G = RT.FAKE_GEOMETRY


def _fake_refs():
    return [(cases.randn(f"rt.pc{s}", 142, 1, P, cases.CHUNK_DC).to(DEV), cases.logmel(f"rt.mel{s}", 142, 1, cases.CHUNK_C, P).to(DEV),
             cases.randn(f"rt.style{s}", 142, 1, 3).to(DEV)) for s, P in enumerate(RT.FAKE_PROMPTS)]


def _engine(max_streams=4, output=False, audio=False):
    from seedvc_amd.pipeline import RealtimeEngine
    cfm, voc = LB.BatchedFakeCFM(DEV), RT.FakeVocoder()
    eng = RealtimeEngine(RT.FakeLR(), cfm, voc, max_streams=max_streams, **G)
    if output:
        eng.attach_output(_resample(LV.FAKE_OUT_PAIR))
    if audio:
        eng.attach_audio(RA.FakeContent(), _resample(FAKE_PAIR), FAKE_M * 441, FAKE_L16, FAKE_CE)
    return eng, cfm, voc


def _content(contents, streams, k):
    return dev(np.stack([contents[s][k] for s in streams]))


def _check_out_step(eng, slots, order, k, models, out, parts):
    for row, s in enumerate(order):
        want_out, want_new, want_o, scores, before, infer = models[s][k]
        assert np.array_equal(parts["infer"][row].cpu().numpy(), infer), (s, k)
        assert int(parts["offsets"][row]) == want_o, (s, k, RT.score_gap(scores))
        assert np.array_equal(out[row].cpu().numpy(), want_out), (s, k)
        assert np.array_equal(eng.state[slots[s]].cpu().numpy(), want_new), (s, k)


def test_engine_at_an_output_rate_equals_the_numpy_session():
    """`attach_output` with the fake rates (200, 250): three streams over five blocks equal the numpy session run at the output
    rate (block 55, Lb 20, Ls 15), bit for bit; and each stream alone equals its rows in the batch."""
    contents = [RT.planted_session(s) for s in range(3)]
    models = [LV.fake_out_session(c) for c in contents]
    assert all(RT.score_gap(m[3]) >= LV.GAP for ms in models for m in ms[1:])           # no block is decided by a near tie
    eng, cfm, voc = _engine(output=True)
    assert eng.state.shape == (4, 20)
    slots = [eng.open(*r) for r in _fake_refs()]
    batch = []
    for k in range(5):
        order = [0, 1, 2] if k < 3 else [2, 0, 1]
        out, parts = eng.step([slots[s] for s in order], _content(contents, order, k), 10, 0.7, return_parts=True)
        assert out.shape == (3, 55) and parts["infer"].shape == (3, 90) and parts["offsets"].dtype == torch.int32
        _check_out_step(eng, slots, order, k, models, out, parts)
        batch.append({s: out[row].clone() for row, s in enumerate(order)})
    assert cfm.batch_sizes == [3] * 5 and not eng.state[3].any()
    refs = _fake_refs()
    for s in range(3):
        one, _, _ = _engine(max_streams=1, output=True)
        slot = one.open(*refs[s])
        for k in range(5):
            out = one.step([slot], _content(contents, [s], k), 10, 0.7)
            assert same(out[0], batch[k][s]), (s, k)


def test_set_speech_mutes_a_stream_before_sola():
    """Stream 1 without speech for blocks 2 - 3: the first muted block is the old buffer's fade-out and then zeros, the next is
    zeros, and after `set_speech(True)` the stream resumes from a zero buffer; the other streams are unaffected, bit for bit.
    With and without an output rate attached (without: the muted steps go through `svc_rt_out` with r = NULL, the others through
    `svc_sola_step`)."""
    contents = [RT.planted_session(s) for s in range(3)]
    for output in (True, False):
        pair = LV.FAKE_OUT_PAIR if output else (200, 200)
        models = [LV.fake_out_session(c, muted=(1, 2) if s == 1 else (), pair=pair) for s, c in enumerate(contents)]
        plain = [LV.fake_out_session(c, pair=pair) for c in contents]
        assert all(RT.score_gap(m[3]) >= LV.GAP for ms in models for m in ms[1:] if m[4].any() and m[5].any())      # zeros on either side: every score is 0
        eng, _, _ = _engine(output=output)
        slots = [eng.open(*r) for r in _fake_refs()]
        Lb = eng.state.size(1)
        for k in range(5):
            eng.set_speech(slots[1], k not in (1, 2))
            before = eng.state[slots[1]].clone()
            out, parts = eng.step(slots, _content(contents, [0, 1, 2], k), 10, 0.7, return_parts=True)
            _check_out_step(eng, slots, [0, 1, 2], k, models, out, parts)
            for s in (0, 2):
                assert np.array_equal(out[s].cpu().numpy(), plain[s][k][0])
            fo = eng._out["fade_out"] if output else eng.fade_out
            if k == 1:
                assert before.any() and torch.equal(out[1, :Lb], before * fo) and not out[1, Lb:].any() and not parts["infer"][1].any()
            if k == 2:
                assert not before.any() and not out[1].any()
            if k in (1, 2):
                assert not eng.state[slots[1]].any() and int(parts["offsets"][1]) == 0
            if k == 3:
                assert not before.any() and out[1].any() and models[1][3][2] == 0


def _gate_sessions():
    """Audio of three streams, five blocks of 2 zc: stream 1 is loud / quiet frames (loud 0 and 7: frames 4 - 6 are muted at
    -40 dB), the others noise.  -> (raw, host-gated, masks of stream 1)."""
    zc = 441
    raw = [(RC.noise(f"rt_live.session{s}", 31, 5, FAKE_M * zc) * 0.5).numpy() for s in range(3)]
    raw[1] = LV.gate_audio({0, 7}, 10, zc, seed=77).reshape(5, FAKE_M * zc)
    power, carry = LV.gate_power(LV.GATE_DB, zc), (0.0, 0.0, 0.0)
    gated, masks = [r.copy() for r in raw], []
    for k in range(5):
        gated[1][k], m, carry = LV.gate_block(raw[1][k], zc, power, carry)
        masks.append(m)
    assert np.concatenate(masks).tolist() == [False] * 4 + [True] * 3 + [False] * 3
    return raw, gated, masks


def test_set_gate_equals_step_audio_on_the_host_gated_block():
    raw, gated, masks = _gate_sessions()
    a, _, _ = _engine(audio=True)
    b, _, _ = _engine(audio=True)
    refs = _fake_refs()
    slots = [a.open(*r) for r in refs]
    assert [b.open(*r) for r in refs] == slots
    a.set_gate(slots[1], LV.GATE_DB)
    for k in range(5):
        order = [0, 1, 2] if k % 2 == 0 else [1, 2, 0]
        sl = [slots[s] for s in order]
        out_a, pa = a.step_audio(sl, dev(np.stack([raw[s][k] for s in order])), 10, 0.7, return_parts=True)
        out_b, pb = b.step_audio(sl, dev(np.stack([gated[s][k] for s in order])), 10, 0.7, return_parts=True)
        assert same(pa["ctx"], pb["ctx"]) and same(pa["content"], pb["content"]) and same(out_a, out_b), k
        assert same(a.state, b.state) and same(a._audio["hist"], b._audio["hist"]) and same(a._audio["ring"], b._audio["ring"]), k
        want = np.zeros((3, FAKE_M), np.int32)
        want[order.index(1)] = masks[k]
        assert torch.equal(pa["gate_mask"].cpu(), torch.from_numpy(want)) and "gate_mask" not in pb, k
    assert not b._audio["gate_e"].any() and a._audio["gate_e"][slots[1]].any()


def test_an_engine_without_the_live_settings_makes_the_calls_it_made_before():
    """`step` against a direct `svc_sola_step` on the returned infer rows, `step_audio` against a direct `svc_rt_push` on copies
    of the state: the same bits, and no live part in the returned dict."""
    from seedvc_amd import _lib
    raw, _, _ = _gate_sessions()
    contents = [RT.planted_session(s) for s in range(3)]
    eng, _, _ = _engine(audio=True)
    slots = [eng.open(*r) for r in _fake_refs()]
    a = eng._audio
    for k in range(3):
        state, hist, ring = eng.state.clone(), a["hist"].clone(), a["ring"].clone()
        if k == 1:
            out, parts = eng.step(slots, _content(contents, [0, 1, 2], k), 10, 0.7, return_parts=True)
        else:
            audio = dev(np.stack([raw[s][k] for s in range(3)]))
            out, parts = eng.step_audio(slots, audio, 10, 0.7, return_parts=True)
            ctx = torch.empty(3, FAKE_L16, device=DEV)
            _lib.check(_lib.lib().svc_rt_push(_resample(FAKE_PAIR)._h, _lib.ptr(audio), audio.stride(0), FAKE_M * 441, 3, i32(slots), 4, 441, 320,
                                              _lib.ptr(hist), _lib.ptr(ring), FAKE_L16, _lib.ptr(ctx), _lib.stream_ptr()))
            assert same(parts["ctx"], ctx) and same(a["hist"], hist) and same(a["ring"], ring), k
        assert "gate_mask" not in parts and parts["infer"].shape == (3, 72) and out.shape == (3, G["block"])
        infer = parts["infer"].contiguous()
        out2, offs2 = torch.empty_like(out), torch.empty(3, dtype=torch.int32, device=DEV)
        _lib.check(_lib.lib().svc_sola_step(_lib.ptr(infer), 72, 0, 3, _lib.ptr(state), 4, i32(slots), _lib.ptr(eng.fade_in), _lib.ptr(eng.fade_out),
                                            G["block"], G["sola_buffer"], G["sola_search"], _lib.ptr(out2), _lib.ptr(offs2), _lib.stream_ptr()))
        assert same(out, out2) and torch.equal(parts["offsets"], offs2) and same(eng.state, state), k
    assert not a["gate_e"].any()                                      # the plain push tracks nothing


LIVE_DB = -25.0


def _live_sessions():
    """Audio of three streams, three blocks of 2 zc, noise of amplitude 0.5; stream 1 has its frames 1 - 4 at a tenth of that, which
    puts frame 4 alone below a gate at -25 dB (every window energy is more than 3 times off the threshold).  The frame after it is
    loud again, so the samples SOLA reads are never all zero and no block is decided by a near tie.
    -> (raw, host-gated, masks of stream 1)."""
    zc = 441
    raw = [(RC.noise(f"rt_live.live{s}", 31, 3, FAKE_M * zc) * 0.5).numpy() for s in range(3)]
    raw[1] = raw[1] * np.repeat(np.array([1, .1, .1, .1, .1, 1], np.float32), zc).reshape(3, FAKE_M * zc)
    power, carry = LV.gate_power(LIVE_DB, zc), (0.0, 0.0, 0.0)
    gated, masks, E = [r.copy() for r in raw], [], []
    for k in range(3):
        E.append(LV.gate_decisions(LV.frame_energies(raw[1][k], zc), power, carry)[1])
        gated[1][k], m, carry = LV.gate_block(raw[1][k], zc, power, carry)
        masks.append(m)
    assert np.concatenate(masks).tolist() == [False] * 4 + [True, False] and LV.gate_margin(np.concatenate(E), power) > 3
    return raw, gated, masks


def test_a_live_step_does_not_synchronise():
    """Gate on for stream 1, stream 2 without speech, an output rate attached: two steps under torch's synchronisation watch, then
    the results against the numpy session (push -> content -> fake chain -> resample -> splice)."""
    raw, gated, masks = _live_sessions()
    zc, z16, _, _ = RA.units(*FAKE_PAIR)
    models = []
    for s in range(3):
        hist, ring, xs = np.zeros(2 * zc, np.float32), np.zeros(FAKE_L16, np.float32), []
        for k in range(3):
            ring, hist = RA.push_model_fp32(hist, ring, gated[s][k], *FAKE_PAIR, zc, z16)
            xs.append(RA.fake_content(ring)[int(FAKE_CE * 50):])
        models.append(LV.fake_out_session(xs, muted=(1, 2) if s == 2 else ()))
    assert all(RT.score_gap(m[3]) >= LV.GAP for ms in models for m in ms[1:] if m[4].any() and m[5].any())      # zeros on either side: every score is 0
    watch = hasattr(torch.cuda, "set_sync_debug_mode")
    eng, _, _ = _engine(output=True, audio=True)
    slots = [eng.open(*r) for r in _fake_refs()]
    eng.set_gate(slots[1], LIVE_DB)
    xs = [dev(np.stack([raw[s][k] for s in range(3)])) for k in range(3)]
    out0, parts0 = eng.step_audio(slots, xs[0], 10, 0.7, return_parts=True)      # the first step stacks the prompts
    _check_out_step(eng, slots, [0, 1, 2], 0, models, out0, parts0)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode() if watch else None
    if watch:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            torch.cuda.set_sync_debug_mode("error")
    try:
        eng.set_speech(slots[2], False)
        out1 = eng.step_audio(slots, xs[1], 10, 0.7)
        out2, parts = eng.step_audio(slots, xs[2], 10, 0.7, return_parts=True)
    finally:
        if watch:
            torch.cuda.set_sync_debug_mode(before)
    for s in range(3):
        assert np.array_equal(out1[s].cpu().numpy(), models[s][1][0]), s
    _check_out_step(eng, slots, [0, 1, 2], 2, models, out2, parts)
    assert torch.equal(parts["gate_mask"].cpu(), torch.from_numpy(np.stack([np.zeros(2, bool), masks[2], np.zeros(2, bool)]).astype(np.int32)))
    assert not out2[2].any() and out2[0].any()
