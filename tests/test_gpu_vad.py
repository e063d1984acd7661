"""The FSMN-VAD on the device against the yardstick of vad_cases.py: `svc_vad_scores` against float64 within
4 x the error of the fp32 yardstick; a clip in a ragged batch against the clip alone and the run split against one run, bit
for bit; `svc_vad_step` block by block against `svc_vad_scores` on the stream, bit for bit; the detector (`svc_vad_detect`, and
the one inside `svc_vad_step`) against the Python integers, exactly; `svc_rt_out_dev` against `svc_rt_out`; and an engine with
the VAD attached against the same steps driven by `set_speech` from the Python detector."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB
import realtime_cases as RT
import rt_audio_cases as RA
import rt_live_cases as LV
import vad_cases as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
i32 = lambda v: (C.c_int32 * len(v))(*[int(x) for x in v])      # noqa: E731
bits = lambda t: t.contiguous().view(torch.int32)                # noqa: E731  (NaN rows compare as integers)
same = lambda a, b: a.shape == b.shape and torch.equal(bits(a), bits(b))      # noqa: E731
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)             # noqa: E731
SLOTS, MAX_SLOTS = (4, 0, 2), 5
NAN = float("nan")
# a detector that opens and closes within a few rows, for streams of a second or two
QUICK = dict(p_max=0.2, win=4, on_count=3, off_count=1, lookback=2, end_silence=3, max_segment=6000, seg_rows=0)
_vads = {}


def _vad(name="random", **cfg):
    from seedvc_amd.vad import FsmnVad
    key = (name, tuple(sorted(cfg.items())))
    if key not in _vads:
        config = dict(V.CONFIG, **cfg)
        if name == "random":
            _vads[key] = FsmnVad(V.random_state_dict(0), *(torch.from_numpy(a) for a in V.cmvn(0)), config=config, device=DEV)
        else:
            _vads[key] = FsmnVad(V.energy_vad_state_dict(*ENERGY), torch.zeros(400), torch.ones(400), config=config, device=DEV)
    return _vads[key]


# ======================================================================================================= svc_vad_scores
@pytest.mark.parametrize("final", [0, 1])
def test_scores_against_float64(final):
    """Six clips of 400 .. 32000 samples in one ragged batch (NaN above every clip's end), random weights: every row's p_sil and
    log(p / (1 - p)) within 4 x the largest error the fp32 yardstick makes on these inputs (vad_cases.REF_ERR; 4: the MFMA's
    k order and the tiled DFT differ from a CPU BLAS's blocking).  No row is excluded.
    Measured on an MI355X: see DESIGN.md 8n."""
    waves, lens = V.score_batch()
    p, rows = _vad().scores_batch(dev(waves), lens, final=bool(final))
    assert rows == [V.rows_of(n, final) for n in lens] and p.shape == (6, V.rows_of(32000, final))
    p = p.cpu().numpy()
    ep = el = 0.0
    for b, (p64, l64) in enumerate(r[0] for r in V.reference(final)):
        got = p[b, :rows[b]]
        assert not p[b, rows[b]:].any()                                      # nothing is written above a clip's rows
        if rows[b]:
            assert np.isfinite(got).all() and (got > 0).all() and (got < 1).all()
            ep, el = max(ep, float(np.abs(got - p64).max())), max(el, float(np.abs(V.logit_of(got) - l64).max()))
    print(f"vad scores final={final}: device |p - p64| = {ep:.3e} (fp32 yardstick {V.REF_ERR[0]:.1e}), "
          f"|logit - logit64| = {el:.3e} (fp32 yardstick {V.REF_ERR[1]:.1e})")
    assert ep <= 4 * V.REF_ERR[0] and el <= 4 * V.REF_ERR[1], (ep, el)


@pytest.mark.parametrize("final", [0, 1])
def test_a_clip_in_a_ragged_batch_equals_the_clip_alone(final):
    waves, lens = V.score_batch()
    order = [3, 0, 5, 1, 4, 2]
    vad = _vad()
    p, rows = vad.scores_batch(dev(waves[order]), [lens[b] for b in order], final=bool(final))
    for row, b in enumerate(order):
        one, r1 = vad.scores_batch(dev(waves[b:b + 1, :lens[b]]), [lens[b]], final=bool(final))
        assert r1 == [rows[row]] and same(one[0, :r1[0]], p[row, :r1[0]]), (b, final)


def test_the_run_split_equals_one_run():
    """198 rows cut into 7 runs of 32 and into 5 of 48 (each run but the first warms up on the 76 rows before it, across tiles of
    16 that start elsewhere), against one run: bit for bit."""
    w = dev(V.noise_clip(32000, 12)[None])
    vad = _vad()
    whole, rows = vad.scores_batch(w, [32000], seg_rows=4096)
    assert rows == [198]
    for seg in (32, 48, 16):
        p, _ = vad.scores_batch(w, [32000], seg_rows=seg)
        assert same(p, whole), seg
    p, _ = vad.scores_batch(w, [32000])                                       # the handle's default: one run here
    assert same(p, whole)


# ========================================================================================================== svc_vad_step
def _row(samples, end, stride):
    """A stream's row of x: its samples so far end at `end`; NaN before its first sample and above `end`."""
    r = np.full(stride, np.nan, np.float32)
    n = min(len(samples), end)
    r[end - n:end] = samples[len(samples) - n:]
    return r


@pytest.mark.parametrize("m", [1, 9])
def test_streaming_equals_scores_on_the_stream_and_the_python_detector(m):
    """Three streams in slots (4, 0, 2) of 5 over six blocks of m 20 ms frames: stream 1 opens two steps late, stream 2 is reset
    before step 3.  The p_sil of a stream, block after block, is `svc_vad_scores(final = 0)` of its samples, bit for bit; events,
    n_events, flags and the state integers are the Python detector's on the device's own p_sil; the state rows and flags of the
    slots that are not listed keep every bit (and so does a listed slot's row in a step that gives it no rows)."""
    from seedvc_amd.vad import CACHE_FLOATS, STATE_WORDS
    cfg = dict(QUICK, p_max=0.6, max_segment=12)
    vad = _vad(**cfg)
    n_new, end, stride = 320 * m, 320 * m + 960, 320 * m + 960 + 7
    audio = [V.noise_clip(6 * n_new, 40 + s) for s in range(3)]
    state, flags = vad.stream_state(MAX_SLOTS)
    state.view(torch.int32).fill_(0x7FC01234)                                 # NaN patterns in every slot ...
    flags.fill_(-7)
    for s in SLOTS:
        state[s].zero_()                                                      # ... but the three fresh streams
        flags[s] = 0
    poison = state.clone()
    runs = {s: [] for s in range(3)}          # stream -> list of [samples, [p blocks], detector state, flag, events]
    for s in range(3):
        runs[s].append(dict(x=np.zeros(0, np.float32), p=[], st=V.fresh_state(), flag=0))
    for k in range(6):
        live = [s for s in range(3) if not (s == 1 and k < 2)]
        if k == 3:                                                            # reset stream 2: fresh state, flag 0, total 0
            state[SLOTS[2]].zero_()
            flags[SLOTS[2]] = 0
            runs[2].append(dict(x=np.zeros(0, np.float32), p=[], st=V.fresh_state(), flag=0))
        if k % 2:
            live = live[::-1]
        total = [len(runs[s][-1]["x"]) for s in live]
        for s in live:
            runs[s][-1]["x"] = np.concatenate([runs[s][-1]["x"], audio[s][k * n_new:(k + 1) * n_new]])
        x = dev(np.stack([_row(runs[s][-1]["x"], end, stride) for s in live]))
        before = state.clone()
        parts = vad.step(x, end, n_new, total, [SLOTS[s] for s in live], state, flags, return_parts=True)
        p, ev, nev = parts["p_sil"].cpu().numpy(), parts["events"].cpu().numpy(), parts["n_events"].cpu().numpy()
        for row, s in enumerate(live):
            r = runs[s][-1]
            n = parts["n_rows"][row]
            assert n == V.rows_of(total[row] + n_new, False) - V.rows_of(total[row], False)
            r["p"].append(p[row, :n].copy())
            want_ev, r["flag"] = V.detect(cfg, r["st"], V.decisions(p[row, :n], cfg["p_max"]), r["flag"])
            assert nev[row] == len(want_ev) and [tuple(e) for e in ev[row, :min(len(want_ev), 8)]] == want_ev[:8], (m, k, s)
            assert int(flags[SLOTS[s]]) == r["flag"], (m, k, s)
            words = state[SLOTS[s], CACHE_FLOATS:].view(torch.int32)[:len(STATE_WORDS)].tolist()
            assert words == [r["st"][w] for w in V.STATE_WORDS], (m, k, s)
            if n == 0:
                assert same(state[SLOTS[s]], before[SLOTS[s]])
        for slot in set(range(MAX_SLOTS)) - {SLOTS[s] for s in live}:
            assert same(state[slot], before[slot]) and (slot in SLOTS or int(flags[slot]) == -7), (m, k, slot)
    assert same(state[1], poison[1]) and same(state[3], poison[3])
    n_events = 0
    for s in range(3):
        for r in runs[s]:
            want, rows = vad.scores_batch(dev(r["x"][None]), [len(r["x"])], final=False)
            got = np.concatenate(r["p"])
            assert len(got) == rows[0] and np.array_equal(got.view(np.int32), want[0, :rows[0]].cpu().numpy().view(np.int32)), (m, s)
            n_events += r["st"]["prev_end"] > 0
    assert m == 1 or n_events >= 2                                            # segments opened and closed in the long streams


# ======================================================================================================== svc_vad_detect
def _patterns():
    """Three streams of 330 frames of 0.01 / 0.99 runs, with the threshold itself, its fp32 neighbours and NaN sprinkled in."""
    lo, hi = np.nextafter(np.float32(0.2), np.float32(0)), np.nextafter(np.float32(0.2), np.float32(1))
    S, Q = np.float32(0.01), np.float32(0.99)
    a = [Q] * 30 + [S] * 40 + [Q] * 100 + [S] * 20 + [Q] * 70 + [S] * 70
    b = [S] * 20 + [Q] * 70 + [S] * 20 + [Q] * 80 + [np.float32(0.2), lo, S] * 20 + [Q] * 80
    c = [np.float32(NAN), hi, Q] * 10 + [S, S, np.float32(0.2), lo, S, hi] * 20 + [np.float32(NAN)] * 90 + [S] * 90
    return [np.array(v, np.float32) for v in (a, b, c)]


@pytest.mark.parametrize("name", ["default", "forced"])
def test_detect_equals_the_python_detector(name):
    """Calls of 1 .. 18 rows (every stream its own count, zero included) through segments that open, close and, with
    max_segment = 40, force-close across call boundaries: events, n_events, flags, frame_speech and the state integers equal the
    Python model after every call."""
    from seedvc_amd.vad import CACHE_FLOATS
    cfg = dict(V.CONFIG) if name == "default" else dict(V.CONFIG, max_segment=40)
    vad = _vad(**({} if name == "default" else dict(max_segment=40)))
    pats = _patterns()
    state, flags = vad.stream_state(MAX_SLOTS)
    state[1].fill_(NAN)
    flags[3] = -7
    st, flag, pos = [V.fresh_state() for _ in range(3)], [0, 0, 0], [0, 0, 0]
    all_events, call = [[], [], []], 0
    while any(pos[s] < len(pats[s]) for s in range(3)):
        n = [min((call * (s + 2) + 5 * s) % 19, len(pats[s]) - pos[s]) for s in range(3)]
        if not any(n):
            first = next(s for s in range(3) if pos[s] < len(pats[s]))
            n[first] = 1
        order = [0, 1, 2] if call % 3 else [2, 0, 1]
        ld = max(max(n), 1) + 2
        p = np.full((3, ld), np.nan, np.float32)
        for row, s in enumerate(order):
            p[row, :n[s]] = pats[s][pos[s]:pos[s] + n[s]]
        d = vad.detect(dev(p), [n[s] for s in order], [SLOTS[s] for s in order], state, flags, frame_speech=True)
        ev, nev, fs = d["events"].cpu().numpy(), d["n_events"].cpu().numpy(), d["frame_speech"].cpu().numpy()
        for row, s in enumerate(order):
            dec = V.decisions(p[row, :n[s]], cfg["p_max"])
            want, flag[s] = V.detect(cfg, st[s], dec, flag[s])
            all_events[s] += want
            assert nev[row] == len(want) <= 8 and [tuple(e) for e in ev[row, :len(want)]] == want, (call, s)
            assert fs[row, :n[s]].tolist() == dec.tolist() and int(flags[SLOTS[s]]) == flag[s], (call, s)
            words = state[SLOTS[s], CACHE_FLOATS:].view(torch.int32)[:len(V.STATE_WORDS)].tolist()
            assert words == [st[s][w] for w in V.STATE_WORDS], (call, s)
            pos[s] += n[s]
        call += 1
    assert bool(torch.isnan(state[1]).all()) and int(flags[3]) == -7 and not state[:, :CACHE_FLOATS][[0, 2, 4]].any()
    kinds = [[k for k, _ in e] for e in all_events]
    assert all(len(k) >= 3 and k[0] == V.BEGIN and V.END in k for k in kinds), kinds
    if name == "forced":
        assert any(e[i + 1][1] - e[i][1] == 390 for e in all_events for i in range(len(e) - 1) if e[i][0] == V.BEGIN)


def test_segments_of_a_clip():
    """`segments`: loud / silent / loud noise through the energy detector and the quick config -> two segments, the second
    still open at the end and closed at the last frame; equal to the Python detector on the float64 yardstick's decisions."""
    vad = _vad("energy", **QUICK)
    rng = np.random.default_rng(5)
    w = np.concatenate([np.zeros(1600), rng.uniform(-0.3, 0.3, 4800), np.zeros(4800), rng.uniform(-0.3, 0.3, 3200)]).astype(np.float32)
    p64, _ = V.scores(V.energy_vad_state_dict(*ENERGY), w, True, np.zeros(400), np.ones(400))
    assert (np.minimum(p64, 1 - p64) < 0.01).all()
    ev, st, _ = V.detect_in_calls(dict(V.CONFIG, **QUICK), V.decisions(p64, 0.2), [])
    from seedvc_amd.vad import events_to_segments
    want = events_to_segments(ev, len(p64) - 1)
    got = vad.segments(dev(w), chunk=17)
    assert got == want and len(got) == 2 and got[1][1] == 10 * (len(p64) - 1) and st["in_seg"] == 1, (got, want)


# ======================================================================================================== svc_rt_out_dev
def _rt_out(pair, Lb_units, w, state, speech, speech_dev, entry):
    from seedvc_amd import _lib
    from seedvc_amd.audio import Resample
    zc_m, zc_o, gm, go = LV.out_units(pair, Lb_units)
    n_in = gm["block"] + gm["Lb"] + gm["Ls"]
    if pair not in _resamplers and pair[0] != pair[1]:
        _resamplers[pair] = Resample(*pair, device=DEV)
    r = None if pair[0] == pair[1] else _resamplers[pair]._h
    fi, fo = (dev(x) for x in RT.gui_windows(go["Lb"]))
    infer, out = torch.full((3, go["n_inf"]), NAN, device=DEV), torch.full((3, go["block"]), NAN, device=DEV)
    offs = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    head = (r, _lib.ptr(w), w.stride(0), 3, n_in, 3, _lib.ptr(state), LV.MAX_SLOTS, i32(LV.SLOTS), None if speech is None else i32(speech))
    tail = (_lib.ptr(fi), _lib.ptr(fo), go["block"], go["Lb"], go["Ls"], _lib.ptr(infer), _lib.ptr(out), _lib.ptr(offs), _lib.stream_ptr())
    if entry == "dev":
        _lib.check(_lib.lib().svc_rt_out_dev(*head, _lib.ptr(speech_dev), *tail))
    else:
        _lib.check(_lib.lib().svc_rt_out(*head, *tail))
    return infer, out, offs


_resamplers = {}


@pytest.mark.parametrize("Lb_units", [1, 4])
@pytest.mark.parametrize("pair", LV.OUT_PAIRS, ids=[f"{a}_{b}" for a, b in LV.OUT_PAIRS])
def test_rt_out_dev_equals_rt_out(pair, Lb_units):
    """The cases of rt_live_cases.out_waves, three steps of 3 streams in slots (4, 0, 2) of 5.  speech_dev NULL: `svc_rt_out`, bit
    for bit (host flags given or not).  Device flags (the middle stream muted at step 1, the first at step 2, an unlisted slot's
    flag 0 throughout) against the same flags as the host array: infer, out, offsets and the state, bit for bit; and both
    kinds of flag together mute either stream."""
    wave, state0 = LV.out_waves(pair, Lb_units, start=3, extra=2)
    sa, sb, sc, sd = (dev(state0) for _ in range(4))
    for t in range(3):
        w = dev(wave[t])
        host = [0 if (t, k) in ((1, 1), (2, 0)) else 1 for k in range(3)]
        flags = torch.ones(LV.MAX_SLOTS, dtype=torch.int32, device=DEV)
        flags[1] = 0                                                          # slot 1 is not listed
        for k in range(3):
            flags[LV.SLOTS[k]] = host[k]
        sp = None if t == 0 else host
        a = _rt_out(pair, Lb_units, w, sa, sp, None, "dev")
        b = _rt_out(pair, Lb_units, w, sb, sp, None, "host")
        assert all(same(x, y) for x, y in zip(a, b)) and same(sa, sb), (pair, Lb_units, t)
        c = _rt_out(pair, Lb_units, w, sc, None, flags, "dev")
        assert all(same(x, y) for x, y in zip(c, b)) and same(sc, sb), (pair, Lb_units, t)
        # host flag mutes stream 2 at step 1 on top of the device's stream 1
        both = _rt_out(pair, Lb_units, w, sd, [1, 1, 0] if t == 1 else None, flags, "dev")
        if t == 1:
            assert not both[0][1].any() and not both[0][2].any() and both[0][0].any()
        if t == 0:
            assert all(same(x, y) for x, y in zip(both, b))
    assert not same(sa, dev(state0))


# ============================================================================================================ the engine
ENERGY = (2.0, 50.0)                           # theta, gain: p_sil = sigmoid(50 (2 - mean of the row))
PAIR48, M, L16 = (48000, 16000), 2, 8 * 320
# loud (1) / silent (0) blocks of 40 ms per stream: the quick detector opens and closes a segment in streams 0 and 1; one silent
# block does not close the segment of stream 2; stream 3 has its VAD off
LOUD = ([1, 1, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0], [1, 0, 1, 0, 1, 0], [1, 1, 0, 0, 1, 1])


def _engine():
    from seedvc_amd.audio import Resample
    from seedvc_amd.pipeline import RealtimeEngine
    if PAIR48 not in _resamplers:
        _resamplers[PAIR48] = Resample(*PAIR48, device=DEV)
    eng = RealtimeEngine(RT.FakeLR(), LB.BatchedFakeCFM(DEV), RT.FakeVocoder(), max_streams=5, **RT.FAKE_GEOMETRY)
    eng.attach_audio(RA.FakeContent(), _resamplers[PAIR48], M * 960, L16, 0.04)
    return eng


def test_engine_with_the_vad_equals_set_speech_from_the_python_detector():
    """Four streams, six blocks of 40 ms at 48 kHz, loud noise or digital silence per block.  Engine A has the energy VAD
    attached and on for streams 0 - 2; engine B is the parent's path: before every step `set_speech` gets the flag of the Python
    detector run on the float64 yardstick's p_sil of the stream's 16 kHz samples (taken from the contexts, which both engines
    compute alike).  Outputs, SOLA state and what SOLA saw are equal, bit for bit; stream 3, its VAD off, plays through."""
    cfg = dict(V.CONFIG, **QUICK)
    vad = _vad("energy", **QUICK)
    sd = V.energy_vad_state_dict(*ENERGY)
    rng = np.random.default_rng(9)
    audio = [np.concatenate([(rng.uniform(-0.3, 0.3, M * 960) * l).astype(np.float32) for l in LOUD[s]]).reshape(6, M * 960)
             for s in range(4)]
    refs = [(cases.randn(f"vad.pc{s}", 143, 1, P, cases.CHUNK_DC).to(DEV), cases.logmel(f"vad.mel{s}", 143, 1, cases.CHUNK_C, P).to(DEV),
             cases.randn(f"vad.style{s}", 143, 1, 3).to(DEV)) for s, P in enumerate(RT.FAKE_PROMPTS + (13,))]
    a, b = _engine(), _engine()
    a.attach_vad(vad)
    slots = [a.open(*r) for r in refs]
    assert [b.open(*r) for r in refs] == slots
    for s in range(3):
        a.set_vad(slots[s], True)
    n_new, end = a._vad["n_new"], a._vad["end"]
    assert (n_new, end) == (640, L16 - 320)
    stream = [np.zeros(0, np.float32) for _ in range(3)]
    st, flag, seen, margins, opened = [V.fresh_state() for _ in range(3)], [0, 0, 0], [0, 0, 0], [], set()
    played = muted_loud = False
    for k in range(6):
        order = [0, 1, 2, 3] if k % 2 == 0 else [3, 2, 0, 1]
        sl = [slots[s] for s in order]
        x = dev(np.stack([audio[s][k] for s in order]))
        out_a, pa = a.step_audio(sl, x, 10, 0.7, return_parts=True)
        ctx = pa["ctx"].cpu().numpy()
        for row, s in enumerate(order):
            if s == 3:
                continue
            stream[s] = np.concatenate([stream[s], ctx[row, end - n_new:end]])
            p64, _ = V.scores(sd, stream[s], False, np.zeros(400), np.ones(400))
            new = p64[seen[s]:]
            margins += np.minimum(new, 1 - new).tolist()
            seen[s] = len(p64)
            ev, flag[s] = V.detect(cfg, st[s], V.decisions(new, cfg["p_max"]), flag[s])
            opened |= {s for kind, _ in ev if kind == V.END}
            b.set_speech(slots[s], bool(flag[s]))
        assert max(margins, default=0.0) < 0.01, max(margins)                 # the precondition: no row is near the threshold
        out_b, pb = b.step_audio(sl, x, 10, 0.7, return_parts=True)
        assert same(pa["ctx"], pb["ctx"]) and same(pa["content"], pb["content"]), k
        assert same(out_a, out_b) and same(pa["infer"], pb["infer"]) and torch.equal(pa["offsets"], pb["offsets"]) and same(a.state, b.state), k
        v = pa["vad"]
        assert v["slots"] == [slots[s] for s in order if s != 3] and v["p_sil"].shape == (3, 4)
        assert [int(v["flags"][slots[s]]) for s in range(3)] == flag and int(v["flags"][slots[3]]) == 1, k
        played |= bool(pa["infer"][order.index(3)].any())                      # the stream without a VAD is never muted
        muted_loud |= any(flag[s] == 0 and bool(pa["mel"][order.index(s)].any()) for s in range(3))
        assert "vad" not in pb
    assert played and muted_loud                                              # the flags muted rows that were not silent anyway
    assert len(margins) == 3 * 20 and opened == {0, 1} and st[2]["prev_end"] == 0
    # VAD off for every listed slot: the engine makes the calls it made before
    a.set_vad(slots[0], False)
    out, parts = a.step_audio([slots[0], slots[3]], dev(np.stack([audio[0][0], audio[3][0]])), 10, 0.7, return_parts=True)
    assert "vad" not in parts and a._vad["flags"][slots[0]] == 1
