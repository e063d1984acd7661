"""CPU side of the streams' pitch step on the context's tail (`svc_rt_pitch_win`, `rmvpe.rt_pitch_win`,
`RealtimeEngine.set_pitch_window` / `set_pitch_memory`): the entry points are declared, exported and bound and the
pinned signatures stay; the statement of rt_pitch_win_cases.py by hand and against its own planted sabotages; the argument checks
of the call, which come before anything touches a device; the frame arithmetic of the tail slice; and the engine's host logic
with stand-ins."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import realtime_cases as RT
import rt_audio_cases as RA
import rt_pitch_cases as PC
import rt_pitch_win_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
f32 = lambda *v: (ctypes.c_float * len(v))(*v)      # noqa: E731


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline, rmvpe
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in ("svc_rt_pitch_win", "svc_rt_pitch_cache_words", "svc_rt_pitch_ring_words"):
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert "enum { SVC_RT_PITCH_WIN_MAX_TF = 4096 };" in header and rmvpe.PITCH_WIN_MAX_TF == WC.MAX_TF == 4096
    for phrase in ("new[i] = f0_win[k][i - (Tf - W)]   for i >= Tf - W + guard", "new[i] = old[i + n_new]",
                   "e = max(0, fill + n_new - memory)", "(head + fill + j) % memory", "head = (head + e) % memory",
                   "Rows of slots that are not listed keep every bit of cache, ring and state",
                   "Refused (non-zero, svc_last_error() names it, nothing touched)"):
        assert phrase in header, phrase
    L = _lib.lib()
    assert len(L.svc_rt_pitch_win.argtypes) == 25
    assert L.svc_rt_pitch_cache_words(8, 48) == 8 * 48 and L.svc_rt_pitch_cache_words(64, 4096) == 64 * 4096
    assert [L.svc_rt_pitch_cache_words(*a) for a in ((0, 48), (8, 0), (8, 4097), (-1, -1))] == [0] * 4
    assert L.svc_rt_pitch_ring_words(8, 10) == 8 * 12 and L.svc_rt_pitch_ring_words(1, 1) == 3
    assert [L.svc_rt_pitch_ring_words(*a) for a in ((8, 0), (0, 10), (8, -2))] == [0] * 3
    sig = lambda f: list(inspect.signature(f).parameters)                              # noqa: E731
    E = pipeline.RealtimeEngine
    assert sig(E.set_pitch_window) == ["self", "window_frames", "guard_frames"] and sig(E.set_pitch_memory) == ["self", "memory_frames"]
    assert sig(rmvpe.rt_pitch_win)[:11] == ["f0_win", "guard", "n_new", "lag", "slots", "cache", "ring", "state", "ref_median", "auto_adjust",
                                            "semitones"]
    # the pinned signatures stay
    assert sig(E.attach_pitch) == ["self", "rmvpe", "lag_frames", "warmup_frames", "max_step_cents", "thred"]
    assert [p.default for p in inspect.signature(E.attach_pitch).parameters.values()][2:] == [8, 50, 100.0, 0.03]
    assert sig(E.step) == ["self", "slots", "content", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.step_audio) == ["self", "slots", "audio", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.open) == ["self", "prompt_condition", "mel2", "style2"]
    assert len(L.svc_rt_pitch.argtypes) == 18


# --------------------------------------------------------------------------------------------------------- the statement
def test_cache_update_and_fifo_by_hand():
    old = np.arange(10, dtype=np.float32) + 100                       # Tf = 10
    win = np.arange(6, dtype=np.float32) + 200                        # W = 6: context frames 4 .. 9
    new = WC.cache_update(old, win, 3, 2)                             # guard 2: frames 6 .. 9 from the window, 0 .. 5 from old[3 .. 8]
    assert new.tolist() == [103, 104, 105, 106, 107, 108, 202, 203, 204, 205]
    assert WC.cache_update(old, win, 3, 3).tolist() == [103, 104, 105, 106, 107, 108, 109, 203, 204, 205]      # W - guard = n_new: old[9] is used
    assert WC.cache_update(old, old + 50, 4, 0).tolist() == (old + 50).tolist()                               # W = Tf, guard 0: the window
    odd = np.array([np.nan, -0.0, np.inf, 1.0], np.float32)
    odd.view(np.int32)[0] |= 0x1234                                   # a NaN payload moves as it is
    assert WC.bits(WC.cache_update(odd, odd[2:], 2, 0)).tolist() == WC.bits(odd)[[2, 3, 2, 3]].tolist()
    assert WC.bits(WC.cache_update(np.roll(odd, 2), odd[2:], 2, 0))[:2].tolist() == WC.bits(odd)[:2].tolist()
    # the FIFO: capacity 5, pushes of 2
    fifo, gone = [], []
    for call in ([1, -1], [2, 3], [4, 5], [-1, 6]):
        fifo, d = WC.fifo_step(fifo, call, 5)
        gone.append(d)
    assert gone == [[], [], [1], [-1, 2]] and fifo == [3, 4, 5, -1, 6]
    assert WC.ring_words([1, -1, 2, 3, 4, 5, -1, 6], 5).tolist() == [5, -1, 6, 3, 4, 3, 5]      # entry t in word t % 5; head 3, fill 5
    assert WC.ring_words([7, 8], 5).tolist() == [7, 8, 0, 0, 0, 0, 2] and WC.ring_words([], 3).tolist() == [0] * 5
    assert WC.entries_of(np.array([500, 64, 0, 128, 999], np.float32), 3, 1) == [256, -1, 512]


def test_win_step_model_by_hand():
    """Tf = 6, W = 4, guard 1, n_new = 2, lag = 1, memory 3: three calls of 64 Hz, then 128 Hz, then unvoiced frames.  The ring of
    three holds [64, 128, 128] after the second call (the first 64 has left: n = 3, median bin 512), and after the third
    [128, -, -]: n = 1."""
    wins = np.array([[7, 64, 64, 999], [64, 128, 128, 999], [128, 0, np.nan, 999]], np.float32)
    words, cache, fifo, ns, bins = np.zeros(PC.WORDS, np.int32), np.zeros(6, np.float32), [], [], []
    for w in wins:
        r = WC.win_step_model(words, cache, fifo, w, 2, 1, 1, 3, 0.0, 0, 0.0, 0, 0.0)
        words, cache, fifo = r["words"], r["cache"], r["fifo"]
        ns.append(int(words[PC.W_N]))
        bins.append(int(words[PC.W_BIN]))
    assert ns == [2, 3, 1] and bins == [256, 512, 512] and fifo == [512, -1, -1]
    assert words[256] == 0 and words[512] == 1 and words[:PC.BINS].sum() == 1
    assert cache[:3].tolist() == [64, 128, 128] and cache[3] == 0 and np.isnan(cache[4]) and cache[5] == 999      # 64 64 | 128 128 | 0 nan
    # without a memory nothing leaves
    r = WC.win_step_model(np.zeros(PC.WORDS, np.int32), np.zeros(6, np.float32), [], wins[0], 2, 1, 1, 0, 0.0, 0, 0.0, 0, 0.0)
    assert r["fifo"] == [] and r["words"][PC.W_N] == 2
    # when n falls below the warm-up the target is 0 again
    ref = float(np.log(256.0))
    warm = WC.win_step_model(words * 0, cache * 0, [], wins[0], 2, 1, 1, 3, ref, 1, 0.0, 2, 0.0)
    assert warm["shift"] == pytest.approx(np.log(256.0 / 64.0), abs=PC.HALF_BIN)
    w2 = WC.win_step_model(warm["words"], warm["cache"], warm["fifo"], wins[2], 2, 1, 1, 3, ref, 1, 0.0, 2, 0.0)
    assert w2["words"][PC.W_N] == 1 and w2["shift"] == 0.0


@pytest.mark.parametrize("sabotage", WC.SABOTAGES)
def test_every_planted_sabotage_is_caught_by_a_case(sabotage):
    """The words, the cache, the FIFO or the shift of at least one call of at least one planted case differ from the clean
    statement.  The guard sabotages have to be caught by the guard case, the capacity ones by a stream whose ring of 10 fills
    in the middle of its third call."""
    caught = [n for n in PC.STREAMS if WC.trace(WC.run_stream(n)) != WC.trace(WC.run_stream(n, sabotage))]
    if WC.trace(WC.run_guard()) != WC.trace(WC.run_guard(sabotage)):
        caught.append("guard")
    print(sabotage, "caught by", caught)
    assert caught
    if sabotage.startswith("guard"):
        assert "guard" in caught
    if sabotage in ("expire_newest", "expire_keeps_n", "cap_minus", "cap_plus"):      # the statistics see it, not only the FIFO
        words = lambda rs: [r["words"].tobytes() for r in rs]                           # noqa: E731
        assert any(words(WC.run_stream(n)) != words(WC.run_stream(n, sabotage)) for n in PC.STREAMS)


def test_the_planted_cases_hold_what_they_promise():
    assert (WC.TF, WC.W, WC.GUARD, WC.N_NEW, WC.LAG, WC.MEMORY) == (48, 20, 6, 4, 2, 10)
    assert WC.TF - WC.W + WC.GUARD <= WC.TF - WC.LAG - WC.N_NEW                       # the counted frames are trusted window frames
    a = WC.run_stream("A")
    assert [len(r["fifo"]) for r in a] == [4, 8, 10, 10, 10, 10]                      # the ring fills in the middle of the third call
    # with no memory the windowed stream counts what the full-context stream counts
    for n in PC.STREAMS:
        assert [r["words"].tobytes() for r in WC.run_stream(n, memory=0)] == [r["words"].tobytes() for r in PC.run_stream(n)], n
    # with it, n is the number of voiced entries held
    for n in PC.STREAMS:
        for r in WC.run_stream(n):
            assert int(r["words"][PC.W_N]) == sum(x >= 0 for x in r["fifo"]) == int(r["words"][:PC.BINS].sum())
    b = WC.run_stream("B")
    assert [int(r["words"][PC.W_N]) for r in b] == [3, 5, 5, 6, 5, 3]
    # the cache of a fresh stream: zeros where the stream never wrote, the provisional junk never below the window
    c = a[-1]["cache"]
    full = PC.stream_rows("A")[-1]
    first = WC.TF - WC.W + WC.GUARD - (WC.N_CALLS - 1) * WC.N_NEW                     # the oldest frame a window ever wrote
    assert not c[:first].any() and np.array_equal(WC.bits(c[first:]), WC.bits(full[first:]))
    # the guard case: clean, the untrusted voiced frame is not taken and the trusted unvoiced one is
    g, keep = WC.run_guard()[0], WC.GUARD_CASE["Tf"] - WC.GUARD_CASE["W"] + WC.GUARD_CASE["guard"]
    assert g["cache"][keep - 1] == 0.0 and g["cache"][keep] == 0.0 and g["words"][PC.W_N] == 3
    assert WC.run_guard("guard_minus")[0]["cache"][keep - 1] == 250.0
    gp = WC.run_guard("guard_plus")[0]
    assert gp["cache"][keep] == 300.0 and gp["words"][PC.W_N] == 4
    # the register case: five calls count the low register, three the high one
    rows = WC.register_rows()
    low, high = PC.bins_of(np.float32([WC.LOW_HZ, WC.HIGH_HZ]))[1]
    res = WC.run_stream("A", memory=3 * WC.N_NEW, rows=rows)
    assert abs(int(res[-1]["words"][PC.W_BIN]) - high) < 40 and abs(int(res[4]["words"][PC.W_BIN]) - low) < 40
    assert abs(int(WC.run_stream("A", memory=0, rows=rows)[-1]["words"][PC.W_BIN]) - low) < 40
    assert len(set(WC.distinct_row(4096, 1).tolist())) == 4096 and (WC.distinct_row(4096, 1) > 1).all()


# ----------------------------------------------------------------------------------------------------- the tail's frames
@pytest.mark.parametrize("L16", [44160 - 1, 44160, 44160 + 1, 44160 + 159, 3840, 3999, 1920 + 77])
@pytest.mark.parametrize("Wn", [4, 12, 64])
def test_the_tail_slice_has_W_frames_centred_on_the_last_context_frames(L16, Wn):
    """RMVPE's frame j of a clip is centred on sample 160 j and a clip of n samples has 1 + n / 160 frames.  The slice that starts
    at s0 = 160 (Tf - W) has exactly W frames whatever L16 mod 160 is, and its frame j is centred on context frame Tf - W + j."""
    from seedvc_amd.rmvpe import RMVPE
    Tf = RMVPE.frames(L16)
    Wn = min(Wn, Tf)
    s0 = RMVPE.HOP * (Tf - Wn)
    assert 0 <= s0 <= L16 and RMVPE.frames(L16 - s0) == Wn
    assert [(s0 + RMVPE.HOP * j) // RMVPE.HOP for j in range(Wn)] == list(range(Tf - Wn, Tf)) and s0 % RMVPE.HOP == 0
    assert RMVPE.frames(L16 - s0 - 1) == Wn - (1 if L16 % RMVPE.HOP == 0 else 0)       # one sample less crosses the edge only there


# ------------------------------------------------------------------------------------------------- refusals without a GPU
# fake, never dereferenced addresses of disjoint buffers: the checks come first
F0, STATE, REF, OUT, SHIFT, CACHE, RING, RAW = (ctypes.c_void_p(a << 20) for a in (1, 2, 4, 5, 6, 7, 8, 9))


def _win(f0=F0, stride=20, W=20, guard=6, Tf=48, n_new=4, lag=2, slots=(0, 2), max_slots=3, cache=CACHE, ring=RING, memory=10, state=STATE,
         ref=REF, auto=(1, 0), semis=(0.0, 2.0), warmup=50, max_step=0.05, out=OUT, out_stride=48, raw=RAW, raw_stride=48, shift=SHIFT,
         N=None):
    from seedvc_amd import _lib
    return _lib.lib().svc_rt_pitch_win(f0, stride, W, guard, Tf, n_new, lag, len(slots) if N is None else N,
                                       i32(*slots) if slots is not None else None, max_slots, cache, ring, memory, state, ref,
                                       i32(*auto) if auto is not None else None, f32(*semis) if semis is not None else None, warmup,
                                       max_step, out, out_stride, raw, raw_stride, shift, None)


at = lambda base, words: ctypes.c_void_p((base << 20) + 4 * words)      # noqa: E731
BAD = dict(
    # what svc_rt_pitch refuses
    n_new_zero=dict(n_new=0), lag_negative=dict(lag=-1), window_before_the_row=dict(n_new=12, lag=40, memory=12), N_zero=dict(slots=(), auto=(), semis=()),
    N_65=dict(slots=tuple(range(65)), auto=(0,) * 65, semis=(0.0,) * 65, max_slots=70), slot_above=dict(slots=(0, 3)),
    slot_negative=dict(slots=(-1, 0)), slot_twice=dict(slots=(2, 2)), stride_below_W=dict(stride=19), out_stride_below_Tf=dict(out_stride=47),
    warmup_negative=dict(warmup=-1), max_step_nan=dict(max_step=float("nan")), semis_inf=dict(semis=(0.0, float("inf"))),
    null_f0=dict(f0=None), null_slots=dict(slots=None, N=2), null_state=dict(state=None), null_ref=dict(ref=None), null_auto=dict(auto=None),
    null_out=dict(out=None), Tf_zero=dict(Tf=0), max_slots_zero=dict(max_slots=0), out_off_4_bytes=dict(out=ctypes.c_void_p((5 << 20) + 2)),
    # the window's own rules
    W_zero=dict(W=0, guard=0), W_above_Tf=dict(W=49, stride=49), guard_negative=dict(guard=-1), window_below_n_new=dict(guard=17),
    Tf_above_the_limit=dict(Tf=4097, out_stride=4097, raw_stride=4097), memory_negative=dict(memory=-1), memory_below_n_new=dict(memory=3),
    null_cache=dict(cache=None), ring_without_memory=dict(memory=0), memory_without_ring=dict(ring=None),
    raw_stride_below_Tf=dict(raw_stride=47),
    # overlaps
    out_is_f0=dict(out=F0), out_in_f0=dict(out=at(1, 39)), out_in_cache=dict(out=at(7, 3 * 48 - 1)), out_in_state=dict(out=at(2, 3 * 1544 - 1)),
    out_in_ring=dict(out=at(8, 3 * 12 - 1)), raw_is_cache=dict(raw=CACHE), raw_in_f0=dict(raw=at(1, 5)), raw_in_state=dict(raw=at(2, 100)),
    raw_in_ring=dict(raw=at(8, 0)), raw_in_out=dict(raw=at(5, 95)), f0_in_out=dict(f0=at(5, 50)), cache_in_state=dict(cache=at(2, 10)),
    ring_in_cache=dict(ring=at(7, 8)), f0_is_cache=dict(f0=CACHE))

@pytest.mark.parametrize("bad", list(BAD.values()), ids=list(BAD))
def test_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _win(**bad) != 0
    assert b"rt_pitch_win" in _lib.lib().svc_last_error()


def test_the_allocators_check_their_sizes():
    from seedvc_amd import rmvpe
    for bad in ((0, 48), (3, 0), (3, 4097)):
        with pytest.raises(ValueError, match="rt_pitch_cache"):
            rmvpe.rt_pitch_cache(*bad, device="cpu")
    with pytest.raises(ValueError, match="rt_pitch_ring"):
        rmvpe.rt_pitch_ring(3, -1, device="cpu")
    assert rmvpe.rt_pitch_ring(3, 0, device="cpu") is None
    c, r = rmvpe.rt_pitch_cache(3, 48, device="cpu"), rmvpe.rt_pitch_ring(3, 10, device="cpu")
    assert c.shape == (3, 48) and c.dtype == torch.float32 and not c.any()
    assert r.shape == (3, 12) and r.dtype == torch.int32 and not r.any()


# --------------------------------------------------------------------------------------------------------------- the engine
class _Cfm:
    device = torch.device("cpu")
    in_channels = 4


class RecordingLR:
    def __init__(self):
        self.cfg = dict(f0_condition=True)
        self.calls = []

    def __call__(self, x, **kw):
        self.calls.append(kw)
        return RT.FakeLR()(x, ylens=kw["ylens"])


class FakeRmvpe:
    """Stand-in RMVPE: `f0_batch` returns planted tracks, row k = 100 (k + 1) + frame index, and records its calls."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def frames(n):
        return 1 + int(n) // 160

    def f0_batch(self, waves, lens=None, thred=0.03):
        self.calls.append((tuple(waves.shape), waves.is_contiguous(), lens, thred))
        T = self.frames(waves.size(1))
        return 100.0 * (torch.arange(waves.size(0)).float()[:, None] + 1) + torch.arange(T).float()[None, :]


def _engine(**kw):
    from seedvc_amd.pipeline import RealtimeEngine
    return RealtimeEngine(RecordingLR(), _Cfm(), None, **{**RT.FAKE_GEOMETRY, **kw})


RS = lambda a, b: types.SimpleNamespace(orig_freq=a, new_freq=b, _h=None)      # noqa: E731
REFS = (torch.zeros(1, 5, 6), torch.zeros(1, 4, 5), torch.zeros(1, 3))


def _attached(L16=3840, lag=3, **kw):
    eng = _engine(max_streams=3, **kw)
    eng.attach_audio(RA.FakeContent(), RS(22050, 16000), 882, L16, 0.04)       # L16 = 3840: 25 f0 frames, a block counts 4, ce = 2
    rm = FakeRmvpe()
    eng.attach_pitch(rm, lag_frames=lag, warmup_frames=7, max_step_cents=1200.0, thred=0.05)
    return eng, rm


def test_the_settings_are_engine_wide_checked_and_off_by_default():
    eng = _engine(max_streams=3)
    for call in (lambda: eng.set_pitch_window(12, 2), lambda: eng.set_pitch_memory(40)):
        with pytest.raises(ValueError, match="attach_pitch has not been called"):
            call()
    eng, rm = _attached()
    p = eng._pitch
    assert p["win"] is None and p["memory"] == 0 and p["cache"] is None and p["ring"] is None          # off unless set
    # Tf = 25, n_new = 4, lag = 3: window - guard >= 7; a window of 4 frames is 480 samples, below RMVPE's 513
    for bad in ((12, -1), (26, 0), (12, 6), (8, 2), (12, None)):
        with pytest.raises(ValueError, match="set_pitch_window"):
            eng.set_pitch_window(*bad)
    short, _ = _attached(lag=2)
    short._pitch["n_new"], short._pitch["lag"] = 1, 2                                                 # let the frame rule pass: the sample rule
    with pytest.raises(ValueError, match="RMVPE takes at least 513"):
        short.set_pitch_window(4, 0)
    short.set_pitch_window(5, 0)                                                                      # 640 samples
    for bad in (3, 0, -5):
        with pytest.raises(ValueError, match="set_pitch_memory"):
            eng.set_pitch_memory(bad)
    assert p["cache"] is None and p["ring"] is None                                                   # a refused call leaves the engine as it was
    eng.set_pitch_window(12, 5)                                                                       # 12 - 5 = 4 + 3
    assert p["win"] == (12, 5) and p["cache"].shape == (3, 25) and p["ring"] is None
    eng.set_pitch_memory(4)
    assert p["memory"] == 4 and p["ring"].shape == (3, 6) and p["ring"].dtype == torch.int32
    eng.set_pitch_window(None)
    assert p["win"] is None and p["cache"].shape == (3, 25) and p["ring"].shape == (3, 6)              # the memory still needs both
    eng.set_pitch_memory(None)
    assert p["memory"] == 0 and p["cache"] is None and p["ring"] is None
    eng.set_pitch_window(25, 0)
    assert p["win"] == (25, 0)
    # refused while a slot is open; open / reset / close zero the slot's rows
    assert eng.open(*REFS) == 0
    for call in (lambda: eng.set_pitch_window(12, 2), lambda: eng.set_pitch_window(None), lambda: eng.set_pitch_memory(40),
                 lambda: eng.set_pitch_memory(None)):
        with pytest.raises(ValueError, match="streams are open"):
            call()
    assert p["win"] == (25, 0)
    eng.close(0)
    eng.set_pitch_memory(9)
    for act in ("open", "reset", "close"):
        if act != "open":
            assert eng.open(*REFS) == 0
        for name in ("state", "cache", "ring"):
            p[name].fill_(7)
        getattr(eng, act)(*(REFS if act == "open" else (0,)))
        for name in ("state", "cache", "ring"):
            assert not p[name][0].any() and (p[name][1:] == 7).all(), (act, name)
        if act != "close":
            eng.close(0)
    # a second attach_pitch starts from everything off
    eng.attach_pitch(rm)
    assert eng._pitch["win"] is None and eng._pitch["memory"] == 0 and eng._pitch["cache"] is None
    # a context above the kernel's limit
    eng._pitch["Tf"] = 4097
    for call in (lambda: eng.set_pitch_window(64, 8), lambda: eng.set_pitch_memory(40)):
        with pytest.raises(ValueError, match="at most 4096"):
            call()


@pytest.mark.parametrize("L16", [3840, 3840 + 159, 4000 - 1])
def test_the_pitch_stage_runs_rmvpe_on_the_tail_and_one_window_step(monkeypatch, L16):
    """`_pitch_track` with a planted RMVPE and a recording `rt_pitch_win`: one f0_batch on the contiguous tail ctx[:, 160 (Tf - W):]
    with the attached threshold, one rt_pitch_win with the slots' settings, the cache and the ring; the regulator's track is the
    shifted one from frame 2 ce on.  With only the memory on the window is the whole context with guard 0.  With neither on the
    step is `rt_pitch` on the whole context, as it was."""
    from seedvc_amd import rmvpe as rmvpe_mod
    eng, rm = _attached(L16=L16)
    p = eng._pitch
    Tf = p["Tf"]
    assert Tf == 1 + L16 // 160
    seen, plain = [], []

    def fake_win(f0_win, guard, n_new, lag, slots, cache, ring, state, ref_median, auto_adjust, semitones=None, warmup=50, max_step=0.0,
                 return_shift=False, return_raw=False):
        seen.append(dict(win=f0_win, guard=guard, n_new=n_new, lag=lag, slots=slots, cache=cache, ring=ring, state=state, ref=ref_median,
                         auto=auto_adjust, semis=semitones, warmup=warmup, max_step=max_step, flags=(return_shift, return_raw)))
        out = torch.full((f0_win.size(0), cache.size(1)), 3.0)
        res = (out,) + ((torch.arange(f0_win.size(0)).float(),) if return_shift else ()) + ((out + 1,) if return_raw else ())
        return res if len(res) > 1 else out

    def fake_plain(f0, *a, **kw):
        plain.append(tuple(f0.shape))
        return (f0, torch.zeros(f0.size(0))) if kw.get("return_shift") else f0

    monkeypatch.setattr(rmvpe_mod, "rt_pitch_win", fake_win)
    monkeypatch.setattr(rmvpe_mod, "rt_pitch", fake_plain)
    eng.set_pitch_window(12, 5)
    assert [eng.open(*REFS) for _ in range(3)] == [0, 1, 2]
    p["has_ref"].add(2)
    eng.set_pitch(2, semitones=12, auto_adjust=True)
    eng.set_pitch(0, semitones=-1.5)
    ctx = torch.arange(2 * L16).float().reshape(2, L16)
    f0, f0_lens, parts = eng._pitch_track([2, 0], ctx, True)
    s0 = 160 * (Tf - 12)
    assert rm.calls == [((2, L16 - s0), True, None, 0.05)] and FakeRmvpe.frames(L16 - s0) == 12
    (c,) = seen
    assert (c["guard"], c["n_new"], c["lag"], c["slots"], c["auto"], c["semis"], c["warmup"], c["flags"]) == \
        (5, 4, 3, [2, 0], [1, 0], [12.0, -1.5], 7, (True, True))
    assert c["cache"] is p["cache"] and c["ring"] is None and c["state"] is p["state"] and c["ref"] is p["ref_median"]
    assert c["max_step"] == pytest.approx(np.log(2.0)) and tuple(c["win"].shape) == (2, 12)
    assert torch.equal(parts["f0_window"], c["win"]) and torch.equal(parts["f0_raw"], torch.full((2, Tf), 4.0))
    assert torch.equal(parts["f0"], torch.full((2, Tf), 3.0)) and parts["pitch_shift"].tolist() == [0.0, 1.0]
    assert f0.shape == (2, Tf - 4) and f0_lens == [Tf - 4] * 2 and plain == []
    f0b, _, none = eng._pitch_track([1], ctx[:1], False)
    assert none is None and seen[-1]["flags"] == (False, False) and f0b.shape == (1, Tf - 4)
    # only the memory: W = Tf, guard 0, the whole context
    for s in (0, 1, 2):
        eng.close(s)
    eng.set_pitch_window(None)
    eng.set_pitch_memory(8)
    assert eng.open(*REFS) == 0
    eng._pitch_track([0], ctx[:1], False)
    assert rm.calls[-1][0] == (1, L16) and tuple(seen[-1]["win"].shape) == (1, Tf) and seen[-1]["guard"] == 0
    assert seen[-1]["ring"] is p["ring"] and p["ring"].shape == (3, 10) and plain == []
    # neither: the svc_rt_pitch path
    eng.close(0)
    eng.set_pitch_memory(None)
    assert eng.open(*REFS) == 0
    n_seen = len(seen)
    _, _, parts = eng._pitch_track([0], ctx[:1], True)
    assert plain == [(1, Tf)] and len(seen) == n_seen and "f0_window" not in parts and rm.calls[-1][0] == (1, L16)
