"""CPU side of the streams' pitch step (`svc_rt_pitch`, `rmvpe.rt_pitch`, `RealtimeEngine.attach_pitch` / `set_reference_f0` /
`set_pitch` / `step_f0`): the entry points are declared, exported and bound and the existing signatures stay; the
statement of rt_pitch_cases.py against hand-computed values and against its own planted sabotages; the argument checks of the
call, which come before anything touches a device; and the engine's host logic with stand-ins: a regulator that records the
f0 it is given, an RMVPE that returns planted tracks."""
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
    for name in ("svc_rt_pitch", "svc_rt_pitch_state_words"):
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert "enum { SVC_RT_PITCH_BINS = 1536, SVC_RT_PITCH_STATE_WORDS = 1536 + 8 };" in header
    for phrase in ("clamp((float_bits(f0) >> 15) - 33792, 0, 1535)", "r = (n - 1) / 2", "((bin + 33792) << 15) | 0x4000",
                   "Rows of slots that are not listed keep every bit", "Refused (non-zero, svc_last_error() names it, nothing touched)"):
        assert phrase in header, phrase
    L = _lib.lib()
    assert len(L.svc_rt_pitch.argtypes) == 18
    assert L.svc_rt_pitch_state_words(1) == PC.WORDS and L.svc_rt_pitch_state_words(64) == 64 * PC.WORDS
    assert L.svc_rt_pitch_state_words(0) == 0 and L.svc_rt_pitch_state_words(-3) == 0
    assert (rmvpe.PITCH_BINS, rmvpe.PITCH_STATE_WORDS) == (PC.BINS, PC.WORDS)
    sig = lambda f: list(inspect.signature(f).parameters)                              # noqa: E731
    E = pipeline.RealtimeEngine
    assert sig(E.attach_pitch) == ["self", "rmvpe", "lag_frames", "warmup_frames", "max_step_cents", "thred"]
    assert [p.default for p in inspect.signature(E.attach_pitch).parameters.values()][2:] == [8, 50, 100.0, 0.03]
    assert sig(E.set_pitch) == ["self", "slot", "semitones", "auto_adjust"]
    assert sig(E.set_reference_f0) == ["self", "slot", "f0_ref", "f0_ref_frames"]
    assert sig(E.step_f0)[:6] == ["self", "slots", "content", "f0", "f0_lens", "n_timesteps"]
    # existing signatures stay
    assert sig(E.step) == ["self", "slots", "content", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.step_audio) == ["self", "slots", "audio", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.open) == ["self", "prompt_condition", "mel2", "style2"] and sig(E.reset) == ["self", "slot"]


# --------------------------------------------------------------------------------------------------------- the statement
def test_binning_against_hand_computed_values():
    """256 bins per octave from 32 Hz: 2^(k / 256) steps are not float edges, but powers of two and their mantissa steps are."""
    v, b = PC.bins_of(np.array([32.0, 64.0, 1024.0, 2047.99, 2048.0, 5000.0, np.inf, 31.0, 1.0, 0.0, np.nan, -440.0, 48.0,
                                np.nextafter(np.float32(48.0), np.float32(0)), 1.0000001], np.float32))
    assert v.tolist() == [True] * 8 + [False] * 4 + [True] * 3
    assert b[:8].tolist() == [0, 256, 1280, 1535, 1535, 1535, 1535, 0]
    assert b[12:].tolist() == [128, 127, 0]                   # 48 = 32 x 1.5: half an octave of mantissa steps
    assert PC.bin_edge(0) == 32.0 and PC.bin_edge(256) == 64.0 and PC.bin_edge(128) == 48.0
    assert PC.bin_centre(0) == np.float32(32.0 * (1 + 2.0 ** -9)) and PC.bin_edge(1) == np.float32(32.0 * (1 + 2.0 ** -8))
    assert PC.count_window(48, 4, 2) == (42, 46) and PC.count_window(25, 4, 8) == (13, 17) and PC.count_window(46, 44, 2) == (0, 44)
    # the rank: lower middle.  counts 3 | 3 -> rank 2 is in the first bin; 3 | 4 -> rank 3 is in the second
    h = np.zeros(PC.BINS, np.int64)
    h[10], h[20] = 3, 3
    assert PC.median_bin(h, 6) == 10 and PC.median_bin(h, 6, "rank") == 20
    h[20] = 4
    assert PC.median_bin(h, 7) == 20 and PC.median_bin(np.zeros(PC.BINS), 0) == 0
    h[:] = 0
    h[1535] = 1
    assert PC.median_bin(h, 1) == 1535


def test_step_model_by_hand():
    """One stream, three calls of 2 counted frames at lag 1 in a row of 5: 64 Hz twice, then 128 Hz twice, then unvoiced.  The
    median stays in the bin of 64 Hz (rank (4 - 1) / 2 = 1 of 2 | 2); reference one octave above it; 0.5 per call."""
    c64 = float(np.log(np.float64(PC.bin_centre(256)) + np.float64(PC.EPS32)))
    ref = c64 + np.log(2.0)
    rows = np.array([[500, 500, 64, 64, 999], [64, 64, 128, 128, 999], [128, 128, 0, np.nan, 999]], np.float32)
    words, shifts = np.zeros(PC.WORDS, np.int32), []
    for r in rows:
        res = PC.step_model(words, r, 2, 1, ref, 1, 12.0, 2, 0.5)
        words = res["words"]
        shifts.append(res["shift"])
    assert words[256] == 2 and words[512] == 2 and words[:PC.BINS].sum() == 4 and words[PC.W_N] == 4 and words[PC.W_BIN] == 256
    assert shifts[0] == 0.5 and shifts[1] == pytest.approx(np.log(2.0), abs=1e-12) and shifts[2] == shifts[1]     # arrival is exact
    assert words[PC.W_SHIFT:PC.W_SHIFT + 1].view(np.float32)[0] == np.float32(shifts[2])
    # the last call's output: voiced frames two octaves up (shift + 12 semitones), unvoiced frames exp(log(f0 + 1e-5))
    out = res["out"]
    assert out[:2] == pytest.approx([512.0, 512.0], rel=1e-6) and out[2] == pytest.approx(1e-5, rel=1e-6) and np.isnan(out[3])
    assert out[4] == pytest.approx(999 * 4, rel=1e-6)
    # below the warm-up, or with auto off, the target is 0 and an applied shift glides back
    res = PC.step_model(words, rows[2], 2, 1, ref, 0, 0.0, 2, 0.5)
    assert res["shift"] == pytest.approx(np.log(2.0) - 0.5) and res["limited"]
    assert PC.step_model(words, rows[2], 2, 1, ref, 1, 0.0, 5, 0.0)["shift"] == 0.0              # step off: at once
    assert PC.step_model(words, rows[2], 2, 1, ref, 1, 0.0, 4, float("inf"))["shift"] == pytest.approx(np.log(2.0))
    # a reference median that is not positive (0: a reference without a voiced frame) is no reference: no automatic shift
    for none in (0.0, -1.0, float("nan")):
        assert PC.step_model(words, rows[2], 2, 1, none, 1, 0.0, 2, 0.0)["shift"] == 0.0
    assert PC.step_model(words, rows[2], 2, 1, 1e-3, 1, 0.0, 2, 0.0)["shift"] == pytest.approx(1e-3 - c64)


def _trace(results):
    return [(r["words"].tobytes(), r["shift"]) for r in results]


@pytest.mark.parametrize("sabotage", PC.SABOTAGES)
def test_every_planted_sabotage_is_caught_by_a_case(sabotage):
    """The cases of the GPU tests tell a kernel with the fault from a correct one: the state words or the applied shift of at
    least one call of at least one planted stream (or of the glide case) differ from the clean statement."""
    caught = [n for n in PC.STREAMS if _trace(PC.run_stream(n)) != _trace(PC.run_stream(n, sabotage))]
    if _trace(PC.run_glide()) != _trace(PC.run_glide(sabotage)):
        caught.append("glide")
    print(sabotage, "caught by", caught)
    assert caught


def test_the_planted_streams_hold_what_they_promise():
    b = PC.run_stream("B")
    n = [int(r["words"][PC.W_N]) for r in b]
    assert n == [3, 5, 6, 10, 10, 11] and PC.WARMUP == 6                       # odd, warmup - 1, warmup, even
    assert [int(r["words"][PC.W_BIN]) for r in b] == [PC.X_BIN] * 3 + [PC.Y_BIN] * 3
    assert b[0]["words"][PC.X_BIN] == 3 and b[0]["words"][:PC.BINS].sum() == 3                  # all frames in one bin
    assert b[2]["words"][PC.X_BIN] == 3 and b[2]["words"][PC.Y_BIN] == 3                        # the tie at the rank
    assert [r["shift"] for r in b[:2]] == [0.0, 0.0] and b[2]["shift"] == 0.25 and b[2]["limited"]
    assert not b[3]["limited"] and b[3]["shift"] == b[4]["shift"] == b[5]["shift"]
    a = PC.run_stream("A")
    assert [int(r["words"][PC.W_N]) for r in a] == [3, 5, 9, 11, 15, 19]
    w = a[-1]["words"]
    assert w[700] == 3 and w[699] == 1 and w[701] == 1      # edge 700, its centre, one ulp below edge 701 | below edge 700 | edge 701
    assert w[0] == 5 and w[1] == 1                          # 1 + ulp, 31, 32, one ulp below 32, one ulp below edge 1 | edge 1
    assert w[1535] == 6 and w[1534] == 1                    # 2047.99, 5000, +inf, one ulp below 2048, 2048, edge 1535 | below it
    c = PC.run_stream("C")
    assert [int(r["words"][PC.W_N]) for r in c] == [1, 4, 8, 10, 10, 13] and all(r["shift"] == 0.0 for r in c)
    g = PC.run_glide()
    assert [r["shift"] for r in g[:2]] == [0.25, 0.5] and g[2]["shift"] == g[3]["shift"] and not g[2]["limited"]
    assert g[2]["shift"] == pytest.approx(np.log(2.0), abs=PC.HALF_BIN)
    st = PC.sentinel_state()
    assert (st[:, :PC.BINS].sum(1) == st[:, PC.W_N]).all()


# ------------------------------------------------------------------------------------------------- refusals without a GPU
# fake, never dereferenced addresses of disjoint buffers: the checks come first
F0, STATE, REF, OUT, SHIFT = (ctypes.c_void_p(a << 20) for a in (1, 2, 4, 5, 6))


def _pitch(f0=F0, stride=48, Tf=48, n_new=4, lag=2, slots=(0, 2), max_slots=3, state=STATE, ref=REF, auto=(1, 0), semis=(0.0, 2.0),
           warmup=50, max_step=0.05, out=OUT, out_stride=48, shift=SHIFT, N=None):
    from seedvc_amd import _lib
    return _lib.lib().svc_rt_pitch(f0, stride, Tf, n_new, lag, len(slots) if N is None else N, i32(*slots) if slots is not None else None,
                                   max_slots, state, ref, i32(*auto) if auto is not None else None,
                                   f32(*semis) if semis is not None else None, warmup, max_step, out, out_stride, shift, None)


BAD = dict(n_new_zero=dict(n_new=0), n_new_negative=dict(n_new=-4), lag_negative=dict(lag=-1), window_before_the_row=dict(n_new=40, lag=9),
           lag_past_the_row=dict(lag=45), N_zero=dict(slots=(), auto=(), semis=()), N_negative=dict(N=-1),
           N_65=dict(slots=tuple(range(65)), auto=(0,) * 65, semis=(0.0,) * 65, max_slots=70),
           slot_above=dict(slots=(0, 3)), slot_negative=dict(slots=(-1, 0)), slot_twice=dict(slots=(2, 2)),
           stride_below_Tf=dict(stride=47), out_stride_below_Tf=dict(out_stride=47), warmup_negative=dict(warmup=-1),
           max_step_nan=dict(max_step=float("nan")), semis_inf=dict(semis=(0.0, float("inf"))), semis_nan=dict(semis=(float("nan"), 0.0)),
           null_f0=dict(f0=None), null_slots=dict(slots=None, N=2), null_state=dict(state=None), null_ref=dict(ref=None),
           null_auto=dict(auto=None), null_out=dict(out=None), out_is_f0=dict(out=F0),
           out_in_f0=dict(out=ctypes.c_void_p((1 << 20) + 4 * 95)), out_in_state=dict(out=ctypes.c_void_p((2 << 20) + 4 * 3 * 1544 - 4)),
           f0_in_out=dict(f0=ctypes.c_void_p((5 << 20) + 4 * 50)), Tf_zero=dict(Tf=0, n_new=1, lag=0), max_slots_zero=dict(max_slots=0),
           out_off_4_bytes=dict(out=ctypes.c_void_p((5 << 20) + 2)))


@pytest.mark.parametrize("bad", list(BAD.values()), ids=list(BAD))
def test_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _pitch(**bad) != 0
    assert b"rt_pitch" in _lib.lib().svc_last_error()


# --------------------------------------------------------------------------------------------------------------- the engine
class _Cfm:
    device = torch.device("cpu")
    in_channels = 4


class RecordingLR:
    """Stand-in regulator: records the keyword arguments of every call and answers as `realtime_cases.FakeLR`."""

    def __init__(self, f0_condition=True):
        self.cfg = dict(f0_condition=f0_condition)
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
        self.calls.append((tuple(waves.shape), lens, thred))
        T = self.frames(waves.size(1))
        return 100.0 * (torch.arange(waves.size(0)).float()[:, None] + 1) + torch.arange(T).float()[None, :]


def _engine(lr=None, **kw):
    from seedvc_amd.pipeline import RealtimeEngine
    return RealtimeEngine(lr, _Cfm(), None, **{**RT.FAKE_GEOMETRY, **kw})


RS = lambda a, b: types.SimpleNamespace(orig_freq=a, new_freq=b, _h=None)      # noqa: E731
REFS = (torch.zeros(1, 5, 6), torch.zeros(1, 4, 5), torch.zeros(1, 3))


def test_attach_pitch_and_set_pitch_errors_need_no_gpu():
    eng = _engine(RecordingLR(), max_streams=3)
    assert eng.open(*REFS) == 0
    rm = FakeRmvpe()
    with pytest.raises(ValueError, match="attach_audio has not been called"):
        eng.attach_pitch(rm)
    with pytest.raises(ValueError, match="attach_pitch has not been called"):
        eng.set_pitch(0, 2.0)
    with pytest.raises(ValueError, match="attach_pitch has not been called"):
        eng.set_reference_f0(0, torch.full((1, 9), 220.0))
    eng.attach_audio(RA.FakeContent(), RS(22050, 24000), 441, 4800, 0.04)
    with pytest.raises(ValueError, match="RMVPE takes 16000"):
        eng.attach_pitch(rm)
    eng.attach_audio(RA.FakeContent(), RS(22050, 16000), 882, 3840, 0.04)       # 25 f0 frames, a block counts 4, ce = 2
    for bad in (dict(lag_frames=1), dict(lag_frames=22),                           # 25 - 22 - 4 < 0
                dict(warmup_frames=-1), dict(max_step_cents=float("nan")), dict(rmvpe=object())):
        with pytest.raises(ValueError, match="attach_pitch"):
            eng.attach_pitch(**{**dict(rmvpe=rm), **bad})
    assert eng._pitch is None                                                      # a refused attach leaves the engine as it was
    plain = _engine(RecordingLR(f0_condition=False), max_streams=3)
    plain.attach_audio(RA.FakeContent(), RS(22050, 16000), 882, 3840, 0.04)
    with pytest.raises(ValueError, match="not f0-conditioned"):
        plain.attach_pitch(rm)
    far = _engine(RecordingLR(), max_streams=3)
    far.attach_audio(RA.FakeContent(), RS(22050, 16000), 882, 3840, 0.26)          # ce = 13: 26 frames dropped of 25
    with pytest.raises(ValueError, match="2 ce"):
        far.attach_pitch(rm)
    eng.attach_pitch(rm, lag_frames=21)                                            # 25 - 21 - 4 = 0: the window starts the row
    eng.attach_pitch(rm)
    p = eng._pitch
    assert (p["lag"], p["warmup"], p["Tf"], p["n_new"], p["thred"]) == (8, 50, 25, 4, 0.03)
    assert p["max_step"] == pytest.approx(np.log(2.0) / 12.0)                      # 100 cents in natural-log units
    assert p["state"].shape == (3, PC.WORDS) and p["state"].dtype == torch.int32 and not p["state"].any()
    assert p["ref_median"].shape == (3,) and p["ref_median"].dtype == torch.float32
    eng.attach_pitch(rm, max_step_cents=0.0)
    assert eng._pitch["max_step"] == 0.0
    eng.attach_pitch(rm)
    p = eng._pitch
    # set_pitch: as set_gate.  No reference median: no automatic shift
    eng.set_pitch(0, semitones=-3)
    assert p["semis"] == {0: -3.0} and p["auto"] == {}
    with pytest.raises(ValueError, match="a second attach would drop"):           # a slot holds a setting: no silent loss
        eng.attach_pitch(rm)
    assert eng._pitch is p
    with pytest.raises(ValueError, match="no reference median"):
        eng.set_pitch(0, auto_adjust=True)
    eng.set_pitch(0, auto_adjust=False)
    assert p["auto"] == {0: False}
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="set_pitch"):
            eng.set_pitch(0, semitones=bad)
    for bad in (1, 3, -1):                                                         # closed or outside
        with pytest.raises(ValueError, match="set_pitch"):
            eng.set_pitch(bad, 1.0)
        with pytest.raises(ValueError, match="set_reference_f0"):
            eng.set_reference_f0(bad, torch.full((1, 9), 220.0))
    for bad in (dict(f0_ref=torch.zeros(2, 9)), dict(f0_ref=torch.zeros(1, 0)), dict(f0_ref=torch.zeros(1, 9), f0_ref_frames=10),
                dict(f0_ref=torch.zeros(1, 9), f0_ref_frames=0)):
        with pytest.raises(ValueError, match="set_reference_f0"):
            eng.set_reference_f0(0, **bad)
    # reset zeroes the slot's statistics and keeps its settings; open and close forget them
    p["state"].fill_(7)
    p["has_ref"].add(0)
    p["ref_median"].fill_(5.0)
    eng.set_pitch(0, auto_adjust=True)
    eng.reset(0)
    assert not p["state"][0].any() and (p["state"][1:] == 7).all()
    assert p["semis"] == {0: -3.0} and p["auto"] == {0: True} and p["has_ref"] == {0} and p["ref_median"][0] == 5.0
    eng.close(0)
    assert p["semis"] == {} and p["auto"] == {} and p["has_ref"] == set() and p["ref_median"].tolist() == [0.0, 5.0, 5.0]
    p["state"].fill_(7)
    assert eng.open(*REFS) == 0 and not p["state"][0].any() and (p["state"][1:] == 7).all()


def test_the_pitch_stage_hands_the_regulator_the_track_from_frame_2_ce(monkeypatch):
    """`_pitch_track` with a planted RMVPE and a recording `rt_pitch`: one f0_batch on the context with the attached threshold,
    one rt_pitch with the slots' settings, and the regulator's track is the shifted one from frame 2 ce on, Tf - 2 ce frames."""
    from seedvc_amd import rmvpe as rmvpe_mod
    lr, rm = RecordingLR(), FakeRmvpe()
    eng = _engine(lr, max_streams=4)
    assert [eng.open(*REFS) for _ in range(3)] == [0, 1, 2]
    eng.attach_audio(RA.FakeContent(), RS(22050, 16000), 882, 3840, 0.04)
    eng.attach_pitch(rm, lag_frames=3, warmup_frames=7, max_step_cents=1200.0, thred=0.05)
    p = eng._pitch
    p["has_ref"].add(2)
    eng.set_pitch(2, semitones=12, auto_adjust=True)
    eng.set_pitch(0, semitones=-1.5)
    seen = []

    def fake_rt_pitch(f0, n_new, lag, slots, state, ref_median, auto_adjust, semitones=None, warmup=50, max_step=0.0, return_shift=False):
        seen.append(dict(f0=f0, n_new=n_new, lag=lag, slots=slots, state=state, ref=ref_median, auto=auto_adjust, semis=semitones,
                         warmup=warmup, max_step=max_step, return_shift=return_shift))
        return (f0 * 2, torch.arange(f0.size(0)).float()) if return_shift else f0 * 2

    monkeypatch.setattr(rmvpe_mod, "rt_pitch", fake_rt_pitch)
    ctx = torch.zeros(2, 3840)
    f0, f0_lens, parts = eng._pitch_track([2, 0], ctx, True)
    assert rm.calls == [((2, 3840), None, 0.05)]
    (c,) = seen
    assert (c["n_new"], c["lag"], c["slots"], c["auto"], c["semis"], c["warmup"], c["return_shift"]) == (4, 3, [2, 0], [1, 0], [12.0, -1.5], 7, True)
    assert c["max_step"] == pytest.approx(np.log(2.0)) and c["state"] is p["state"] and c["ref"] is p["ref_median"]
    raw = rm.f0_batch(ctx)
    assert torch.equal(c["f0"], raw) and torch.equal(parts["f0_raw"], raw) and torch.equal(parts["f0"], raw * 2)
    assert f0.shape == (2, 21) and f0_lens == [21, 21] and torch.equal(f0, (raw * 2)[:, 4:])      # ce = 2: four frames dropped
    assert parts["pitch_shift"].tolist() == [0.0, 1.0] and parts["pitch_voiced"].tolist() == [0, 0]
    f0b, _, none = eng._pitch_track([0], ctx[:1], False)
    assert none is None and seen[-1]["return_shift"] is False and seen[-1]["auto"] == [0] and f0b.shape == (1, 21)
    # the regulator call: the track and its lengths with a pitch track, the call it always was without one
    content = torch.zeros(2, 10, 6)
    eng._regulate(content, 2, f0, f0_lens)
    eng._regulate(content, 2, None, None)
    with_f0, without = lr.calls
    assert sorted(with_f0) == ["f0", "f0_lens", "n_quantizers", "ylens"] and with_f0["f0"] is f0 and with_f0["f0_lens"] == [21, 21]
    assert sorted(without) == ["f0", "n_quantizers", "ylens"] and without["f0"] is None and without["n_quantizers"] == 3
    assert without["ylens"].tolist() == [RT.FAKE_GEOMETRY["S"]] * 2 and with_f0["ylens"].tolist() == without["ylens"].tolist()


class _Stop(Exception):
    """Raised by the recording regulator: the step has made the call under test, what follows needs a device."""


class StoppingLR(RecordingLR):
    def __call__(self, x, **kw):
        self.calls.append(kw)
        raise _Stop


def test_a_step_without_pitch_calls_the_regulator_as_before_and_step_f0_adds_the_track(monkeypatch):
    """`step` itself, up to its regulator call (the device context manager replaced by a null one, the regulator stops the
    step): without a pitch track the keywords are exactly ylens, n_quantizers = 3 and f0 = None -- no f0_lens, the call the
    engine made before pitch existed, with or without `attach_pitch`; `step_f0` adds the caller's track and its lengths."""
    import contextlib
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    lr = StoppingLR()
    eng = _engine(lr, max_streams=2)
    assert [eng.open(*REFS), eng.open(*REFS)] == [0, 1]
    content = torch.zeros(2, 10, 6)
    for attach in (False, True):
        if attach:
            eng.attach_audio(RA.FakeContent(), RS(22050, 16000), 882, 3840, 0.04)
            eng.attach_pitch(FakeRmvpe())
        with pytest.raises(_Stop):
            eng.step([1, 0], content, 3, 0.7)
        kw = lr.calls.pop()
        assert sorted(kw) == ["f0", "n_quantizers", "ylens"] and kw["f0"] is None and kw["n_quantizers"] == 3, attach
        assert kw["ylens"].tolist() == [RT.FAKE_GEOMETRY["S"]] * 2
    f0 = torch.full((2, 9), 220.0)
    with pytest.raises(_Stop):
        eng.step_f0([1, 0], content, f0, [9, 7], 3, 0.7)
    kw = lr.calls.pop()
    assert sorted(kw) == ["f0", "f0_lens", "n_quantizers", "ylens"] and kw["f0"] is f0 and kw["f0_lens"] == [9, 7]
    assert lr.calls == []


def test_step_f0_argument_errors_need_no_gpu():
    eng = _engine(RecordingLR(), max_streams=2)
    assert eng.open(*REFS) == 0
    content = torch.zeros(1, 10, 6)
    for bad in (dict(f0=None), dict(f0=torch.zeros(2, 9)), dict(f0=torch.zeros(9)), dict(f0_lens=[10]), dict(f0_lens=[3, 3]), dict(f0_lens=[-1])):
        with pytest.raises(ValueError, match="step_f0"):
            eng.step_f0([0], content, **{**dict(f0=torch.zeros(1, 9), f0_lens=None), **bad}, n_timesteps=3, inference_cfg_rate=0.7)
    assert eng.length_regulator.calls == []
