"""CPU side of the FSMN-VAD (`svc_vad_*`, `svc_rt_out_dev`, `seedvc_amd.vad`, `RealtimeEngine.attach_vad` / `set_vad`; DESIGN.md
8n): the entry points are declared, exported and bound; the row counts and the streaming history against hand-computed values;
the detector model of vad_cases.py on hand-made decision sequences, cut at every position; the exactness of the run split in
float64; the yardstick's fbank against a direct DFT; the spread and the fp32 error of the random case; and every refusal of
every new entry and of the engine, which come before anything touches a device."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import realtime_cases as RT
import rt_audio_cases as RA
import vad_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)      # noqa: E731
NEW = ("svc_vad_create", "svc_vad_destroy", "svc_vad_rows", "svc_vad_history", "svc_vad_state_floats", "svc_vad_scores", "svc_vad_detect",
       "svc_vad_step", "svc_rt_out_dev")


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, vad
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    L = _lib.lib()
    assert len(L.svc_rt_out_dev.argtypes) == len(L.svc_rt_out.argtypes) + 1 == 20
    assert len(L.svc_vad_scores.argtypes) == 9 and len(L.svc_vad_detect.argtypes) == 13 and len(L.svc_vad_step.argtypes) == 16
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert L.svc_vad_state_floats(3) == 3 * vad.STATE_FLOATS == 3 * (4 * 19 * 128 + 32) and L.svc_vad_state_floats(0) == 0
    assert ctypes.sizeof(_lib.VadConfig) == 32
    c = vad.vad_config()
    assert c == dict(V.CONFIG, p_max=c["p_max"]) and abs(c["p_max"] - 0.2) < 1e-12
    with pytest.raises(ValueError, match="speech_2_noise_ratio"):
        vad.vad_config(speech_2_noise_ratio=1.2)
    with pytest.raises(ValueError, match="unknown"):
        vad.vad_config(snr_thres=3)
    for bad in (dict(win=33), dict(win=0), dict(on_count=21), dict(off_count=-1), dict(end_silence=0), dict(seg_rows=8), dict(p_max=1.5)):
        with pytest.raises(ValueError, match="FsmnVad"):
            vad.check_config(dict(c, **bad))


# ----------------------------------------------------------------------------------------------------- rows and the history
def test_rows_and_history_against_hand_computed_values():
    from seedvc_amd import _lib
    L = _lib.lib()
    # n:       399  400  559  560  640  960  2880
    frames = {399: 0, 400: 1, 559: 1, 560: 2, 640: 2, 960: 4, 2880: 16}
    for n, F in frames.items():
        assert V.frames_of(n) == F
        assert L.svc_vad_rows(n, 1) == V.rows_of(n, True) == F
        assert L.svc_vad_rows(n, 0) == V.rows_of(n, False) == max(0, F - 2)
    assert L.svc_vad_rows(0, 0) == 0 and L.svc_vad_rows(32000, 1) == 198 and L.svc_vad_rows(32000, 0) == 196
    # a block of m 20 ms frames renews n_new = 320 m samples.  Row i stacks frames i - 2 .. i + 2 and frame f starts at sample
    # 160 f.  After `total` = 160 j samples (j >= 6) the stream has j - 2 frames, so rows 0 .. j - 5 are out; the next row,
    # j - 4, starts with frame j - 6 at sample 160 (j - 6) = total - 960.  Below j = 6 the first frame read is frame 0.
    for m in (1, 9):
        total, rows = 0, 0
        for step in range(12):
            n_new = 320 * m
            want = total if total <= 960 else 960
            assert L.svc_vad_history(total) == V.history_of(total) == want, (m, step)
            r0, r1 = L.svc_vad_rows(total, 0), L.svc_vad_rows(total + n_new, 0)
            assert r0 == rows and r1 - r0 <= n_new // 160
            # the first frame of the first new row and the last frame of the last one lie inside [total - history, total + n_new)
            if r1 > r0:
                assert 160 * max(0, r0 - 2) == total - want and 160 * (r1 + 1) + 400 <= total + n_new
            total, rows = total + n_new, r1
        assert rows == total // 160 - 4
    assert [L.svc_vad_history(160 * j) for j in range(9)] == [0, 160, 320, 480, 640, 800, 960, 960, 960]


# -------------------------------------------------------------------------------------------------------------- the detector
def _events(cfg, dec):
    return V.detect(cfg, V.fresh_state(), dec)[0]


def test_detector_model_on_hand_made_sequences():
    cfg = V.CONFIG
    # 30 silent frames, then speech: the window holds 15 speech frames at frame 44, the 15th; lookback 20 -> begin at 24
    dec = [0] * 30 + [1] * 40 + [0] * 100
    ev = _events(cfg, dec)
    assert ev[0] == (V.BEGIN, 240)
    # speech ends at frame 69; the window sum falls to 15 at frame 74 (5 silent frames in the window): the window state is Sil
    # from there, the 65th such frame is 74 + 64 = 138
    assert ev[1:] == [(V.END, 1380)]
    # speech from frame 0: the 15th speech frame is 14, lookback is clamped at 0
    assert _events(cfg, [1] * 20)[0] == (V.BEGIN, 0)
    # a second segment right behind the first: its lookback is clamped at the end of the first
    dec2 = [1] * 20 + [0] * 70 + [1] * 20
    ev2 = _events(cfg, dec2)
    # speech ends at frame 19, the window state is Sil from frame 24, the segment ends at 24 + 64 = 88; the second one opens at
    # frame 90 + 14 = 104, and 104 - 20 = 84 lies before the end of the first
    assert ev2 == [(V.BEGIN, 0), (V.END, 880), (V.BEGIN, 880)]
    # one transition per frame, on first: with on_count = off_count a window that stays at 15 flips back the frame after
    st = V.fresh_state()
    V.detect(cfg, st, [1] * 15)
    assert st["win_state"] == 1 and st["sum"] == 15
    V.detect(cfg, st, [0])
    assert st["win_state"] == 0
    # forced end with a small config: the segment reaches max_segment frames, the ring is cleared, it reopens 15 frames later
    small = dict(cfg, max_segment=40)
    ev3 = _events(small, [1] * 100)
    assert ev3[:2] == [(V.BEGIN, 0), (V.END, 390)]
    assert ev3[2] == (V.BEGIN, 10 * max(39, 54 - 20)) and ev3[3] == (V.END, 10 * (39 + 39))
    # the flag: 1 while inside a segment at any frame of the call, the call that closes it included; an empty call keeps it
    st = V.fresh_state()
    assert V.detect(cfg, st, [0] * 10)[1] == 0
    assert V.detect(cfg, st, [1] * 15)[1] == 1
    assert V.detect(cfg, st, [], flag=1)[1] == 1
    assert V.detect(cfg, st, [0] * 70)[1] == 1 and st["in_seg"] == 0
    assert V.detect(cfg, st, [0])[1] == 0
    # decisions: <= in float32, NaN is silence
    lo, hi = np.nextafter(np.float32(0.2), np.float32(0)), np.nextafter(np.float32(0.2), np.float32(1))
    assert V.decisions([0.01, 0.99, np.float32(0.2), lo, hi, np.nan], 0.2).tolist() == [1, 0, 1, 1, 0, 0]


@pytest.mark.parametrize("name", ["open_close", "two_segments", "forced"])
def test_detector_model_gives_the_same_events_wherever_the_sequence_is_cut(name):
    cfg = V.CONFIG if name != "forced" else dict(V.CONFIG, max_segment=40)
    dec = {"open_close": [0] * 30 + [1] * 40 + [0] * 100, "two_segments": [1] * 20 + [0] * 70 + [1] * 20 + [0] * 80,
           "forced": [1] * 100 + [0] * 70}[name]
    ev, st, _ = V.detect_in_calls(cfg, dec, [])
    assert len(ev) >= 2
    for cut in range(len(dec) + 1):
        ev2, st2, _ = V.detect_in_calls(cfg, dec, [cut])
        assert ev2 == ev and st2 == st, cut
    ev3, st3, _ = V.detect_in_calls(cfg, dec, list(range(7, len(dec), 7)))
    assert ev3 == ev and st3 == st


# ------------------------------------------------------------------------------------------------------- the run split
def test_a_run_with_76_rows_of_warm_up_equals_the_unsplit_run_in_float64():
    """The claim behind svc_vad_scores' runs: started from zero caches 76 rows before its first row, a run gives the bits of the
    unsplit run.  (75 rows are not enough: the check would be vacuous if any warm-up did.)"""
    sd = V.random_state_dict(3)
    m = V.encoder(sd)
    x = torch.randn(200, V.D_IN, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    with V.rowwise():
        full = m(x)[0]
        for edge in (96, 131):
            part = m(x[edge - V.WARM:])[0][V.WARM:]
            assert torch.equal(part, full[edge:]), edge
            short = m(x[edge - V.WARM + 1:])[0][V.WARM - 1:]
            assert not torch.equal(short[:1], full[edge:edge + 1])
        # carried caches: cut anywhere, bit for bit
        a, cache = m(x[:57])
        b, _ = m(x[57:], cache)
        assert torch.equal(torch.cat([a, b]), full)


# ------------------------------------------------------------------------------------------------------------ the yardstick
def test_yardstick_fbank_against_a_direct_dft_on_two_frames():
    w = V.noise_clip(560, 11)
    got = V.fbank(w)
    assert got.shape == (2, 80)
    x = w.astype(np.float64) * 32768.0
    bank = V.mel_bank(np.float64)
    for f in range(2):
        fr = x[160 * f:160 * f + 400].copy()
        fr -= fr.mean()
        fr = np.concatenate([[fr[0] - 0.97 * fr[0]], fr[1:] - 0.97 * fr[:-1]])
        fr *= 0.54 - 0.46 * np.cos(2 * np.pi * np.arange(400) / 399)
        spec = np.array([sum(fr[n] * np.exp(-2j * np.pi * k * n / 512) for n in range(400)) for k in range(257)])
        want = np.log(np.maximum(bank @ (np.abs(spec) ** 2), V.EPS32))
        assert np.abs(got[f] - want).max() < 1e-9
    # the triangles: unit peak spacing in mel, nothing at DC or at Nyquist, every bin has weight
    assert bank.shape == (80, 257) and not bank[:, 0].any() and not bank[:, 256].any() and (bank.sum(1) > 0.5).all()
    assert np.abs(V.mel_bank(np.float32) - bank).max() < 1e-4
    # LFR: row 0 repeats frame 0 three times; a final call repeats the last frame, a non-final one stops two rows early
    feat = np.arange(6 * 80, dtype=np.float64).reshape(6, 80)
    zero, one = np.zeros(400), np.ones(400)
    rows = V.lfr_cmvn(feat, True, zero, one).reshape(6, 5, 80)
    assert rows[0, :, 0].tolist() == [0, 0, 0, 80, 160] and rows[5, :, 0].tolist() == [240, 320, 400, 400, 400]
    assert np.array_equal(V.lfr_cmvn(feat, False, zero, one), rows.reshape(6, 400)[:4])
    assert np.array_equal(V.lfr_cmvn(feat, True, one, 2 * one), (rows.reshape(6, 400) + 1) * 2)
    # digital silence sits on the epsilon floor
    assert np.array_equal(V.fbank(np.zeros(400, np.float32)), np.full((1, 80), np.log(V.EPS32)))


def test_random_case_spreads_and_its_fp32_error_is_the_recorded_one():
    ps = np.concatenate([p64 for final in (0, 1) for (p64, _), _ in V.reference(final)])
    assert len(ps) == sum(V.rows_of(n, f) for f in (0, 1) for n in V.SCORE_LENS) == 610
    assert ps.min() > 0.01 and ps.max() < 0.99                                  # the logit is well conditioned on every row
    q = np.percentile(ps, [5, 95])
    assert q[0] < 0.15 and q[1] > 0.85 and 0.05 < (ps <= 0.2).mean() < 0.5       # both decisions occur
    ep, el = V.reference_error()
    # the recorded constants are this measurement (BLAS builds block fp32 sums differently: a factor of 2 either way)
    assert V.REF_ERR[0] / 2 <= ep <= V.REF_ERR[0] * 2 and V.REF_ERR[1] / 2 <= el <= V.REF_ERR[1] * 2, (ep, el)


def test_energy_vad_is_a_sigmoid_of_the_mean():
    sd = V.energy_vad_state_dict(2.0, 3.0)
    m = V.encoder(sd)
    x = torch.zeros(5, 400, dtype=torch.float64)
    for r, mean in enumerate((-16.0, 1.0, 2.0, 3.0, 20.0)):
        x[r] = mean + torch.linspace(-1, 1, 400, dtype=torch.float64)
    p, _ = V.p_and_logit(m(x)[0])
    want = 1.0 / (1.0 + np.exp(-3.0 * (2.0 - np.array([-16.0, 1.0, 2.0, 3.0, 20.0]))))
    assert np.abs(p.numpy() - want).max() < 1e-6         # the dict is float32: 1 / 400 is rounded


# ------------------------------------------------------------------------------------------------- refusals without a GPU
# fake, never dereferenced addresses of disjoint buffers: the checks come first, the handle last
A = lambda mb, off=0: ctypes.c_void_p((mb << 20) + off)      # noqa: E731
WAVE, PS, STATE, FS, EV, NEV, FLAGS, X = (A(a) for a in (16, 32, 48, 64, 80, 81, 82, 96))


def _err():
    from seedvc_amd import _lib
    return _lib.lib().svc_last_error().decode()


def _scores(wave=WAVE, lens=(400, 1000), L=1000, final=1, seg=0, p=PS):
    from seedvc_amd import _lib
    return _lib.lib().svc_vad_scores(None, wave, i32(*lens) if lens is not None else None, len(lens) if lens is not None else 2, L, final,
                                     seg, p, None)


SCORES_BAD = dict(lens_above_L=dict(lens=(400, 1001)), lens_negative=dict(lens=(-1, 5)), lens_null=dict(lens=None), L_zero=dict(L=0, lens=(0, 0)),
                  final_2=dict(final=2), seg_rows_8=dict(seg=8), seg_rows_negative=dict(seg=-16), wave_null=dict(wave=None), p_null=dict(p=None),
                  p_in_wave=dict(p=A(16, 4000)), p_off_4_bytes=dict(p=A(32, 2)), B_65=dict(lens=(400,) * 65), B_0=dict(lens=()))


@pytest.mark.parametrize("bad", list(SCORES_BAD.values()), ids=list(SCORES_BAD))
def test_scores_argument_errors_need_no_gpu(bad):
    assert _scores(**bad) != 0
    assert "svc_vad_scores" in _err() and "vad is NULL" not in _err()


def _detect(p=PS, ld=50, n_rows=(50, 0), slots=(2, 0), max_slots=3, state=STATE, fs=FS, ev=EV, nev=NEV, flags=FLAGS):
    from seedvc_amd import _lib
    return _lib.lib().svc_vad_detect(None, p, ld, i32(*n_rows) if n_rows is not None else None, len(slots),
                                     i32(*slots) if slots is not None else None, max_slots, state, fs, ev, nev, flags, None)


DETECT_BAD = dict(n_rows_above_ld=dict(n_rows=(51, 0)), n_rows_negative=dict(n_rows=(-1, 0)), n_rows_6001=dict(ld=7000, n_rows=(6001, 0)),
                  slot_twice=dict(slots=(1, 1)), slot_above=dict(slots=(0, 3)), slot_negative=dict(slots=(-1, 0)), ld_zero=dict(ld=0, n_rows=(0, 0)),
                  max_slots_zero=dict(max_slots=0), p_null=dict(p=None), state_null=dict(state=None), events_null=dict(ev=None),
                  n_events_null=dict(nev=None), flags_null=dict(flags=None), n_rows_null=dict(n_rows=None),
                  flags_in_state=dict(flags=A(48, 8)), events_in_p=dict(ev=A(32, 16)), frame_speech_is_p=dict(fs=PS),
                  n_events_in_events=dict(nev=A(80, 8)), state_off_4_bytes=dict(state=A(48, 1)), flags_in_events=dict(flags=A(80, 120)),
                  N_65=dict(slots=tuple(range(65)), n_rows=(0,) * 65, max_slots=65))


@pytest.mark.parametrize("bad", list(DETECT_BAD.values()), ids=list(DETECT_BAD))
def test_detect_argument_errors_need_no_gpu(bad):
    assert _detect(**bad) != 0
    assert "svc_vad_detect" in _err() and "vad is NULL" not in _err()


def _step(x=X, stride=4000, end=3680, n_new=320, total=(0, 3200), slots=(1, 0), max_slots=2, state=STATE, flags=FLAGS, p=PS, max_rows=2,
          ev=EV, nev=NEV):
    from seedvc_amd import _lib
    return _lib.lib().svc_vad_step(None, x, stride, end, n_new, i64(*total) if total is not None else None, len(slots),
                                   i32(*slots) if slots is not None else None, max_slots, state, flags, p, max_rows, ev, nev, None)


STEP_BAD = dict(n_new_off_the_grid=dict(n_new=300), n_new_zero=dict(n_new=0), n_new_above=dict(n_new=16160, end=17000, stride=17000),
                end_past_the_row=dict(end=4001), end_below_n_new=dict(end=300), history_missing=dict(end=1279),    # 1279 - 320 < 960
                history_missing_young_stream=dict(end=800, total=(0, 640)),                                        # 480 < 640
                total_off_the_grid=dict(total=(0, 100)), total_negative=dict(total=(-160, 0)), total_null=dict(total=None),
                slot_twice=dict(slots=(0, 0)), slot_above=dict(slots=(0, 2)), max_rows_short=dict(max_rows=1), x_null=dict(x=None),
                state_null=dict(state=None), flags_null=dict(flags=None), events_without_count=dict(nev=None),
                count_without_events=dict(ev=None), flags_in_state=dict(flags=A(48, 64)), p_in_x=dict(p=A(96, 1000)),
                state_in_x=dict(state=A(96, 4 * 7000)), events_in_p=dict(ev=A(32, 0)), x_off_4_bytes=dict(x=A(96, 2)),
                N_65=dict(slots=tuple(range(65)), total=(0,) * 65, max_slots=65))


@pytest.mark.parametrize("bad", list(STEP_BAD.values()), ids=list(STEP_BAD))
def test_step_argument_errors_need_no_gpu(bad):
    assert _step(**bad) != 0
    assert "svc_vad_step" in _err() and "vad is NULL" not in _err()


def test_good_arguments_reach_the_handle_check_and_create_refuses_without_a_device():
    """The cases above differ from these calls in one argument each: these pass every check but the last, the handle."""
    from seedvc_amd import _lib
    for call, name in ((_scores, "svc_vad_scores"), (_detect, "svc_vad_detect"), (_step, "svc_vad_step")):
        assert call() != 0
        assert _err().endswith(f"{name}: vad is NULL"), _err()
    assert _step(end=1280) != 0 and _err().endswith("vad is NULL")                # exactly 960 samples of history
    assert _step(p=None, ev=None, nev=None) != 0 and _err().endswith("vad is NULL")
    assert _detect(fs=None) != 0 and _err().endswith("vad is NULL")
    L = _lib.lib()
    out = ctypes.c_void_p()
    cfg = _lib.VadConfig(0.2, 20, 15, 15, 20, 65, 6000, 0)
    descs = (_lib.TensorDesc * 1)()
    for bad in (dict(win=33), dict(on_count=0), dict(off_count=21), dict(end_silence=0), dict(seg_rows=15), dict(lookback=-1)):
        c = _lib.VadConfig(0.2, 20, 15, 15, 20, 65, 6000, 0)
        for k, v in bad.items():
            setattr(c, k, v)
        assert L.svc_vad_create(ctypes.byref(c), descs, 1, A(1), A(2), None, ctypes.byref(out)) != 0 and "svc_vad_create" in _err()
    assert L.svc_vad_create(None, descs, 1, A(1), A(2), None, ctypes.byref(out)) != 0
    assert L.svc_vad_create(ctypes.byref(cfg), descs, 1, None, A(2), None, ctypes.byref(out)) != 0 and not out.value


WAVE2, STATE2, FI, FO, INFER, OUT, OFFS, SPD = (ctypes.c_void_p(a << 20) for a in (1, 2, 3, 4, 5, 6, 7, 9))


def _out_dev(wave=WAVE2, stride=40, start=4, n_in=30, slots=(1, 0), state=STATE2, max_slots=2, speech=(1, 0), spd=SPD, fi=FI, fo=FO, block=20,
             Lb=8, Ls=2, infer=INFER, out=OUT, offs=OFFS, N=None):
    from seedvc_amd import _lib
    return _lib.lib().svc_rt_out_dev(None, wave, stride, start, n_in, len(slots) if N is None else N, state, max_slots, i32(*slots),
                                     i32(*speech) if speech is not None else None, spd, fi, fo, block, Lb, Ls, infer, out, offs, None)


OUT_DEV_BAD = dict(n_in_is_not_n_inf=dict(n_in=29), past_the_row=dict(start=11), infer_null=dict(infer=None), speech_2=dict(speech=(1, 2)),
                   infer_is_out=dict(infer=OUT), slot_twice=dict(slots=(1, 1)), slot_above=dict(slots=(0, 2)), null_out=dict(out=None),
                   dev_is_infer=dict(spd=INFER), dev_in_wave=dict(spd=ctypes.c_void_p((1 << 20) + 64)), dev_is_state=dict(spd=STATE2),
                   dev_is_out=dict(spd=OUT), dev_is_fade_in=dict(spd=FI), dev_is_fade_out=dict(spd=FO), dev_on_offsets=dict(spd=ctypes.c_void_p((7 << 20) + 4)),
                   dev_off_4_bytes=dict(spd=ctypes.c_void_p((9 << 20) + 2)))


@pytest.mark.parametrize("bad", list(OUT_DEV_BAD.values()), ids=list(OUT_DEV_BAD))
def test_rt_out_dev_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _out_dev(**bad) != 0
    assert b"rt_out_dev" in _lib.lib().svc_last_error()
    assert _out_dev(N=0) == 0                                                     # the good arguments pass every check (N = 0 launches nothing)


# ----------------------------------------------------------------------------------------------------------- the engine
class _Cfm:
    device = torch.device("cpu")
    in_channels = 4


class _Vad:
    def step(self, *a, **k):
        raise AssertionError("no step in this test")


def test_engine_attach_vad_set_vad_and_state_zeroing_need_no_gpu():
    from seedvc_amd.pipeline import RealtimeEngine
    from seedvc_amd.vad import CACHE_FLOATS, STATE_FLOATS
    rs = lambda a, b: types.SimpleNamespace(orig_freq=a, new_freq=b, _h=None)      # noqa: E731
    eng = RealtimeEngine(None, _Cfm(), None, max_streams=3, **RT.FAKE_GEOMETRY)
    with pytest.raises(ValueError, match=r"RealtimeEngine\.attach_vad: attach_audio"):
        eng.attach_vad(_Vad())
    eng.attach_audio(RA.FakeContent(), rs(250, 150), 45, 200, 0.04)               # content rate 150 Hz
    with pytest.raises(ValueError, match=r"RealtimeEngine\.attach_vad: the content rate"):
        eng.attach_vad(_Vad())
    eng.attach_audio(RA.FakeContent(), rs(48000, 16000), 960, 1600, 0.04)          # 1600 - 320 - 320 = 960: just enough
    with pytest.raises(ValueError, match=r"RealtimeEngine\.attach_vad: vad has no step"):
        eng.attach_vad(object())
    eng.attach_audio(RA.FakeContent(), rs(48000, 16000), 960, 1280, 0.04)          # 640 samples of history
    with pytest.raises(ValueError, match=r"RealtimeEngine\.attach_vad: the context keeps 640"):
        eng.attach_vad(_Vad())
    assert eng._vad is None
    pc, mel, style = torch.zeros(1, 5, 6), torch.zeros(1, 4, 5), torch.zeros(1, 3)
    assert eng.open(pc, mel, style) == 0
    with pytest.raises(ValueError, match=r"set_vad: attach_vad has not been called"):
        eng.set_vad(0, True)
    eng.attach_audio(RA.FakeContent(), rs(48000, 16000), 9 * 960, 9 * 320 + 320 + 960, 0.04)
    eng.attach_vad(_Vad())
    v = eng._vad
    assert (v["n_new"], v["end"]) == (9 * 320, 9 * 320 + 960)
    assert v["state"].shape == (3, STATE_FLOATS) and v["state"].dtype == torch.float32 and not v["state"].any()
    assert v["flags"].dtype == torch.int32 and v["flags"].tolist() == [1, 1, 1] and v["on"] == set()
    for bad in (1, 3, -1):
        with pytest.raises(ValueError, match="set_vad"):
            eng.set_vad(bad, True)
    # on: the slot's state is zeroed, its flag starts at 0 and its sample count at 0; the others keep every bit
    v["state"].fill_(2.0)
    v["state"][:, CACHE_FLOATS:].view(torch.int32).fill_(7)
    eng.set_vad(0, True)
    assert v["on"] == {0} and v["flags"].tolist() == [0, 1, 1] and v["total"][0] == 0
    assert not v["state"][0].view(torch.int32).any() and (v["state"][1:, :CACHE_FLOATS] == 2).all()
    assert (v["state"][1:, CACHE_FLOATS:].view(torch.int32) == 7).all()
    # set again to the same value: nothing restarts
    v["state"][0].fill_(3.0)
    v["total"][0] = 2880
    v["flags"][0] = 1
    eng.set_vad(0, True)
    assert (v["state"][0] == 3).all() and v["total"][0] == 2880 and v["flags"].tolist() == [1, 1, 1]
    # reset restarts the stream's VAD and keeps it on; _speech keeps its meaning
    eng.set_speech(0, False)
    eng.reset(0)
    assert v["on"] == {0} and not v["state"][0].view(torch.int32).any() and v["total"][0] == 0 and v["flags"].tolist() == [0, 1, 1]
    assert eng._speech == {0: True}
    # off: the flag is held at 1
    v["state"][0].fill_(3.0)
    eng.set_vad(0, False)
    assert v["on"] == set() and v["flags"].tolist() == [1, 1, 1] and not v["state"][0].any()
    # close and open: off, zeroed
    eng.set_vad(0, True)
    v["state"][0].fill_(3.0)
    eng.close(0)
    assert v["on"] == set() and v["flags"].tolist() == [1, 1, 1] and not v["state"][0].any()
    assert eng.open(pc, mel, style) == 0 and v["on"] == set() and v["flags"].tolist() == [1, 1, 1]
