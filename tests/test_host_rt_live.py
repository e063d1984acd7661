"""CPU side of the live block step (`svc_rt_push_gated`, `svc_rt_out`, `RealtimeEngine.attach_output` / `set_speech` / `set_gate`,
`pipeline.realtime_output_geometry`): the entry points are declared, exported and bound and the existing
signatures stay; the output geometry against hand-computed values; the float64 gate model of rt_live_cases.py on a hand-made
energy sequence; the preconditions of the GPU tests (score gaps, gate margins, patterns that cross a block); and the argument
checks of the two calls and of the engine, which come before anything touches a device."""
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
import rt_live_cases as LV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
f32 = lambda *v: (ctypes.c_float * len(v))(*v)      # noqa: E731


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in ("svc_rt_push_gated", "svc_rt_out"):
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    L = _lib.lib()
    assert len(L.svc_rt_push_gated.argtypes) == 17 and len(L.svc_rt_out.argtypes) == 19
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    sig = lambda f: list(inspect.signature(f).parameters)                              # noqa: E731
    E = pipeline.RealtimeEngine
    assert sig(E.step) == ["self", "slots", "content", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.step_seeded) == ["self", "slots", "content", "n_timesteps", "inference_cfg_rate", "seeds", "vocoder_kwargs",
                                  "return_parts"]
    assert sig(E.step_audio) == ["self", "slots", "audio", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.step_audio_seeded) == ["self", "slots", "audio", "n_timesteps", "inference_cfg_rate", "seeds", "vocoder_kwargs",
                                        "return_parts"]
    assert sig(E.attach_audio) == ["self", "content", "resample", "Lin", "L16", "ce_dit_difference"]
    assert sig(E.attach_output) == ["self", "resample_out", "fade_in", "fade_out"]
    assert sig(E.set_speech) == ["self", "slot", "detected"] and sig(E.set_gate) == ["self", "slot", "threshold_db"]
    assert sig(pipeline.realtime_output_geometry) == ["g", "sr_model", "sr_out"]


# -------------------------------------------------------------------------------------------------------------- geometry
def test_output_geometry_against_hand_computed_values():
    from seedvc_amd.pipeline import realtime_geometry, realtime_output_geometry
    g = realtime_geometry(22050, 256, 0.18, 0.04, 2.5, 0.02, 2.0)
    assert (g["block"], g["Lb"], g["Ls"]) == (9 * 441, 2 * 441, 441)
    # 9, 2 and 1 units of 20 ms: 960 samples each at 48 kHz
    assert realtime_output_geometry(g, 22050, 48000) == dict(zc=960, block=8640, Lb=1920, Ls=960, n_inf=11520)
    g44 = realtime_geometry(44100, 512, 0.18, 0.04, 2.5, 0.02, 2.0)
    assert (g44["block"], g44["Lb"], g44["Ls"]) == (9 * 882, 2 * 882, 882)
    assert realtime_output_geometry(g44, 44100, 48000) == dict(zc=960, block=8640, Lb=1920, Ls=960, n_inf=11520)
    assert realtime_output_geometry(g, 22050, 22050) == dict(zc=441, block=3969, Lb=882, Ls=441, n_inf=5292)
    assert realtime_output_geometry(dict(block=6, Lb=3, Ls=0), 150, 250) == dict(zc=5, block=10, Lb=5, Ls=0, n_inf=15)
    for bad in ((g, 11025, 48000), (g, 22050, 48010), (g, 22050, 0), (dict(g, block=3970), 22050, 48000),
                (dict(g, Lb=440), 22050, 48000), (dict(g, Ls=1), 22050, 48000), (g, 44100, 48000)):      # 441-sample units at 44100
        with pytest.raises(ValueError, match="realtime_output_geometry"):
            realtime_output_geometry(*bad)


def test_gate_power_is_the_energy_of_80_ms_at_the_threshold():
    from seedvc_amd.pipeline import gate_power
    assert gate_power(None, 441) == 0.0 and gate_power(-60.0, 441) == 0.0 and gate_power(-75, 441) == 0.0
    assert gate_power(-40.0, 960) == float(np.float32(4 * 960 * 1e-4)) == float(LV.gate_power(-40.0, 960))
    assert gate_power(-59.9, 441) > 0.0 and gate_power(0.0, 5) == 20.0
    # a frame of constant magnitude a has RMS a: 4 such frames sit exactly on the threshold 20 log10(a) dB
    assert np.isclose(4 * LV.frame_energies(np.full(441, 0.01, np.float32), 441)[0], gate_power(-40.0, 441), rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------ the gate model
def test_gate_model_on_a_hand_made_energy_sequence():
    """Threshold 10.  The first three frames see zeros before the stream's start; a loud frame (100) keeps its own and the next
    three windows open, the fourth quiet frame after it is the first muted one; the carry hands the last three energies on."""
    e = [1.0, 2.0, 3.0, 3.5, 100.0, 1.0, 1.0, 1.0, 1.0, 8.0, 0.5]
    muted, E, carry = LV.gate_decisions(e, 10.0)
    assert E.tolist() == [1.0, 3.0, 6.0, 9.5, 108.5, 107.5, 105.5, 103.0, 4.0, 11.0, 10.5]
    assert muted.tolist() == [True, True, True, True, False, False, False, False, True, False, False]
    assert carry == (1.0, 8.0, 0.5)
    # block by block with the carry: the same decisions wherever the sequence is cut
    for cut in range(1, len(e)):
        m1, _, c1 = LV.gate_decisions(e[:cut], 10.0)
        m2, _, c2 = LV.gate_decisions(e[cut:], 10.0, c1)
        assert np.concatenate([m1, m2]).tolist() == muted.tolist() and c2 == carry, cut
    # E < power: an energy on the threshold is not muted, a NaN energy never mutes, power 0 mutes nothing
    assert LV.gate_decisions([2.5, 2.5, 2.5, 2.5], 10.0)[0].tolist() == [True, True, True, False]
    assert LV.gate_decisions([float("nan"), 0.0, 0.0, 0.0, 0.0], 10.0)[0].tolist() == [False, False, False, False, True]
    assert not LV.gate_decisions([0.0, 0.0], 0.0)[0].any()
    # a block through the gate: muted frames are +0.0, the others keep their bits, the carry holds RAW energies
    x = np.concatenate([np.full(4, 0.5, np.float32), np.full(4, 2.0, np.float32), np.full(4, -0.5, np.float32)])
    y, m, c = LV.gate_block(x, 4, 3.0, (0.0, 0.0, 0.0))
    assert m.tolist() == [True, False, False] and c == (1.0, 16.0, 1.0)
    assert not y[:4].any() and not np.signbit(y[:4]).any() and np.array_equal(y[4:], x[4:])


@pytest.mark.parametrize("m", [1, 9])
@pytest.mark.parametrize("pair", LV.GATE_PAIRS, ids=[f"{a}_{b}" for a, b in LV.GATE_PAIRS])
def test_gate_inputs_are_far_from_the_threshold_and_cross_a_block(pair, m):
    """The inputs of the GPU gate tests: every float64 window energy is at least 25 times off the -40 dB threshold (no frame is
    excluded), every stream's pattern has a run that the carried energies decide, and both decisions occur."""
    zc = pair[0] // 50
    power = LV.gate_power(LV.GATE_DB, zc)
    for s, loud in enumerate(LV.LOUD_FRAMES[m]):
        assert LV.pattern_crosses_a_block(loud, 6 * m, m), (s, loud)
        x = LV.gate_audio(loud, 6 * m, zc, seed=100 * m + s)
        muted, E, _ = LV.gate_decisions(LV.frame_energies(x, zc), power)
        assert LV.gate_margin(E, power) >= 24.9, (s, LV.gate_margin(E, power))
        assert muted.any() and not muted.all()
        first = min(f for f in loud if f + 4 < 6 * m and not (set(range(f + 1, f + 5)) & set(loud)) and (f + 4) // m > f // m)
        assert not muted[first:first + 4].any() and muted[first + 4]         # muting starts exactly at the fourth quiet frame


# ------------------------------------------------------------------------------------------- preconditions of the output tests
@pytest.mark.parametrize("Lb_units", [1, 4])
@pytest.mark.parametrize("pair", LV.OUT_PAIRS, ids=[f"{a}_{b}" for a, b in LV.OUT_PAIRS])
def test_output_cases_are_not_decided_by_a_near_tie(pair, Lb_units):
    """Every step of every stream of the GPU output tests has a float64 score gap of at least 1e-3, with and without the mute of
    step 2 of the middle stream where the buffer it leaves is not all zero (the precondition the GPU test asserts again)."""
    wave, state = LV.out_waves(pair, Lb_units, start=3, extra=2)
    for muted in ((), ((1, 1),)):
        for t, row in enumerate(LV.out_session(pair, Lb_units, wave, state, 3, muted)):
            for k, r in enumerate(row):
                if (t, k) in muted or not r["before"].any():
                    assert r["o"] == 0                                         # every score is 0: the lowest offset
                else:
                    assert RT.score_gap(r["scores"]) >= LV.GAP, (pair, Lb_units, t, k, RT.score_gap(r["scores"]))


# ------------------------------------------------------------------------------------------------- refusals without a GPU
# fake, never dereferenced addresses of disjoint buffers: the checks come first
BLOCK, HIST, RING, CTX, GE, GM = (ctypes.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 8 << 20, 12 << 20, 13 << 20))


def _push(block=BLOCK, stride=45, Lin=45, slots=(0, 2), max_slots=3, zc=5, z16=5, hist=HIST, ring=RING, L16=200, ctx=CTX,
          pow=(1.0, 0.0), ge=GE, gm=GM):
    from seedvc_amd import _lib
    return _lib.lib().svc_rt_push_gated(None, block, stride, Lin, len(slots), i32(*slots), max_slots, zc, z16, hist, ring, L16, ctx,
                                        f32(*pow) if pow is not None else None, ge, gm, None)


PUSH_BAD = dict(gate_e_null=dict(ge=None), pow_negative=dict(pow=(1.0, -1.0)), pow_nan=dict(pow=(float("nan"), 0.0)),
                gate_e_in_ring=dict(ge=ctypes.c_void_p((3 << 20) + 64)), gate_e_is_hist=dict(ge=HIST),
                mask_in_ctx=dict(gm=ctypes.c_void_p((8 << 20) + 400)), mask_is_block=dict(gm=BLOCK),
                mask_in_gate_e=dict(gm=ctypes.c_void_p((12 << 20) + 8)), gate_e_off_4_bytes=dict(ge=ctypes.c_void_p((12 << 20) + 2)),
                frames_257=dict(Lin=257 * 5, stride=257 * 5, L16=258 * 5 + 5),
                Lin_off_the_grid=dict(Lin=44), slot_twice=dict(slots=(2, 2)), null_ctx=dict(ctx=None))


@pytest.mark.parametrize("bad", list(PUSH_BAD.values()), ids=list(PUSH_BAD))
def test_gated_push_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _push(**bad) != 0
    assert b"rt_push" in _lib.lib().svc_last_error()


WAVE, STATE, FI, FO, INFER, OUT, OFFS = (ctypes.c_void_p(a << 20) for a in (1, 2, 3, 4, 5, 6, 7))


def _out(wave=WAVE, stride=40, start=4, n_in=30, slots=(1, 0), state=STATE, max_slots=2, speech=(1, 0), fi=FI, fo=FO, block=20, Lb=8,
         Ls=2, infer=INFER, out=OUT, offs=OFFS):
    from seedvc_amd import _lib
    return _lib.lib().svc_rt_out(None, wave, stride, start, n_in, len(slots), state, max_slots, i32(*slots),
                                 i32(*speech) if speech is not None else None, fi, fo, block, Lb, Ls, infer, out, offs, None)


OUT_BAD = dict(n_in_is_not_n_inf=dict(n_in=29), past_the_row=dict(start=11), infer_null=dict(infer=None), speech_2=dict(speech=(1, 2)),
               speech_negative=dict(speech=(-1, 1)), infer_is_out=dict(infer=OUT), infer_in_wave=dict(infer=ctypes.c_void_p((1 << 20) + 64)),
               infer_is_state=dict(infer=STATE), infer_is_fade=dict(infer=FO), infer_on_offsets=dict(infer=ctypes.c_void_p((7 << 20) - 236)),
               slot_twice=dict(slots=(1, 1)), slot_above=dict(slots=(0, 2)), block_zero=dict(block=0, n_in=10), null_out=dict(out=None),
               lds=dict(Lb=8000, Ls=200, block=20, n_in=8220, stride=9000))


@pytest.mark.parametrize("bad", list(OUT_BAD.values()), ids=list(OUT_BAD))
def test_rt_out_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _out(**bad) != 0
    assert b"rt_out" in _lib.lib().svc_last_error()


class _Cfm:
    device = torch.device("cpu")
    in_channels = 4


def test_engine_settings_and_refusals_need_no_gpu():
    from seedvc_amd.pipeline import RealtimeEngine, gate_power
    rs = lambda a, b: types.SimpleNamespace(orig_freq=a, new_freq=b, _h=None)      # noqa: E731
    eng = RealtimeEngine(None, _Cfm(), None, max_streams=3, **RT.FAKE_GEOMETRY)      # block 44, Lb 16, Ls 12
    for bad in (rs(150, 250),                # 20 ms = 3 samples: 44 is not a multiple
                rs(205, 250), rs(200, 260),  # off the 20 ms grid
                rs(400, 300)):               # zc 8: 44 and 12 are not multiples
        with pytest.raises(ValueError, match="attach_output"):
            eng.attach_output(bad)
    with pytest.raises(ValueError, match="attach_output"):
        eng.attach_output(rs(200, 250), fade_in=torch.zeros(20))
    with pytest.raises(ValueError, match="attach_output"):
        eng.attach_output(rs(200, 250), fade_in=torch.zeros(16), fade_out=torch.zeros(16))    # Lb_out is 20
    assert eng._out is None and eng.state.shape == (3, 16)
    eng.state.fill_(1.0)
    eng.attach_output(rs(200, 250))          # zc 4 -> 5
    o = eng._out
    assert (o["zc"], o["block"], o["Lb"], o["Ls"], o["n_inf"]) == (5, 55, 20, 15, 90)
    assert eng.state.shape == (3, 20) and not eng.state.any() and o["fade_in"].shape == (20,)
    assert torch.equal(o["fade_in"], torch.from_numpy(RT.gui_windows(20)[0]))
    out, parts = eng.step([], torch.zeros(0, 5, 6), 10, 0.7, return_parts=True)
    assert out.shape == (0, 55) and parts["infer"].shape == (0, 90)
    pc, mel, style = torch.zeros(1, 5, 6), torch.zeros(1, 4, 5), torch.zeros(1, 3)
    assert eng.open(pc, mel, style) == 0
    with pytest.raises(ValueError, match="streams are open"):
        eng.attach_output(rs(200, 300))
    # speech: True on open and reset, per slot
    assert eng._speech == {0: True}
    eng.set_speech(0, False)
    assert eng._speech[0] is False
    eng.reset(0)
    assert eng._speech[0] is True
    for bad in (1, 3, -1):
        with pytest.raises(ValueError, match="set_speech"):
            eng.set_speech(bad, False)
    # the gate needs attach_audio; off on open, kept across reset, dropped on close
    with pytest.raises(ValueError, match="attach_audio has not been called"):
        eng.set_gate(0, -40.0)
    eng.attach_audio(RA.FakeContent(), rs(22050, 16000), 441, 2560, 0.04)
    a = eng._audio
    assert a["gate_e"].shape == (3, 3) and a["gate_e"].dtype == torch.float32 and not a["gate_e"].any()
    a["gate_e"].fill_(2.0)
    eng.set_gate(0, -40.0)
    assert eng._gate == {0: gate_power(-40.0, 441)} and not a["gate_e"][0].any() and (a["gate_e"][1:] == 2).all()
    a["gate_e"].fill_(2.0)
    eng.set_gate(0, -30.0)                   # a change of an open gate keeps the tracked energies
    assert (a["gate_e"] == 2).all()
    eng.reset(0)
    assert eng._gate == {0: gate_power(-30.0, 441)} and not a["gate_e"][0].any() and (a["gate_e"][1:] == 2).all()
    for off in (None, -60.0, -100):
        eng.set_gate(0, -40.0)
        eng.set_gate(0, off)
        assert eng._gate == {}
    with pytest.raises(ValueError, match="set_gate"):
        eng.set_gate(0, float("nan"))
    with pytest.raises(ValueError, match="set_gate"):
        eng.set_gate(1, -40.0)
    eng.set_gate(0, -40.0)
    eng.close(0)
    assert eng._gate == {} and eng._speech == {}
    assert eng.open(pc, mel, style) == 0 and eng._gate == {} and eng._speech == {0: True}
