"""CPU side of real-time sessions (`svc_sola_step`, `pipeline.realtime_geometry`, `pipeline.RealtimeEngine`): the entry point
is declared, exported and bound; its argument checks come before anything touches a device; the geometry reproduces the
published configuration; and the numpy model the GPU tests compare with equals a transcription of the reference GUI's own
SOLA lines on planted-peak inputs, bit for bit."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import realtime_cases as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
ONE = ctypes.c_void_p(16)                           # never dereferenced: the checks come first


def test_sola_entry_point_is_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    assert "svc_sola_step" in declared, "svc_sola_step is not declared in include/seedvc_hip.h"
    assert "svc_sola_step" in _lib.EXPORTS, "svc_sola_step is not in _lib.EXPORTS"
    assert hasattr(lib, "svc_sola_step"), "svc_sola_step is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert callable(pipeline.realtime_geometry)
    p = inspect.signature(pipeline.RealtimeEngine.__init__).parameters
    assert list(p)[1:] == ["length_regulator", "cfm", "vocoder", "S", "hop", "block", "sola_buffer", "sola_search", "tail",
                           "max_streams", "fade_in", "fade_out"]
    assert p["tail"].default == 0 and p["max_streams"].default == 64 and p["fade_in"].default is None
    p = inspect.signature(pipeline.RealtimeEngine.step).parameters
    assert list(p)[1:] == ["slots", "content", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]


def _sola(stride=100, start=4, slots=(0, 2), max_slots=3, block=40, Lb=16, Ls=8, wave=ONE, state=ONE, fade_in=ONE, fade_out=ONE,
          out=ONE, N=None):
    from seedvc_amd import _lib
    return _lib.lib().svc_sola_step(wave, stride, start, len(slots) if N is None else N, state, max_slots, i32(*slots), fade_in,
                                    fade_out, block, Lb, Ls, out, None, None)


def test_empty_call_touches_nothing():
    assert _sola(slots=(), wave=None, state=None, fade_in=None, fade_out=None, out=None) == 0
    assert _sola(slots=(), max_slots=0, wave=None, state=None, fade_in=None, fade_out=None, out=None) == 0


@pytest.mark.parametrize("bad", [dict(N=-1), dict(stride=-1), dict(start=-1), dict(max_slots=-1), dict(block=0), dict(block=-3),
                                 dict(Lb=0), dict(Ls=-1), dict(start=37), dict(stride=67), dict(slots=(0, 3)), dict(slots=(-1, 0)),
                                 dict(slots=(2, 0, 2)), dict(slots=(1, 1)), dict(wave=None), dict(state=None), dict(fade_in=None),
                                 dict(fade_out=None), dict(out=None), dict(Lb=8000, Ls=200, stride=20000)],
                         ids=["N_negative", "stride_negative", "start_negative", "max_slots_negative", "block_zero",
                              "block_negative", "Lb_zero", "Ls_negative", "start_past_the_row", "stride_below_the_window",
                              "slot_above", "slot_negative", "slot_twice", "slot_twice_adjacent", "null_wave", "null_state",
                              "null_fade_in", "null_fade_out", "null_out", "above_the_lds_limit"])
def test_sola_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _sola(**bad) != 0
    assert b"sola_step" in _lib.lib().svc_last_error()


def test_a_rejected_empty_call_is_still_rejected():
    """N == 0 excuses the pointers, not the sizes."""
    assert _sola(slots=(), block=0, wave=None, state=None, fade_in=None, fade_out=None, out=None) != 0
    assert _sola(slots=(), start=37, wave=None, state=None, fade_in=None, fade_out=None, out=None) != 0


# ------------------------------------------------------------------------------------------------------------- geometry
def test_geometry_of_the_published_configuration():
    from seedvc_amd.pipeline import realtime_geometry
    g = realtime_geometry(22050, 256, 0.18, 0.04, 2.5, 0.02, 2.0)
    assert g == dict(S=65, block=3969, Lb=882, Ls=441, tail=441, start=10907, n_inf=5292, skip_head=125, skip_tail=1,
                     return_length=12)
    assert g["start"] == g["S"] * 256 - g["tail"] - g["n_inf"] and g["n_inf"] == g["block"] + g["Lb"] + g["Ls"]
    g = realtime_geometry(22050, 256, 0.25, 0.25, 2.5, 0.02, 2.0)              # a long crossfade is capped at 4 * zc
    assert g["Lb"] == 4 * 441 and g["block"] == 12 * 441                       # 0.25 s = 12.5 units, rounded half to even


def test_geometry_raises_where_the_step_is_too_short():
    from seedvc_amd.pipeline import realtime_geometry
    with pytest.raises(ValueError, match="realtime_geometry"):
        realtime_geometry(22050, 256, 0.18, 0.04, 0.5, 0.02, 2.0)              # skip_head 25 units < the 100 the DiT drops
    with pytest.raises(ValueError, match="realtime_geometry"):
        realtime_geometry(22050, 256, 0.18, 0.04, 2.5, 0.02, 2.8)


def test_engine_refusals_need_no_gpu():
    from seedvc_amd.pipeline import RealtimeEngine

    class _Cfm:
        device = torch.device("cpu")
        in_channels = 4
    mk = lambda **kw: RealtimeEngine(None, _Cfm(), None, **{**RT.FAKE_GEOMETRY, **kw})      # noqa: E731
    for bad in (dict(block=0), dict(sola_buffer=0), dict(sola_search=-1), dict(tail=-1), dict(tail=25), dict(max_streams=0),
                dict(fade_in=np.ones(16, np.float32)), dict(fade_in=np.ones(15, np.float32), fade_out=np.ones(15, np.float32))):
        with pytest.raises(ValueError, match="RealtimeEngine"):
            mk(**bad)
    eng = mk(max_streams=2)
    assert (eng.start, eng.n_inf) == (16, 72) and eng.state.shape == (2, 16)
    pc, mel, style = torch.zeros(1, 5, 6), torch.zeros(1, 4, 5), torch.zeros(1, 3)
    with pytest.raises(ValueError, match="open"):
        eng.open(pc, torch.zeros(1, 4, 6), style)                              # prompt frames disagree
    assert [eng.open(pc, mel, style), eng.open(pc, mel, style)] == [0, 1]
    with pytest.raises(ValueError, match="in use"):
        eng.open(pc, mel, style)
    eng.close(0)
    assert eng.open(pc, mel, style) == 0                                       # the lowest free slot
    eng.close(1)
    x = torch.zeros(2, 12, 6)
    for slots in ([0, 0], [0, 1], [0, 2], [-1, 0]):                            # twice / closed / out of range
        with pytest.raises(ValueError, match="step"):
            eng.step(slots, x, 10, 0.7)
    with pytest.raises(ValueError, match="content"):
        eng.step([0], x, 10, 0.7)
    with pytest.raises(ValueError):
        eng.close(1)
    with pytest.raises(ValueError):
        eng.reset(1)


# ----------------------------------------------------------------------------- the model the GPU tests are compared with
PLANTED = [("gui", 3969, 882, 441, 137, 1.0), ("gui_end", 3969, 882, 441, 441, 0.5), ("short_block", 8, 32, 10, 6, 2.0),
           ("equal", 32, 32, 7, 0, 1.0), ("no_search", 40, 16, 0, 0, 1.0), ("x4", 64, 16, 12, 12, 0.25)]


@pytest.mark.parametrize("name,block,Lb,Ls,offset,gain", PLANTED, ids=[p[0] for p in PLANTED])
def test_sola_model_equals_the_gui_lines(name, block, Lb, Ls, offset, gain):
    infer, buf = RT.planted_input("rt.planted." + name, 151, block, Lb, Ls, offset, gain)
    fi, fo = RT.gui_windows(Lb)
    out, new, o, scores = RT.sola_model(infer, buf, fi, fo, block, Ls)
    if Ls > 0:      # the test's own inputs: a wide gap, so that fp32 and float64 scores agree on the winner
        assert RT.score_gap(scores) >= 1e-2 * np.linalg.norm(buf.astype(np.float64))
    assert o == offset
    t_out, t_new, t_o = RT.gui_sola_torch(*(torch.from_numpy(a) for a in (infer, buf, fi, fo)), block, Ls)
    assert t_o == o
    assert np.array_equal(t_out.numpy(), out) and np.array_equal(t_new.numpy(), new)
    if block < Lb:  # the new buffer starts inside the faded region
        assert not np.array_equal(new[:Lb - block], infer[o + block:o + Lb])


def test_sola_model_zero_buffer_and_given_offset():
    infer, _ = RT.planted_input("rt.zero", 152, 40, 16, 8, 3)
    fi, fo = RT.gui_windows(16)
    out, new, o, scores = RT.sola_model(infer, np.zeros(16, np.float32), fi, fo, 40, 8)
    assert o == 0 and not scores.any()
    assert np.array_equal(out[16:], infer[16:40]) and np.array_equal(new, infer[40:56])
    assert np.array_equal(out[:16], infer[:16] * fi + np.zeros(16, np.float32) * fo)
    out5, new5, o5, _ = RT.sola_model(infer, np.zeros(16, np.float32), fi, fo, 40, 8, offset=5)
    assert o5 == 5 and np.array_equal(new5, infer[45:61])


def test_planted_sessions_follow_their_offsets():
    """The exact stand-in chain in numpy: every step after the first finds its buffer again at the planted offset, with the
    score gap the GPU test relies on."""
    fi, fo = RT.gui_windows(RT.FAKE_GEOMETRY["sola_buffer"])
    for stream in range(3):
        steps = RT.session_model(RT.planted_session(stream), fi, fo)
        assert [s[2] for s in steps] == RT.FAKE_OFFSETS[stream]
        assert not steps[0][4].any()
        for out, new, o, scores, before in steps[1:]:
            nb = np.linalg.norm(before.astype(np.float64))
            assert RT.score_gap(scores) >= 1e-2 * nb and abs(scores[o] - nb) < 1e-6 * nb
