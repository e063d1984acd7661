"""CPU side of audio-in real-time sessions (`svc_rt_push`, `pipeline.realtime_input_geometry`, `RealtimeEngine.attach_audio` /
`step_audio`): the numpy push model the GPU tests compare with equals a transcription of the reference GUI's own lines; pushing
a stream block by block gives the one-shot conversion of the whole stream wherever a sample's taps lay inside the audio received
(the phase-alignment argument of DESIGN.md 8l); the geometry reproduces the published configuration; the entry points are
declared, exported and bound, and their argument checks come before anything touches a device."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import realtime_cases as RT
import resample_cases as RC
import rt_audio_cases as RA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
REAL_PAIRS = [(22050, 16000), (44100, 16000), (48000, 16000)]


# ------------------------------------------------------------------------------------------------------------ push model
@pytest.mark.parametrize("pair,m", [((22050, 16000), 9), ((22050, 16000), 1), ((48000, 16000), 2), ((250, 150), 3)],
                         ids=["22050_m9", "22050_m1", "48000_m2", "250_m3"])
def test_push_model_equals_the_gui_lines(pair, m):
    """Six consecutive blocks.  Before every block the model is given the GUI's own state (the last 2 zc samples of `input_wav`,
    `input_wav_res`); after it the kept samples are equal, the new ones within `fp32_bound` of the GUI's float32 conv1d (the
    textbook bound holds for any summation order), and the history is the end of the GUI's ring."""
    orig, new = pair
    zc, z16, o, n = RA.units(orig, new)
    Lin, total = m * zc, (m + 14) * zc                          # the GUI's ring: extra context + crossfade + search + block + right
    L16 = z16 * total // zc
    n_new = (m + 1) * z16
    input_wav, input_wav_res = torch.zeros(total), torch.zeros(L16)
    for k in range(6):
        indata = RC.noise(f"rt_audio.gui.{orig}.{m}", k, Lin)
        hist, ring = input_wav[-2 * zc:].numpy().copy(), input_wav_res.numpy().copy()
        RA.gui_push_torch(input_wav, input_wav_res, indata, orig, new)
        c, h = RA.push_model(hist, ring, indata.numpy(), orig, new, zc, z16)
        got = input_wav_res.numpy()
        assert c.dtype == np.float64 and h.dtype == np.float32
        assert np.array_equal(c[:L16 - n_new], got[:L16 - n_new]), k                        # float32 values, exactly
        bound = RA.push_bound(hist, np.zeros(L16), indata.numpy(), orig, new, zc, z16)[L16 - n_new:]
        err = np.abs(c[L16 - n_new:] - got[L16 - n_new:])
        print(f"{orig} -> {new}, m = {m}, block {k}: max |model - GUI| over the new samples {err.max():.3e}, bound there "
              f"{bound[err.argmax()]:.3e}")
        assert (err <= bound).all(), k
        assert np.array_equal(h, input_wav[-2 * zc:].numpy()), k
        assert got[L16 - n_new:].any()


def test_fp32_emulation_is_inside_the_bound_of_the_float64_model():
    """`push_model_fp32` (the device's FMA chain in numpy) against `push_model`: the same push, within `fp32_bound`; and its
    `fma32` is a correctly rounded fused multiply-add."""
    orig, new = 22050, 16000
    zc, z16, _, _ = RA.units(orig, new)
    hist, ring, block = (RC.noise("rt_audio.emul." + t, 3, k).numpy() for t, k in (("h", 2 * zc), ("r", 6 * z16), ("b", 2 * zc)))
    c64, h64 = RA.push_model(hist, ring, block, orig, new, zc, z16)
    c32, h32 = RA.push_model_fp32(hist, ring, block, orig, new, zc, z16)
    bound = RA.push_bound(hist, np.zeros(6 * z16), block, orig, new, zc, z16)
    assert c32.dtype == np.float32 and np.array_equal(h32, h64)
    assert (np.abs(c32 - c64) <= bound).all() and np.array_equal(c32[:3 * z16], ring[2 * z16:5 * z16])
    assert np.abs(c32 - c64).max() > 0                           # it is fp32 arithmetic, not the float64 sum rounded
    # `fma32` rounds once: cases where float32(float64(a * b + c)) is wrong, because the double sum lands on a float32 tie and the
    # bits it lost decide
    f = np.float32
    ulp = 2.0 ** -23                                             # of 1.0; 1 + ulp / 2 is half way between 1 and 1 + ulp
    p, q = f(2.0 ** -12 + 2.0 ** -30), f(2.0 ** -12 - 2.0 ** -30)    # p q = 2^-24 - 2^-60 exactly: just short of ulp / 2
    a = np.array([p, -p, f(2.0 ** -12), f(1.0)], f)
    b = np.array([q, q, f(2.0 ** -12), f(1.0)], f)
    c = np.array([1 + ulp, 1 + ulp, 1 + ulp, 0.5], f)
    # 1 + 3/2 ulp - 2^-60: below the tie -> 1 + ulp | 1 + ulp / 2 + 2^-60: above the tie -> 1 + ulp | the tie itself: even,
    # 1 + 2 ulp | 1.5
    want = [1 + ulp, 1 + ulp, 1 + 2 * ulp, 1.5]
    assert RA.fma32(a, b, c).tolist() == want
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f).tolist()
    assert twice == [1 + 2 * ulp, 1.0, 1 + 2 * ulp, 1.5]         # float64 cannot hold the 2^-60: rounding twice gets two wrong


# -------------------------------------------------------------------------------------------------------- phase alignment
@pytest.mark.parametrize("pair", REAL_PAIRS, ids=[str(p[0]) for p in REAL_PAIRS])
def test_streamed_model_equals_the_one_shot_conversion(pair):
    """o divides zc, so every block starts at resampling phase 0 and a context sample is the one-shot sample of the whole stream
    wherever all of its taps lay inside the audio received when it was computed last.  After every one of 7 pushes of one long
    signal: equal at the supported positions -- to the rounding of the two float64 sums, (ntaps + 2) 2^-53 sum |K| |x| =
    fp32_bound 2^-29: the same non-zero terms, but conv1d is free to add them in another order for another length -- and the
    excluded samples are at most the last ceil((width + 1) n / o) + 1 of the context."""
    orig, new = pair
    zc, z16, o, n = RA.units(orig, new)
    o_, n_, width, first, taps = RA.taps_of(orig, new)
    assert (o_, n_) == (o, n) and zc % o == 0 and z16 % n == 0 and zc * n == z16 * o and width <= zc
    m, pushes = 2, 7
    Lin, L16 = m * zc, 10 * z16
    cap = RA.excluded_cap(orig, new)
    signal = RC.noise(f"rt_audio.stream.{orig}", 5, (pushes + 1) * Lin)         # one block more than is ever pushed
    Y = RC.resample_dense(orig, new, signal[None])[0].numpy()
    tol = RC.fp32_bound(orig, new, signal[None], taps.shape[1])[0].numpy() * 2.0 ** -29
    hist, ring = np.zeros(2 * zc, np.float32), np.zeros(L16)
    for b in range(pushes):
        ring, hist = RA.push_model(hist, ring, signal[b * Lin:(b + 1) * Lin].numpy(), orig, new, zc, z16)
        M, ok = RA.supported(orig, new, Lin, L16, b + 1)
        live = M >= 0
        assert not ring[M < -cap].any()                # before the stream began: the empty context (and the filter's pre-ringing)
        assert (np.abs(ring[ok] - Y[M[ok]]) <= tol[M[ok]]).all(), b
        excluded = np.flatnonzero(live & ~ok)
        assert len(excluded) <= cap and (len(excluded) == 0 or excluded.min() >= L16 - cap), (b, len(excluded), cap)
        assert len(excluded) > 0 and (ring[excluded] != Y[M[excluded]]).any()  # the rule is not vacuous: the next block is missing
        assert ok.sum() == live.sum() - len(excluded) and ok.sum() >= min(L16, (b + 1) * m * z16) - cap


# ---------------------------------------------------------------------------------------------------------------- geometry
def test_input_geometry_of_the_published_configuration():
    from seedvc_amd.pipeline import realtime_geometry, realtime_input_geometry
    g = realtime_input_geometry(22050, 0.18, 0.04, 2.5, 0.02)
    # input_wav: 125 + 2 + 1 + 9 + 1 = 138 units of 441 samples
    assert g == dict(zc=441, z16=320, Lin=3969, L16=138 * 320, hist=882, rows=137)
    assert g["L16"] % 320 == 0
    assert g["Lin"] == realtime_geometry(22050, 256, 0.18, 0.04, 2.5, 0.02, 2.0)["block"]
    import w2v_cases as W
    assert W.frames(W.CFG_F, g["L16"]) == g["rows"]                            # what the XLS-R extractor yields for the context
    g48 = realtime_input_geometry(48000, 0.5, 0.04, 2.5, 0.02)
    assert (g48["zc"], g48["Lin"], g48["L16"]) == (960, 24000, 320 * (125 + 2 + 1 + 25 + 1))


def test_input_geometry_refuses_rates_off_the_20_ms_grid():
    from seedvc_amd.pipeline import realtime_input_geometry
    with pytest.raises(ValueError, match="realtime_input_geometry"):
        realtime_input_geometry(11025, 0.18, 0.04, 2.5, 0.02)
    with pytest.raises(ValueError, match="realtime_input_geometry"):
        realtime_input_geometry(22050, 0.18, 0.04, 2.5, 0.02, content_rate=16010)


# ------------------------------------------------------------------------------------------------------- ABI and refusals
def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in ("svc_rt_push", "svc_rt_push_tiles", "svc_rt_ring_floats"):
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    sig = lambda f: list(inspect.signature(f).parameters)                              # noqa: E731
    assert sig(pipeline.realtime_input_geometry) == ["sr", "block_time", "crossfade_time", "extra_time_ce", "extra_time_right",
                                                     "content_rate"]
    E = pipeline.RealtimeEngine
    assert sig(E.attach_audio) == ["self", "content", "resample", "Lin", "L16", "ce_dit_difference"]
    assert sig(E.step_audio) == ["self", "slots", "audio", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.step_audio_seeded) == ["self", "slots", "audio", "n_timesteps", "inference_cfg_rate", "seeds", "vocoder_kwargs",
                                        "return_parts"]
    # existing signatures stay
    assert sig(E.step) == ["self", "slots", "content", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.open) == ["self", "prompt_condition", "mel2", "style2"] and sig(E.reset) == ["self", "slot"]
    L = _lib.lib()
    assert L.svc_rt_ring_floats(70, 1000) == 2 * 70 * 1001 and L.svc_rt_ring_floats(0, 5) == 0
    assert L.svc_rt_push_tiles(1) == 2 and L.svc_rt_push_tiles(2048) == 2 and L.svc_rt_push_tiles(2049) == 3


# fake, never dereferenced addresses of four disjoint buffers: the checks come first
BLOCK, HIST, RING, CTX = (ctypes.c_void_p(a) for a in (1 << 20, 2 << 20, 3 << 20, 8 << 20))


def _push(r=None, block=BLOCK, stride=45, Lin=45, slots=(0, 2), max_slots=3, zc=5, z16=5, hist=HIST, ring=RING, L16=200, ctx=CTX,
          N=None):
    """Equal rates (r = NULL, o = n = 1) unless a handle is given."""
    from seedvc_amd import _lib
    return _lib.lib().svc_rt_push(r, block, stride, Lin, len(slots) if N is None else N, i32(*slots), max_slots, zc, z16, hist, ring,
                                  L16, ctx, None)


BAD = dict(Lin_zero=dict(Lin=0), Lin_negative=dict(Lin=-5), Lin_off_the_grid=dict(Lin=44), Lin_below_zc=dict(Lin=3),
           L16_below_n_new=dict(L16=49), x_too_short=dict(z16=6, L16=400), N_zero=dict(slots=()), N_65=dict(slots=tuple(range(65)), max_slots=70),
           N_negative=dict(N=-1), slot_above=dict(slots=(0, 3)), slot_negative=dict(slots=(-1, 0)), slot_twice=dict(slots=(2, 0, 2)),
           stride_below_Lin=dict(stride=44), null_block=dict(block=None), null_hist=dict(hist=None), null_ring=dict(ring=None),
           null_ctx=dict(ctx=None), hist_in_ring=dict(hist=ctypes.c_void_p((3 << 20) + 64)),
           ctx_in_ring=dict(ctx=ctypes.c_void_p((3 << 20) + 4 * 2 * 3 * 200)),            # on the tickets behind the planes
           block_in_ctx=dict(block=ctypes.c_void_p((8 << 20) + 4 * 399)), ctx_is_hist=dict(ctx=HIST),
           ring_off_8_bytes=dict(ring=ctypes.c_void_p((3 << 20) + 4)), zc_zero=dict(zc=0), max_slots_zero=dict(max_slots=0, slots=(0,)))


@pytest.mark.parametrize("bad", list(BAD.values()), ids=list(BAD))
def test_push_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _push(**bad) != 0
    assert b"rt_push" in _lib.lib().svc_last_error()


class _Cfm:
    device = torch.device("cpu")
    in_channels = 4


def _engine(**kw):
    from seedvc_amd.pipeline import RealtimeEngine
    return RealtimeEngine(None, _Cfm(), None, **{**RT.FAKE_GEOMETRY, **kw})


def test_engine_refusals_need_no_gpu():
    content = RA.FakeContent()
    resample = types.SimpleNamespace(orig_freq=22050, new_freq=16000, _h=None)
    eng = _engine(max_streams=3)
    pc, mel, style = torch.zeros(1, 5, 6), torch.zeros(1, 4, 5), torch.zeros(1, 3)
    assert [eng.open(pc, mel, style), eng.open(pc, mel, style)] == [0, 1]
    with pytest.raises(ValueError, match="attach_audio has not been called"):
        eng.step_audio([0], torch.zeros(1, 441), 10, 0.7)                      # stepping before attach_audio
    for bad in (dict(Lin=440), dict(Lin=0), dict(Lin=-441), dict(L16=639), dict(ce_dit_difference=-1.0), dict(content=object()),
                dict(resample=types.SimpleNamespace(orig_freq=11025, new_freq=16000, _h=None))):
        with pytest.raises(ValueError, match="attach_audio"):
            eng.attach_audio(**{**dict(content=content, resample=resample, Lin=441, L16=2560, ce_dit_difference=0.04), **bad})
    with pytest.raises(ValueError, match="attach_audio has not been called"):
        eng.step_audio([0], torch.zeros(1, 441), 10, 0.7)                      # a refused attach leaves the engine as it was
    eng.attach_audio(content, resample, 441, 2560, 0.04)
    a = eng._audio
    assert a["hist"].shape == (3, 882) and a["planes"].shape == (2, 3, 2560) and a["tickets"].shape == (3,) and a["ce"] == 2
    assert not a["ring"].any() and not a["hist"].any() and a["tickets"].dtype == torch.int64
    for slots, audio in (([0, 0], torch.zeros(2, 441)),                        # a slot twice
                         ([0, 2], torch.zeros(2, 441)),                        # a slot that is not open
                         ([0, 1], torch.zeros(2, 440)), ([0, 1], torch.zeros(1, 441)), ([0], torch.zeros(441)), ([], torch.zeros(0, 441))):
        with pytest.raises(ValueError, match="step_audio"):
            eng.step_audio(slots, audio, 10, 0.7)
    with pytest.raises(ValueError, match="seeds is None"):
        eng.step_audio_seeded([0], torch.zeros(1, 441), 10, 0.7, None)
    # open and reset zero a slot's rows of both planes and of the history, and nothing else
    a["planes"].fill_(1.0)
    a["hist"].fill_(2.0)
    eng.reset(1)
    assert not a["planes"][:, 1].any() and not a["hist"][1].any()
    assert (a["planes"][:, [0, 2]] == 1).all() and (a["hist"][[0, 2]] == 2).all()
    assert eng.open(pc, mel, style) == 2
    assert not a["planes"][:, 2].any() and not a["hist"][2].any() and (a["planes"][:, 0] == 1).all()
