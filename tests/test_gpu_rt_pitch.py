"""GPU side of the streams' pitch step (`svc_rt_pitch`, csrc/rt_pitch.hip) against the yardstick of
rt_pitch_cases.py: every state word against the exact-integer statement call by call, the output against the float64
statement within the fp32 bound of the chain, auto off against `svc_f0_adjust` bit for bit, the settled shift against the
offline medians within half a bin, the glide, isolation from the batch, refusals that touch nothing, and the engine:
`step_audio` with pitch attached against the same steps made by hand.

max_slots = 64, Tf = 48, n_new = 4, lag = 2 unless a test says otherwise."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import cases
import resample_cases as RC
import rmvpe_cases as R
import rt_audio_cases as RA
import rt_pitch_cases as PC
import w2v_cases as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
MS, TF, NN, LAG = PC.MAX_SLOTS, PC.TF, PC.N_NEW, PC.LAG
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)      # noqa: E731


def _call(rows, slots, state, ref, auto, semis, warmup=PC.WARMUP, max_step=PC.MAX_STEP, n_new=NN, lag=LAG):
    """One `rt_pitch` call on numpy rows -> (out numpy (N, Tf), shift numpy (N,))."""
    from seedvc_amd.rmvpe import rt_pitch
    out, shift = rt_pitch(torch.from_numpy(np.ascontiguousarray(rows, np.float32)).to(DEV), n_new, lag, slots, state, ref, auto, semis,
                          warmup=warmup, max_step=max_step, return_shift=True)
    return out.cpu().numpy(), shift.cpu().numpy()


def _fresh(ref_by_slot=None):
    from seedvc_amd.rmvpe import rt_pitch_state
    state = rt_pitch_state(MS, DEV)
    ref = torch.zeros(MS, device=DEV)
    for s, v in (ref_by_slot or {}).items():
        ref[s] = v
    return state, ref


def _check_call(name, c, words_before, row, dev_words, dev_out, dev_shift, ref, auto, semis, warmup, max_step, worst):
    """One stream of one call against the statement, the state before the call taken as exact."""
    m = PC.step_model(words_before, row, NN, LAG, ref, auto, semis, warmup, max_step)
    keep = np.ones(PC.WORDS, bool)
    keep[PC.W_SHIFT] = False
    assert np.array_equal(dev_words[keep], m["words"][keep]), (name, c, np.flatnonzero(dev_words != m["words"]))
    s_dev = float(dev_words[PC.W_SHIFT:PC.W_SHIFT + 1].view(np.float32)[0])
    assert s_dev == float(dev_shift), (name, c)
    if m["limited"] or m["shift"] == 0.0:                   # a glide step is one exact fp32 sum, a zero target is +0.0
        assert dev_words[PC.W_SHIFT] == m["words"][PC.W_SHIFT], (name, c, s_dev, m["shift"])
    else:
        assert abs(s_dev - m["shift"]) <= PC.SHIFT_ATOL, (name, c, s_dev, m["shift"])
    err = PC.rel_err(dev_out, PC.output_model(row, s_dev, semis))
    worst[0] = max(worst[0], err)
    assert err <= PC.OUT_RTOL, (name, c, err)
    return m


# ---------------------------------------------------------------------------------------------- 1, 2: state and output
def test_state_words_and_output_of_the_planted_streams():
    """Six consecutive calls on the three planted streams (slots 5, 63, 0 in one call): after every call every integer word
    equals the statement, word 1537 equals it exactly on glide steps and within one log rounding on arrival, and every output
    frame is within 2e-6 of the float64 statement."""
    names, slots = ["A", "B", "C"], [5, 63, 0]
    S = [PC.STREAMS[n] for n in names]
    state, ref = _fresh({s: st["ref"] for s, st in zip(slots, S)})
    rows = np.stack([PC.stream_rows(n) for n in names])                          # (3, calls, Tf)
    before = np.zeros((3, PC.WORDS), np.int32)
    worst, arrived = [0.0], 0
    for c in range(PC.N_CALLS):
        out, shift = _call(rows[:, c], slots, state, ref, [st["auto"] for st in S], [st["semis"] for st in S])
        words = state.cpu().numpy()
        for k, (n, st) in enumerate(zip(names, S)):
            m = _check_call(n, c, before[k], rows[k, c], words[slots[k]], out[k], shift[k], np.float32(st["ref"]), st["auto"],
                            st["semis"], PC.WARMUP, PC.MAX_STEP, worst)
            arrived += (not m["limited"]) and m["shift"] != 0.0
            before[k] = words[slots[k]]
        others = np.delete(words, slots, axis=0)
        assert not others.any(), c                                               # unlisted slots keep every bit
    print(f"max relative error of the output against float64: {worst[0]:.3e} (cap {PC.OUT_RTOL:.1e})")
    assert arrived >= 3
    assert int(before[1][PC.W_N]) == 11 and int(before[0][PC.W_N]) == 19 and int(before[2][PC.W_N]) == 13


# ---------------------------------------------------------------------------------------------------------- 3: auto off
@pytest.mark.parametrize("semis", [0.0, -12.0, 7.0, 0.37])
def test_auto_off_is_f0_adjust_without_the_median_shift_bit_for_bit(semis):
    from seedvc_amd.rmvpe import f0_adjust
    rows = np.stack([PC.stream_rows(n)[2] for n in ("A", "B", "C")])
    state, ref = _fresh({1: 5.0, 2: 5.5, 3: 6.0})
    out, shift = _call(rows, [1, 2, 3], state, ref, [0, 0, 0], [semis] * 3, warmup=0)
    t = torch.from_numpy(rows).to(DEV)
    want = f0_adjust(t, [TF] * 3, t, [TF] * 3, auto_f0_adjust=False, pitch_shift=semis).cpu().numpy()
    assert np.array_equal(bits(out), bits(want)) and not shift.any()
    assert np.isnan(out[0]).sum() == np.isnan(rows[0]).sum()


# --------------------------------------------------------------------------------------------------- 4: offline cross-check
def test_a_history_that_fits_one_call_settles_where_the_offline_step_does():
    """n_new = Tf - lag, the step off, warmup 0: the applied shift is within half a bin (plus the chain's 2e-6) of
    `svc_f0_adjust`'s m_ori - m_alt over the same frames."""
    from seedvc_amd.rmvpe import f0_adjust
    g = np.random.default_rng(77)
    n = TF - LAG
    src = (90.0 * 2.0 ** g.uniform(0, 3, (4, TF))).astype(np.float32)
    src[g.random((4, TF)) < 0.3] = 0.0
    src[3, :n] = 0.0
    src[3, 7] = 523.25                                                           # a single voiced frame
    tgt = (300.0 * 2.0 ** g.uniform(0, 2, (4, 60))).astype(np.float32)
    tgt[g.random((4, 60)) < 0.2] = 0.0
    a, o = torch.from_numpy(src).to(DEV), torch.from_numpy(tgt).to(DEV)
    _, med = f0_adjust(a, [n] * 4, o, [60] * 4, return_medians=True)
    state, ref = _fresh()
    slots = [9, 8, 40, 2]
    ref[slots] = med[:, 1]
    _, shift = _call(src, slots, state, ref, [1] * 4, None, warmup=0, max_step=0.0, n_new=n)
    med = med.cpu().numpy().astype(np.float64)
    err = np.abs(shift - (med[:, 1] - med[:, 0]))
    print("applied shift - (m_ori - m_alt):", err)
    assert (err <= PC.HALF_BIN + PC.OUT_RTOL).all() and (np.abs(shift) > 0.01).all()
    voiced = (src[:, :n] > 1).sum(1)
    assert state[slots, PC.W_N].cpu().tolist() == voiced.tolist()


# ------------------------------------------------------------------------------------------------------------ 5: the glide
def test_the_shift_glides_arrives_exactly_and_glides_back():
    G = PC.GLIDE
    state, ref = _fresh({3: G["ref"]})
    row = PC.glide_rows(1)
    shifts = [float(_call(row, [3], state, ref, [1], None, warmup=0, max_step=G["max_step"])[1][0]) for _ in range(4)]
    model = [r["shift"] for r in PC.run_glide()]
    assert shifts[:2] == [0.25, 0.5] == model[:2]
    assert abs(shifts[2] - model[2]) <= PC.SHIFT_ATOL and shifts[3] == shifts[2] and 0.5 < shifts[2] < 0.75      # no overshoot
    d = shifts[2]
    back = [float(_call(row, [3], state, ref, [0], None, warmup=0, max_step=G["max_step"])[1][0]) for _ in range(4)]
    assert back[0] == float(np.float32(d) - np.float32(0.25)) and back[1] == float(np.float32(back[0]) - np.float32(0.25))
    assert back[2] == 0.0 and back[3] == 0.0 and back[1] > 0.0
    # max_step = 0: at once, there and back
    assert float(_call(row, [3], state, ref, [1], None, warmup=0, max_step=0.0)[1][0]) == d
    out, s = _call(row, [3], state, ref, [0], None, warmup=0, max_step=0.0)
    assert float(s[0]) == 0.0 and int(state[3, PC.W_N]) == 10 * NN
    assert np.array_equal(bits(out), bits(_call(row, [4], state, ref, [0], None, warmup=0, max_step=0.0)[0]))


def test_a_reference_without_a_voiced_frame_gives_no_automatic_shift():
    """`svc_f0_adjust`'s median of an unvoiced reference is 0.0, written to ref_median on the device as `set_reference_f0` does:
    the stream gets no shift (as offline, where a side without a voiced frame means none), its twin with a voiced reference
    does; so do a negative and a NaN median."""
    from seedvc_amd.rmvpe import f0_adjust
    ref_tracks = torch.zeros(2, 30, device=DEV)
    ref_tracks[0, ::3] = 0.7                                                     # below the voicing threshold
    ref_tracks[1, 4:20] = 330.0
    _, med = f0_adjust(ref_tracks, [30, 30], ref_tracks, [30, 30], auto_f0_adjust=False, return_medians=True)
    state, ref = _fresh({20: -1.0, 21: float("nan")})
    ref[10:12] = med[:, 1]
    rows = PC.glide_rows(1).repeat(4, 0)
    for _ in range(2):
        out, shift = _call(rows, [10, 11, 20, 21], state, ref, [1] * 4, None, warmup=0, max_step=0.0)
    assert float(med[0, 1]) == 0.0 and float(med[1, 1]) > 5.0
    assert bits(shift)[[0, 2, 3]].tolist() == [0, 0, 0] and abs(float(shift[1]) - np.log(330.0 / 220.0)) <= PC.HALF_BIN + PC.OUT_RTOL
    assert np.array_equal(bits(out[0]), bits(out[2])) and np.array_equal(bits(out[0]), bits(out[3]))
    assert PC.rel_err(out[0], PC.output_model(rows[0], 0.0, 0.0)) <= PC.OUT_RTOL
    assert state[[10, 11, 20, 21], PC.W_N].cpu().tolist() == [2 * NN] * 4


# ------------------------------------------------------------------------------------------------------------ 6: isolation
def test_a_stream_does_not_see_its_batch():
    """Stream B run alone in slot 7 (N = 1), and as row 40 of a call of 64 streams in slot 33: the same state bits and output
    bits call by call; the rows of unlisted slots, filled with a sentinel, keep every bit."""
    from seedvc_amd.rmvpe import rt_pitch_state
    st = PC.STREAMS["B"]
    rows = PC.stream_rows("B")
    g = np.random.default_rng(12)
    sent = PC.sentinel_state()
    alone = torch.from_numpy(sent.copy()).to(DEV)
    alone[7].zero_()
    crowd = rt_pitch_state(MS, DEV)
    ref_a = torch.full((MS,), 5.0, device=DEV)
    ref_a[7] = st["ref"]
    ref_c = torch.from_numpy(g.uniform(4.5, 6.0, MS).astype(np.float32)).to(DEV)
    ref_c[33] = st["ref"]
    order = [int(v) for v in g.permutation(MS)]
    order.remove(33)
    order.insert(40, 33)
    for c in range(PC.N_CALLS):
        out1, s1 = _call(rows[c:c + 1], [7], alone, ref_a, [st["auto"]], [st["semis"]])
        batch = (100.0 * 2.0 ** g.uniform(0, 3, (MS, TF))).astype(np.float32)
        batch[40] = rows[c]
        auto, semis = [int(v) for v in g.integers(0, 2, MS)], [float(v) for v in g.uniform(-12, 12, MS)]
        auto[40], semis[40] = st["auto"], st["semis"]
        out64, s64 = _call(batch, order, crowd, ref_c, auto, semis)
        assert np.array_equal(bits(out1[0]), bits(out64[40])) and bits(s1)[0] == bits(s64)[40], c
        assert torch.equal(alone[7], crowd[33]), c
    a = alone.cpu().numpy()
    assert np.array_equal(np.delete(a, 7, axis=0), np.delete(sent, 7, axis=0))
    assert a[7][PC.W_N] == 11 and a[7][:PC.BINS].sum() == 11


# ------------------------------------------------------------------------------------------------------------- 7: refusals
def test_every_refusal_leaves_the_state_untouched():
    from seedvc_amd import _lib
    sent = PC.sentinel_state()
    state = torch.from_numpy(sent.copy()).to(DEV)
    ref = torch.full((MS,), 5.0, device=DEV)
    f0 = torch.full((2, TF), 220.0, device=DEV)
    out0 = np.full((2, TF), 7.0, np.float32)
    out = torch.from_numpy(out0.copy()).to(DEV)
    wide = torch.zeros(65, TF, device=DEV)
    i32, f32 = _lib.i32_host, lambda v: (ctypes.c_float * len(v))(*v)      # noqa: E731
    good = dict(f0=f0, stride=TF, Tf=TF, n_new=NN, lag=LAG, slots=[4, 1], max_slots=MS, state=state, ref=ref, auto=[1, 0],
                semis=[0.0, 1.0], warmup=3, max_step=0.1, out=out, out_stride=TF)
    bad = dict(n_new_zero=dict(n_new=0), lag_negative=dict(lag=-1), window_before_the_row=dict(n_new=44, lag=5), N_zero=dict(slots=[]),
               N_65=dict(f0=wide, out=wide.clone(), slots=list(range(65)), auto=[0] * 65, semis=[0.0] * 65, max_slots=70),
               slot_above=dict(slots=[0, MS]), slot_negative=dict(slots=[-1, 0]), slot_twice=dict(slots=[1, 1]),
               stride_below_Tf=dict(stride=TF - 1), out_stride_below_Tf=dict(out_stride=TF - 1), warmup_negative=dict(warmup=-1),
               max_step_nan=dict(max_step=float("nan")), semis_inf=dict(semis=[float("-inf"), 0.0]), null_f0=dict(f0=None),
               null_state=dict(state=None), null_ref=dict(ref=None), null_out=dict(out=None), out_is_f0=dict(out=f0),
               out_in_state=dict(out=state.view(torch.float32)[10]), state_in_out=dict(state=out.view(torch.int32)))

    def run(a):
        n = len(a["slots"])
        return _lib.lib().svc_rt_pitch(_lib.ptr(a["f0"]), a["stride"], a["Tf"], a["n_new"], a["lag"], n, i32(a["slots"]), a["max_slots"],
                                       _lib.ptr(a["state"]), _lib.ptr(a["ref"]), i32(a["auto"][:max(n, 1)]), f32(a["semis"][:max(n, 1)]),
                                       a["warmup"], a["max_step"], _lib.ptr(a["out"]), a["out_stride"], None, _lib.stream_ptr())

    for name, kw in bad.items():
        assert run({**good, **kw}) != 0, name
        assert b"rt_pitch" in _lib.lib().svc_last_error(), name
    torch.cuda.synchronize()
    assert np.array_equal(state.cpu().numpy(), sent) and np.array_equal(out.cpu().numpy(), out0)
    assert run(good) == 0                                                        # and the good call is good
    torch.cuda.synchronize()
    now = state.cpu().numpy()
    assert now[4, PC.W_N] == sent[4, PC.W_N] + NN and now[1, PC.W_N] == sent[1, PC.W_N] + NN
    assert np.array_equal(np.delete(now, [4, 1], axis=0), np.delete(sent, [4, 1], axis=0))
    assert np.array_equal(now[4, PC.W_BIN + 1:], sent[4, PC.W_BIN + 1:])         # the reserved words are kept


# --------------------------------------------------------------------------------------------------------------- 8: engine
def _real_engines(n_engines):
    """W.CFG_S behind the tiny_r DiT as test_gpu_rt_audio.py builds it, with an f0-conditioned regulator and the shallow RMVPE:
    2 zc samples per block, a context of 12 rows = 25 f0 frames, ce = 2."""
    from seedvc_amd import specs, weights
    from seedvc_amd.audio import Resample
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import RealtimeEngine
    from seedvc_amd.rmvpe import RMVPE
    from seedvc_amd.vocoder import BigVGAN
    from seedvc_amd.wav2vec2 import Wav2Vec2Content
    pair = (22050, 16000)
    zc, z16, _, _ = RA.units(*pair)
    cfg, sd, _, _ = cases.dit_case("tiny_r")
    lcfg = specs.lr_config("tiny", channels=64, in_channels=W.CFG_S["d_model"], out_channels=cfg["Dc"], f0_condition=True, n_f0_bins=32)
    lr = InterpolateRegulator(lcfg, weights.make_state_dict(specs.lr_state_spec(lcfg), seed=76, prefix="lr."), DEV)
    cfm = CFM(cfg, sd, DEV)
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")
    voc = BigVGAN(h, vsd, DEV)
    w2v = Wav2Vec2Content(W.make_state_dict(W.CFG_S, seed=21), W.CFG_S, device=DEV, precision=1)
    c, rsd, _ = R.model("shallow")
    rm = RMVPE(rsd, mel_basis=R.basis(), device=DEV, cfg=c)
    engines = [RealtimeEngine(lr, cfm, voc, 40, 8, 96, 32, 16, tail=8, max_streams=3) for _ in range(n_engines)]
    prompts = (16, 11)
    refs = [(cases.randn(f"rt_pitch.pc{i}", 146, 1, P, cfg["Dc"]), cases.logmel(f"rt_pitch.mel{i}", 146, 1, cfg["C"], P),
             cases.randn(f"rt_pitch.style{i}", 146, 1, cfg["style_dim"])) for i, P in enumerate(prompts)]
    return dict(engines=engines, lr=lr, w2v=w2v, rm=rm, cfg=cfg, refs=refs, prompts=prompts, Lin=2 * zc, L16=12 * z16, ce=2, S=40,
                resample=lambda: Resample(*pair, device=DEV))


def _audio(k, Lin):
    """Block k of two streams: the gliding tones of rmvpe_cases (voiced for the shallow net or not, the track is what it is)."""
    x = torch.stack([R.clip(i, 4 * Lin)[k * Lin:(k + 1) * Lin] for i in (0, 1)])
    return (x + RC.noise(f"rt_pitch.audio{k}", 146, 2, Lin) * 0.05).to(DEV)


def test_step_audio_with_pitch_equals_the_steps_made_by_hand():
    """Engine A steps from audio with pitch attached; by hand: `f0_batch` on A's context, `rt_pitch` on a state of our own,
    the track from frame 2 ce to engine B's `step_f0`.  Three blocks, two streams: blocks, SOLA buffers, tracks and statistics
    are equal bit for bit.  Then +12 semitones doubles the voiced frames of parts["f0"] exactly and changes nothing before the
    regulator; and after `reset` the next block is the first block of a fresh stream."""
    from seedvc_amd.rmvpe import rt_pitch, rt_pitch_state
    M = _real_engines(3)
    A, B, Cn = M["engines"]
    rm, ce, S, Lin = M["rm"], M["ce"], M["S"], M["Lin"]
    for e in (A, Cn):
        e.attach_audio(M["w2v"], M["resample"](), Lin, M["L16"], 0.04)
        e.attach_pitch(rm, lag_frames=2, warmup_frames=1, max_step_cents=300.0, thred=0.0)      # thred 0: every frame is voiced
    for e in M["engines"]:
        assert [e.open(*M["refs"][0]), e.open(*M["refs"][1])] == [0, 1]
    f0_ref = rm.f0_batch(R.clip(2, 16000)[None].to(DEV), thred=0.0)
    for e in (A, Cn):
        e.set_reference_f0(0, f0_ref)
        e.set_reference_f0(1, f0_ref[:, :40], 30)
        e.set_pitch(1, semitones=-2.0)
    p = A._pitch
    assert (p["Tf"], p["n_new"]) == (25, 4)
    slots = [1, 0]
    state, first = rt_pitch_state(3, DEV), None
    for k in range(3):
        z = cases.randn(f"rt_pitch.z{k}", 146, 2, M["cfg"]["C"], max(M["prompts"]) + S).to(DEV)
        out_a, parts = A.step_audio(slots, _audio(k, Lin), 3, 0.7, z=z, return_parts=True)
        raw = rm.f0_batch(parts["ctx"], thred=0.0)
        f0, shift = rt_pitch(raw, 4, 2, slots, state, p["ref_median"], [1, 1], [-2.0, 0.0], warmup=1, max_step=p["max_step"],
                             return_shift=True)
        assert torch.equal(parts["f0_raw"], raw) and torch.equal(parts["f0"], f0) and torch.equal(parts["pitch_shift"], shift), k
        assert torch.equal(p["state"], state) and parts["pitch_voiced"].tolist() == [4 * (k + 1)] * 2, k
        out_b = B.step_f0(slots, parts["content"], f0[:, 2 * ce:], [25 - 2 * ce] * 2, 3, 0.7, z=z)
        assert torch.equal(out_a, out_b) and torch.equal(A.state, B.state), k
        assert bool(torch.isfinite(out_a).all()) and bool(out_a.abs().max() > 0)
        out_plain = B.step(slots, parts["content"], 3, 0.7, z=z)                 # the track reaches the regulator
        assert not torch.equal(out_plain, out_a)
        B.state.copy_(A.state)
        first = first if first is not None else (out_a.clone(), {n: parts[n].clone() for n in ("f0", "f0_raw", "pitch_shift")})
    assert bool((shift != 0).all())                                              # an automatic shift was applied
    # +12 semitones on slot 0 of the twin engine: the same blocks, slot 0's voiced frames doubled, nothing else moved
    Cn.set_pitch(0, semitones=12.0)
    for k in range(3):
        z = cases.randn(f"rt_pitch.z{k}", 146, 2, M["cfg"]["C"], max(M["prompts"]) + S).to(DEV)
        _, pc = Cn.step_audio(slots, _audio(k, Lin), 3, 0.7, z=z, return_parts=True)
    for n in ("ctx", "content", "f0_raw", "pitch_shift", "pitch_voiced"):
        assert torch.equal(pc[n], parts[n]), n
    assert torch.equal(pc["f0"][0], parts["f0"][0])
    voiced = parts["f0_raw"][1] > 1
    assert bool(voiced.all()) and torch.equal(pc["f0"][1], parts["f0"][1] * 2.0)
    assert torch.equal(Cn._pitch["state"], state)
    # the pitch stage with its parts under torch's synchronisation watch: f0_batch, svc_rt_pitch and the voiced counts are
    # enqueued from host integers (a device tensor indexed by a Python list would be a blocking host-to-device copy)
    watch = hasattr(torch.cuda, "set_sync_debug_mode")
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode() if watch else None
    if watch:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            torch.cuda.set_sync_debug_mode("error")
    try:
        _, lens, pw = Cn._pitch_track(slots, pc["ctx"], True)
    finally:
        if watch:
            torch.cuda.set_sync_debug_mode(before)
    assert lens == [25 - 2 * ce] * 2 and pw["pitch_voiced"].tolist() == [16, 16] and pw["pitch_voiced"].dtype == torch.int32
    # reset: the next block of slot 1 is the first block of a fresh stream (slot 0 goes on)
    A.reset(1)
    assert not A._pitch["state"][1].any() and bool(A._pitch["state"][0].any())
    z = cases.randn("rt_pitch.z0", 146, 2, M["cfg"]["C"], max(M["prompts"]) + S).to(DEV)
    out_r, pr = A.step_audio(slots, _audio(0, Lin), 3, 0.7, z=z, return_parts=True)
    assert torch.equal(out_r[0], first[0][0])
    for n in ("f0", "f0_raw", "pitch_shift"):
        assert torch.equal(pr[n][0], first[1][n][0]), n
    assert pr["pitch_voiced"].tolist() == [4, 16]
