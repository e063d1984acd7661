"""GPU side of the streams' pitch step on the context's tail (`svc_rt_pitch_win`, csrc/rt_pitch.hip) against the
yardstick of rt_pitch_win_cases.py: every integer word, cache word and ring word against the exact statement call by call; with no
memory, bit-identity with `svc_rt_pitch` (on the same rows when the window is the whole context, on the call's raw_out
otherwise), which pins the float path to the existing kernel without a tolerance; the in-place shift of the cache with every
value distinct, up to the largest supported Tf and with n_new above the 256 threads; forgetting; isolation from the batch;
refusals that touch nothing; and the engine with window and memory on against the same steps made by hand.

max_slots = 8, Tf = 48, W = 20, guard = 6, n_new = 4, lag = 2, memory = 10 unless a test says otherwise."""
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
import rt_pitch_win_cases as WC
import w2v_cases as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
MS, TF, WN, GUARD, NN, LAG, MEM = WC.MAX_SLOTS, WC.TF, WC.W, WC.GUARD, WC.N_NEW, WC.LAG, WC.MEMORY
bits = WC.bits
NAMES, SLOTS = ["A", "B", "C"], [5, 7, 0]
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731


def _fresh(max_slots=MS, Tf=TF, memory=MEM, ref_by_slot=None):
    from seedvc_amd.rmvpe import rt_pitch_cache, rt_pitch_ring, rt_pitch_state
    ref = torch.zeros(max_slots, device=DEV)
    for s, v in (ref_by_slot or {}).items():
        ref[s] = v
    return dict(state=rt_pitch_state(max_slots, DEV), cache=rt_pitch_cache(max_slots, Tf, DEV), ring=rt_pitch_ring(max_slots, memory, DEV),
                ref=ref)


def _win(wins, slots, b, auto, semis, warmup=PC.WARMUP, max_step=PC.MAX_STEP, guard=GUARD, n_new=NN, lag=LAG):
    """One `rt_pitch_win` call on numpy windows -> (out (N, Tf), shift (N,), raw (N, Tf)) numpy."""
    from seedvc_amd.rmvpe import rt_pitch_win
    res = rt_pitch_win(dev(np.asarray(wins, np.float32)), guard, n_new, lag, slots, b["cache"], b["ring"], b["state"], b["ref"], auto, semis,
                       warmup=warmup, max_step=max_step, return_shift=True, return_raw=True)
    return tuple(t.cpu().numpy() for t in res)


def _plain(rows, slots, state, ref, auto, semis, warmup=PC.WARMUP, max_step=PC.MAX_STEP, n_new=NN, lag=LAG):
    from seedvc_amd.rmvpe import rt_pitch
    out, shift = rt_pitch(dev(np.asarray(rows, np.float32)), n_new, lag, slots, state, ref, auto, semis, warmup=warmup, max_step=max_step,
                          return_shift=True)
    return out.cpu().numpy(), shift.cpu().numpy()


def _check_words(tag, dev_words, m, dev_shift):
    """The slot's row against a `win_step_model` result whose state before the call was the device's own."""
    keep = np.ones(PC.WORDS, bool)
    keep[PC.W_SHIFT] = False
    assert np.array_equal(dev_words[keep], m["words"][keep]), (tag, np.flatnonzero(dev_words != m["words"]))
    s_dev = float(dev_words[PC.W_SHIFT:PC.W_SHIFT + 1].view(np.float32)[0])
    assert s_dev == float(dev_shift), tag
    if m["limited"] or m["shift"] == 0.0:                   # a glide step is one exact fp32 sum, a zero target is +0.0
        assert dev_words[PC.W_SHIFT] == m["words"][PC.W_SHIFT], (tag, s_dev, m["shift"])
    else:
        assert abs(s_dev - m["shift"]) <= PC.SHIFT_ATOL, (tag, s_dev, m["shift"])


# ------------------------------------------------------------------------------------------------ (a) the statement, call by call
def test_words_cache_and_ring_of_the_planted_streams():
    """Six consecutive calls on the three planted streams (slots 5, 7, 0 of 8 in one call), window 20 of 48, guard 6, memory 10:
    after every call every integer word, every cache word and every ring word equals the statement; raw_out is the cache row."""
    S = [PC.STREAMS[n] for n in NAMES]
    b = _fresh(ref_by_slot={s: st["ref"] for s, st in zip(SLOTS, S)})
    wins = np.stack([WC.win_rows(n) for n in NAMES])                             # (3, calls, W)
    before = np.zeros((3, PC.WORDS), np.int32)
    cache, fifo, pushed = [np.zeros(TF, np.float32)] * 3, [[], [], []], [[], [], []]
    for c in range(WC.N_CALLS):
        out, shift, raw = _win(wins[:, c], SLOTS, b, [st["auto"] for st in S], [st["semis"] for st in S])
        words, dc, dr = b["state"].cpu().numpy(), b["cache"].cpu().numpy(), b["ring"].cpu().numpy()
        for k, (n, st) in enumerate(zip(NAMES, S)):
            m = WC.win_step_model(before[k], cache[k], fifo[k], wins[k, c], NN, LAG, GUARD, MEM, np.float32(st["ref"]), st["auto"],
                                  st["semis"], PC.WARMUP, PC.MAX_STEP)
            _check_words((n, c), words[SLOTS[k]], m, shift[k])
            assert np.array_equal(bits(dc[SLOTS[k]]), bits(m["cache"])) and np.array_equal(bits(raw[k]), bits(m["cache"])), (n, c)
            pushed[k] = pushed[k] + m["entries"]
            assert np.array_equal(dr[SLOTS[k]], WC.ring_words(pushed[k], MEM)), (n, c, dr[SLOTS[k]])
            assert int(words[SLOTS[k]][PC.W_N]) == sum(x >= 0 for x in m["fifo"])
            before[k], cache[k], fifo[k] = words[SLOTS[k]], m["cache"], m["fifo"]
        for t in (words, dc, dr):
            assert not np.delete(t, SLOTS, axis=0).any(), c                      # unlisted slots keep every bit
    assert [int(w[PC.W_N]) for w in before] == [8, 3, 4]                         # what the rings hold at the end


# ------------------------------------------------------------------------------------- (b), (c) bit-identity with svc_rt_pitch
def test_the_whole_context_as_window_is_svc_rt_pitch_bit_for_bit():
    """memory = 0, W = Tf, guard = 0: state, out and shift_out equal `svc_rt_pitch` on the same rows over all calls."""
    from seedvc_amd.rmvpe import rt_pitch_state
    S = [PC.STREAMS[n] for n in NAMES]
    b = _fresh(memory=0, ref_by_slot={s: st["ref"] for s, st in zip(SLOTS, S)})
    assert b["ring"] is None
    plain = rt_pitch_state(MS, DEV)
    rows = np.stack([PC.stream_rows(n) for n in NAMES])
    auto, semis = [st["auto"] for st in S], [st["semis"] for st in S]
    for c in range(PC.N_CALLS):
        out, shift, raw = _win(rows[:, c], SLOTS, b, auto, semis, guard=0)
        out_p, shift_p = _plain(rows[:, c], SLOTS, plain, b["ref"], auto, semis)
        assert np.array_equal(bits(out), bits(out_p)) and np.array_equal(bits(shift), bits(shift_p)), c
        assert torch.equal(b["state"], plain), c
        assert np.array_equal(bits(raw), bits(rows[:, c])) and np.array_equal(bits(b["cache"][SLOTS].cpu().numpy()), bits(rows[:, c]))
    assert bool((b["state"][SLOTS, PC.W_SHIFT] != 0).any())


def test_a_general_window_is_svc_rt_pitch_on_the_calls_raw_out():
    """memory = 0, window 20 of 48, guard 6: after each call state, out and shift_out are bit-identical to `svc_rt_pitch`
    applied to the call's raw_out on a copy of the state before the call."""
    S = [PC.STREAMS[n] for n in NAMES]
    b = _fresh(memory=0, ref_by_slot={s: st["ref"] for s, st in zip(SLOTS, S)})
    wins = np.stack([WC.win_rows(n) for n in NAMES])
    auto, semis = [st["auto"] for st in S], [st["semis"] for st in S]
    for c in range(WC.N_CALLS):
        copy = b["state"].clone()
        out, shift, raw = _win(wins[:, c], SLOTS, b, auto, semis)
        out_p, shift_p = _plain(raw, SLOTS, copy, b["ref"], auto, semis)
        assert np.array_equal(bits(out), bits(out_p)) and np.array_equal(bits(shift), bits(shift_p)), c
        assert torch.equal(b["state"], copy), c
    assert b["state"][SLOTS, PC.W_N].cpu().tolist() == [19, 11, 13]              # rt_pitch_cases' counts: nothing forgotten


# ------------------------------------------------------------------------------------------------ (d) the in-place shift
@pytest.mark.parametrize("Tf, n_new, Wn, guard, memory", [(600, 4, 40, 8, 0), (600, 300, 320, 10, 310), (WC.MAX_TF, 18, 64, 16, 40),
                                                         (WC.MAX_TF, 2047, WC.MAX_TF, 0, 0), (257, 1, 4, 1, 3)])
def test_the_in_place_shift_moves_every_frame_once(Tf, n_new, Wn, guard, memory):
    """Every cache value distinct, two slots in one call, three calls: the row is longer than the 256 threads and n_new is
    below, above and far above them, so a frame stored before its old value was loaded would show as a wrong word.  Words,
    cache and ring against the statement."""
    b = _fresh(Tf=Tf, memory=memory)
    slots, lag = [6, 2], 2
    start = np.stack([WC.distinct_row(Tf, 100 + k) for k in range(2)])
    b["cache"][slots] = dev(start)
    cache, fifo, pushed = [start[0], start[1]], [[], []], [[], []]
    before = np.zeros((2, PC.WORDS), np.int32)
    for c in range(3):
        wins = np.stack([WC.distinct_row(Wn, 200 + 10 * c + k) + np.float32(1100.0) for k in range(2)])
        out, shift, raw = _win(wins, slots, b, [0, 0], None, warmup=0, max_step=0.0, guard=guard, n_new=n_new, lag=lag)
        words, dc = b["state"].cpu().numpy(), b["cache"].cpu().numpy()
        for k in range(2):
            m = WC.win_step_model(before[k], cache[k], fifo[k], wins[k], n_new, lag, guard, memory, 0.0, 0, 0.0, 0, 0.0)
            assert np.array_equal(bits(dc[slots[k]]), bits(m["cache"])), (c, k, np.flatnonzero(bits(dc[slots[k]]) != bits(m["cache"]))[:8])
            assert np.array_equal(bits(raw[k]), bits(m["cache"])), (c, k)
            _check_words((c, k), words[slots[k]], m, shift[k])
            pushed[k] = pushed[k] + m["entries"]
            if memory:
                assert np.array_equal(b["ring"][slots[k]].cpu().numpy(), WC.ring_words(pushed[k], memory)), (c, k)
            before[k], cache[k], fifo[k] = words[slots[k]], m["cache"], m["fifo"]
        assert not np.delete(dc, slots, axis=0).any() and not np.delete(words, slots, axis=0).any()
    assert len(set(bits(cache[0]).tolist())) > Tf // 2                            # the values stayed distinct: the check could see a swap


def test_above_the_largest_context_is_refused():
    from seedvc_amd import _lib
    from seedvc_amd.rmvpe import rt_pitch_state
    Tf = WC.MAX_TF + 1
    state, ref = rt_pitch_state(2, DEV), torch.zeros(2, device=DEV)
    cache, win, out = torch.full((2, Tf), 5.0, device=DEV), torch.zeros(1, 20, device=DEV), torch.full((1, Tf), 7.0, device=DEV)
    i32 = _lib.i32_host
    rc = _lib.lib().svc_rt_pitch_win(_lib.ptr(win), 20, 20, 6, Tf, 4, 2, 1, i32([1]), 2, _lib.ptr(cache), None, 0, _lib.ptr(state), _lib.ptr(ref),
                                     i32([0]), None, 0, 0.0, _lib.ptr(out), Tf, None, 0, None, _lib.stream_ptr())
    assert rc != 0 and b"SVC_RT_PITCH_WIN_MAX_TF" in _lib.lib().svc_last_error()
    torch.cuda.synchronize()
    assert bool((cache == 5.0).all()) and bool((out == 7.0).all()) and not state.any()


# -------------------------------------------------------------------------------------------------------- (e) forgetting
def test_a_memory_of_three_calls_holds_the_last_three_calls():
    """memory = 3 n_new, no step limit: after eight calls histogram, n, median bin and shift equal those of a fresh slot without
    a memory that was fed only the last three calls' windows.  The stream sings around 110 Hz for five calls and around 440 Hz
    for three: with the memory it ends at the high register's median bin, without it at the low one's."""
    rows = WC.register_rows()
    ref = float(np.log(300.0))
    mem, no_mem = _fresh(memory=3 * NN, ref_by_slot={3: ref}), _fresh(memory=0, ref_by_slot={3: ref, 4: ref})
    for c in range(WC.REGISTER_CALLS):
        _win(rows[c:c + 1], [3], mem, [1], None, warmup=1, max_step=0.0)
        _win(rows[c:c + 1], [3], no_mem, [1], None, warmup=1, max_step=0.0)
        if c >= WC.REGISTER_CALLS - 3:
            _win(rows[c:c + 1], [4], no_mem, [1], None, warmup=1, max_step=0.0)
    m, n = mem["state"].cpu().numpy(), no_mem["state"].cpu().numpy()
    assert np.array_equal(m[3][:PC.W_BIN + 1], n[4][:PC.W_BIN + 1])              # histogram, n, the shift's bits, the median bin
    assert m[3][PC.W_N] == 3 * NN and n[3][PC.W_N] == WC.REGISTER_CALLS * NN and m[3][PC.W_SHIFT] != 0
    low, high = (int(v) for v in PC.bins_of(np.float32([WC.LOW_HZ, WC.HIGH_HZ]))[1])
    want = WC.run_stream("A", memory=3 * NN, rows=rows)[-1]["words"]
    assert m[3][PC.W_BIN] == want[PC.W_BIN] and abs(int(m[3][PC.W_BIN]) - high) < 40
    assert abs(int(n[3][PC.W_BIN]) - low) < 40
    assert np.array_equal(m[3][:PC.W_SHIFT], want[:PC.W_SHIFT])
    assert np.array_equal(bits(mem["cache"][3].cpu().numpy()), bits(no_mem["cache"][3].cpu().numpy()))


# --------------------------------------------------------------------------------------------------------- (f) isolation
def test_a_stream_does_not_see_its_batch():
    """Stream B alone in slot 7 (N = 1) and as row 40 of a call of 64 streams in slot 33: the same state, cache, ring and output
    bits call by call; the rows of unlisted slots, filled with a sentinel, keep every bit."""
    ms = 64
    st, wins = PC.STREAMS["B"], WC.win_rows("B")
    g = np.random.default_rng(12)
    sent = dict(state=PC.sentinel_state(ms), cache=(50.0 + 400.0 * g.random((ms, TF))).astype(np.float32), ring=WC.sentinel_ring(ms, MEM))
    alone = {k: dev(v.copy()) for k, v in sent.items()}
    for k in alone:
        alone[k][7].zero_()
    alone["ref"] = torch.full((ms,), 5.0, device=DEV)
    alone["ref"][7] = st["ref"]
    crowd = _fresh(max_slots=ms)
    crowd["ref"] = dev(g.uniform(4.5, 6.0, ms).astype(np.float32))
    crowd["ref"][33] = st["ref"]
    order = [int(v) for v in g.permutation(ms)]
    order.remove(33)
    order.insert(40, 33)
    for c in range(WC.N_CALLS):
        out1, s1, raw1 = _win(wins[c:c + 1], [7], alone, [st["auto"]], [st["semis"]])
        batch = (100.0 * 2.0 ** g.uniform(0, 3, (ms, WN))).astype(np.float32)
        batch[40] = wins[c]
        auto, semis = [int(v) for v in g.integers(0, 2, ms)], [float(v) for v in g.uniform(-12, 12, ms)]
        auto[40], semis[40] = st["auto"], st["semis"]
        out64, s64, raw64 = _win(batch, order, crowd, auto, semis)
        assert np.array_equal(bits(out1[0]), bits(out64[40])) and bits(s1)[0] == bits(s64)[40], c
        assert np.array_equal(bits(raw1[0]), bits(raw64[40])), c
        for k in ("state", "cache", "ring"):
            assert torch.equal(alone[k][7].view(torch.int32), crowd[k][33].view(torch.int32)), (c, k)      # bits: the stream holds a NaN
    for k in ("state", "cache", "ring"):
        assert np.array_equal(np.delete(alone[k].cpu().numpy(), 7, axis=0).view(np.int32), np.delete(sent[k], 7, axis=0).view(np.int32)), k
    assert alone["ring"][7].cpu().numpy().tolist() == WC.ring_words(sum((r["entries"] for r in WC.run_stream("B")), []), MEM).tolist()


# ---------------------------------------------------------------------------------------------------------- (g) refusals
def test_every_refusal_leaves_state_cache_and_ring_untouched():
    from seedvc_amd import _lib
    g = np.random.default_rng(3)
    sent = dict(state=PC.sentinel_state(MS), cache=(50.0 + 400.0 * g.random((MS, TF))).astype(np.float32), ring=WC.sentinel_ring(MS, MEM))
    t = {k: dev(v.copy()) for k, v in sent.items()}
    ref = torch.full((MS,), 5.0, device=DEV)
    win = torch.full((2, WN), 220.0, device=DEV)
    out0 = np.full((2, TF), 7.0, np.float32)
    out, raw = dev(out0.copy()), dev(out0.copy())
    wide, wide_out = torch.zeros(65, WN, device=DEV), torch.zeros(65, TF, device=DEV)
    i32, f32 = _lib.i32_host, lambda v: (ctypes.c_float * len(v))(*v)      # noqa: E731
    good = dict(win=win, stride=WN, W=WN, guard=GUARD, Tf=TF, n_new=NN, lag=LAG, slots=[4, 1], max_slots=MS, cache=t["cache"], ring=t["ring"],
                memory=MEM, state=t["state"], ref=ref, auto=[1, 0], semis=[0.0, 1.0], warmup=3, max_step=0.1, out=out, out_stride=TF, raw=raw,
                raw_stride=TF)
    as_f, as_i = lambda x: x.view(torch.float32), lambda x: x.view(torch.int32)      # noqa: E731
    bad = dict(
        n_new_zero=dict(n_new=0), lag_negative=dict(lag=-1), window_before_the_row=dict(n_new=10, lag=40), N_zero=dict(slots=[]),
        N_65=dict(win=wide, out=wide_out, raw=None, slots=list(range(65)), auto=[0] * 65, semis=[0.0] * 65, max_slots=70,
                  cache=torch.zeros(70, TF, device=DEV), state=torch.zeros(70, PC.WORDS, device=DEV, dtype=torch.int32),
                  ref=torch.zeros(70, device=DEV), ring=None, memory=0),
        slot_above=dict(slots=[0, MS]), slot_negative=dict(slots=[-1, 0]), slot_twice=dict(slots=[1, 1]), stride_below_W=dict(stride=WN - 1),
        out_stride_below_Tf=dict(out_stride=TF - 1), warmup_negative=dict(warmup=-1), max_step_nan=dict(max_step=float("nan")),
        semis_inf=dict(semis=[float("-inf"), 0.0]), null_win=dict(win=None), null_state=dict(state=None), null_ref=dict(ref=None),
        null_out=dict(out=None),
        W_zero=dict(W=0, guard=0), W_above_Tf=dict(W=TF + 1), guard_negative=dict(guard=-1), window_below_n_new=dict(guard=WN - NN + 1),
        memory_negative=dict(memory=-1), memory_below_n_new=dict(memory=NN - 1), null_cache=dict(cache=None),
        ring_without_memory=dict(memory=0), memory_without_ring=dict(ring=None), raw_stride_below_Tf=dict(raw_stride=TF - 1),
        out_is_win=dict(out=win), out_in_cache=dict(out=t["cache"][2]), out_in_state=dict(out=as_f(t["state"])[3]),
        out_in_ring=dict(out=as_f(t["ring"]).reshape(-1)[5:]), raw_in_cache=dict(raw=t["cache"][MS - 2]), raw_in_state=dict(raw=as_f(t["state"])[0]),
        raw_in_ring=dict(raw=as_f(t["ring"]).reshape(-1)), raw_is_out=dict(raw=out), raw_is_win=dict(raw=win),
        state_in_out=dict(state=as_i(out)), cache_is_win=dict(cache=win), ring_in_cache=dict(ring=as_i(t["cache"])[1]))

    def run(a):
        n = len(a["slots"])
        return _lib.lib().svc_rt_pitch_win(_lib.ptr(a["win"]), a["stride"], a["W"], a["guard"], a["Tf"], a["n_new"], a["lag"], n, i32(a["slots"]),
                                           a["max_slots"], _lib.ptr(a["cache"]), _lib.ptr(a["ring"]), a["memory"], _lib.ptr(a["state"]),
                                           _lib.ptr(a["ref"]), i32(a["auto"][:max(n, 1)]), f32(a["semis"][:max(n, 1)]), a["warmup"],
                                           a["max_step"], _lib.ptr(a["out"]), a["out_stride"], _lib.ptr(a["raw"]), a["raw_stride"], None,
                                           _lib.stream_ptr())

    for name, kw in bad.items():
        assert run({**good, **kw}) != 0, name
        assert b"rt_pitch_win" in _lib.lib().svc_last_error(), name
    torch.cuda.synchronize()
    for k in sent:
        assert np.array_equal(t[k].cpu().numpy().view(np.int32), sent[k].view(np.int32)), k
    assert np.array_equal(out.cpu().numpy(), out0) and np.array_equal(raw.cpu().numpy(), out0)
    # the edges of the rules are good calls: W - guard = n_new, memory = n_new (on buffers of their own), and the good call itself
    own = _fresh(memory=NN)
    for kw in (dict(guard=WN - NN), dict(raw=None, raw_stride=0), dict(W=TF, stride=TF, guard=0, win=torch.full((2, TF), 220.0, device=DEV))):
        assert run({**good, **{k: own[k] for k in ("cache", "ring", "state")}, "memory": NN, **kw}) == 0, kw
    assert run(good) == 0
    torch.cuda.synchronize()
    now = {k: t[k].cpu().numpy() for k in sent}
    for k in sent:
        assert np.array_equal(np.delete(now[k], [4, 1], axis=0).view(np.int32), np.delete(sent[k], [4, 1], axis=0).view(np.int32)), k
    assert np.array_equal(now["state"][4, PC.W_BIN + 1:], sent["state"][4, PC.W_BIN + 1:])       # the reserved words are kept
    for s in (4, 1):
        assert (now["cache"][s, TF - WN + GUARD:] == 220.0).all() and np.array_equal(now["cache"][s, :TF - WN + GUARD - NN],
                                                                                    sent["cache"][s, NN:TF - WN + GUARD])
        assert now["ring"][s, MEM + 1] == min(sent["ring"][s, MEM + 1] + NN, MEM)


# --------------------------------------------------------------------------------------------------------------- (h) engine
class RecordingLR:
    """The regulator, with the keywords of every call recorded."""

    def __init__(self, lr):
        self.lr, self.cfg, self.calls = lr, lr.cfg, []

    def __call__(self, x, **kw):
        self.calls.append(sorted(kw))
        return self.lr(x, **kw)


def _real_engines(n_engines):
    """The reduced models of test_gpu_rt_pitch.py's engine test: W.CFG_S behind the tiny_r DiT with an f0-conditioned regulator and
    the shallow RMVPE; 2 zc samples per block, a context of 12 rows = 25 f0 frames, ce = 2."""
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
    lr = RecordingLR(InterpolateRegulator(lcfg, weights.make_state_dict(specs.lr_state_spec(lcfg), seed=76, prefix="lr."), DEV))
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
    x = torch.stack([R.clip(i, 6 * Lin)[k * Lin:(k + 1) * Lin] for i in (0, 1)])
    return (x + RC.noise(f"rt_pitch_win.audio{k}", 146, 2, Lin) * 0.05).to(DEV)


def test_step_audio_with_window_and_memory_equals_the_steps_made_by_hand():
    """Engine A steps from audio with a window of 12 of 25 frames (guard 4) and a memory of 8 frames; by hand: `f0_batch` on the
    tail of A's context, `rt_pitch_win` on buffers of our own, the track from frame 2 ce to engine B's `step_f0`.  Five blocks,
    two streams: blocks, SOLA buffers, tracks, statistics, caches and rings are equal bit for bit.  Engine C with
    `set_pitch_window(Tf, 0)` equals engine D, which has neither setting and runs `svc_rt_pitch` as before.  After `reset` the next
    block is the first block of a fresh stream; the settings are refused while a slot is open."""
    from seedvc_amd.rmvpe import rt_pitch, rt_pitch_state, rt_pitch_win
    M = _real_engines(4)
    A, B, Cn, D = M["engines"]
    rm, ce, S, Lin = M["rm"], M["ce"], M["S"], M["Lin"]
    Tf, Wn, guard, mem = 25, 12, 4, 8
    for e in (A, Cn, D):
        e.attach_audio(M["w2v"], M["resample"](), Lin, M["L16"], 0.04)
        e.attach_pitch(rm, lag_frames=2, warmup_frames=1, max_step_cents=300.0, thred=0.0)      # thred 0: every frame is voiced
    A.set_pitch_window(Wn, guard)
    A.set_pitch_memory(mem)
    Cn.set_pitch_window(Tf, 0)
    for e in M["engines"]:
        assert [e.open(*M["refs"][0]), e.open(*M["refs"][1])] == [0, 1]
    for call in (lambda: A.set_pitch_window(16, 4), lambda: A.set_pitch_window(None), lambda: D.set_pitch_memory(8)):
        with pytest.raises(ValueError, match="streams are open"):
            call()
    f0_ref = rm.f0_batch(R.clip(2, 16000)[None].to(DEV), thred=0.0)
    for e in (A, Cn, D):
        e.set_reference_f0(0, f0_ref)
        e.set_reference_f0(1, f0_ref[:, :40], 30)
        e.set_pitch(1, semitones=-2.0)
    p = A._pitch
    assert (p["Tf"], p["n_new"], p["win"], p["memory"]) == (Tf, 4, (Wn, guard), mem) and D._pitch["cache"] is None
    slots = [1, 0]
    own = _fresh(max_slots=3, Tf=Tf, memory=mem)
    plain_state, first = rt_pitch_state(3, DEV), None
    s0 = 160 * (Tf - Wn)
    zs = lambda k: cases.randn(f"rt_pitch_win.z{k}", 146, 2, M["cfg"]["C"], max(M["prompts"]) + S).to(DEV)      # noqa: E731
    for k in range(5):
        z = zs(k)
        out_a, parts = A.step_audio(slots, _audio(k, Lin), 3, 0.7, z=z, return_parts=True)
        win = rm.f0_batch(parts["ctx"][:, s0:].contiguous(), thred=0.0)
        assert tuple(win.shape) == (2, Wn)
        f0, shift, raw = rt_pitch_win(win, guard, 4, 2, slots, own["cache"], own["ring"], own["state"], p["ref_median"], [1, 1], [-2.0, 0.0],
                                      warmup=1, max_step=p["max_step"], return_shift=True, return_raw=True)
        assert torch.equal(parts["f0_window"], win) and torch.equal(parts["f0_raw"], raw) and torch.equal(parts["f0"], f0), k
        assert torch.equal(parts["pitch_shift"], shift) and torch.equal(parts["f0_raw"], p["cache"][slots]), k
        for name in ("state", "cache", "ring"):
            assert torch.equal(p[name], own[name]), (k, name)
        assert parts["pitch_voiced"].tolist() == [min(4 * (k + 1), mem)] * 2, k                  # the ring holds two blocks
        out_b = B.step_f0(slots, parts["content"], f0[:, 2 * ce:], [Tf - 2 * ce] * 2, 3, 0.7, z=z)
        assert torch.equal(out_a, out_b) and torch.equal(A.state, B.state), k
        assert bool(torch.isfinite(out_a).all()) and bool(out_a.abs().max() > 0)
        # the window as long as the context against no window at all, and that against svc_rt_pitch by hand
        out_c, pc = Cn.step_audio(slots, _audio(k, Lin), 3, 0.7, z=z, return_parts=True)
        M["lr"].calls.clear()
        out_d, pd = D.step_audio(slots, _audio(k, Lin), 3, 0.7, z=z, return_parts=True)
        assert M["lr"].calls == [["f0", "f0_lens", "n_quantizers", "ylens"]], k
        full = rm.f0_batch(pd["ctx"], thred=0.0)
        f0_p, shift_p = rt_pitch(full, 4, 2, slots, plain_state, D._pitch["ref_median"], [1, 1], [-2.0, 0.0], warmup=1,
                                 max_step=D._pitch["max_step"], return_shift=True)
        assert torch.equal(pd["f0"], f0_p) and torch.equal(pd["pitch_shift"], shift_p) and torch.equal(D._pitch["state"], plain_state), k
        assert "f0_window" not in pd and torch.equal(pd["f0_raw"], full)
        assert torch.equal(out_c, out_d) and torch.equal(Cn.state, D.state), k
        for name in ("f0", "f0_raw", "pitch_shift", "pitch_voiced", "ctx"):
            assert torch.equal(pc[name], pd[name]), (k, name)
        assert torch.equal(pc["f0_window"], full) and torch.equal(Cn._pitch["state"], D._pitch["state"]), k
        if k == 0:
            first = (out_a.clone(), {n: parts[n].clone() for n in ("f0", "f0_raw", "pitch_shift", "f0_window")})
    assert bool((shift != 0).all())                                              # an automatic shift was applied
    # the pitch stage with its parts under torch's synchronisation watch: the tail copy, f0_batch, svc_rt_pitch_win and the
    # voiced counts are enqueued from host integers
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
    assert lens == [Tf - 2 * ce] * 2 and pw["pitch_voiced"].tolist() == [24, 24] and tuple(pw["f0_window"].shape) == (2, Tf)
    # reset: the next block of slot 1 is the first block of a fresh stream (slot 0 goes on)
    A.reset(1)
    for name in ("state", "cache", "ring"):
        assert not p[name][1].any() and bool(p[name][0].any()), name
    out_r, pr = A.step_audio(slots, _audio(0, Lin), 3, 0.7, z=zs(0), return_parts=True)
    assert torch.equal(out_r[0], first[0][0])
    for n in ("f0", "f0_raw", "pitch_shift", "f0_window"):
        assert torch.equal(pr[n][0], first[1][n][0]), n
    assert pr["pitch_voiced"].tolist() == [4, mem]
