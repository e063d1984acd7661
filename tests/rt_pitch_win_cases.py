"""The yardstick of the streams' pitch step on the context's tail (`svc_rt_pitch_win`), shared by
test_host_rt_pitch_win.py and test_gpu_rt_pitch_win.py.

`cache_update`, `fifo_step` and `ring_words` state the cache update, the FIFO of counted bins and the ring's words in exact
integers, in numpy on the int32 view of the floats; binning, counting window, rank, median bin, glide and output are those of
rt_pitch_cases (`bins_of`, `count_window`, `median_bin`, `step_model`), which `win_step_model` calls on the new cache row after it
has taken the expired entries out of the histogram.  The FIFO is stated entry by entry (push one, drop one when full), the ring
words in closed form (the t-th counted frame of a stream sits in word t mod memory): neither restates the device's batched form.

`SABOTAGES` are planted faults of the statement; every one has to change the words, the cache, the FIFO or the shift of at
least one planted case (test_host_rt_pitch_win.py), so the cases can tell a kernel with that fault from a correct one.

The planted streams are rt_pitch_cases' (edge floats, ties, a melody), placed in window frames: the window of call c is the
last W frames of `stream_rows(name)[c]`.  Tf = 48, W = 20, guard = 6, n_new = 4, lag = 2, memory = 10: the counted frames
[42, 46) lie inside the trusted part [34, 48) of the window, and the ring of 10 fills in the middle of the third call."""
import numpy as np

import rt_pitch_cases as PC

TF, W, GUARD, N_NEW, LAG, MEMORY, MAX_SLOTS, N_CALLS = PC.TF, 20, 6, PC.N_NEW, PC.LAG, 10, 8, PC.N_CALLS
MAX_TF = 4096                                              # SVC_RT_PITCH_WIN_MAX_TF
SABOTAGES = ("shift_minus", "shift_plus", "guard_minus", "guard_plus", "window_early", "expire_newest", "expire_keeps_n", "cap_minus",
             "cap_plus")
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)      # noqa: E731


# ---------------------------------------------------------------------------------------------------- the integer statement
def cache_update(old, win, n_new, guard, sabotage=None):
    """old float32 [Tf], win float32 [W] -> new float32 [Tf], moved as int32 words (NaN payloads and -0.0 survive):
    new[i] = win[i - (Tf - W)] for i >= Tf - W + guard, old[i + n_new] below."""
    ob, wb = bits(old), bits(win)
    Tf, Wn = len(ob), len(wb)
    assert 0 <= guard and Wn <= Tf and Wn - guard >= n_new
    shift = n_new + {"shift_minus": -1, "shift_plus": 1}.get(sabotage, 0)
    g = guard + {"guard_minus": -1, "guard_plus": 1}.get(sabotage, 0)
    w0 = Tf - Wn - (1 if sabotage == "window_early" else 0)            # early: window frame j taken for context frame Tf - W + j - 1
    i = np.arange(Tf)
    new = np.where(i >= Tf - Wn + g, wb[np.clip(i - w0, 0, Wn - 1)], ob[np.clip(i + shift, 0, Tf - 1)])
    return new.astype(np.int32).view(np.float32)


def entries_of(new, n_new, lag):
    """The counted frames of a row as ring entries, in frame order: the bin of a voiced frame, -1 for an unvoiced one."""
    lo, hi = PC.count_window(len(new), n_new, lag)
    voiced, b = PC.bins_of(np.asarray(new, np.float32)[lo:hi])
    return [int(x) if v else -1 for v, x in zip(voiced, b)]


def fifo_step(fifo, entries, memory, sabotage=None):
    """fifo: the entries held, oldest first.  Every entry is pushed; a push onto a full FIFO drops the oldest.
    -> (the FIFO after the call, the dropped entries)."""
    cap = memory + {"cap_minus": -1, "cap_plus": 1}.get(sabotage, 0)
    fifo, dropped = list(fifo), []
    for x in entries:
        fifo.append(x)
        if len(fifo) > cap:
            dropped.append(fifo.pop(-2 if sabotage == "expire_newest" else 0))
    return fifo, dropped


def ring_words(pushed, memory):
    """The slot's ring row int32 [memory + 2] after a fresh stream has counted the entries `pushed` (all of them, in order): the
    t-th sits in word t % memory, head is the word of the oldest entry held, fill the number held."""
    w = np.zeros(memory + 2, np.int32)
    fill = min(len(pushed), memory)
    for t in range(len(pushed) - fill, len(pushed)):
        w[t % memory] = pushed[t]
    w[memory], w[memory + 1] = (len(pushed) - fill) % memory, fill
    return w


def win_step_model(words, cache, fifo, win, n_new, lag, guard, memory, ref_median, auto, semitones, warmup, max_step, sabotage=None):
    """One call for one stream.  words int32 [WORDS], cache float32 [Tf], fifo (list) before the call; win float32 [W].
    -> `rt_pitch_cases.step_model`'s dict over the new row, plus cache (the new row), fifo and entries (this call's)."""
    new = cache_update(cache, win, n_new, guard, sabotage)
    entries = entries_of(new, n_new, lag)
    words = np.asarray(words, np.int32).copy()
    if memory:
        fifo, dropped = fifo_step(fifo, entries, memory, sabotage)
        for x in dropped:
            if x >= 0:
                words[x] -= 1
                if sabotage != "expire_keeps_n":
                    words[PC.W_N] -= 1
    else:
        fifo = []
    m = PC.step_model(words, new, n_new, lag, ref_median, auto, semitones, warmup, max_step)     # counts [Tf - lag - n_new, Tf - lag) of new
    return dict(m, cache=new, fifo=fifo, entries=entries)


# ---------------------------------------------------------------------------------------------------- the planted streams
def win_rows(name, n_calls=N_CALLS, Tf=TF, Wn=W):
    """(n_calls, W): the windows of a planted stream, the last W frames of its context rows."""
    return PC.stream_rows(name, n_calls, Tf)[:, Tf - Wn:].copy()


def run_stream(name, sabotage=None, memory=MEMORY, guard=GUARD, warmup=PC.WARMUP, max_step=PC.MAX_STEP, rows=None):
    """The model's session of a planted stream from a fresh slot -> list of `win_step_model` results, one per call."""
    s = PC.STREAMS[name]
    words, cache, fifo, res = np.zeros(PC.WORDS, np.int32), np.zeros(TF, np.float32), [], []
    for win in (win_rows(name) if rows is None else rows):
        res.append(win_step_model(words, cache, fifo, win, N_NEW, LAG, guard, memory, s["ref"], s["auto"], s["semis"], warmup, max_step,
                                  sabotage))
        words, cache, fifo = res[-1]["words"], res[-1]["cache"], res[-1]["fifo"]
    return res


def trace(results):
    return [(r["words"].tobytes(), bits(r["cache"]).tobytes(), tuple(r["fifo"]), r["shift"]) for r in results]


# the guard case: one call with W - guard = n_new + lag, so the first trusted window frame is the first counted frame.  Window
# frame guard - 1 is voiced against an unvoiced cache (a guard one too small takes it), window frame guard is unvoiced against a
# voiced cache (a guard one too large keeps the cache's and counts it)
GUARD_CASE = dict(Tf=24, W=12, guard=6, n_new=4, lag=2)


def guard_case():
    g = GUARD_CASE
    keep = g["Tf"] - g["W"] + g["guard"]
    old = np.zeros(g["Tf"], np.float32)
    old[keep + g["n_new"]] = 300.0
    win = np.zeros(g["W"], np.float32)
    win[g["guard"] - 1] = 250.0
    win[g["guard"] + 1:] = 200.0
    return old, win


def run_guard(sabotage=None):
    g = GUARD_CASE
    old, win = guard_case()
    return [win_step_model(np.zeros(PC.WORDS, np.int32), old, [], win, g["n_new"], g["lag"], g["guard"], 0, 0.0, 0, 0.0, 0, 0.0, sabotage)]


# the register case: a stream that sings around 110 Hz for five calls and around 440 Hz for three; memory = 3 n_new
LOW_HZ, HIGH_HZ, REGISTER_CALLS = 110.0, 440.0, 8


def register_rows(Wn=W, seed=9):
    """(8, W) windows of one long sequence of voiced frames, every value distinct."""
    g = np.random.default_rng(seed)
    total = TF + REGISTER_CALLS * N_NEW
    turn = TF - LAG + 5 * N_NEW                              # the first frame counted by call 5
    seq = np.where(np.arange(total) < turn, LOW_HZ, HIGH_HZ) * 2.0 ** g.uniform(-0.1, 0.1, total)
    seq = seq.astype(np.float32)
    return np.stack([seq[(c + 1) * N_NEW + TF - Wn:(c + 1) * N_NEW + TF] for c in range(REGISTER_CALLS)])


def distinct_row(n, seed):
    """n distinct voiced floats in a random order (for the shift of the cache: a frame in the wrong place is a wrong word)."""
    g = np.random.default_rng(seed)
    return (100.0 + g.permutation(n).astype(np.float32) * np.float32(0.25)).astype(np.float32)


def sentinel_ring(max_slots, memory, seed=6):
    """Consistent ring rows no refused call may change: random entries, a head and a fill."""
    g = np.random.default_rng(seed)
    r = np.zeros((max_slots, memory + 2), np.int32)
    r[:, :memory] = g.integers(-1, PC.BINS, (max_slots, memory))
    r[:, memory] = g.integers(0, memory, max_slots)
    r[:, memory + 1] = g.integers(0, memory + 1, max_slots)
    return r
