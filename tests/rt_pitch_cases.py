"""The yardstick of the streams' pitch step (`svc_rt_pitch`), shared by test_host_rt_pitch.py and
test_gpu_rt_pitch.py.

`bins_of`, `count_window`, `median_bin` state the binning, the counting window, the rank and the median bin in exact integers,
in numpy on the int32 view of the floats: the device has to give the same words.  `step_model` adds the float64 statement of
the running median, the glide and the per-frame output for one stream and one call, as include/seedvc_hip.h words them.

`SABOTAGES` are planted faults of the statement; `step_model(..., sabotage=name)` computes with one of them.  The host test
runs every case below clean and sabotaged: every sabotage has to change the state or the shift of at least one case, so the
cases can tell a kernel with that fault from a correct one.

The planted streams: three streams of six calls (`STREAMS`, `stream_rows`), a context of Tf = 48 frames of which a call counts
n_new = 4 at lag = 2.  A stream is one long sequence of f0 values; the row of call c is the window seq[4 c : 4 c + 48] with its
last `lag` frames replaced by voiced junk that changes from call to call (provisional frames must not be counted)."""
import numpy as np

BINS, WORDS, W_N, W_SHIFT, W_BIN, BIN0 = 1536, 1536 + 8, 1536, 1537, 1538, 33792
TF, N_NEW, LAG, MAX_SLOTS = 48, 4, 2, 64
SABOTAGES = ("rank", "window_lo", "window_hi", "edge", "overshoot", "warmup_gt", "median_before")
OUT_RTOL = 2e-6            # four fp32 roundings of a chain whose largest log is 7.7: 4 x 4.8e-7 (the issue's bound)
SHIFT_ATOL = 1e-6          # word 1537 on arrival: one rounding of a log <= 7.7 (4.8e-7), of c + 1e-5 and of the difference (6e-8 each)
HALF_BIN = 2e-3            # ln(1 + 2^-8) / 2 = 1.95e-3 rounded up: a bin's centre against any float of the bin, in the log domain
EPS32 = np.float32(1e-5)


def f32(bits):
    """float32 of an int bit pattern."""
    return np.array([bits], np.uint32).view(np.float32)[0]


def bin_edge(b):
    """The lowest float of bin b."""
    return f32((b + BIN0) << 15)


def bin_centre(b):
    return f32(((int(b) + BIN0) << 15) | 0x4000)


# ---------------------------------------------------------------------------------------------------- the integer statement
def bins_of(f0, sabotage=None):
    """f0 float32 array -> (voiced bool, bin int64): voiced iff f0 > 1 (NaN is not), bin = clamp((bits >> 15) - 33792, 0, 1535)."""
    f = np.ascontiguousarray(f0, np.float32)
    bits = f.view(np.int32).astype(np.int64)
    with np.errstate(invalid="ignore"):
        voiced = f > np.float32(1.0)
    if sabotage == "edge":
        bits = bits - 1                                   # a float exactly on an edge falls into the bin below
    return voiced, np.clip((bits >> 15) - BIN0, 0, BINS - 1)


def count_window(Tf, n_new, lag, sabotage=None):
    lo, hi = Tf - lag - n_new, Tf - lag
    if sabotage == "window_lo":
        lo -= 1
    if sabotage == "window_hi":
        hi += 1
    return max(lo, 0), min(hi, Tf)


def median_bin(hist, n, sabotage=None):
    """The first bin whose cumulative count exceeds the lower-middle rank (n - 1) // 2; 0 while n == 0."""
    if n <= 0:
        return 0
    r = n // 2 if sabotage == "rank" else (n - 1) // 2
    return int(min(np.searchsorted(np.cumsum(np.asarray(hist, np.int64)), r, side="right"), BINS - 1))


def count_row(words, row, n_new, lag, sabotage=None):
    """words int32 [WORDS] (not changed), row float32 [Tf] -> (new histogram int64 [BINS], new n, median bin)."""
    hist, n = np.asarray(words[:BINS], np.int64).copy(), int(words[W_N])
    lo, hi = count_window(len(row), n_new, lag, sabotage)
    voiced, b = bins_of(np.asarray(row, np.float32)[lo:hi], sabotage)
    before = median_bin(hist, n, sabotage)
    np.add.at(hist, b[voiced], 1)
    n += int(voiced.sum())
    return hist, n, (before if sabotage == "median_before" else median_bin(hist, n, sabotage))


# ---------------------------------------------------------------------------------------------------- the float64 statement
def step_model(words, row, n_new, lag, ref_median, auto, semitones, warmup, max_step, sabotage=None):
    """One call for one stream.  words int32 [WORDS]: the slot's row before the call (word 1537 the bits of the applied shift).
    -> dict(words int32 [WORDS] after the call, with word 1537 = float32(shift); shift float64; limited: the glide cut the step;
    out float64 [Tf]; m_run float64)."""
    words = np.asarray(words, np.int32)
    row = np.asarray(row, np.float32)
    hist, n, b = count_row(words, row, n_new, lag, sabotage)
    m_run = float(np.log(np.float64(bin_centre(b)) + np.float64(EPS32)))
    warm = n > max(warmup, 1) if sabotage == "warmup_gt" else n >= max(warmup, 1)
    has_ref = float(ref_median) > 0.0                       # 0 (the median of an unvoiced reference), negative, NaN: no reference
    d = float(ref_median) - m_run if auto and warm and has_ref else 0.0
    s_old = float(words[W_SHIFT:W_SHIFT + 1].view(np.float32)[0])
    step = float(np.float32(max_step))
    off = not (0.0 < step < float("inf"))
    if sabotage == "overshoot":
        arrive = off
    else:
        arrive = off or abs(d - s_old) <= step
    s_new = d if arrive else (s_old + step if d > s_old else s_old - step)
    out_words = words.copy()
    out_words[:BINS] = hist
    out_words[W_N], out_words[W_BIN] = n, b
    out_words[W_SHIFT:W_SHIFT + 1] = np.array([s_new], np.float32).view(np.int32)
    return dict(words=out_words, shift=s_new, limited=not arrive, m_run=m_run,
                out=output_model(row, float(np.float32(s_new)), semitones))


def output_model(row, shift, semitones):
    """float64: voiced frames exp(log(f0 + 1e-5) + shift) 2^(semitones / 12), the others exp(log(f0 + 1e-5)); f0 + 1e-5 is the
    device's own float32 sum (its rounding is part of the input, as the log's argument)."""
    row = np.asarray(row, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        voiced = row > np.float32(1.0)
        lg = np.log((row + EPS32).astype(np.float64))
        factor = 2.0 ** (float(np.float32(semitones)) / 12.0)
        return np.where(voiced, np.exp(lg + shift) * factor, np.exp(lg))


def rel_err(got, want):
    """max |got - want| / |want| over the finite entries; the others must be of the same kind (NaN, +inf)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    return float((np.abs(got[fin] - want[fin]) / np.abs(want[fin])).max()) if fin.any() else 0.0


# ---------------------------------------------------------------------------------------------------- the planted streams
NAN, INF = np.float32("nan"), np.float32("inf")
X_BIN, Y_BIN = 600, 760                                    # two bins of the tie stream
_below = lambda x: np.nextafter(np.float32(x), np.float32(0))          # noqa: E731
_above = lambda x: np.nextafter(np.float32(x), INF)                    # noqa: E731


def _counted_a():
    """Stream A, 24 counted frames: floats on a bin edge and one ulp below it, 1.0, 1.0 + ulp, 0, NaN, 31, 32, 2047.99, 5000, +inf."""
    e1, e2 = bin_edge(700), bin_edge(701)
    return np.array([e1, _below(e1), 1.0, _above(1.0),
                     0.0, NAN, 31.0, 32.0,
                     2047.99, 5000.0, INF, e2,
                     _below(e2), bin_centre(700), 0.5, -3.0,
                     _below(32.0), _below(2048.0), 2048.0, 220.0,
                     bin_edge(1535), _below(bin_edge(1535)), bin_edge(1), _below(bin_edge(1))], np.float32)


def _counted_b():
    """Stream B: all frames in one bin (n = 3, odd), then n = 5 = warmup - 1, then n = 6 = warmup with a two-bin tie at the rank
    (X: 3, Y: 3; the lower-middle rank 2 is in X, rank 3 would be in Y), then four more in Y (n = 10, even: the median moves to Y,
    which a median taken before the call's frames misses), then unvoiced only, then one in X (n = 11)."""
    x, y, u = bin_centre(X_BIN), bin_centre(Y_BIN), np.float32(0.0)
    return np.array([x, u, _above(bin_edge(X_BIN)), _below(bin_edge(X_BIN + 1)),
                     y, u, u, bin_edge(Y_BIN),
                     u, u, _below(bin_edge(Y_BIN + 1)), u,
                     y, y, y, y,
                     u, NAN, u, 0.9,
                     u, x, u, u], np.float32)


def _counted_c():
    """Stream C: a melody, voiced and unvoiced frames mixed, 1, 3, 4, 2, 0, 3 voiced frames per call."""
    g = np.random.default_rng(411)
    hz = (110.0 * 2.0 ** (g.uniform(0, 2.5, 24))).astype(np.float32)
    keep = np.array([1, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1, 1], bool)
    return np.where(keep, hz, np.float32(0.0)).astype(np.float32)


WARMUP = 6                       # stream B reaches n = 5 after call 1 and n = 6 after call 2
MAX_STEP = 0.25
STREAMS = dict(
    A=dict(counted=_counted_a, ref=float(np.log(300.0)), auto=1, semis=0.0, junk=440.0),
    B=dict(counted=_counted_b, ref=float(np.log(bin_centre(X_BIN) + 1e-5)) + 0.6, auto=1, semis=3.0, junk=55.0),
    C=dict(counted=_counted_c, ref=float(np.log(180.0)), auto=0, semis=-12.0, junk=3000.0),
)
N_CALLS = 6


def stream_rows(name, n_calls=N_CALLS, Tf=TF, n_new=N_NEW, lag=LAG):
    """The n_calls rows (n_calls, Tf) float32 of a planted stream: its counted frames sit at [Tf - lag - n_new, Tf - lag) of their
    call's row and move n_new frames to the left per call; the frames before the first counted one are voiced filler that no
    call may count, the last `lag` frames of every row are voiced junk that differs from call to call."""
    s = STREAMS[name]
    counted = s["counted"]()
    assert counted.shape == (n_calls * n_new,)
    lo = Tf - lag - n_new
    g = np.random.default_rng(sum(map(ord, name)))
    seq = np.concatenate([(150.0 + 40.0 * g.random(lo)).astype(np.float32), counted, np.zeros(lag, np.float32)])
    rows = np.stack([seq[c * n_new:c * n_new + Tf] for c in range(n_calls)]).copy()
    for c in range(n_calls):
        rows[c, Tf - lag:] = np.float32(s["junk"]) * np.float32(1.0 + 0.01 * c)
    return rows


def run_stream(name, sabotage=None, warmup=WARMUP, max_step=MAX_STEP, n_calls=N_CALLS):
    """The model's session of a planted stream from a fresh state -> list of `step_model` results, one per call."""
    s, words, res = STREAMS[name], np.zeros(WORDS, np.int32), []
    for row in stream_rows(name, n_calls):
        res.append(step_model(words, row, N_NEW, LAG, s["ref"], s["auto"], s["semis"], warmup, max_step, sabotage))
        words = res[-1]["words"]
    return res


# the glide case: a constant 220 Hz stream under a reference an octave up; 0.25 per call arrives in exactly 3 calls
GLIDE = dict(hz=220.0, ref=float(np.float32(np.log(440.0))), max_step=0.25, calls_to_arrive=3)       # a float32, as the device holds it


def glide_rows(n_calls):
    return np.full((n_calls, TF), np.float32(GLIDE["hz"]), np.float32)


def run_glide(sabotage=None, n_calls=4):
    words, res = np.zeros(WORDS, np.int32), []
    for row in glide_rows(n_calls):
        res.append(step_model(words, row, N_NEW, LAG, GLIDE["ref"], 1, 0.0, 0, GLIDE["max_step"], sabotage))
        words = res[-1]["words"]
    return res


def sentinel_state(max_slots=MAX_SLOTS, seed=5):
    """A state of consistent rows that no call may change: a random histogram per slot, its total, a shift and its median bin."""
    g = np.random.default_rng(seed)
    st = np.zeros((max_slots, WORDS), np.int32)
    st[:, :BINS] = g.integers(0, 3, (max_slots, BINS))
    st[:, W_N] = st[:, :BINS].sum(1)
    st[:, W_SHIFT] = g.uniform(-0.5, 0.5, max_slots).astype(np.float32).view(np.int32)
    st[:, W_BIN] = [median_bin(st[s, :BINS], int(st[s, W_N])) for s in range(max_slots)]
    st[:, W_BIN + 1:] = g.integers(-9, 9, (max_slots, WORDS - W_BIN - 1))
    return st
