"""The yardstick and the cases of the FSMN-VAD tests (test_host_vad.py, test_gpu_vad.py).

funasr is not available to the tests, so this file is the reference: the front-end (Kaldi fbank with a Hamming window, LFR
m = 5 / n = 1, CMVN) in numpy at a chosen precision, the encoder as torch modules whose `state_dict()` carries funasr's names
(one dict feeds the yardstick and the device), and the detector as plain Python integers, all as include/seedvc_hip.h states
them.  Run at float64 they are the reference; run at float32 on the CPU they give the error an fp32 implementation makes on
the same inputs, which is what the device's error is held against (REF_ERR below, measured by `reference_error`)."""
import contextlib
import math

import numpy as np
import torch

WIN, SHIFT, NFFT, NB, BINS = 400, 160, 512, 257, 80
D_IN, D_AFF, D_LIN, D_PROJ, LORDER, LAYERS, D_OUT = 400, 140, 250, 128, 20, 4, 248
HIST = LORDER - 1
WARM = LAYERS * HIST                     # 76 rows
EPS32 = float(np.finfo(np.float32).eps)
BEGIN, END = 1, 2
MAX_EVENTS = 8
CONFIG = dict(p_max=0.2, win=20, on_count=15, off_count=15, lookback=20, end_silence=65, max_segment=6000, seg_rows=0)

# The largest error of the yardstick run in float32 on the CPU against float64, on the inputs of `score_batch()` with
# `random_state_dict(0)` (every row of every clip, final 0 and 1; measured by `reference_error`, asserted again in
# test_host_vad.py): (|p_sil - p64|, |logit - logit64|).  The device must stay within 4 x these.
REF_ERR = (4.8e-06, 2.3e-05)
SCORE_LENS = (400, 559, 560, 1999, 16000, 32000)


# ------------------------------------------------------------------------------------------------------------ the front-end
def frames_of(n):
    return 0 if n < WIN else (n - WIN) // SHIFT + 1


def rows_of(n, final):
    return frames_of(n) if final else max(0, frames_of(n) - 2)


def history_of(total):
    """Samples before the new ones that a streaming step reads: the first frame of its first new row starts there."""
    return total - SHIFT * max(0, rows_of(total, False) - 2)


def mel_bank(dtype):
    """Kaldi's triangles (torchaudio.compliance.kaldi.get_mel_banks: 20 Hz .. Nyquist, no warp) -> [80][257], arithmetic in dtype."""
    t = dtype
    melf = lambda f: t(1127.0) * np.log(t(1.0) + f / t(700.0))                                    # noqa: E731
    lo, hi = melf(t(20.0)), melf(t(8000.0))
    delta = (hi - lo) / t(BINS + 1)
    b = np.arange(BINS, dtype=t)[:, None]
    left, center, right = lo + b * delta, lo + (b + t(1.0)) * delta, lo + (b + t(2.0)) * delta
    m = melf(t(16000.0 / NFFT) * np.arange(NFFT // 2, dtype=t))[None, :]
    up, down = (m - left) / (center - left), (right - m) / (right - center)
    bank = np.maximum(t(0.0), np.minimum(up, down)).astype(t)
    return np.concatenate([bank, np.zeros((BINS, 1), t)], 1)


def hamming(dtype):
    return (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(WIN) / (WIN - 1))).astype(dtype)


def window_frames(wave, dtype):
    """wave (n,) -> [F][512]: x 32768, DC removal, pre-emphasis 0.97, Hamming, zero-padded."""
    w = np.asarray(wave, np.float32).astype(dtype) * dtype(32768.0)
    F = frames_of(len(w))
    fr = w[np.arange(F)[:, None] * SHIFT + np.arange(WIN)[None, :]] if F else np.zeros((0, WIN), dtype)
    fr = fr - fr.mean(1, keepdims=True, dtype=dtype)
    fr = fr - dtype(0.97) * np.concatenate([fr[:, :1], fr[:, :-1]], 1)
    return np.concatenate([fr * hamming(dtype), np.zeros((F, NFFT - WIN), dtype)], 1)


def dft_basis(dtype):
    ang = 2.0 * np.pi * ((np.arange(NB)[:, None] * np.arange(NFFT)[None, :]) % NFFT) / NFFT
    return np.cos(ang).astype(dtype), (-np.sin(ang)).astype(dtype)


def fbank(wave, dtype=np.float64):
    """kaldi.fbank(wave * 32768, num_mel_bins=80, dither=0, energy_floor=0, window_type="hamming") -> [F][80] log energies."""
    fr = window_frames(wave, dtype)
    c, s = dft_basis(dtype)
    re, im = fr @ c.T, fr @ s.T
    e = (re * re + im * im) @ mel_bank(dtype).T
    return np.log(np.maximum(e, dtype(EPS32)))


def lfr_cmvn(feat, final, shift, scale):
    """[F][80] -> [R][400]: row i = frames i-2 .. i+2 (below 0: frame 0; at a final call above F - 1: frame F - 1), CMVN."""
    F = len(feat)
    R = F if final else max(0, F - 2)
    idx = np.clip(np.arange(R)[:, None] + np.arange(-2, 3)[None, :], 0, max(F - 1, 0))
    x = feat[idx].reshape(R, 5 * BINS) if R else np.zeros((0, 5 * BINS), feat.dtype)
    return (x + np.asarray(shift).astype(feat.dtype)) * np.asarray(scale).astype(feat.dtype)


def frontend(wave, final, shift, scale, dtype=np.float64):
    return lfr_cmvn(fbank(wave, dtype), final, shift, scale)


# --------------------------------------------------------------------------------------------------------------- the encoder
class _Lin(torch.nn.Module):
    ROWWISE = False                      # `rowwise()`: one matrix-vector product per row

    def __init__(self, i, o, bias=True):
        super().__init__()
        self.linear = torch.nn.Linear(i, o, bias=bias)

    def forward(self, x):
        if not _Lin.ROWWISE:
            return self.linear(x)
        y = torch.stack([torch.mv(self.linear.weight, r) for r in x])
        return y if self.linear.bias is None else y + self.linear.bias


@contextlib.contextmanager
def rowwise():
    """Inside: the yardstick's linears run row by row, so a row's bits cannot depend on how many rows a call has (a BLAS
    matrix product may block its sums by the row count).  For the checks that compare runs of different lengths with ==."""
    _Lin.ROWWISE = True
    try:
        yield
    finally:
        _Lin.ROWWISE = False


class _Memory(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv_left = torch.nn.Conv2d(D_PROJ, D_PROJ, (LORDER, 1), groups=D_PROJ, bias=False)

    def forward(self, p, cache):
        """p [T][128], cache [19][128] (the rows before) -> y[t] = p[t] + sum_k w[c][k] p[t - 19 + k], the new cache."""
        full = torch.cat([cache, p], 0)
        w = self.conv_left.weight[:, 0, :, 0]                            # [128][20]
        T = p.size(0)
        y = p.clone()
        for k in range(LORDER):
            y = y + w[:, k][None, :] * full[k:k + T]
        return y, full[-HIST:]


class _Layer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear = _Lin(D_LIN, D_PROJ, bias=False)
        self.fsmn_block = _Memory()
        self.affine = _Lin(D_PROJ, D_LIN)


class Fsmn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.in_linear1, self.in_linear2 = _Lin(D_IN, D_AFF), _Lin(D_AFF, D_LIN)
        self.fsmn = torch.nn.ModuleList([_Layer() for _ in range(LAYERS)])
        self.out_linear1, self.out_linear2 = _Lin(D_LIN, D_AFF), _Lin(D_AFF, D_OUT)

    def zero_cache(self):
        p = self.in_linear1.linear.weight
        return [torch.zeros(HIST, D_PROJ, dtype=p.dtype) for _ in range(LAYERS)]

    @torch.no_grad()
    def forward(self, x, cache=None):
        """x [T][400] -> (logits [T][248], the caches after these rows)."""
        cache = self.zero_cache() if cache is None else cache
        h = torch.relu(self.in_linear2(self.in_linear1(x)))
        new = []
        for ly, c in zip(self.fsmn, cache):
            y, c2 = ly.fsmn_block(ly.linear(h), c)
            new.append(c2)
            h = torch.relu(ly.affine(y))
        return self.out_linear2(self.out_linear1(h)), new


def encoder(sd, dtype=torch.float64):
    m = Fsmn().to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return m.eval()


def p_and_logit(logits):
    """logits [T][248] -> (p_sil = softmax column 0, log(p_sil / (1 - p_sil))) in the logits' precision."""
    lse_all = torch.logsumexp(logits, 1)
    lse_rest = torch.logsumexp(logits[:, 1:], 1)
    return torch.exp(logits[:, 0] - lse_all), logits[:, 0] - lse_rest


def scores(sd, wave, final, shift, scale, precision=64):
    """The yardstick end to end at float64 (the reference) or float32 -> (p_sil, logit) as float64 numpy arrays [R]."""
    nd, td = (np.float64, torch.float64) if precision == 64 else (np.float32, torch.float32)
    x = frontend(wave, final, shift, scale, nd)
    if len(x) == 0:
        return np.zeros(0), np.zeros(0)
    p, lg = p_and_logit(encoder(sd, td)(torch.from_numpy(np.ascontiguousarray(x)))[0])
    return p.double().numpy(), lg.double().numpy()


def logit_of(p):
    """fp32 probabilities -> log(p / (1 - p)) in float64 (what the device's output is compared by)."""
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


# ------------------------------------------------------------------------------------------------------------------ weights
def cmvn(seed=0):
    """(shift, scale) [400] float32 near what noise at the amplitudes of `noise_clip` needs: rows of about unit scale."""
    rng = np.random.default_rng(1000 + seed)
    return ((-17.0 + rng.uniform(-1, 1, D_IN)).astype(np.float32), (0.35 * (1.0 + 0.2 * rng.uniform(-1, 1, D_IN))).astype(np.float32))


def random_state_dict(seed=0):
    """Random weights at fan-in scale; the 247 other classes sit at about -log 247 so that P(silence) of `noise_clip`
    spreads over (0.05, 0.95) (test_host_vad.py checks the spread)."""
    g = torch.Generator().manual_seed(seed)
    m = Fsmn()
    sd = {}
    for k, v in m.state_dict().items():
        if k.endswith("conv_left.weight"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.15
        elif k.endswith(".weight"):
            sd[k] = torch.randn(v.shape, generator=g) * (1.6 / math.sqrt(v.shape[1]))
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
    # calibrate the last layer on a probe of unit-scale rows: logit 0 to mean 0 and deviation 2, the others to deviation 0.3
    # around -log 247
    probe = torch.randn(300, D_IN, generator=g, dtype=torch.float64)
    lg = encoder(sd)(probe)[0]
    w, b = sd["out_linear2.linear.weight"], sd["out_linear2.linear.bias"]
    mean, std = lg.mean(0).float(), lg.std(0).float()
    tgt = torch.full((D_OUT,), 0.3)
    tgt[0] = 2.0
    off = torch.full((D_OUT,), -math.log(D_OUT - 1.0))
    off[0] = 0.0
    k = tgt / std
    sd["out_linear2.linear.weight"] = w * k[:, None]
    sd["out_linear2.linear.bias"] = (b - mean) * k + off
    return sd


def energy_vad_state_dict(theta, gain):
    """A hand-built energy detector in the encoder's clothes: m = the mean of the row's 400 inputs (in_linear1 row 0);
    a = (m - theta)+ and b = (theta - m)+ carried through every ReLU on channels 0 and 1 with all memory taps 0;
    logit 0 = gain (b - a), logit 1 = 0, the other 246 at -40: p_sil = sigmoid(gain (theta - m)) to 246 e^-40."""
    sd = {k: torch.zeros_like(v) for k, v in Fsmn().state_dict().items()}
    sd["in_linear1.linear.weight"][0, :] = 1.0 / D_IN
    sd["in_linear2.linear.weight"][0, 0], sd["in_linear2.linear.bias"][0] = 1.0, -float(theta)
    sd["in_linear2.linear.weight"][1, 0], sd["in_linear2.linear.bias"][1] = -1.0, float(theta)
    for l in range(LAYERS):
        for name in (f"fsmn.{l}.linear.linear.weight", f"fsmn.{l}.affine.linear.weight"):
            sd[name][0, 0] = sd[name][1, 1] = 1.0
    sd["out_linear1.linear.weight"][0, 0] = sd["out_linear1.linear.weight"][1, 1] = 1.0
    sd["out_linear2.linear.weight"][0, 0], sd["out_linear2.linear.weight"][0, 1] = -float(gain), float(gain)
    sd["out_linear2.linear.bias"][2:] = -40.0
    return sd


# -------------------------------------------------------------------------------------------------------------------- inputs
def noise_clip(n, seed):
    """White noise whose level wanders between about 0.003 and 0.3 every few hundred samples."""
    rng = np.random.default_rng(seed)
    knots = rng.uniform(-2.5, -0.5, n // 800 + 2)
    env = 10.0 ** np.interp(np.arange(n) / 800.0, np.arange(len(knots)), knots)
    return (rng.standard_normal(n) * env).astype(np.float32)


def score_batch(lens=SCORE_LENS, seed=7):
    """(waves [B][max lens] float32 with NaN above each clip's end, lens)."""
    w = np.full((len(lens), max(lens)), np.nan, np.float32)
    for b, n in enumerate(lens):
        w[b, :n] = noise_clip(n, seed + b)
    return w, list(lens)


_REF = {}


def reference(final, seed=0):
    """Per clip of `score_batch()`: (p64, logit64) and (p32, logit32) of the yardstick; computed once per process."""
    key = (int(final), seed)
    if key not in _REF:
        sd, (shift, scale) = random_state_dict(seed), cmvn(seed)
        w, lens = score_batch()
        _REF[key] = [(scores(sd, w[b, :n], final, shift, scale, 64), scores(sd, w[b, :n], final, shift, scale, 32))
                     for b, n in enumerate(lens)]
    return _REF[key]


def reference_error():
    """(max |p32 - p64|, max |logit32 - logit64|) over every row of `reference(0)` and `reference(1)`."""
    ep = el = 0.0
    for final in (0, 1):
        for (p64, l64), (p32, l32) in reference(final):
            if len(p64):
                ep, el = max(ep, float(np.abs(p32 - p64).max())), max(el, float(np.abs(l32 - l64).max()))
    return ep, el


# ------------------------------------------------------------------------------------------------------------ the detector
STATE_WORDS = ("t", "bits", "pos", "sum", "win_state", "in_seg", "beg", "sil_run", "prev_end")


def fresh_state():
    return dict.fromkeys(STATE_WORDS, 0)


def decisions(p, p_max):
    """Frame decisions as the device takes them: float32 p <= float32 p_max, NaN is silence."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore"):
        return (p <= np.float32(p_max)).astype(np.int32)


def detect(cfg, st, dec, flag=0):
    """The detector on a run of frame decisions (0 / 1), from and into the state dict `st` (updated in place) ->
    (events [(kind, time_ms), ...] every one of the call, the stream's flag after it)."""
    events, touched = [], 0
    t, bits, pos, s, win, inseg, beg, silrun, prev_end = (st[k] for k in STATE_WORDS)
    for d in dec:
        d = int(d)
        s += d - ((bits >> pos) & 1)
        bits = (bits & ~(1 << pos)) | (d << pos)
        pos = 0 if pos + 1 == cfg["win"] else pos + 1
        opened = False
        if win == 0:
            if s >= cfg["on_count"]:
                win, opened = 1, True
        elif s <= cfg["off_count"]:
            win = 0
        if not inseg and opened:
            inseg, silrun = 1, 0
            beg = max(prev_end, t - cfg["lookback"])
            events.append((BEGIN, 10 * beg))
        if inseg:
            touched = 1
            silrun = silrun + 1 if win == 0 else 0
            if silrun >= cfg["end_silence"]:
                events.append((END, 10 * t))
                inseg, prev_end, silrun = 0, t, 0
            elif t - beg + 1 >= cfg["max_segment"]:
                events.append((END, 10 * t))
                inseg, prev_end, silrun = 0, t, 0
                bits, s, win = 0, 0, 0
        t += 1
    st.update(zip(STATE_WORDS, (t, bits, pos, s, win, inseg, beg, silrun, prev_end)))
    return events, (touched if len(dec) else flag)


def detect_in_calls(cfg, dec, cuts):
    """`detect` over dec cut at the positions `cuts` (ascending) with the state carried -> (all events, final state, flags per call)."""
    st, events, flags, flag = fresh_state(), [], [], 0
    for a, b in zip([0] + list(cuts), list(cuts) + [len(dec)]):
        ev, flag = detect(cfg, st, dec[a:b], flag)
        events += ev
        flags.append(flag)
    return events, st, flags
