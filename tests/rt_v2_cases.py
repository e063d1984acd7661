"""Stand-ins and the numpy session shared by the v2 real-time tests (test_host_rt_v2.py, test_gpu_rt_v2.py).

`FakeTokenizer` turns a 16 kHz context into ids that are an exact integer function of it -- id[t] = trunc(frame[t][0] * 2^20) mod K
of the 320-sample frames: a power-of-two product is exact in fp32 and its truncation is the same integer in numpy and torch --
and `FakeTokenLR` is a discrete length regulator whose embedding is a table of dyadic rationals and whose interpolation is the
nearest row of `realtime_cases.FakeLR` (frame s of the output is row (s * Tin) // S of the input, times 0.5).  Behind them
`long_batch_cases.BatchedFakeCFM` and `realtime_cases.FakeVocoder` make an engine step exactly rounded, so `sessions` states
whole `step_audio` sessions of a token-mode engine in numpy: `rt_audio_cases.push_model_fp32` -> `fake_tokens` -> `TABLE` ->
`realtime_cases.session_model`."""
import functools

import numpy as np
import torch

import cases
import realtime_cases as RT
import resample_cases as RC
import rt_audio_cases as RA

K = 64                                                       # codebook of the stand-ins
# the sizes of the audio-engine test (test_gpu_rt_audio.py): blocks of 2 zc, 8 content rows of which 2 are dropped
FAKE_PAIR, FAKE_M, FAKE_L16, FAKE_CE = (22050, 16000), 2, 8 * 320, 0.04
N_BLOCKS = 5
AUDIO_SEED = 42                                              # chosen on the CPU: `sessions` asserts that no block is a near tie


def _table():
    """(K, CHUNK_DC) float32: integers in [-128, 128) over 64, a fixed pseudo-random table"""
    rng = np.random.default_rng(811)
    return (rng.integers(-128, 128, (K, cases.CHUNK_DC)).astype(np.float32) / np.float32(64.0)).astype(np.float32)


TABLE = _table()


def fake_tokens(ctx):
    """numpy: ctx (L16,) float32 -> (L16 // 320,) int32, what `FakeTokenizer` gives"""
    ctx = np.asarray(ctx, np.float32)
    first = ctx[:len(ctx) // 320 * 320].reshape(-1, 320)[:, 0]
    return ((first * np.float32(2.0 ** 20)).astype(np.int64) % K).astype(np.int32)


class FakeTokenizer:
    """Stand-in tokenizer with the call surface `RealtimeEngine.attach_audio` reads in token mode; every head gives the same
    ids.  `calls` records (n, L, head) of every call."""

    def __init__(self, codebook=K):
        self.codebook, self.calls = codebook, []

    def codebook_size(self, head=0):
        return self.codebook

    def tokens_fn(self, waves_16k, head=0):
        n, L = waves_16k.shape
        self.calls.append((n, L, head))
        first = waves_16k[:, :L // 320 * 320].reshape(n, L // 320, 320)[:, :, 0]
        return ((first * float(2 ** 20)).to(torch.int64) % K).to(torch.int32)


class FakeTokenLR:
    """Stand-in discrete length regulator with the v2 regulator's call and return: (n, Tin) integer ids ->
    (TABLE[ids][:, (s * Tin) // S] * 0.5 (n, S, CHUNK_DC), ylens)."""

    def __init__(self, device="cpu", codebook=K):
        self.cfg = dict(is_discrete=True, codebook_size=codebook, f0_condition=False)
        self.table = torch.from_numpy(TABLE).to(device)

    def __call__(self, x, ylens=None, f0=None):
        assert x.dim() == 2 and not x.is_floating_point() and f0 is None
        S, Tin = int(ylens.max()), x.size(1)
        idx = (torch.arange(S, device=x.device) * Tin) // S
        return self.table[x.long()][:, idx] * 0.5, ylens


def fake_content(tokens):
    """numpy: ids (Tin,) -> the (Tin, CHUNK_DC) rows `realtime_cases.fake_wave` takes (it applies FakeLR's own nearest row and 0.5)"""
    return TABLE[np.asarray(tokens, np.int64)]


@functools.lru_cache(maxsize=None)
def sessions():
    """Three streams of N_BLOCKS blocks: dict(audio [s] (N_BLOCKS, Lin), ctx [s][k] (L16,), tokens [s][k] (6,) int32, models [s] =
    `realtime_cases.session_model` of the streams' table rows).  Computed once; asserts that no block after the first (whose
    buffer is zero) is decided by a score gap under 1e-4."""
    fi, fo = RT.gui_windows(RT.FAKE_GEOMETRY["sola_buffer"])
    zc, z16, _, _ = RA.units(*FAKE_PAIR)
    ce = int(FAKE_CE * 50)
    audio, ctxs, toks, models = [], [], [], []
    for s in range(3):
        blocks = (RC.noise(f"rt_v2.session{s}", AUDIO_SEED, N_BLOCKS, FAKE_M * zc) * 0.5).numpy()
        hist, ring = np.zeros(2 * zc, np.float32), np.zeros(FAKE_L16, np.float32)
        cs, ts = [], []
        for k in range(N_BLOCKS):
            ring, hist = RA.push_model_fp32(hist, ring, blocks[k], *FAKE_PAIR, zc, z16)
            cs.append(ring)
            ts.append(fake_tokens(ring)[ce:])
        audio.append(blocks)
        ctxs.append(cs)
        toks.append(ts)
        models.append(RT.session_model([fake_content(t) for t in ts], fi, fo))
    gaps = [RT.score_gap(m[3]) for ms in models for m in ms[1:]]
    assert min(gaps) > 1e-4, f"a block of the model is decided by a score gap of {min(gaps):.3e}: choose another AUDIO_SEED"
    return dict(audio=audio, ctx=ctxs, tokens=toks, models=models, min_gap=min(gaps))
