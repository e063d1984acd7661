"""Models and stand-ins shared by the real-time session tests (test_host_realtime.py, test_gpu_realtime.py).

`sola_model` is the numpy statement of one SOLA splice as include/seedvc_hip.h (`svc_sola_step`) and
`pipeline.RealtimeEngine` state it: float64 scores, separately rounded fp32 fade.  `gui_sola_torch` is a direct transcription
of the reference GUI's lines (real-time-gui.py, `audio_callback`, from memory): the host test holds the model to it on
planted-peak inputs.  `FakeLR`, `FakeVocoder` and the numpy chain `fake_wave` complete `long_batch_cases.BatchedFakeCFM` to an
exactly rounded engine step, and `planted_session` cuts the steps' content out of one long sequence so that every
step's SOLA buffer reappears in the next step's input at a known offset (score = |buffer|, a wide gap to every other)."""
import numpy as np
import torch
import torch.nn.functional as F

import cases


def gui_windows(Lb):
    """(fade_in, fade_out) of the GUI, float32 numpy."""
    from seedvc_amd.pipeline import gui_fade_windows
    return tuple(w.numpy() for w in gui_fade_windows(Lb))


def sola_scores(infer, buf, Ls):
    """float64 score[o] = <infer[o : o + Lb], buf> / sqrt(|infer[o : o + Lb]|^2 + 1e-8), o = 0 .. Ls."""
    x, b = np.asarray(infer, np.float64), np.asarray(buf, np.float64)
    Lb = len(b)
    return np.array([x[o:o + Lb] @ b / np.sqrt(x[o:o + Lb] @ x[o:o + Lb] + 1e-8) for o in range(Ls + 1)])


def sola_model(infer, buf, fade_in, fade_out, block, Ls, offset=None):
    """infer (block + Lb + Ls,) float32, buf / fade_in / fade_out (Lb,) float32 -> (out (block,), new buffer (Lb,), o*, scores).
    `offset` evaluates the splice at a given offset instead of the model's own argmax (the lowest maximiser)."""
    infer, buf = np.asarray(infer, np.float32), np.asarray(buf, np.float32)
    Lb = len(buf)
    assert infer.shape == (block + Lb + Ls,) and fade_in.dtype == fade_out.dtype == np.float32
    scores = sola_scores(infer, buf, Ls)
    o = int(np.argmax(scores)) if offset is None else int(offset)
    y = infer[o:o + block + Lb].copy()
    y[:Lb] = y[:Lb] * fade_in + buf * fade_out                  # float32 arrays: two rounded products, one rounded sum
    return y[:block].copy(), y[block:block + Lb].copy(), o, scores


def score_gap(scores):
    """Distance of the best score to the second best."""
    s = np.sort(scores)
    return float(s[-1] - s[-2]) if len(s) > 1 else float("inf")


def gui_sola_torch(infer, buf, fade_in, fade_out, block, Ls):
    """The GUI's own statements on torch tensors (fp32): -> (out, new buffer, offset)."""
    infer_wav, sola_buffer = infer.clone(), buf.clone()
    Lb = sola_buffer.numel()
    conv_input = infer_wav[None, None, :Lb + Ls]
    cor_nom = F.conv1d(conv_input, sola_buffer[None, None, :])
    cor_den = torch.sqrt(F.conv1d(conv_input ** 2, torch.ones(1, 1, Lb, device=infer_wav.device)) + 1e-8)
    sola_offset = torch.argmax(cor_nom[0, 0] / cor_den[0, 0])
    infer_wav = infer_wav[sola_offset:]
    infer_wav[:Lb] *= fade_in
    infer_wav[:Lb] += sola_buffer * fade_out
    sola_buffer[:] = infer_wav[block:block + Lb]
    return infer_wav[:block].clone(), sola_buffer, int(sola_offset)


def planted_input(tag, seed, block, Lb, Ls, offset, gain=1.0):
    """(infer, buf): noise with `gain * buf` written at `offset`, so that offset's score is about |buf|."""
    buf = cases.randn(tag + ".buf", seed, Lb).numpy()
    infer = cases.randn(tag + ".x", seed, block + Lb + Ls).numpy()
    infer[offset:offset + Lb] = buf * np.float32(gain)
    return infer, buf


# ------------------------------------------------------------------------------------------ the exactly rounded engine step
FAKE_GEOMETRY = dict(S=12, hop=cases.CHUNK_HOP, block=44, sola_buffer=16, sola_search=12, tail=8)      # start = 16
# frames the content window advances between consecutive steps: the planted offset moves by block - advance * hop samples
FAKE_ADVANCES = ([5, 5, 5, 7], [4, 6, 6, 5], [5, 6, 4, 7])
FAKE_OFFSETS = ([0, 4, 8, 12, 0], [0, 12, 8, 4, 8], [0, 4, 0, 12, 0])
FAKE_PROMPTS = (20, 11, 16)


class FakeLR:
    """Stand-in length regulator: frame s of the output is frame (s * Tin) // S of the input times 0.5 (one exact fp32
    multiply), with the v1 regulator's return tuple."""

    def __call__(self, x, ylens=None, n_quantizers=None, f0=None):
        S, Tin = int(ylens.max()), x.size(1)
        idx = (torch.arange(S, device=x.device) * Tin) // S
        return x.float()[:, idx] * 0.5, ylens, None, None, None


class FakeVocoder:
    """Stand-in vocoder, any B: sample t * hop + j = mel[0, t] * (j + 1) / 8 + mel[1, t] * (-1)^j (single fp32 operations).
    `cases.fake_vocoder` without the sign keeps neighbouring samples alike; the alternating term makes a one-sample shift
    visible in the SOLA score.  `calls` records (B, S) of every call."""

    def __init__(self):
        self.calls = []

    def __call__(self, mel):
        self.calls.append((mel.size(0), mel.size(2)))
        k = torch.arange(cases.CHUNK_HOP, device=mel.device)
        j = (k.float() + 1.0) * 0.125
        sign = torch.where(k % 2 == 0, 1.0, -1.0)
        w = mel[:, 0][:, :, None] * j[None, None, :] + mel[:, 1][:, :, None] * sign[None, None, :]
        return w.reshape(mel.size(0), 1, -1).contiguous()


def fake_wave(content, S):
    """numpy: content (Tin, Dc) float32 -> the S * hop samples FakeLR -> long_batch_cases.BatchedFakeCFM -> FakeVocoder give for it."""
    content = np.asarray(content, np.float32)
    m = (content[(np.arange(S) * content.shape[0]) // S] * np.float32(0.5)).T                      # (Dc, S)
    mel = [m[c] * np.float32(0.5) + m[c + 1] * np.float32(c + 1) * np.float32(0.25) for c in range(2)]
    j = (np.arange(cases.CHUNK_HOP, dtype=np.float32) + np.float32(1.0)) * np.float32(0.125)
    sign = np.where(np.arange(cases.CHUNK_HOP) % 2 == 0, np.float32(1.0), np.float32(-1.0))
    return (mel[0][:, None] * j[None, :] + mel[1][:, None] * sign[None, :]).reshape(-1)


def planted_session(stream, n_steps=5):
    """Content of `n_steps` consecutive steps of fake stream `stream`: windows of S frames of one long random sequence, the
    window of step k + 1 starting FAKE_ADVANCES[stream][k] frames after that of step k.  -> list of (S, Dc) float32 arrays."""
    S = FAKE_GEOMETRY["S"]
    adv = FAKE_ADVANCES[stream][:n_steps - 1]
    seq = cases.randn(f"rt.session{stream}", 141, sum(adv) + S, cases.CHUNK_DC).numpy()
    first = np.concatenate([[0], np.cumsum(adv)]).astype(int)
    return [seq[f:f + S].copy() for f in first]


def session_model(contents, fade_in, fade_out, g=FAKE_GEOMETRY):
    """The numpy session: the fake chain and `sola_model` step by step from a zero buffer.
    -> list of (out, buffer after the step, offset, scores, buffer before the step)."""
    S, hop, block, Lb, Ls, tail = (g[k] for k in ("S", "hop", "block", "sola_buffer", "sola_search", "tail"))
    n_inf = block + Lb + Ls
    start = S * hop - tail - n_inf
    buf, steps = np.zeros(Lb, np.float32), []
    for c in contents:
        infer = fake_wave(c, S)[start:start + n_inf]
        out, new, o, scores = sola_model(infer, buf, fade_in, fade_out, block, Ls)
        steps.append((out, new, o, scores, buf))
        buf = new
    return steps
