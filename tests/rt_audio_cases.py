"""Models shared by the audio-in tests of real-time sessions (test_host_rt_audio.py, test_gpu_rt_audio.py).

`push_model` is the numpy statement of one `svc_rt_push` for one stream as include/seedvc_hip.h states it, with its resampled
samples from `resample_cases.resample_dense` (float64): the device differs from it by its fp32 accumulation only, bounded by
`resample_cases.fp32_bound` (`push_bound` carries that bound along with the samples as they move through the context).
`gui_push_torch` is a transcription of the reference GUI's four lines (real-time-gui.py, `audio_callback`, from memory) with
the whole `input_wav` ring and torchaudio's dense-kernel resampler; the host test holds the model to it.

`push_model_fp32` is the same push with the device's own arithmetic emulated in numpy: per output one chain of correctly
rounded float32 FMAs over the taps in ascending order (`fma32`), so a whole engine session can be stated in numpy bit for bit.
`supported` tells which samples of a context equal the one-shot conversion of the whole stream."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import cases
import resample_cases as RC

PAIRS = [(250, 150), (22050, 16000), (44100, 16000), (48000, 16000)]      # zc / z16: 5 / 3, 441 / 320, 882 / 320, 960 / 320


def units(orig, new):
    """(zc, z16, o, n): samples per 20 ms at the two rates, as `pipeline.realtime_input_geometry` states them, and the reduced
    rates."""
    from seedvc_amd.pipeline import realtime_input_geometry
    geo = realtime_input_geometry(orig, 0.02, 0.0, 0.0, 0.0, content_rate=new)
    g = math.gcd(orig, new)
    return geo["zc"], geo["z16"], orig // g, new // g


def taps_of(orig, new):
    """(o, n, width, first int64 [n], taps float32 [n][ntaps]) as the library is given them."""
    from seedvc_amd.audio import sinc_resample_taps
    o, n, width, first, taps = sinc_resample_taps(orig, new)
    return o, n, width, first.numpy().astype(np.int64), taps.numpy()


# ------------------------------------------------------------------------------------------------------ the float64 model
def _sizes(Lin, zc, z16, L16):
    assert Lin >= zc and Lin % zc == 0
    m = Lin // zc
    shift, n_new = m * z16, (m + 1) * z16
    assert L16 >= n_new
    return shift, n_new


def push_model(hist, ring, block, orig, new, zc, z16):
    """hist (2 zc,) float32, ring (L16,) float32 | float64, block (Lin,) float32 -> (new ring (L16,) float64, new hist (2 zc,)
    float32).  The kept samples are the old ring's values, the last n_new are `resample_dense` of hist ‖ block (the samples
    themselves where the rates are equal)."""
    hist, block = np.asarray(hist, np.float32), np.asarray(block, np.float32)
    ring = np.asarray(ring, np.float64)
    L16 = len(ring)
    shift, n_new = _sizes(len(block), zc, z16, L16)
    x = np.concatenate([hist, block])
    assert len(hist) == 2 * zc
    y = x.astype(np.float64) if orig == new else RC.resample_dense(orig, new, torch.from_numpy(x)[None])[0].numpy()
    assert len(y) >= z16 + n_new
    return np.concatenate([ring[shift:L16 - z16], y[z16:z16 + n_new]]), x[-2 * zc:].copy()


def push_bound(hist, bound, block, orig, new, zc, z16):
    """The fp32 bound of every sample of the new ring: the kept samples carry theirs along, the new ones get
    `resample_cases.fp32_bound` of hist ‖ block (0 where the rates are equal: copies).  bound (L16,) float64 -> (L16,) float64."""
    bound = np.asarray(bound, np.float64)
    L16 = len(bound)
    shift, n_new = _sizes(len(block), zc, z16, L16)
    x = np.concatenate([np.asarray(hist, np.float32), np.asarray(block, np.float32)])
    if orig == new:
        b = np.zeros(len(x))
    else:
        ntaps = taps_of(orig, new)[4].shape[1]
        b = RC.fp32_bound(orig, new, torch.from_numpy(x)[None], ntaps)[0].numpy()
    return np.concatenate([bound[shift:L16 - z16], b[z16:z16 + n_new]])


def torchaudio_resample(K32, o, n, width, x):
    """torchaudio.functional.resample's `_apply_sinc_resample_kernel` on a float32 signal x (L,), restated: pad (width, width + o),
    conv1d with the dense kernel at stride o, interleave the phases, the first ceil(n L / o) samples."""
    y = F.conv1d(F.pad(x[None, None, :], (width, width + o)), K32[:, None, :], stride=o)
    return y.transpose(1, 2).reshape(-1)[:RC.out_len(o, n, x.numel())]


def gui_push_torch(input_wav, input_wav_res, indata, orig, new):
    """The GUI's lines on torch CPU tensors (float32), in place: `input_wav` is the whole stream-rate ring."""
    zc, z16, o, n = units(orig, new)
    _, _, width, K32 = RC.dense_kernel(orig, new)
    Lin = indata.numel()
    m = Lin // zc
    input_wav[:-Lin] = input_wav[Lin:].clone()
    input_wav[-Lin:] = indata
    input_wav_res[:-m * z16] = input_wav_res[m * z16:].clone()
    input_wav_res[-z16 * (m + 1):] = torchaudio_resample(K32, o, n, width, input_wav[-Lin - 2 * zc:])[z16:]


# ------------------------------------------------------------------------------------------- the device's own arithmetic
def fma32(a, b, c):
    """Correctly rounded float32 fma(a, b, c) of float32 arrays.  a * b is exact in float64 (48 bits); s = p + c in float64 with
    its exact error e (TwoSum); float32(s) is the answer unless s lies exactly half way between two float32 values while the true
    sum does not, the one case where rounding twice differs from rounding once: then e decides."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.where(r64 > s, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))).astype(np.float64)
    tie = (r64 != s) & (np.abs(s - r64) == np.abs(other - s)) & (e != 0) & np.isfinite(s)
    toward_other = tie & (np.sign(e) == np.sign(other - r64))
    return np.where(toward_other, other, r64).astype(np.float32)


def resample_fp32(orig, new, x):
    """x (L,) float32 -> (ceil(n L / o),) float32: `svc_resample` in numpy, out[i n + j] = one FMA chain over k ascending of
    taps[j][k] * xx[i o + first[j] + k - width], xx = x inside [0, L) and 0.0 outside."""
    x = np.asarray(x, np.float32)
    if orig == new:
        return x.copy()
    o, n, width, first, taps = taps_of(orig, new)
    ntaps = taps.shape[1]
    nout = RC.out_len(o, n, len(x))
    mm = np.arange(nout)
    i, j = mm // n, mm % n
    pad = width + ntaps + o
    xx = np.concatenate([np.zeros(width, np.float32), x, np.zeros(pad, np.float32)])       # xx[p + width] = x[p]
    base = i * o + first[j]
    acc = np.zeros(nout, np.float32)
    for k in range(ntaps):
        acc = fma32(taps[j, k], xx[base + k], acc)
    return acc


def push_model_fp32(hist, ring, block, orig, new, zc, z16):
    """`push_model` with `resample_fp32` for the new samples: float32 in, float32 out, the device's bits."""
    hist, ring, block = (np.asarray(v, np.float32) for v in (hist, ring, block))
    L16 = len(ring)
    shift, n_new = _sizes(len(block), zc, z16, L16)
    x = np.concatenate([hist, block])
    y = resample_fp32(orig, new, x)
    return np.concatenate([ring[shift:L16 - z16], y[z16:z16 + n_new]]), x[-2 * zc:].copy()


# ------------------------------------------------------------------------------------------------ streamed against one-shot
def supported(orig, new, Lin, L16, pushes):
    """The context of a stream after `pushes` blocks of Lin samples from an empty state against the one-shot conversion Y of the
    whole stream (any length >= pushes * Lin).  -> (M int64 [L16], ok bool [L16]): ring[i] sits at Y[M[i]] (M < 0: before the
    stream began), and ok[i] says that every tap of that sample lay inside x = hist ‖ block of the push that computed it last --
    push b' = min(pushes - 1, (M + z16) // shift), whose x covers the stream's samples [b' Lin - 2 zc, (b' + 1) Lin) -- or on the
    zeros before the stream's start, which are the one-shot padding too.  Where ok, the two FMA chains have the same terms."""
    zc, z16, o, n = units(orig, new)
    shift = (Lin // zc) * z16
    M = pushes * shift - L16 + np.arange(L16)
    if orig == new:
        return M, M >= 0
    _, _, width, first, taps = taps_of(orig, new)
    ntaps = taps.shape[1]
    Mc = np.maximum(M, 0)
    b = np.minimum(pushes - 1, (Mc + z16) // shift)
    lo = (Mc // n) * o + first[Mc % n] - width                   # the first and the last sample a tap reads
    hi = lo + ntaps - 1
    ok = (M >= 0) & (hi < (b + 1) * Lin) & ((lo >= b * Lin - 2 * zc) | (b * Lin - 2 * zc <= 0))
    return M, ok


def excluded_cap(orig, new):
    """ceil((width + 1) n / o) + 1: the most samples at the end of a context that the next block still changes (their right
    context was padding); where width <= zc nothing else is excluded."""
    o, n, width, _ = RC.dense_kernel(orig, new)
    return -((-(width + 1) * n) // o) + 1


# ------------------------------------------------------------------------------------------------------- ring layout
def ring_planes(ring, max_slots, L16):
    """The flat float32 `ring` buffer of `svc_rt_push` (numpy) -> (planes float32 [2][max_slots][L16], tickets uint64 [max_slots])."""
    ring = np.ascontiguousarray(ring, np.float32)
    k = 2 * max_slots * L16
    assert ring.size == k + 2 * max_slots
    return ring[:k].reshape(2, max_slots, L16), ring[k:].view(np.uint64)


def current_plane(tickets, tiles):
    """Per slot, the plane that holds its context: (tickets / svc_rt_push_tiles(L16)) & 1."""
    return ((np.asarray(tickets, np.uint64) // np.uint64(tiles)) & np.uint64(1)).astype(np.int64)


# ------------------------------------------------------------------------------------------------------- stand-ins
class FakeContent:
    """Stand-in content encoder: (n, L16) samples -> (n, L16 // 320, CHUNK_DC); row t, channel d = frame[t][5 d] - 0.25 *
    frame[t][5 d + 2] of the 320-sample frames (an exact product and one rounded fp32 subtraction)."""

    def semantic_fn(self, waves_16k):
        n, L = waves_16k.shape
        fr = waves_16k[:, :L // 320 * 320].reshape(n, L // 320, 320)
        d = torch.arange(cases.CHUNK_DC, device=waves_16k.device) * 5
        return fr[:, :, d] - fr[:, :, d + 2] * 0.25


def fake_content(ctx):
    """numpy: ctx (L16,) float32 -> (L16 // 320, CHUNK_DC) float32, what `FakeContent` gives."""
    ctx = np.asarray(ctx, np.float32)
    fr = ctx[:len(ctx) // 320 * 320].reshape(-1, 320)
    d = np.arange(cases.CHUNK_DC) * 5
    return fr[:, d] - fr[:, d + 2] * np.float32(0.25)
