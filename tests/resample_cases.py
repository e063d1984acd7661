"""Rate pairs, inputs and the yardstick shared by the resampler tests (test_host_resample.py, test_gpu_resample.py).

The yardstick is torchaudio's `resample` with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), restated
from memory (torchaudio is absent from the build image): the dense kernel K [n][2 width + o] in float64 cast to float32, the
signal padded by (width, width + o) zeros, `F.conv1d(stride=o)`, the first ceil(n L / o) samples.  `resample_dense` runs it with
the float32 K and the signal both promoted to float64, so the device differs from it by its fp32 accumulation only.  Padding
samples of ragged batches are NaN: a read of one as a value shows up as a non-finite output."""
import math

import torch
import torch.nn.functional as F

import cases

# (orig, new): o / n, width, ntaps -- the longest run of non-zero float32 entries of a phase of K
TABLE = {
    (22050, 16000): (441, 320, 9, 17),
    (44100, 16000): (441, 160, 17, 34),
    (48000, 16000): (3, 1, 19, 37),
    (24000, 16000): (3, 2, 10, 19),
    (22050, 48000): (147, 320, 7, 13),
    (16000, 22050): (320, 441, 7, 13),
}
GPU_PAIRS = [(22050, 16000), (44100, 16000), (24000, 16000), (22050, 48000), (16000, 22050)]
SINE_PAIRS = [(22050, 16000), (44100, 16000), (48000, 16000), (22050, 44100), (22050, 48000), (16000, 22050)]
NAN = float("nan")
_dense = {}


def dense_kernel(orig, new, lpw=6, rolloff=0.99):
    """-> (o, n, width, K float32 [n][2 width + o]), computed once per pair."""
    key = (orig, new, lpw, rolloff)
    if key not in _dense:
        g = math.gcd(orig, new)
        o, n = orig // g, new // g
        base = min(o, n) * rolloff
        width = math.ceil(lpw * o / base)
        idx = torch.arange(-width, width + o, dtype=torch.float64) / o
        t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx[None, :]) * base
        t = t.clamp(-lpw, lpw)
        win = torch.cos(t * math.pi / lpw / 2) ** 2
        t = t * math.pi
        K = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * win * (base / o)
        _dense[key] = (o, n, width, K.to(torch.float32))
    return _dense[key]


def out_len(o, n, L):
    return -((-n * L) // o)


def _conv(K64, x64, o, width):
    y = F.pad(x64, (width, width + o))
    out = F.conv1d(y[:, None, :], K64[:, None, :], stride=o)            # (B, n, periods)
    return out.transpose(1, 2).reshape(x64.size(0), -1)


def resample_dense(orig, new, x):
    """x (B, L) -> float64 (B, ceil(n L / o)): the dense statement, float32 K and x promoted to float64."""
    o, n, width, K32 = dense_kernel(orig, new)
    return _conv(K32.double(), x.double(), o, width)[:, :out_len(o, n, x.size(1))]


def fp32_bound(orig, new, x, ntaps):
    """Per output, (ntaps + 2) 2^-24 sum_k |K[j][k]| |x_k|: the textbook bound of an fp32 dot product of ntaps terms (each
    product and each partial sum rounded once: gamma_ntaps <= ntaps u / (1 - ntaps u), with FMA one rounding fewer per term), plus
    one unit for the comparison with the float64 sum.  float64 (B, ceil(n L / o))."""
    o, n, width, K32 = dense_kernel(orig, new)
    s = _conv(K32.double().abs(), x.double().abs(), o, width)[:, :out_len(o, n, x.size(1))]
    return (ntaps + 2) * 2.0 ** -24 * s


def noise(tag, seed, *shape):
    """Uniform noise in [-1, 1], float32."""
    return cases.rand("resample." + tag, seed, *shape) * 2.0 - 1.0


def ragged_batch(x, lens):
    """Row b = x[b, :lens[b]], NaN above."""
    y = torch.full((len(lens), max(lens)), NAN)
    for b, n in enumerate(lens):
        y[b, :n] = x[b, :n]
    return y
