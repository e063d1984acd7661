"""Host-side mirror of the log-mel front-end over the C ABI (first half).

`MelSpectrogram(**mel_fn_args)(y)` has the call surface of `to_mel = lambda x: mel_spectrogram(x, **mel_fn_args)`
(inference.py:315-327, modules/audio.py:45-82): y (B, L) in [-1, 1] -> (B, num_mels, frames).
The mel filterbank is `librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)` in the reference; pass the reference's own
cached tensor as `mel_basis=` when it is available, otherwise `slaney_mel_basis` restates librosa's default
(Slaney scale, area normalisation) -- parity of that restatement is unpinned (librosa is absent from the build image).

`Resample(orig_freq, new_freq)(x)` is `torchaudio.functional.resample(x, orig_freq, new_freq)` with its defaults, the step the
drivers run in front of every 16 kHz model (inference.py:380-406): the filter is built here in float64 (`sinc_resample_taps`) and
the library runs it as a polyphase dot product (`svc_resample`).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib


def slaney_mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel defaults (htk=False, norm='slaney'), float32 [n_mels][n_fft // 2 + 1]."""
    return torch.from_numpy(_slaney_weights(sr, n_fft, n_mels, fmin, fmax).astype(np.float32))


def whisper_mel_basis(n_mels=80):
    """The filterbank of `WhisperFeatureExtractor` (16 kHz, n_fft 400, 0 .. 8000 Hz, Slaney scale, Slaney normalisation:
    `transformers.audio_utils.mel_filter_bank(201, n_mels, 0, 8000, 16000, "slaney", "slaney")` transposed), float64
    [n_mels][201].  Pinned to that function by the host tests."""
    return torch.from_numpy(_slaney_weights(16000, 400, n_mels, 0.0, 8000.0))


def _slaney_weights(sr, n_fft, n_mels, fmin, fmax):
    fmax = sr / 2.0 if fmax in (None, "None") else float(fmax)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0

    def hz_to_mel(f):
        f = np.asarray(f, dtype=np.float64)
        return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-12) / min_log_hz) / logstep, f / f_sp)

    def mel_to_hz(m):
        m = np.asarray(m, dtype=np.float64)
        return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)

    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w


def htk_mel_basis(sr, n_fft, n_mels, fmin=0.0, fmax=None):
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=True) with its default Slaney area normalisation, float32
    [n_mels][n_fft // 2 + 1]: triangles on the HTK scale mel = 2595 log10(1 + f / 700), each scaled by 2 / (its width in Hz).
    RMVPE's basis (16 kHz, 1024, 128, 30, 8000).  Unpinned like `slaney_mel_basis`: librosa is absent from the build image."""
    fmax = sr / 2.0 if fmax in (None, "None") else float(fmax)

    def hz_to_mel(f):
        return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)

    def mel_to_hz(m):
        return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)

    fftfreqs = np.linspace(0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, 1 + n_fft // 2))
    for i in range(n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return torch.from_numpy(w.astype(np.float32))


class MelSpectrogram:
    def __init__(self, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin=0, fmax=None, center=False, mel_basis=None,
                 device="cuda:0"):
        assert not center, "the reference drivers call mel_spectrogram with center=False"
        self.device = torch.device(device)
        self.n_fft, self.hop, self.n_mels = int(n_fft), int(hop_size), int(num_mels)
        if mel_basis is None:
            mel_basis = slaney_mel_basis(sampling_rate, n_fft, num_mels, fmin, fmax)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            win = torch.hann_window(int(win_size)).to(self.device)
            mb = _lib.f32c(mel_basis, self.device)
            _lib.check(_lib.lib().svc_mel_create(self.n_fft, self.hop, int(win_size), self.n_mels, _lib.ptr(win), _lib.ptr(mb),
                                                 _lib.stream_ptr(), C.byref(self._h)))

    @torch.inference_mode()
    def __call__(self, y, lens=None, pad_value=0.0):
        """y (B, L) -> (B, n_mels, frames).  lens (B host integers): a batch of clips of different lengths in one call
        (`svc_mel_forward_ragged`): row b's first lens[b] // hop frames are the log-mel of y[b, :lens[b]] run alone (samples above
        its end are never read); the frames above are pad_value."""
        with torch.cuda.device(self.device):
            yy = _lib.f32c(y, self.device)
            B, L = yy.shape
            frames = 1 + (L - self.hop) // self.hop
            out = torch.empty(B, self.n_mels, frames, device=self.device)
            if lens is None:
                _lib.check(_lib.lib().svc_mel_forward(self._h, _lib.ptr(yy), B, L, _lib.ptr(out), _lib.stream_ptr()))
            else:
                lens = _lib.int_list(lens)
                if len(lens) != B:
                    raise ValueError(f"MelSpectrogram: {len(lens)} lens for a batch of {B}")
                _lib.check(_lib.lib().svc_mel_forward_ragged(self._h, _lib.ptr(yy), _lib.i32_host(lens), B, L, float(pad_value),
                                                             _lib.ptr(out), _lib.stream_ptr()))
        return out

    def __del__(self):
        try:
            if self._h:
                _lib.lib().svc_mel_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


# ----------------------------------------------------------------------------------------- sample-rate conversion
def _sinc_resample_kernel(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """torchaudio's `_get_sinc_resample_kernel` with its defaults (sinc_interp_hann), restated: float64 throughout, cast to
    float32 at the end.  -> (o, n, width, K float32 [n][2 width + o])."""
    g = math.gcd(int(orig), int(new))
    o, n = int(orig) // g, int(new) // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64) / o
    t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx[None, :]) * base
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    win = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    K = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * win * (base / o)
    return o, n, width, K.to(torch.float32)


def sinc_resample_taps(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """The non-zero part of torchaudio's resampling kernel, for `svc_resampler_create`: -> (o, n, width, first int32 [n], taps
    float32 [n][ntaps]).  In float32 the dense kernel K [n][2 width + o] is exactly 0.0 outside one contiguous run per phase (the
    Hann window reaches zero where the argument is clamped); first[j] is the column where phase j's run starts, taps[j] the run,
    padded with 0.0 at the end up to the longest one.  The values are K's, bit for bit."""
    o, n, width, K = _sinc_resample_kernel(orig, new, lowpass_filter_width, rolloff)
    nz = K != 0
    count = nz.sum(dim=1)
    first = nz.to(torch.int32).argmax(dim=1)
    last = K.size(1) - 1 - nz.flip(1).to(torch.int32).argmax(dim=1)
    assert bool((count > 0).all()) and bool((last - first + 1 == count).all()), "a phase's non-zero taps are not contiguous"
    ntaps = int(count.max())
    cols = first[:, None] + torch.arange(ntaps)[None, :]
    taps = torch.where(cols < K.size(1), K.gather(1, cols.clamp(max=K.size(1) - 1)), torch.zeros(()))
    return o, n, width, first.to(torch.int32), taps.contiguous()


class Resample:
    """`torchaudio.transforms.Resample(orig_freq, new_freq)` (sinc_interp_hann) on the device: `svc_resample`."""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, device="cuda:0"):
        self.device = torch.device(device)
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        g = math.gcd(self.orig_freq, self.new_freq)
        self.o, self.n = self.orig_freq // g, self.new_freq // g
        self._h = C.c_void_p()
        self.tile = 0
        if self.o == self.n:
            return
        o, n, width, first, taps = sinc_resample_taps(orig_freq, new_freq, lowpass_filter_width, rolloff)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().svc_resampler_create(o, n, width, taps.size(1), _lib.i32_host(first.tolist()),
                                                       (C.c_float * taps.numel())(*taps.flatten().tolist()), _lib.stream_ptr(),
                                                       C.byref(self._h)))
        self.tile = int(_lib.lib().svc_resampler_tile(self._h))           # outputs one workgroup owns

    def out_len(self, L):
        """Samples at the new rate for L at the old one: ceil(n L / o)."""
        return -((-self.n * int(L)) // self.o)

    @torch.inference_mode()
    def __call__(self, x, lens=None):
        """x (B, L) or (L,) -> (B, out_len(L)).  lens (B host integers): clips of different lengths in one call -> (out, out_lens);
        row b's first out_len(lens[b]) samples are those of x[b, :lens[b]] run alone, bit for bit, the samples above are 0.0 and
        nothing at or above lens[b] is read as a value.  Equal rates return a copy.  Nothing is synchronised."""
        with torch.cuda.device(self.device):
            xx = _lib.f32c(x, self.device)
            if xx.dim() == 1:
                xx = xx[None, :]
            B, L = xx.shape
            if lens is not None:
                lens = _lib.int_list(lens)
                if len(lens) != B:
                    raise ValueError(f"Resample: {len(lens)} lens for a batch of {B}")
            if self.o == self.n:
                out = xx.clone()
            else:
                out = torch.empty(B, self.out_len(L), device=self.device)
                _lib.check(_lib.lib().svc_resample(self._h, _lib.ptr(xx), _lib.i32_host(lens) if lens is not None else None, B, L,
                                                   _lib.ptr(out), out.size(1), _lib.stream_ptr()))
        return out if lens is None else (out, [self.out_len(v) for v in lens])

    def __del__(self):
        try:
            if self._h:
                _lib.lib().svc_resampler_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass
