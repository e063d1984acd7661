"""Host-side mirror of the Whisper content encoder over the C ABI (csrc/whisper.hip).

`WhisperContent(state_dict).semantic_fn(waves_16k)` has the drivers' closure signature: (1, L <= 480 000) samples at 16 kHz in,
(1, L // 320 + 1, 768) content features out (`whisper_feature_extractor` + `whisper_model.encoder` + the crop).
`content_batch` is the same for up to 64 clips of any length in one call, with the drivers' loop over 30 s windows (5 s
overlap) done on the device; `mel` and `encode` expose the two stages.  The state dict is `WhisperEncoder.state_dict()`
(`WhisperModel.state_dict()` loads unchanged: the `encoder.` prefix is accepted and decoder keys are ignored).
"""
import ctypes as C

import torch

from . import _lib, specs
from .audio import whisper_mel_basis

SAMPLES_PER_ROW = 320       # hop 160, conv2 stride 2


def window_plan(L, W, O):
    """The drivers' windows of a clip of L samples, window W and overlap O samples: a list of (start, samples, first_kept_row,
    rows) per window; window 0 always exists, window j >= 1 iff W + (j - 1)(W - O) < L; a window of n samples has
    min(W // 320, n // 320 + 1) rows, of which every window but the first drops O // 320."""
    L, W, O = int(L), int(W), int(O)
    if L < 1 or W < SAMPLES_PER_ROW or not 0 <= O < W or W % SAMPLES_PER_ROW or O % SAMPLES_PER_ROW:
        raise ValueError("window_plan: L >= 1, W and O multiples of 320 samples, 0 <= O < W")
    plan, j = [], 0
    while j == 0 or W + (j - 1) * (W - O) < L:
        start = j * (W - O)
        n = min(W, L - start)
        plan.append((start, n, O // SAMPLES_PER_ROW if j else 0, min(W // SAMPLES_PER_ROW, n // SAMPLES_PER_ROW + 1)))
        j += 1
    return plan


class WhisperContent:
    SR = 16000

    def __init__(self, state_dict, cfg=None, mel_basis=None, device="cuda:0", precision=1):
        self.cfg = specs.whisper_config() if cfg is None else cfg
        self.device = torch.device(device)
        self.P, self.D = int(self.cfg["max_source_positions"]), int(self.cfg["d_model"])
        self.W = self.P * SAMPLES_PER_ROW
        if mel_basis is None:
            mel_basis = whisper_mel_basis(self.cfg["n_mels"])
        c = _lib.WhisperConfig()
        for k in ("n_mels", "d_model", "n_heads", "n_layers", "ffn_dim", "max_source_positions"):
            setattr(c, k, int(self.cfg[k]))
        c.precision = int(precision)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            mb = _lib.f32c(mel_basis, self.device)
            if tuple(mb.shape) != (self.cfg["n_mels"], 201):
                raise ValueError(f"WhisperContent: mel_basis must be ({self.cfg['n_mels']}, 201), got {tuple(mb.shape)}")
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            _lib.check(_lib.lib().svc_whisper_create(C.byref(c), descs, n, _lib.ptr(mb), _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep

    def eval(self):
        return self

    def rows(self, n_samples, overlap_rows=250):
        """content rows of a clip of n_samples (the window plan's kept rows)"""
        r = _lib.lib().svc_whisper_rows(self.P, int(overlap_rows), int(n_samples))
        _lib.check(int(r < 0))
        return r

    def set_window_group(self, windows):
        """Windows computed side by side (0 = the default): bounds the workspace; results do not depend on it."""
        _lib.check(_lib.lib().svc_whisper_set_window_group(self._h, int(windows)))

    def set_timing(self, on):
        """Measurement aid: record HIP events around the stages of `content_batch` (see `last_timing`)."""
        _lib.check(_lib.lib().svc_whisper_set_timing(self._h, int(bool(on))))

    def last_timing(self):
        """dict of milliseconds of the last window group of the last `content_batch` (synchronises)."""
        ms = (C.c_float * 4)()
        _lib.check(_lib.lib().svc_whisper_last_timing(self._h, ms))
        return dict(zip(("mel", "stem", "layers", "assemble"), [float(v) for v in ms]))

    @staticmethod
    def _lens(lens, B):
        lens = _lib.int_list(lens)
        if len(lens) != B:
            raise ValueError(f"WhisperContent: {len(lens)} lens for a batch of {B}")
        return lens

    @torch.inference_mode()
    def mel(self, waves, lens):
        """waves (B, L) at 16 kHz, lens B host integers in 1 .. min(L, W) -> (B, n_mels, 2 P): each clip as one zero-padded window."""
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves, self.device)
            B, L = w.shape
            out = torch.empty(B, self.cfg["n_mels"], 2 * self.P, device=self.device)
            _lib.check(_lib.lib().svc_whisper_mel(self._h, _lib.ptr(w), _lib.i32_host(self._lens(lens, B)), B, L, _lib.ptr(out),
                                                  _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def encode(self, feats):
        """feats (B, n_mels, 2 P) -> (B, P, D): the encoder alone."""
        with torch.cuda.device(self.device):
            f = _lib.f32c(feats, self.device)
            if f.dim() != 3 or tuple(f.shape[1:]) != (self.cfg["n_mels"], 2 * self.P):
                raise ValueError(f"WhisperContent.encode: feats must be (B, {self.cfg['n_mels']}, {2 * self.P}), got {tuple(f.shape)}")
            out = torch.empty(f.shape[0], self.P, self.D, device=self.device)
            _lib.check(_lib.lib().svc_whisper_encode(self._h, _lib.ptr(f), f.shape[0], _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def content_batch(self, waves, lens=None, overlap_s=5.0):
        """waves (B, L) at 16 kHz (B <= 64), lens B host integers or None -> (S (B, Rmax, D) on the device, rows [B]): row b holds
        the rows[b] content rows of waves[b, :lens[b]] as the drivers' window loop gives them, zeros above.  Nothing is synchronised."""
        ov = int(round(float(overlap_s) * self.SR)) // SAMPLES_PER_ROW
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves, self.device)
            B, L = w.shape
            lens = [L] * B if lens is None else self._lens(lens, B)
            rows = [self.rows(n, ov) for n in lens]
            out = torch.empty(B, max(rows), self.D, device=self.device)
            _lib.check(_lib.lib().svc_whisper_content(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, ov, _lib.ptr(out), max(rows),
                                                      _lib.stream_ptr()))
        return out, rows

    def semantic_fn(self, waves_16k):
        """The drivers' closure: (1, L <= W) -> (1, L // 320 + 1, D)."""
        w = torch.as_tensor(waves_16k, dtype=torch.float32)
        if w.dim() != 2 or w.size(1) > self.W:
            raise ValueError(f"WhisperContent.semantic_fn: (B, L <= {self.W}) samples, got {tuple(w.shape)}")
        return self.content_batch(w, None, overlap_s=0.0)[0]

    def close(self):
        if self._h:
            _lib.lib().svc_whisper_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
