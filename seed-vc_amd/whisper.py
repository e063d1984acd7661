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
from .content import SAMPLES_PER_ROW, ContentEncoder, window_plan      # noqa: F401  (window_plan is re-exported)


class WhisperContent(ContentEncoder):
    ABI, STAGES = "whisper", ("mel", "stem", "layers", "assemble")

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

    def rows(self, n_samples, overlap_rows=250):
        """content rows of a clip of n_samples (the window plan's kept rows)"""
        r = _lib.lib().svc_whisper_rows(self.P, int(overlap_rows), int(n_samples))
        _lib.check(int(r < 0))
        return r

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
