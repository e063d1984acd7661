"""Host-side mirror of the wav2vec 2.0 content encoder over the C ABI (csrc/wav2vec2.hip).

`Wav2Vec2Content(state_dict).semantic_fn(waves_16k)` has the drivers' closure signature for the xlsr models: (1, L <= 480 000)
samples at 16 kHz in, (1, frames(L), 1024) content features out (`Wav2Vec2FeatureExtractor` + the first 12 layers of
facebook/wav2vec2-xls-r-300m + `encoder.layer_norm`).  `content_batch` is the same for up to 64 clips of any length in one call,
with the drivers' loop over 30 s windows (5 s overlap) done on the device; `normalize`, `features`, `posconv` and `encode` expose
the stages.  The state dict is `Wav2Vec2Model.state_dict()`; `HubertModel.state_dict()` of the same shape loads unchanged.

A cfg of the base family (`specs.wav2vec2_base_config()`: facebook/hubert-base-ls960, facebook/wav2vec2-base and their fine-tunes:
feat_extract_norm "group", do_stable_layer_norm False, 768 / 16 = 48 channels per positional-conv group) or one that names
`do_normalize` is created through svc_w2v_create_ex; everything else here serves both families.
"""
import ctypes as C

import torch

from . import _lib, specs
from .content import SAMPLES_PER_ROW, ContentEncoder, window_plan as _window_plan


def c_config(cfg, precision=1):
    """cfg dict (specs.wav2vec2_config) -> _lib.W2vConfig"""
    c = _lib.W2vConfig()
    ks, ss = [int(v) for v in cfg["conv_kernel"]], [int(v) for v in cfg["conv_stride"]]
    if len(ks) != len(ss) or not 2 <= len(ks) <= 8:
        raise ValueError("wav2vec2: conv_kernel and conv_stride must have the same 2 .. 8 entries")
    c.conv_dim, c.n_conv = int(cfg["conv_dim"]), len(ks)
    for i, (k, s) in enumerate(zip(ks, ss)):
        c.conv_kernel[i], c.conv_stride[i] = k, s
    for k in ("d_model", "n_heads", "n_layers", "ffn_dim", "pos_k", "pos_groups", "window_samples"):
        setattr(c, k, int(cfg[k]))
    c.feat_extract_norm_layer = int(cfg.get("feat_extract_norm", "layer") == "layer")
    c.do_stable_layer_norm = int(bool(cfg.get("do_stable_layer_norm", True)))
    c.conv_bias = int(bool(cfg.get("conv_bias", True)))
    c.precision = int(precision)
    return c


def c_ext(cfg):
    """The second argument of svc_w2v_create_ex for a cfg of the base family (group-norm extractor, post-LN encoder) or one that names
    `do_normalize`; None for every other cfg, which goes through svc_w2v_create as it always did."""
    if not (specs.wav2vec2_is_base(cfg) or "do_normalize" in cfg):
        return None
    e = _lib.W2vExt()
    e.do_normalize = int(bool(cfg.get("do_normalize", True)))
    e.feat_proj_layer_norm = int(bool(cfg.get("feat_proj_layer_norm", True)))
    return e


def frames(cfg, n):
    """rows the extractor yields for n samples in one piece: (n - k) // s + 1 through every conv"""
    n = int(n)
    for k, s in zip(cfg["conv_kernel"], cfg["conv_stride"]):
        n = (n - k) // s + 1 if n >= k else 0
    return n


def window_plan(cfg, L, overlap_rows):
    """The drivers' windows of a clip of L samples (content.window_plan: the loop is shared by all tokenizers) with this encoder's
    row rule: a list of (start, samples, first_kept_row, rows); a later window with rows <= first_kept_row contributes nothing."""
    return [(s, n, d, frames(cfg, n)) for s, n, d, _ in _window_plan(L, cfg["window_samples"], int(overlap_rows) * SAMPLES_PER_ROW)]


class Wav2Vec2Content(ContentEncoder):
    ABI, STAGES = "w2v", ("extractor", "posconv", "layers", "assemble")

    def __init__(self, state_dict, cfg=None, device="cuda:0", precision=1):
        self.cfg = specs.wav2vec2_config() if cfg is None else cfg
        self.device = torch.device(device)
        self.D, self.W = int(self.cfg["d_model"]), int(self.cfg["window_samples"])
        self._c = c_config(self.cfg, precision)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            ext = c_ext(self.cfg)
            if ext is None:
                _lib.check(_lib.lib().svc_w2v_create(C.byref(self._c), descs, n, _lib.stream_ptr(), C.byref(self._h)))
            else:
                _lib.check(_lib.lib().svc_w2v_create_ex(C.byref(self._c), C.byref(ext), descs, n, _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep

    def frames(self, n_samples):
        return frames(self.cfg, n_samples)

    def rows(self, n_samples, overlap_rows=250):
        """content rows of a clip of n_samples (the window plan's kept rows)"""
        r = _lib.lib().svc_w2v_rows(C.byref(self._c), int(overlap_rows), int(n_samples))
        _lib.check(int(r < 0))
        return r

    @torch.inference_mode()
    def normalize(self, waves, lens, out=None):
        """waves (B, L), lens B host integers in 1 .. L -> (B, L): samples below lens[b] zero-mean / unit-variance normalised; the
        others keep what `out` held (zeros when `out` is None)."""
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves, self.device)
            B, L = w.shape
            out = torch.zeros(B, L, device=self.device) if out is None else out
            _lib.check(_lib.lib().svc_w2v_normalize(self._h, _lib.ptr(w), _lib.i32_host(self._lens(lens, B)), B, L, _lib.ptr(out),
                                                    _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def features(self, waves_norm, lens, out=None):
        """normalised waves (B, L) -> (projected rows (B, Tmax, D), rows [B]); rows at and above a clip's count keep what `out` held."""
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves_norm, self.device)
            B, L = w.shape
            lens = self._lens(lens, B)
            rows = [self.frames(n) for n in lens]
            T = max(max(rows), 1) if out is None else out.size(1)
            out = torch.zeros(B, T, self.D, device=self.device) if out is None else out
            _lib.check(_lib.lib().svc_w2v_features(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, _lib.ptr(out), T, _lib.stream_ptr()))
        return out, rows

    def _rows_call(self, fn, h, rows, out):
        with torch.cuda.device(self.device):
            x = _lib.f32c(h, self.device)
            if x.dim() != 3 or x.size(2) != self.D:
                raise ValueError(f"Wav2Vec2Content: rows must be (B, T, {self.D}), got {tuple(x.shape)}")
            B, T, _ = x.shape
            out = torch.zeros_like(x) if out is None else out
            _lib.check(fn(self._h, _lib.ptr(x), _lib.i32_host(self._lens(rows, B)), B, T, _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def posconv(self, h, rows, out=None):
        """h (B, T, D), rows [B] -> h + gelu(pos_conv(h)) on each clip's own rows; the rows above keep what `out` held."""
        return self._rows_call(_lib.lib().svc_w2v_posconv, h, rows, out)

    @torch.inference_mode()
    def encode(self, h, rows, out=None):
        """projected rows (B, T, D), rows [B] -> (B, T, D): positional conv, the layers and encoder.layer_norm."""
        return self._rows_call(_lib.lib().svc_w2v_encode, h, rows, out)
