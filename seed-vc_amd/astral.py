"""Host-side mirror of the ASTRAL tokenizer over the C ABI (csrc/astral.hip): the content tokens of the v2 model.

`AstralTokenizer(hubert_state_dict, [wide_head_sd, narrow_head_sd]).tokens_batch(waves_16k, lens)` runs HuBERT-large once per
window (18 layers, no final LayerNorm) and every head (ConvNeXt V2 stage + binary spherical quantizer) on the same rows, for up to 64
clips of any length with the drivers' loop over 30 s windows (5 s overlap) done on the device.  `tokenize` has the reference's call
shape for one head, `ssl`, `convnext` and `logits` expose the stages, `reduce` is the duration reduction of the narrow tokens
(`torch.unique_consecutive` per clip).  A head's state dict uses the canonical key names of `specs.astral_head_state_spec`.
"""
import ctypes as C

import torch

from . import _lib, specs, wav2vec2
from .content import SAMPLES_PER_ROW, ContentEncoder, window_plan as _window_plan


def c_config(cfg, precision=1):
    """cfg dict (specs.astral_config) -> _lib.AstralConfig"""
    heads = cfg["heads"]
    if not 1 <= len(heads) <= 2:
        raise ValueError("astral: one or two heads")
    c = _lib.AstralConfig()
    c.ssl = wav2vec2.c_config(cfg["ssl"], precision)
    c.n_heads = len(heads)
    for k, h in enumerate(heads):
        for name in ("dim", "intermediate_dim", "n_blocks", "bits"):
            setattr(c.head[k], name, int(h[name]))
        c.head[k].dw_kernel = int(h.get("dw_kernel", 7))
    return c


def window_rows(cfg, n):
    """rows of a window of n samples: min(frames(n), n // 320) (the reference trims to attention_mask.sum() // 320)"""
    return min(wav2vec2.frames(cfg["ssl"], n), int(n) // SAMPLES_PER_ROW)


def window_plan(cfg, L, overlap_rows):
    """content.window_plan with this tokenizer's row rule: a list of (start, samples, first_kept_row, rows)"""
    return [(s, n, d, window_rows(cfg, n)) for s, n, d, _ in _window_plan(L, cfg["ssl"]["window_samples"], int(overlap_rows) * SAMPLES_PER_ROW)]


def bsq_index(z):
    """logits (..., bits) -> MSB-first index of the strictly positive ones (host formula of svc_op_bsq_index)"""
    bits = z.shape[-1]
    w = 2 ** torch.arange(bits - 1, -1, -1, dtype=torch.int64, device=z.device)
    return ((z > 0).to(torch.int64) * w).sum(-1)


class AstralTokenizer(ContentEncoder):
    ABI, STAGES = "astral", ("ssl", "convnext", "bsq", "assemble")

    def __init__(self, ssl_state_dict, head_state_dicts, cfg=None, device="cuda:0", precision=1):
        self.cfg = specs.astral_config() if cfg is None else cfg
        if len(head_state_dicts) != len(self.cfg["heads"]):
            raise ValueError(f"AstralTokenizer: {len(head_state_dicts)} head state dicts for {len(self.cfg['heads'])} heads")
        self.device = torch.device(device)
        self.n_heads = len(self.cfg["heads"])
        self.D, self.W = int(self.cfg["ssl"]["d_model"]), int(self.cfg["ssl"]["window_samples"])
        self._c = c_config(self.cfg, precision)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            descs, n, keep = _lib.make_descs(ssl_state_dict, self.device)
            heads = [_lib.make_descs(sd, self.device) for sd in head_state_dicts]
            hp = (C.c_void_p * self.n_heads)(*[C.cast(d, C.c_void_p) for d, _, _ in heads])
            hn = (C.c_int * self.n_heads)(*[k for _, k, _ in heads])
            _lib.check(_lib.lib().svc_astral_create(C.byref(self._c), descs, n, hp, hn, _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep, heads

    def content_batch(self, waves, lens=None, overlap_s=5.0):
        raise NotImplementedError("AstralTokenizer yields tokens, not features: use tokens_batch")

    def semantic_fn(self, waves_16k):
        raise NotImplementedError("AstralTokenizer yields tokens, not features: use tokenize (real-time sessions: tokens_fn)")

    def rows(self, n_samples, overlap_rows=250):
        """tokens of a clip of n_samples (the window plan's kept rows)"""
        r = _lib.lib().svc_astral_rows(C.byref(self._c), int(overlap_rows), int(n_samples))
        _lib.check(int(r < 0))
        return r

    def codebook_size(self, head=0):
        """ids of head `head` lie in [0, 2 ** bits)"""
        return 2 ** int(self.cfg["heads"][self._head(head, "codebook_size")]["bits"])

    def _head(self, head, what):
        k = int(head)
        if not 0 <= k < self.n_heads:
            raise ValueError(f"AstralTokenizer.{what}: head {head!r} outside [0, {self.n_heads})")
        return k

    @torch.inference_mode()
    def tokens_batch(self, waves, lens=None, overlap_s=5.0, reduce_head=None, heads=None):
        """waves (B, L) at 16 kHz (B <= 64), lens B host integers or None -> (tokens (n_heads, B, Rmax) int32 on the device, rows [B]):
        tokens[k, b, :rows[b]] are head k's indices of waves[b, :lens[b]] as the drivers' window loop gives them, -1 above.  With
        reduce_head = k also (reduced (B, Rmax) int32, counts (B,) int32 on the device) of that head.  heads: None (the call it
        always was), or a tuple of distinct head indices: only those heads run (`svc_astral_tokens_heads`), tokens has len(heads)
        planes in ascending head order, and reduce_head must be one of them.  Nothing is synchronised."""
        ov = int(round(float(overlap_s) * self.SR)) // SAMPLES_PER_ROW
        mask = None
        if heads is not None:
            hs = [self._head(k, "tokens_batch") for k in heads]
            if not hs or len(set(hs)) != len(hs):
                raise ValueError(f"AstralTokenizer.tokens_batch: heads {tuple(heads)!r} must be distinct head indices, at least one")
            if reduce_head is not None and int(reduce_head) not in hs:
                raise ValueError(f"AstralTokenizer.tokens_batch: reduce_head {reduce_head!r} is not in heads {tuple(hs)}")
            mask = sum(1 << k for k in hs)
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves, self.device)
            B, L = w.shape
            lens = [L] * B if lens is None else self._lens(lens, B)
            rows = [self.rows(n, ov) for n in lens]
            R = max(rows)
            out = torch.empty(self.n_heads if mask is None else len(hs), B, R, dtype=torch.int32, device=self.device)
            red = cnt = None
            if reduce_head is not None:
                red = torch.empty(B, R, dtype=torch.int32, device=self.device)
                cnt = torch.empty(B, dtype=torch.int32, device=self.device)
            rh = -1 if reduce_head is None else int(reduce_head)
            if mask is None:
                _lib.check(self._fn("tokens")(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, ov, _lib.ptr(out), R, rh, _lib.ptr(red),
                                              _lib.ptr(cnt), _lib.stream_ptr()))
            else:
                _lib.check(self._fn("tokens_heads")(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, ov, mask, _lib.ptr(out), R, rh,
                                                    _lib.ptr(red), _lib.ptr(cnt), _lib.stream_ptr()))
        return (out, rows) if reduce_head is None else (out, rows, red, cnt)

    @torch.inference_mode()
    def tokens_fn(self, waves_16k, head=0):
        """The per-block call of a real-time session (`RealtimeEngine.attach_audio`): (n, L <= window_samples)
        full-length rows -> (n, rows(L)) int32 on the device, head `head` alone from one `svc_astral_tokens_heads` call (the other
        head launches nothing).  Nothing is synchronised."""
        k = self._head(head, "tokens_fn")
        if waves_16k.dim() != 2 or not 1 <= waves_16k.size(0) <= 64 or waves_16k.size(1) > self.W:
            raise ValueError(f"AstralTokenizer.tokens_fn: (n <= 64, L <= {self.W}) samples, got {tuple(waves_16k.shape)}")
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves_16k, self.device)
            n, L = w.shape
            R = window_rows(self.cfg, L)
            if R < 1:
                raise ValueError(f"AstralTokenizer.tokens_fn: {L} samples are shorter than the extractor's receptive field")
            out = torch.empty(n, R, dtype=torch.int32, device=self.device)
            _lib.check(self._fn("tokens_heads")(self._h, _lib.ptr(w), None, n, L, 0, 1 << k, _lib.ptr(out), R, -1, None, None,
                                                _lib.stream_ptr()))
        return out

    def tokenize(self, waves_16k, lens=None, head=0):
        """The reference's call for one head: (B, L <= 480 000) samples, lens -> (None, indices (B, T) int64, feature_lens (B,) int64);
        `quantized` (project_out of the signs) is not computed: nothing in v2 reads it."""
        w = torch.as_tensor(waves_16k, dtype=torch.float32)
        if w.dim() != 2 or w.size(1) > self.W:
            raise ValueError(f"AstralTokenizer.tokenize: (B, L <= {self.W}) samples, got {tuple(w.shape)}")
        tok, rows = self.tokens_batch(w, lens, overlap_s=0.0)
        return None, tok[head].long(), torch.tensor(rows, dtype=torch.int64, device=self.device)

    @torch.inference_mode()
    def ssl(self, waves, lens, out=None):
        """waves (B, L <= window), lens -> (rows (B, T, D) of the residual stream after the last SSL layer, rows [B]); rows at and
        above a clip's count keep what `out` held (zeros when `out` is None)."""
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves, self.device)
            B, L = w.shape
            lens = self._lens(lens, B)
            rows = [window_rows(self.cfg, n) for n in lens]
            T = max(max(rows), 1) if out is None else out.size(1)
            out = torch.zeros(B, T, self.D, device=self.device) if out is None else out
            _lib.check(self._fn("ssl")(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, _lib.ptr(out), T, _lib.stream_ptr()))
        return out, rows

    def _rows_call(self, name, k, x, width, out_width, rows, out):
        with torch.cuda.device(self.device):
            x = _lib.f32c(x, self.device)
            if x.dim() != 3 or x.size(2) != width:
                raise ValueError(f"AstralTokenizer.{name}: rows must be (B, T, {width}), got {tuple(x.shape)}")
            B, T, _ = x.shape
            out = torch.zeros(B, T, out_width, device=self.device) if out is None else out
            _lib.check(self._fn(name)(self._h, int(k), _lib.ptr(x), _lib.i32_host(self._lens(rows, B)), B, T, _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def convnext(self, k, h, rows, out=None):
        """head k: SSL rows h (B, T, D), rows [B] -> x (B, T, dim) after the last ConvNeXt block, each clip over its own rows; the
        rows above keep what `out` held."""
        return self._rows_call("convnext", k, h, self.D, int(self.cfg["heads"][k]["dim"]), rows, out)

    @torch.inference_mode()
    def logits(self, k, x, rows, out=None):
        """head k: x (B, T, dim), rows [B] -> project_in(x) (B, T, bits), fp32"""
        hk = self.cfg["heads"][k]
        return self._rows_call("logits", k, x, int(hk["dim"]), int(hk["bits"]), rows, out)

    @torch.inference_mode()
    def reduce(self, tokens, rows):
        """tokens (B, R) int32 on the device, rows [B] -> (list of B (n_b,) int64 tensors of the run heads, counts [B]); one host
        synchronisation: the counts"""
        red, cnt = reduce_tokens(tokens, rows)
        counts = cnt.tolist()
        return [red[b, :n].long() for b, n in enumerate(counts)], counts


@torch.inference_mode()
def reduce_tokens(tokens, rows):
    """svc_tokens_reduce: tokens (B, R) int32 on the device, rows B host integers -> (reduced (B, R) int32, -1 above the count;
    counts (B,) int32 on the device).  Nothing is synchronised."""
    rows = _lib.int_list(rows)
    with torch.cuda.device(tokens.device):
        t = tokens.to(torch.int32).contiguous()
        B, R = t.shape
        red, cnt = torch.empty_like(t), torch.empty(B, dtype=torch.int32, device=t.device)
        _lib.check(_lib.lib().svc_tokens_reduce(_lib.ptr(t), _lib.i32_host(rows), B, R, _lib.ptr(red), _lib.ptr(cnt), _lib.stream_ptr()))
    return red, cnt


@torch.inference_mode()
def bsq_index_device(z):
    """svc_op_bsq_index: z (rows, bits) fp32 on the device -> (rows,) int32"""
    with torch.cuda.device(z.device):
        z = _lib.f32c(z)
        out = torch.empty(z.shape[0], dtype=torch.int32, device=z.device)
        _lib.check(_lib.lib().svc_op_bsq_index(_lib.ptr(z), _lib.ptr(out), z.shape[0], z.shape[1], _lib.stream_ptr()))
    return out
