"""What the 16 kHz content encoders' host mirrors share (whisper.py, wav2vec2.py; csrc/content_encoder.h): the drivers' window
plan and the handle plumbing of a tokenizer class."""
import ctypes as C

import torch

from . import _lib

SAMPLES_PER_ROW = 320       # 16 kHz samples per content row (50 rows/s)


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


class ContentEncoder:
    """Base of the tokenizer classes.  A subclass sets ABI (its entry points are svc_<ABI>_*), STAGES (the names of
    `last_timing`'s four stages), `_h`, `device`, `D`, `W`, and has `rows(n_samples, overlap_rows)`."""
    SR = 16000
    ABI = None
    STAGES = ()

    def _fn(self, name):
        return getattr(_lib.lib(), f"svc_{self.ABI}_{name}")

    def eval(self):
        return self

    def set_window_group(self, windows):
        """Windows computed side by side (0 = the default): bounds the workspace; results do not depend on it."""
        _lib.check(self._fn("set_window_group")(self._h, int(windows)))

    def set_timing(self, on):
        """Measurement aid: record HIP events around the stages of `content_batch` (see `last_timing`)."""
        _lib.check(self._fn("set_timing")(self._h, int(bool(on))))

    def last_timing(self):
        """dict of milliseconds of the last window group of the last `content_batch` (synchronises)."""
        ms = (C.c_float * 4)()
        _lib.check(self._fn("last_timing")(self._h, ms))
        return dict(zip(self.STAGES, [float(v) for v in ms]))

    def _lens(self, lens, B):
        lens = _lib.int_list(lens)
        if len(lens) != B:
            raise ValueError(f"{type(self).__name__}: {len(lens)} lens for a batch of {B}")
        return lens

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
            _lib.check(self._fn("content")(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, ov, _lib.ptr(out), max(rows), _lib.stream_ptr()))
        return out, rows

    def semantic_fn(self, waves_16k):
        """The drivers' closure: (1, L <= W) samples -> (1, rows(L), D)."""
        w = torch.as_tensor(waves_16k, dtype=torch.float32)
        if w.dim() != 2 or w.size(1) > self.W:
            raise ValueError(f"{type(self).__name__}.semantic_fn: (B, L <= {self.W}) samples, got {tuple(w.shape)}")
        return self.content_batch(w, None, overlap_s=0.0)[0]

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
