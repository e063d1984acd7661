"""Host-side mirror of the RMVPE pitch extractor over the C ABI.

`RMVPE(state_dict).infer_from_audio(audio_16k, thred=0.03)` has the call surface of the reference's
`rmvpe.infer_from_audio(wave_16k, thred=0.03)`: one clip in, numpy F0 (Hz, 100 frames/s, 0 = unvoiced) out.
`f0_batch` is the same for up to 64 clips of different lengths in one call, on the device, without a synchronisation;
`mel`, `salience` and `decode` expose the three stages.  The state dict is the one of RVC's `E2E` module (`rmvpe.pt`).
The default mel basis restates librosa's HTK filterbank (`audio.htk_mel_basis`, unpinned); pass the reference's own
`mel_basis=` tensor (128, 513) when it is at hand.
"""
import ctypes as C

import torch

from . import _lib, specs
from .audio import htk_mel_basis


class RMVPE:
    SR, HOP, N_FFT, FMIN, FMAX = 16000, 160, 1024, 30, 8000

    def __init__(self, state_dict, mel_basis=None, device="cuda:0", cfg=None):
        self.cfg = specs.rmvpe_config() if cfg is None else cfg
        self.device = torch.device(device)
        if mel_basis is None:
            mel_basis = htk_mel_basis(self.SR, self.N_FFT, self.cfg["n_mels"], self.FMIN, self.FMAX)
        c = _lib.RmvpeConfig()
        for k in ("n_mels", "en_de_layers", "inter_layers", "n_blocks", "en_out_channels", "gru_hidden", "n_bins"):
            setattr(c, k, int(self.cfg[k]))
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            mb = _lib.f32c(mel_basis, self.device)
            if tuple(mb.shape) != (self.cfg["n_mels"], self.N_FFT // 2 + 1):
                raise ValueError(f"RMVPE: mel_basis must be ({self.cfg['n_mels']}, {self.N_FFT // 2 + 1}), got {tuple(mb.shape)}")
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            _lib.check(_lib.lib().svc_rmvpe_create(C.byref(c), descs, n, _lib.ptr(mb), _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep

    def eval(self):
        return self

    @staticmethod
    def frames(n_samples):
        return 1 + int(n_samples) // RMVPE.HOP

    @staticmethod
    def _lens(lens, B, what):
        lens = _lib.int_list(lens)
        if len(lens) != B:
            raise ValueError(f"RMVPE: {len(lens)} {what} for a batch of {B}")
        return lens

    def set_plane_budget(self, n_bytes):
        """Bytes one level-0 plane of a group of clips may take (0 = the default, 256 MiB): larger batches run in groups."""
        _lib.check(_lib.lib().svc_rmvpe_set_plane_budget(self._h, int(n_bytes)))

    def set_timing(self, on):
        """Measurement aid: record HIP events around the network's stages (see `last_timing`)."""
        _lib.check(_lib.lib().svc_rmvpe_set_timing(self._h, int(bool(on))))

    def last_timing(self):
        """dict of milliseconds of the last network pass (synchronises): unet, gru_in, gru, head."""
        ms = (C.c_float * 4)()
        _lib.check(_lib.lib().svc_rmvpe_last_timing(self._h, ms))
        return dict(zip(("unet", "gru_in", "gru", "head"), [float(v) for v in ms]))

    @torch.inference_mode()
    def mel(self, waves, lens):
        """waves (B, L) at 16 kHz, lens B host integers -> (B, n_mels, frames(L)); zero above a clip's own frames."""
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves, self.device)
            B, L = w.shape
            lens = self._lens(lens, B, "lens")
            out = torch.empty(B, self.cfg["n_mels"], self.frames(L), device=self.device)
            _lib.check(_lib.lib().svc_rmvpe_mel(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def salience(self, mel, frame_lens=None):
        """mel (B, n_mels, T) -> (B, T, n_bins): the network alone.  frame_lens: B host integers (default: all T)."""
        with torch.cuda.device(self.device):
            m = _lib.f32c(mel, self.device)
            B, _, T = m.shape
            fl = [T] * B if frame_lens is None else self._lens(frame_lens, B, "frame_lens")
            out = torch.empty(B, T, self.cfg["n_bins"], device=self.device)
            _lib.check(_lib.lib().svc_rmvpe_salience(self._h, _lib.ptr(m), _lib.i32_host(fl), B, T, _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def decode(self, salience, frame_lens=None, thred=0.03):
        """salience (B, T, 360) -> F0 (B, T) in Hz, 0 on unvoiced frames and above a clip's frames."""
        with torch.cuda.device(self.device):
            s = _lib.f32c(salience, self.device)
            B, T, n = s.shape
            if n != 360:
                raise ValueError("RMVPE.decode: the cents mapping is defined for 360 bins")
            fl = [T] * B if frame_lens is None else self._lens(frame_lens, B, "frame_lens")
            out = torch.empty(B, T, device=self.device)
            _lib.check(_lib.lib().svc_rmvpe_decode(_lib.ptr(s), _lib.i32_host(fl), B, T, float(thred), _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def f0_batch(self, waves, lens=None, thred=0.03):
        """waves (B, L) at 16 kHz (B <= 64), lens B host integers or None -> device F0 (B, frames(L)); row b holds the
        frames(lens[b]) values of waves[b, :lens[b]] run alone, zeros above.  Nothing is synchronised."""
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves, self.device)
            B, L = w.shape
            hl = None if lens is None else _lib.i32_host(self._lens(lens, B, "lens"))
            out = torch.empty(B, self.frames(L), device=self.device)
            _lib.check(_lib.lib().svc_rmvpe_f0(self._h, _lib.ptr(w), hl, B, L, float(thred), _lib.ptr(out), _lib.stream_ptr()))
        return out

    def infer_from_audio(self, audio, thred=0.03):
        """audio: 1-D numpy array or tensor at 16 kHz -> numpy F0 (frames,), as the reference returns it."""
        a = torch.as_tensor(audio, dtype=torch.float32).reshape(1, -1)
        return self.f0_batch(a, None, thred)[0].cpu().numpy()

    def close(self):
        if self._h:
            _lib.lib().svc_rmvpe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@torch.inference_mode()
def f0_adjust(f0_alt, alt_lens, f0_ori, ori_lens, auto_f0_adjust=True, pitch_shift=0, return_medians=False):
    """The drivers' pitch step (`svc_f0_adjust`): f0_alt (B, Talt) source track, f0_ori (B, Tori) reference track, host frame
    counts per row; pitch_shift a number of semitones or one per row -> shifted f0_alt (B, Talt)."""
    dev = f0_alt.device
    with torch.cuda.device(dev):
        a, o = _lib.f32c(f0_alt), _lib.f32c(f0_ori, dev)
        B, Talt = a.shape
        Tori = o.shape[1]
        al, ol = _lib.int_list(alt_lens), _lib.int_list(ori_lens)
        if len(al) != B or len(ol) != B or o.shape[0] != B:
            raise ValueError(f"f0_adjust: lengths and tracks must all have {B} rows")
        if torch.is_tensor(pitch_shift):
            pitch_shift = pitch_shift.tolist()
        semis = [float(x) for x in pitch_shift] if isinstance(pitch_shift, (list, tuple)) else [float(pitch_shift)] * B
        if len(semis) != B:
            raise ValueError(f"f0_adjust: {len(semis)} pitch shifts for {B} rows")
        out = torch.empty(B, Talt, device=dev)
        med = torch.empty(B, 2, device=dev) if return_medians else None
        _lib.check(_lib.lib().svc_f0_adjust(_lib.ptr(a), _lib.i32_host(al), _lib.ptr(o), _lib.i32_host(ol), B, Talt, Tori,
                                            int(bool(auto_f0_adjust)), (C.c_float * B)(*semis), _lib.ptr(out), _lib.ptr(med),
                                            _lib.stream_ptr()))
    return (out, med) if return_medians else out


PITCH_BINS, PITCH_STATE_WORDS = 1536, 1536 + 8         # SVC_RT_PITCH_BINS, SVC_RT_PITCH_STATE_WORDS


def rt_pitch_state(max_slots, device="cuda:0"):
    """The per-slot running pitch statistics of `rt_pitch`: (max_slots, PITCH_STATE_WORDS) int32 zeros, a fresh stream per row
    (words 0 .. 1535 the histogram, 1536 the voiced count, 1537 the bits of the applied log shift, 1538 the median bin)."""
    n = int(_lib.lib().svc_rt_pitch_state_words(int(max_slots)))
    if n <= 0:
        raise ValueError(f"rt_pitch_state: max_slots = {max_slots!r}")
    return torch.zeros(int(max_slots), n // int(max_slots), device=device, dtype=torch.int32)


@torch.inference_mode()
def rt_pitch(f0, n_new, lag, slots, state, ref_median, auto_adjust, semitones=None, warmup=50, max_step=0.0, return_shift=False):
    """The pitch step of live streams (`svc_rt_pitch`): f0 (N, Tf) device float32, row k the RMVPE track of the
    context of stream slots[k]; the n_new frames that lie `lag` frames before the end are counted into the slot's row of `state`
    (`rt_pitch_state`), the applied log shift glides by at most max_step per call towards ref_median[slot] - running median
    where auto_adjust[k] is set, ref_median[slot] is positive (0: a reference without a voiced frame) and the slot has
    counted `warmup` voiced frames (else towards 0), and every frame is shifted
    by it and by semitones[k].  slots, auto_adjust, semitones: N host values (semitones: one number for all, or None = 0).
    -> the shifted track (N, Tf); with return_shift also the applied log shifts (N,).  Nothing is synchronised."""
    dev = f0.device
    with torch.cuda.device(dev):
        f = f0 if f0.dtype == torch.float32 and f0.stride(-1) == 1 and f0.dim() == 2 else _lib.f32c(f0)
        if f.dim() != 2:
            raise ValueError(f"rt_pitch: f0 {tuple(f0.shape)} is not (N, Tf)")
        N, Tf = f.shape
        slots, aut = _lib.int_list(slots), [int(bool(v)) for v in _lib.int_list(auto_adjust)]
        if torch.is_tensor(semitones):
            semitones = semitones.tolist()
        semis = None if semitones is None else \
            [float(x) for x in semitones] if isinstance(semitones, (list, tuple)) else [float(semitones)] * N
        if len(slots) != N or len(aut) != N or (semis is not None and len(semis) != N):
            raise ValueError(f"rt_pitch: slots, auto_adjust and semitones must all have {N} entries")
        if state.dtype != torch.int32 or state.dim() != 2 or state.size(1) != PITCH_STATE_WORDS or not state.is_contiguous():
            raise ValueError(f"rt_pitch: state must be contiguous int32 (max_slots, {PITCH_STATE_WORDS})")
        if ref_median.dtype != torch.float32 or ref_median.numel() != state.size(0) or not ref_median.is_contiguous():
            raise ValueError("rt_pitch: ref_median must be contiguous float32 (max_slots,)")
        out = torch.empty(N, Tf, device=dev)
        shift = torch.empty(N, device=dev) if return_shift else None
        _lib.check(_lib.lib().svc_rt_pitch(_lib.ptr(f), f.stride(0), Tf, int(n_new), int(lag), N, _lib.i32_host(slots), state.size(0),
                                           _lib.ptr(state), _lib.ptr(ref_median), _lib.i32_host(aut),
                                           None if semis is None else (C.c_float * N)(*semis), int(warmup), float(max_step),
                                           _lib.ptr(out), out.stride(0), _lib.ptr(shift), _lib.stream_ptr()))
    return (out, shift) if return_shift else out


PITCH_WIN_MAX_TF = 4096                                # SVC_RT_PITCH_WIN_MAX_TF


def rt_pitch_cache(max_slots, Tf, device="cuda:0"):
    """The per-slot raw pitch track of `rt_pitch_win`: (max_slots, Tf) float32 zeros, Hz; a fresh stream per row (0 Hz is unvoiced).
    Tf is at most PITCH_WIN_MAX_TF."""
    n = int(_lib.lib().svc_rt_pitch_cache_words(int(max_slots), int(Tf)))
    if n <= 0:
        raise ValueError(f"rt_pitch_cache: max_slots = {max_slots!r}, Tf = {Tf!r} (1 .. {PITCH_WIN_MAX_TF})")
    return torch.zeros(int(max_slots), int(Tf), device=device, dtype=torch.float32)


def rt_pitch_ring(max_slots, memory, device="cuda:0"):
    """The per-slot ring of `rt_pitch_win`'s last `memory` counted frames: (max_slots, memory + 2) int32 zeros (words 0 .. memory - 1
    the entries, a bin or -1 for an unvoiced frame; then head and fill), a fresh stream per row.  memory = 0 -> None: the
    statistics never forget."""
    if int(memory) == 0:
        return None
    n = int(_lib.lib().svc_rt_pitch_ring_words(int(max_slots), int(memory)))
    if n <= 0:
        raise ValueError(f"rt_pitch_ring: max_slots = {max_slots!r}, memory = {memory!r}")
    return torch.zeros(int(max_slots), n // int(max_slots), device=device, dtype=torch.int32)


@torch.inference_mode()
def rt_pitch_win(f0_win, guard, n_new, lag, slots, cache, ring, state, ref_median, auto_adjust, semitones=None, warmup=50, max_step=0.0,
                 return_shift=False, return_raw=False):
    """`rt_pitch` on the context's tail (`svc_rt_pitch_win`): f0_win (N, W) device float32, row k the RMVPE track of
    the LAST samples of the context of stream slots[k], its frame j being context frame Tf - W + j.  The slot's row of `cache`
    (`rt_pitch_cache`, (max_slots, Tf) raw Hz) moves n_new frames to the left and takes the window's frames from `guard` on; the
    counted frames, the statistics, the glide and the shifted track (N, Tf) are `rt_pitch`'s over that row.  ring
    (`rt_pitch_ring`, or None = never forget): the bins of the slot's last `memory` counted frames; what is pushed out of it leaves
    the histogram, so the median is over the last `memory` frames.  Needs W - guard >= n_new, W <= Tf <= PITCH_WIN_MAX_TF and
    memory >= n_new.  -> the shifted track; with return_shift / return_raw also the applied shifts (N,) / the new cache rows
    (N, Tf), in this order.  Nothing is synchronised."""
    dev = f0_win.device
    with torch.cuda.device(dev):
        f = f0_win if f0_win.dtype == torch.float32 and f0_win.stride(-1) == 1 and f0_win.dim() == 2 else _lib.f32c(f0_win)
        if f.dim() != 2:
            raise ValueError(f"rt_pitch_win: f0_win {tuple(f0_win.shape)} is not (N, W)")
        N, W = f.shape
        slots, aut = _lib.int_list(slots), [int(bool(v)) for v in _lib.int_list(auto_adjust)]
        if torch.is_tensor(semitones):
            semitones = semitones.tolist()
        semis = None if semitones is None else \
            [float(x) for x in semitones] if isinstance(semitones, (list, tuple)) else [float(semitones)] * N
        if len(slots) != N or len(aut) != N or (semis is not None and len(semis) != N):
            raise ValueError(f"rt_pitch_win: slots, auto_adjust and semitones must all have {N} entries")
        if state.dtype != torch.int32 or state.dim() != 2 or state.size(1) != PITCH_STATE_WORDS or not state.is_contiguous():
            raise ValueError(f"rt_pitch_win: state must be contiguous int32 (max_slots, {PITCH_STATE_WORDS})")
        ms = state.size(0)
        if ref_median.dtype != torch.float32 or ref_median.numel() != ms or not ref_median.is_contiguous():
            raise ValueError("rt_pitch_win: ref_median must be contiguous float32 (max_slots,)")
        if cache.dtype != torch.float32 or cache.dim() != 2 or cache.size(0) != ms or not cache.is_contiguous():
            raise ValueError("rt_pitch_win: cache must be contiguous float32 (max_slots, Tf)")
        Tf = cache.size(1)
        if ring is not None and (ring.dtype != torch.int32 or ring.dim() != 2 or ring.size(0) != ms or ring.size(1) < 3 or
                                 not ring.is_contiguous()):
            raise ValueError("rt_pitch_win: ring must be contiguous int32 (max_slots, memory + 2) or None")
        memory = 0 if ring is None else ring.size(1) - 2
        out = torch.empty(N, Tf, device=dev)
        shift = torch.empty(N, device=dev) if return_shift else None
        raw = torch.empty(N, Tf, device=dev) if return_raw else None
        _lib.check(_lib.lib().svc_rt_pitch_win(_lib.ptr(f), f.stride(0), W, int(guard), Tf, int(n_new), int(lag), N, _lib.i32_host(slots),
                                               ms, _lib.ptr(cache), _lib.ptr(ring), memory, _lib.ptr(state), _lib.ptr(ref_median),
                                               _lib.i32_host(aut), None if semis is None else (C.c_float * N)(*semis), int(warmup),
                                               float(max_step), _lib.ptr(out), out.stride(0), _lib.ptr(raw), Tf, _lib.ptr(shift),
                                               _lib.stream_ptr()))
    res = (out,) + ((shift,) if return_shift else ()) + ((raw,) if return_raw else ())
    return res if len(res) > 1 else out
