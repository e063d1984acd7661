"""Host-side mirror of the FSMN voice activity detector: funasr's `fsmn-vad` -- WavFrontendOnline, the FSMN
encoder and a causal statement of E2EVadModel's window detector -- restated from memory; parity with the released
checkpoint is not pinned.

`FsmnVad(state_dict, cmvn_shift, cmvn_scale)` takes the encoder's state dict (names with or without an `encoder.` prefix) and
the two 400-vectors of `am.mvn` as tensors: parsing the Kaldi text file stays with the caller.  `scores_batch` gives P(silence)
per 10 ms row for a ragged batch, `segments` the [[beg_ms, end_ms], ...] of one clip, `detect` is the detector on
probabilities of the caller's, and `stream_state` / `step` carry live streams (`RealtimeEngine.attach_vad`).
"""
import ctypes as C

import torch

from . import _lib

STATE_FLOATS = 4 * 19 * 128 + 32
CACHE_FLOATS = 4 * 19 * 128
MAX_EVENTS = 8
MAX_ROWS = 6000
BEGIN, END = 1, 2
# names of the detector's integers inside a slot's state row (int32 view, after the caches)
STATE_WORDS = ("t", "bits", "pos", "sum", "win_state", "in_seg", "beg", "sil_run", "prev_end")

# the checkpoint's config.yaml as remembered (times in ms)
FUNASR_DEFAULTS = dict(speech_noise_thres=0.6, speech_2_noise_ratio=1.0, frame_in_ms=10, window_size_ms=200,
                       sil_to_speech_time_thres=150, speech_to_sil_time_thres=150, lookback_time_start_point=200,
                       max_end_silence_time=800, max_single_segment_time=60000)


def vad_config(seg_rows=0, **funasr):
    """funasr's VADXOptions names -> dict(p_max, win, on_count, off_count, lookback, end_silence, max_segment, seg_rows) in frames.
    p_max = (1 - speech_noise_thres) / 2: `1 - p >= p + thres` with speech_2_noise_ratio 1, the only ratio taken."""
    unknown = set(funasr) - set(FUNASR_DEFAULTS)
    if unknown:
        raise ValueError(f"vad_config: unknown options {sorted(unknown)}")
    o = dict(FUNASR_DEFAULTS, **funasr)
    if float(o["speech_2_noise_ratio"]) != 1.0:
        raise ValueError(f"vad_config: speech_2_noise_ratio = {o['speech_2_noise_ratio']!r}; only 1 is supported")
    if int(o["frame_in_ms"]) != 10:
        raise ValueError("vad_config: frame_in_ms must be 10")
    ms = lambda k: int(o[k]) // 10                                                               # noqa: E731
    return dict(p_max=(1.0 - float(o["speech_noise_thres"])) / 2.0, win=ms("window_size_ms"), on_count=ms("sil_to_speech_time_thres"),
                off_count=ms("speech_to_sil_time_thres"), lookback=ms("lookback_time_start_point"),
                end_silence=(int(o["max_end_silence_time"]) - int(o["speech_to_sil_time_thres"])) // 10,
                max_segment=ms("max_single_segment_time"), seg_rows=int(seg_rows))


def check_config(cfg, what="FsmnVad"):
    """The refusals of svc_vad_create's config, as ValueError."""
    if not 1 <= cfg["win"] <= 32:
        raise ValueError(f"{what}: win = {cfg['win']} outside 1 .. 32")
    if not 1 <= cfg["on_count"] <= cfg["win"] or not 0 <= cfg["off_count"] <= cfg["win"]:
        raise ValueError(f"{what}: on_count outside 1 .. win or off_count outside 0 .. win")
    if cfg["lookback"] < 0 or cfg["end_silence"] < 1 or cfg["max_segment"] < 1:
        raise ValueError(f"{what}: lookback, end_silence or max_segment")
    if cfg["seg_rows"] != 0 and cfg["seg_rows"] < 16:
        raise ValueError(f"{what}: seg_rows is neither 0 nor at least 16")
    if not 0.0 <= cfg["p_max"] <= 1.0:
        raise ValueError(f"{what}: p_max outside 0 .. 1")


def vad_rows(n_samples, final=True):
    return int(_lib.lib().svc_vad_rows(int(n_samples), int(bool(final))))


def vad_history(total):
    return int(_lib.lib().svc_vad_history(int(total)))


def events_to_segments(events, last_frame):
    """[(kind, time_ms), ...] in order -> [[beg_ms, end_ms], ...]; a segment still open closes at 10 * last_frame."""
    segs, beg = [], None
    for kind, t in events:
        if kind == BEGIN:
            beg = t
        elif kind == END and beg is not None:
            segs.append([beg, t])
            beg = None
    if beg is not None:
        segs.append([beg, 10 * last_frame])
    return segs


class FsmnVad:
    def __init__(self, state_dict, cmvn_shift, cmvn_scale, config=None, device="cuda:0"):
        self.device = torch.device(device)
        self.config = dict(vad_config() if config is None else config)
        check_config(self.config)
        shift, scale = (torch.as_tensor(v).reshape(-1) for v in (cmvn_shift, cmvn_scale))
        if shift.numel() != 400 or scale.numel() != 400:
            raise ValueError("FsmnVad: cmvn_shift and cmvn_scale must have 400 entries")
        c = _lib.VadConfig()
        c.p_max = float(self.config["p_max"])
        for k in ("win", "on_count", "off_count", "lookback", "end_silence", "max_segment", "seg_rows"):
            setattr(c, k, int(self.config[k]))
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            shift, scale = _lib.f32c(shift, self.device), _lib.f32c(scale, self.device)
            _lib.check(_lib.lib().svc_vad_create(C.byref(c), descs, n, _lib.ptr(shift), _lib.ptr(scale), _lib.stream_ptr(),
                                                 C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep

    @torch.inference_mode()
    def scores_batch(self, waves_16k, lens, final=True, seg_rows=0):
        """waves (B, L) at 16 kHz, lens B host integers in 0 .. L -> (p_sil (B, vad_rows(L, final)), rows list): row b holds
        rows[b] = vad_rows(lens[b], final) probabilities of silence, one per 10 ms; what lies above them is not written."""
        with torch.cuda.device(self.device):
            w = _lib.f32c(waves_16k, self.device)
            if w.dim() == 1:
                w = w.unsqueeze(0)
            B, L = w.shape
            lens = _lib.int_list(lens)
            if len(lens) != B:
                raise ValueError(f"FsmnVad.scores_batch: {len(lens)} lens for a batch of {B}")
            p = torch.zeros(B, max(vad_rows(L, final), 0), device=self.device, dtype=torch.float32)
            _lib.check(_lib.lib().svc_vad_scores(self._h, _lib.ptr(w), _lib.i32_host(lens), B, L, int(bool(final)), int(seg_rows),
                                                 _lib.ptr(p), _lib.stream_ptr()))
        return p, [vad_rows(n, final) for n in lens]

    def stream_state(self, max_slots):
        """(state (max_slots, STATE_FLOATS) float32, flags (max_slots,) int32), zeros: fresh streams, flags 0."""
        n = int(_lib.lib().svc_vad_state_floats(int(max_slots)))
        return (torch.zeros(n, device=self.device, dtype=torch.float32).view(int(max_slots), STATE_FLOATS),
                torch.zeros(int(max_slots), device=self.device, dtype=torch.int32))

    @staticmethod
    def state_words(state):
        """The detector's integers of every slot: (max_slots, 32) int32 view of `state`."""
        return state[:, CACHE_FLOATS:].view(torch.int32)

    @torch.inference_mode()
    def detect(self, p_sil, n_rows, slots, state, flags, frame_speech=False):
        """The detector alone (`svc_vad_detect`): p_sil (N, ld) device float32, row k holding n_rows[k] new frames of stream
        slots[k] -> dict(events (N, 8, 2) int32 (kind, time_ms), n_events (N,) int32[, frame_speech (N, ld) int32]); state and
        flags are updated in place."""
        with torch.cuda.device(self.device):
            p = _lib.f32c(p_sil, self.device)
            N, ld = p.shape
            n_rows, slots = _lib.int_list(n_rows), _lib.int_list(slots)
            if len(n_rows) != N or len(slots) != N:
                raise ValueError(f"FsmnVad.detect: {len(n_rows)} n_rows and {len(slots)} slots for {N} rows of p_sil")
            ev = torch.zeros(N, MAX_EVENTS, 2, device=self.device, dtype=torch.int32)
            nev = torch.zeros(N, device=self.device, dtype=torch.int32)
            fs = torch.zeros(N, ld, device=self.device, dtype=torch.int32) if frame_speech else None
            _lib.check(_lib.lib().svc_vad_detect(self._h, _lib.ptr(p), ld, _lib.i32_host(n_rows), N, _lib.i32_host(slots), state.size(0),
                                                 _lib.ptr(state), _lib.ptr(fs), _lib.ptr(ev), _lib.ptr(nev), _lib.ptr(flags),
                                                 _lib.stream_ptr()))
        out = dict(events=ev, n_events=nev)
        if frame_speech:
            out["frame_speech"] = fs
        return out

    @torch.inference_mode()
    def step(self, x, end, n_new, total, slots, state, flags, return_parts=False):
        """One block of live streams (`svc_vad_step`): row k of x (N, stride) holds the 16 kHz samples of stream slots[k] ending
        at x[k, end), the last n_new new, total[k] before them.  Updates state and flags; with return_parts ->
        dict(p_sil (N, n_new / 160), n_rows list, events, n_events)."""
        with torch.cuda.device(self.device):
            N = x.size(0)
            total, slots = _lib.int_list(total), _lib.int_list(slots)
            p = ev = nev = None
            mr = int(n_new) // 160
            if return_parts:
                p = torch.zeros(N, mr, device=self.device, dtype=torch.float32)
                ev = torch.zeros(N, MAX_EVENTS, 2, device=self.device, dtype=torch.int32)
                nev = torch.zeros(N, device=self.device, dtype=torch.int32)
            _lib.check(_lib.lib().svc_vad_step(self._h, _lib.ptr(x), x.stride(0), int(end), int(n_new), _lib.i64_host(total), N,
                                               _lib.i32_host(slots), state.size(0), _lib.ptr(state), _lib.ptr(flags), _lib.ptr(p), mr,
                                               _lib.ptr(ev), _lib.ptr(nev), _lib.stream_ptr()))
        if return_parts:
            return dict(p_sil=p, n_rows=[vad_rows(t + int(n_new), False) - vad_rows(t, False) for t in total], events=ev, n_events=nev)
        return None

    def segments(self, wave_16k, chunk=256):
        """One clip (L,) or (1, L) at 16 kHz -> [[beg_ms, end_ms], ...]: one final `scores_batch`, then the detector over the
        rows in calls of `chunk` frames (a call keeps 8 events: a chunk that made more is run again in halves); a segment
        still open at the end closes at the last frame.  Reads the events back, so it synchronises."""
        w = torch.as_tensor(wave_16k).reshape(1, -1)
        p, rows = self.scores_batch(w, [w.size(1)], final=True)
        R = rows[0]
        state, flags = self.stream_state(1)
        events, pos = [], 0
        while pos < R:
            n = min(int(chunk), R - pos, MAX_ROWS)
            keep = state.clone()
            d = self.detect(p[:, pos:pos + n].contiguous(), [n], [0], state, flags)
            ne = int(d["n_events"][0])
            if ne > MAX_EVENTS and n > 1:
                state.copy_(keep)
                chunk = max(1, n // 2)
                continue
            events += [(int(k), int(t)) for k, t in d["events"][0, :ne].tolist()]
            pos += n
        return events_to_segments(events, max(R - 1, 0))

    def close(self):
        if self._h:
            _lib.lib().svc_vad_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
