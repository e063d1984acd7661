"""The hot path as the reference drivers run it: CFM sampler -> strip prompt -> vocoder, plus the
chunk / crossfade loop around it (reference: inference.py:470-527, seed_vc_wrapper.py:561-623) and the
multi-GPU sharding of utterance batches.
"""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

_PITCH_HOP = 160                 # samples per f0 frame at 16 kHz (RMVPE.HOP): frame j of a clip is centred on sample 160 j


def _cos2_windows(n):
    """(fade_in, fade_out) of the drivers' cos^2 crossfade over n samples, float64 (reference: inference.py:343-350).  The
    one place they are computed: `svc_crossfade` and `svc_chunks_assemble` take them as arrays and `crossfade` is their
    yardstick, so the host and device paths agree bit for bit."""
    return np.cos(np.linspace(np.pi / 2, 0, n)) ** 2, np.cos(np.linspace(0, np.pi / 2, n)) ** 2


def crossfade(chunk1, chunk2, overlap):
    """cos^2 crossfade on numpy chunks, in place on chunk2 (reference: inference.py:343-350)."""
    fade_in, fade_out = _cos2_windows(overlap)
    if len(chunk2) < overlap:
        chunk2[:overlap] = chunk2[:overlap] * fade_in[:len(chunk2)] + (chunk1[-overlap:] * fade_out)[:len(chunk2)]
    else:
        chunk2[:overlap] = chunk2[:overlap] * fade_in + chunk1[-overlap:] * fade_out
    return chunk2


def stream_wave_chunks(vc_wave, processed_frames, n_target_frames, overlap_wave_len, overlap_frame_len, chunks,
                       previous_chunk, is_last_chunk):
    """One turn of the drivers' chunk state machine (reference: `SeedVCWrapper._stream_wave_chunks`,
    seed_vc_wrapper.py:201-285, non-streaming leg; the same statements inline at inference.py:507-527): appends this
    chunk's share of the output to `chunks` and returns (processed_frames, previous_chunk, should_break).
    vc_wave: (1, L) tensor.  The first chunk gives everything but its last `overlap_wave_len` samples, a middle chunk is
    crossfaded over its first `overlap_wave_len` samples with the tail kept from its predecessor and gives everything
    but its own tail, the last chunk is crossfaded and given whole; `processed_frames` advances by the chunk's frames
    minus `overlap_frame_len` (not at all when the first chunk is also the last, as in the reference)."""
    if processed_frames == 0:
        if is_last_chunk:
            chunks.append(vc_wave[0].cpu().numpy())
            return processed_frames, previous_chunk, True
        chunks.append(vc_wave[0, :-overlap_wave_len].cpu().numpy())
        return processed_frames + n_target_frames - overlap_frame_len, vc_wave[0, -overlap_wave_len:], False
    if is_last_chunk:
        chunks.append(crossfade(previous_chunk.cpu().numpy(), vc_wave[0].cpu().numpy(), overlap_wave_len))
        return processed_frames + n_target_frames - overlap_frame_len, previous_chunk, True
    chunks.append(crossfade(previous_chunk.cpu().numpy(), vc_wave[0, :-overlap_wave_len].cpu().numpy(), overlap_wave_len))
    return processed_frames + n_target_frames - overlap_frame_len, vc_wave[0, -overlap_wave_len:], False


def chunk_plan(n_src, max_source_window, overlap_frame_len):
    """Chunk boundaries of the reference driver's loop (inference.py:473-527): [(first source frame, frames, is_last)].
    They depend on lengths only: each chunk takes up to `max_source_window` frames and the next one starts
    `overlap_frame_len` frames before its end."""
    plan, processed = [], 0
    while processed < n_src:
        s_len = min(max_source_window, n_src - processed)
        is_last = processed + max_source_window >= n_src
        plan.append((processed, s_len, is_last))
        if is_last:
            break
        processed += s_len - overlap_frame_len
    return plan


def long_batch_plan(n_srcs, prompt_lens, max_context_window, overlap_frame_len=16, hop=1, max_chunks=64):
    """Chunk table of `HotPath.convert_long_batch` from lengths alone.  n_srcs[u] source frames and prompt_lens[u] prompt
    frames per utterance.  Each utterance is cut by `chunk_plan(n_src, max_context_window - P_u, overlap_frame_len)`, the
    chunks of all utterances are listed utterance-major:
      chunks       [(utterance, first source frame, frames, is_first, is_last)]
      bodies       [output samples chunk k contributes: (frames - (0 if is_last else overlap_frame_len)) * hop]
      out_lens     [output samples of utterance u] (0 for an utterance without source frames: it has no chunks)
      micro_batches[(k0, k1)]: consecutive ranges of at most `max_chunks` chunks, in plan order
    ValueError where the drivers' loop would not terminate (an utterance that needs more than one chunk while its window
    max_context_window - P_u does not exceed the overlap) and for max_chunks < 1."""
    if max_chunks < 1:
        raise ValueError(f"long_batch_plan: max_chunks = {max_chunks}, at least one chunk per micro-batch is needed")
    if len(n_srcs) != len(prompt_lens):
        raise ValueError("long_batch_plan: n_srcs and prompt_lens must have one entry per utterance")
    chunks, bodies, out_lens = [], [], []
    for u, (n_src, P) in enumerate(zip(n_srcs, prompt_lens)):
        n_src, window = int(n_src), int(max_context_window) - int(P)
        if n_src > window and window <= overlap_frame_len:
            raise ValueError(f"long_batch_plan: utterance {u} has {n_src} source frames, a window of {window} frames "
                             f"(max_context_window {max_context_window} - prompt {P}) and an overlap of {overlap_frame_len}: "
                             f"the chunk loop would not advance")
        total = 0
        for k, (p0, s_len, is_last) in enumerate(chunk_plan(n_src, window, overlap_frame_len)):
            chunks.append((u, p0, s_len, k == 0, is_last))
            bodies.append((s_len - (0 if is_last else overlap_frame_len)) * hop)
            total += bodies[-1]
        out_lens.append(total)
    micro = [(k0, min(k0 + max_chunks, len(chunks))) for k0 in range(0, len(chunks), max_chunks)]
    return dict(chunks=chunks, bodies=bodies, out_lens=out_lens, micro_batches=micro)


# ------------------------------------------------------------ long-form streaming: the schedule and the splice, on the host
def _ramp_size(m, first_chunks, growth, max_chunks):
    """Chunks of micro-batch m of the streaming ramp: min(max_chunks, ceil(first_chunks * growth ** m))."""
    size = first_chunks
    for _ in range(m):
        if size >= max_chunks:
            break
        size *= growth
    return min(int(max_chunks), int(math.ceil(size)))


def _ramp_args(what, n_chunks, first_chunks, growth, max_chunks):
    """The ramp's (first_chunks, growth, max_chunks) behind their checks; first_chunks None = one chunk per file that has one."""
    if max_chunks < 1:
        raise ValueError(f"{what}: max_chunks = {max_chunks}, at least one chunk per micro-batch is needed")
    if growth < 1:
        raise ValueError(f"{what}: growth = {growth}, a ramp that shrinks never reaches max_chunks")
    if first_chunks is None:
        first_chunks = max(1, sum(1 for n in n_chunks if n > 0))
    if first_chunks < 1:
        raise ValueError(f"{what}: first_chunks = {first_chunks}, the first micro-batch needs at least one chunk")
    return min(first_chunks, max_chunks), growth, int(max_chunks)


def stream_schedule(n_chunks, first_chunks=None, growth=4, max_chunks=64):
    """The order in which `convert_long_stream` runs the chunks of its files, from the chunk counts alone.  n_chunks[u]: chunks
    of file u.
      order        [(file, chunk)], chunk-major: chunk 0 of every file that has one, then chunk 1, ... -- every file's first
                   audio comes before any file's tail (`long_batch_plan` lists utterance-major: best for the whole call)
      micro_batches[(i0, i1)]: consecutive ranges of `order`; micro-batch m has min(max_chunks, ceil(first_chunks * growth ** m))
                   chunks, first_chunks None = one per file with chunks (capped at max_chunks): small early micro-batches
                   bring the first audio forward, large late ones use the device as the pool does.  growth 4 is the
                   measured choice: first audio as early as with 2, less of the call spent in small batches.
    growth=1, first_chunks=max_chunks with one file is `long_batch_plan`'s partition.  ValueError for first_chunks < 1,
    growth < 1, max_chunks < 1."""
    n_chunks = [int(n) for n in n_chunks]
    first_chunks, growth, max_chunks = _ramp_args("stream_schedule", n_chunks, first_chunks, growth, max_chunks)
    order = [(u, k) for k in range(max(n_chunks, default=0)) for u, n in enumerate(n_chunks) if k < n]
    micro, i0, m = [], 0, 0
    while i0 < len(order):
        i1 = min(len(order), i0 + _ramp_size(m, first_chunks, growth, max_chunks))
        micro.append((i0, i1))
        i0, m = i1, m + 1
    return dict(order=order, micro_batches=micro)


_SplicePiece = collections.namedtuple("_SplicePiece", "file offset chunk len prev_chunk prev_len begin end final")


class _StreamSplicer:
    """Which samples of which chunk waves may be handed out, as the chunks of `n_files` files complete in any order (host
    integers only).  chunks_per_file[u]: chunks of file u by plan; ov: samples of the cross-fade.

    `complete(file, chunk, samples, plan_is_last)` -> the pieces that became deliverable, in file order:
    _SplicePiece(file, offset = the piece's first sample in the file, chunk, len, prev_chunk (-1: no seam), prev_len, begin,
    end, final) -- samples begin .. end - 1 of `chunk`, cross-faded below ov with the last ov samples of `prev_chunk`, the
    arguments of `svc_chunks_emit` once the caller has mapped chunks to rows.  A chunk's piece is released only when every
    earlier chunk of its file is complete.  The keep rule is `v2_seam_plan`'s: kept = samples >= 2 ov, or the file's last
    chunk by plan; an empty chunk is never kept.  keep_all (a v1 plan, `long_batch_plan`): every chunk is kept, as
    `svc_chunks_assemble` takes them -- a window may be shorter than two overlaps there, and a chunk before the last has at
    least ov samples (ValueError otherwise).  A kept chunk that may still get a kept successor delivers
    [0, len - ov) and holds its tail for the seam; when the file's last chunk is not kept, the held tail of the last kept
    chunk is one more piece of that chunk (chunk = its index, [len - ov, len)).  The piece that ends a file has final=True;
    a file without a kept chunk ends with one empty final piece (chunk -1), and `start()` gives those of the files without
    chunks.  Over any completion order a file's pieces laid end to end are `v2_seam_plan` / `long_batch_plan` +
    `svc_chunks_assemble` on the same lengths."""

    def __init__(self, n_files, chunks_per_file, ov, keep_all=False):
        if len(chunks_per_file) != n_files:
            raise ValueError("_StreamSplicer: chunks_per_file must have one entry per file")
        self.ov, self.keep_all = int(ov), bool(keep_all)
        self.n = [int(c) for c in chunks_per_file]
        self.lens = [[None] * c for c in self.n]
        self.next = [0] * n_files               # first chunk of the file that is not spliced yet
        self.held = [None] * n_files            # (chunk, len, prev_chunk, prev_len) of the kept chunk whose tail waits
        self.offset = [0] * n_files             # samples of the file handed out so far

    def start(self):
        return [_SplicePiece(u, 0, -1, 0, -1, 0, 0, 0, True) for u, c in enumerate(self.n) if c == 0]

    def _piece(self, u, chunk, n, prev, begin, end, final):
        p = _SplicePiece(u, self.offset[u], chunk, n, prev[0], prev[1], begin, end, final)
        self.offset[u] += end - begin
        return p

    def complete(self, file, chunk, samples, plan_is_last):
        u, k, ov = int(file), int(chunk), self.ov
        if not 0 <= u < len(self.n) or not 0 <= k < self.n[u] or self.lens[u][k] is not None or samples < 0:
            raise ValueError(f"_StreamSplicer: file {file}, chunk {chunk}: no such chunk, completed twice, or a negative length")
        if bool(plan_is_last) != (k == self.n[u] - 1):
            raise ValueError(f"_StreamSplicer: file {file}, chunk {chunk}: the plan's last chunk is the file's last chunk, and no other")
        self.lens[u][k] = int(samples)
        out = []
        while self.next[u] < self.n[u] and self.lens[u][self.next[u]] is not None:
            j = self.next[u]
            n, ends = self.lens[u][j], j == self.n[u] - 1
            self.next[u] += 1
            held = self.held[u]
            prev = (held[0], held[1]) if held is not None else (-1, 0)
            if self.keep_all or (n > 0 and (n >= 2 * ov or ends)):
                if ends:
                    out.append(self._piece(u, j, n, prev, 0, n, True))
                    self.held[u] = None
                else:
                    if n < ov:
                        raise ValueError(f"_StreamSplicer: file {u}, chunk {j}: {n} samples, shorter than the overlap of {ov}")
                    if n > ov:
                        out.append(self._piece(u, j, n, prev, 0, n - ov, False))
                    self.held[u] = (j, n) + prev
            elif ends:
                if held is not None:
                    out.append(self._piece(u, held[0], held[1], held[2:], held[1] - ov, held[1], True))
                    self.held[u] = None
                else:
                    out.append(self._piece(u, -1, 0, (-1, 0), 0, 0, True))
        return out


StreamPiece = collections.namedtuple("StreamPiece", "file offset wave final parts", defaults=(None,))
StreamPiece.__doc__ = """One piece of a file's audio as `convert_long_stream` hands it out: samples offset .. offset + n - 1 of
file `file` in `wave` (1, n), float32 or int16; final: the piece that ends its file (it may be empty); parts: the v2 call's
return_parts (the per-chunk dicts of the chunks whose waves completed with this piece), else None."""


def collect_stream(pieces, n_files):
    """The pieces of `convert_long_stream` -> a list of n_files (1, L_u) tensors, what `convert_long_batch` returns.
    ValueError unless every file's pieces are contiguous, start at 0 and end with exactly one `final`."""
    waves, at, done = [[] for _ in range(n_files)], [0] * n_files, [False] * n_files
    for p in pieces:
        if not 0 <= p.file < n_files:
            raise ValueError(f"collect_stream: a piece of file {p.file}, {n_files} files expected")
        if done[p.file]:
            raise ValueError(f"collect_stream: file {p.file}: a piece after its final piece")
        if p.offset != at[p.file]:
            raise ValueError(f"collect_stream: file {p.file}: a piece at sample {p.offset}, {at[p.file]} expected (a gap or an overlap)")
        waves[p.file].append(p.wave)
        at[p.file] += p.wave.size(1)
        done[p.file] = bool(p.final)
    missing = [u for u in range(n_files) if not done[u]]
    if missing:
        raise ValueError(f"collect_stream: files {missing} have no final piece")
    return [torch.cat(w, dim=1) for w in waves]


def derive_seed(seed, index):
    """The seed of part `index` (a chunk of a file, a block of a stream) of the request seeded `seed`: the splitmix64
    finaliser of (seed + (index + 1) * 0x9E3779B97F4A7C15) mod 2^64.  A pure host function, a bijection of the 64-bit
    state for every index and injective in index for every seed; the one way the composite calls here make per-part seeds."""
    seed, index = int(seed), int(index)
    if not 0 <= seed < 1 << 64 or index < 0:
        raise ValueError(f"derive_seed: seed {seed} outside [0, 2^64) or index {index} negative")
    m = (1 << 64) - 1
    x = (seed + (index + 1) * 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _seed_list(what, seeds, n, z=None, vocoder_kwargs=None):
    """seeds of a pipeline call -> n host integers in [0, 2^64) (None stays None).  ValueError, before anything touches a
    device, for a wrong count, a seed out of range, and seeds given together with the tensors they stand for."""
    if seeds is None:
        return None
    if z is not None:
        raise ValueError(f"{what}: give seeds or z, not both")
    if vocoder_kwargs and ("phase0" in vocoder_kwargs or "noise" in vocoder_kwargs):
        raise ValueError(f"{what}: give seeds or phase0 / noise in vocoder_kwargs, not both")
    return _lib.seed_ints(seeds, n, what)


def _cfm_seeds(seeds):
    """The sampler call's seeds keyword, passed only when there are seeds (a stand-in sampler need not know it)."""
    return {} if seeds is None else {"seeds": seeds}


# ------------------------------------------------- the second half of every composite call: prompts, strip, vocoder
LOG_MEL_FLOOR = -11.512925464970229        # log(1e-5): the mel front-end's clamp (modules/audio.py:45-82)


def _file_settings(what, sampler, n, n_timesteps, inference_cfg_rate, random_voice=False):
    """`sampler=` of the long-form entry points -> None (sampler is None: the calls made without it), or one
    `cfm.sampler_setting` tuple per file, a file whose entry is None getting the call's arguments."""
    if sampler is None:
        return None
    from .cfm import sampler_setting
    sampler = list(sampler)
    if len(sampler) != n:
        raise ValueError(f"{what}: {len(sampler)} sampler entries for {n} files")
    call = sampler_setting((n_timesteps, inference_cfg_rate, 1.0, random_voice), what)
    return [call if e is None else sampler_setting(e, f"{what}: sampler[{u}]") for u, e in enumerate(sampler)]


def _stack_prompts(records, device=None):
    """records: [(prompt_condition (1, P_b, Dc), mel (1, C, P_b), style (1, Ds))], one per reference -> dict(prompt_condition
    (n, Pmax, Dc), mel (n, C, Pmax), style (n, Ds), P = [P_b], Pmax), zero beyond each P_b."""
    device = records[0][0].device if device is None else device
    P = [int(mel.size(2)) for _, mel, _ in records]
    Pmax = max(P)
    pc = torch.zeros(len(records), Pmax, records[0][0].size(2), device=device)
    mel = torch.zeros(len(records), records[0][1].size(1), Pmax, device=device)
    for b, (c, m, _) in enumerate(records):
        pc[b, :P[b]] = c[0]
        mel[b, :, :P[b]] = m[0]
    return dict(prompt_condition=pc, mel=mel, style=torch.cat([_lib.f32c(s, device) for _, _, s in records]), P=P, Pmax=Pmax)


@torch.inference_mode()
def enrol_references(mel_fn, campplus, waves, lens, waves_16k, lens_16k):
    """B reference clips of different lengths -> their prompt mels and style vectors, in three library calls instead of B x
    (mel + fbank + CAMPPlus): mel_fn a `MelSpectrogram`, campplus a `CAMPPlus`; waves (B, L) at the mel rate with lens[b]
    samples each, waves_16k (B, L16) at 16 kHz with lens_16k[b] samples each (`to_16k` makes them on the device;
    `enrol_references_audio` is this call with that step in front).
    -> dict(prompt (B, n_mels, Pmax) with zeros above each clip's frames, prompt_lens [P_b], style (B, E)): `prompt`,
    `prompt_lens` and `style` of `HotPath.convert_batch_ragged`; prompt[b:b + 1, :, :P_b] and style[b:b + 1] are the
    `target_mel` and `style` of `V2HotPath.prepare_target`.  Row b is what `mel_fn(waves[b:b + 1, :lens[b]])` and
    `campplus.style(waves_16k[b, :lens_16k[b]])` give (`svc_mel_forward_ragged`, `svc_kaldi_fbank_ragged`,
    `svc_campplus_forward_ragged`).  Everything is enqueued from the host integers: no synchronisation.  Pass waves with
    L == max(lens): columns above the longest clip are cut off before the mel call, which costs a copy of the batch."""
    lens, lens_16k = _lib.int_list(lens), _lib.int_list(lens_16k)
    B = waves.size(0)
    if len(lens) != B or len(lens_16k) != B or waves_16k.size(0) != B:
        raise ValueError(f"enrol_references: {len(lens)} lens and {len(lens_16k)} lens_16k for {B} and {waves_16k.size(0)} clips")
    prompt = mel_fn(waves[:, :max(lens)], lens=lens, pad_value=0.0)
    return dict(prompt=prompt, prompt_lens=[n // mel_fn.hop for n in lens], style=campplus.style_batch(waves_16k, lens_16k))


@torch.inference_mode()
def to_16k(resample, waves, lens):
    """B clips at the file's rate -> (waves_16k (B, resample.out_len(L)), lens_16k): the drivers'
    `torchaudio.functional.resample(wave, sr, 16000)` (inference.py:380-406) for a batch of clips of different lengths, in one
    `svc_resample` call.  resample: an `audio.Resample(sr, 16000)`; waves (B, L) with lens[b] samples each (host integers).  Row b's
    first lens_16k[b] = resample.out_len(lens[b]) samples are clip b resampled alone, the samples above are 0.0.  This is the one
    place the 16 kHz length is computed; what it returns is what `enrol_references`, `f0_conditions`, `content_conditions` and
    `v2_content_tokens` take.  Nothing is synchronised."""
    return resample(waves, lens)


@torch.inference_mode()
def enrol_references_audio(mel_fn, campplus, resample, waves, lens):
    """`enrol_references` from audio at the mel rate alone: the 16 kHz copies come from `to_16k` (resample: an
    `audio.Resample(mel rate, 16000)`), so the prompt mels and style vectors of up to 64 reference clips take four library calls."""
    return enrol_references(mel_fn, campplus, waves, lens, *to_16k(resample, waves, lens))


@torch.inference_mode()
def f0_conditions(rmvpe, src_16k, src_lens, ref_16k, ref_lens, auto_f0_adjust=True, pitch_shift=0):
    """The drivers' F0 block for B (source, reference) pairs: `F0_ori = rmvpe.infer_from_audio(ref_16k)`,
    `F0_alt = rmvpe.infer_from_audio(src_16k)`, the voiced-median shift in the log domain and the semitone shift, in two
    `RMVPE.f0_batch` calls and one `svc_f0_adjust`.  src_16k (B, Ls) / ref_16k (B, Lr) at 16 kHz with src_lens[b] / ref_lens[b]
    samples each (host integers; `to_16k` gives both from audio at the file's rate); pitch_shift a number of semitones or one per row.
    -> (F0_ori (B, To), ori_frames, shifted_f0_alt (B, Ta), alt_frames): the tracks and host frame counts that
    `length_regulator(mel2, ylens=..., f0=F0_ori, f0_lens=ori_frames)` and `length_regulator(S_alt, ylens=..., f0=shifted_f0_alt,
    f0_lens=alt_frames)` take.  Nothing is synchronised."""
    from .rmvpe import f0_adjust
    src_lens, ref_lens = _lib.int_list(src_lens), _lib.int_list(ref_lens)
    B = src_16k.size(0)
    if len(src_lens) != B or len(ref_lens) != B or ref_16k.size(0) != B:
        raise ValueError(f"f0_conditions: {len(src_lens)} src_lens and {len(ref_lens)} ref_lens for {B} and {ref_16k.size(0)} clips")
    f0_ori = rmvpe.f0_batch(ref_16k, ref_lens)
    f0_alt = rmvpe.f0_batch(src_16k, src_lens)
    ori_frames = [rmvpe.frames(n) for n in ref_lens]
    alt_frames = [rmvpe.frames(n) for n in src_lens]
    shifted = f0_adjust(f0_alt, alt_frames, f0_ori, ori_frames, auto_f0_adjust, pitch_shift)
    return f0_ori, ori_frames, shifted, alt_frames


@torch.inference_mode()
def content_conditions(whisper, length_regulator, src_16k, src_lens, src_ylens, ref_16k, ref_lens, ref_ylens, f0_src=None, f0_ref=None,
                       overlap_s=5.0):
    """The drivers' content block for B (source, reference) pairs: `S_alt = semantic_fn(src_16k)`, `S_ori = semantic_fn(ref_16k)`
    (with their loop over the windows of a long clip), `cond = length_regulator(S_alt, ylens=..., f0=shifted_f0_alt)[0]` and
    `prompt_condition = length_regulator(S_ori, ylens=..., f0=F0_ori)[0]`: one `WhisperContent.content_batch` call over the 2 B clips
    and two regulator calls, with no host round trip between the stages.  src_16k (B, Ls) / ref_16k (B, Lr) at 16 kHz with
    src_lens[b] / ref_lens[b] samples each (host integers; `to_16k` gives both from audio at the file's rate); src_ylens /
    ref_ylens: the target frame counts (B integers);
    f0_src / f0_ref: None, or (track (B, T), frames) pairs as `f0_conditions` returns them; overlap_s: the windows' overlap (the
    drivers' 5 s).
    -> (cond (B, max(src_ylens), C), prompt_condition (B, max(ref_ylens), C))."""
    src_lens, ref_lens = _lib.int_list(src_lens), _lib.int_list(ref_lens)
    B = src_16k.size(0)
    if len(src_lens) != B or len(ref_lens) != B or ref_16k.size(0) != B:
        raise ValueError(f"content_conditions: {len(src_lens)} src_lens and {len(ref_lens)} ref_lens for {B} and {ref_16k.size(0)} clips")
    L = max(src_16k.size(1), ref_16k.size(1))
    waves = torch.zeros(2 * B, L, device=whisper.device)
    waves[:B, :src_16k.size(1)] = _lib.f32c(src_16k, whisper.device)
    waves[B:, :ref_16k.size(1)] = _lib.f32c(ref_16k, whisper.device)
    S, rows = whisper.content_batch(waves, src_lens + ref_lens, overlap_s=overlap_s)
    ylens = lambda v: torch.as_tensor(_lib.int_list(v), dtype=torch.long)      # noqa: E731
    f0a, fla = f0_src if f0_src is not None else (None, None)
    f0o, flo = f0_ref if f0_ref is not None else (None, None)
    cond = length_regulator(S[:B], ylens=ylens(src_ylens), f0=f0a, in_lens=rows[:B], f0_lens=fla)[0]
    prompt_condition = length_regulator(S[B:], ylens=ylens(ref_ylens), f0=f0o, in_lens=rows[B:], f0_lens=flo)[0]
    return cond, prompt_condition


def _assemble_cond(prompt_condition, P, cond, S, T):
    """mu (n, T, Dc): row b is prompt_condition[b, :P[b]], then cond[b, :S[b]], then zeros (`svc_v2_assemble_cond`).
    prompt_condition (n, Pmax, Dc) and cond (n, >= max(S), Dc) on one device, P / S host integers."""
    cond = _lib.f32c(cond, prompt_condition.device)
    n, Dc = cond.size(0), cond.size(2)
    mu = torch.empty(n, T, Dc, device=cond.device)
    _lib.check(_lib.lib().svc_v2_assemble_cond(_lib.ptr(prompt_condition), _lib.i32_host(P), _lib.ptr(cond), _lib.i32_host(S), n,
                                               prompt_condition.size(1), max(S), Dc, T, _lib.ptr(mu), _lib.stream_ptr()))
    return mu


def _strip_prompt(mel, P, x_lens, Smax):
    """vc (n, C, Smax): row b is mel[b, :, P[b]:x_lens[b]], then the log-mel floor (`svc_mel_strip_prompt`; inference.py:505
    for a ragged batch).  mel (n, C, T) as the sampler returns it, P / x_lens host integers."""
    mel = _lib.f32c(mel)
    n, Cm, T = mel.shape
    vc = torch.empty(n, Cm, Smax, device=mel.device)
    _lib.check(_lib.lib().svc_mel_strip_prompt(_lib.ptr(mel), _lib.i32_host(P), _lib.i32_host(x_lens), n, Cm, T, Smax,
                                               C.c_float(LOG_MEL_FLOOR), _lib.ptr(vc), _lib.stream_ptr()))
    return vc


def group_by_length(lengths):
    """{S: [indices b with lengths[b] == S]} for S > 0, in order of first appearance: the grouped vocoder path runs once
    per group, because a plain vocoder call has no length argument and its convolutions would see another utterance's
    padding (the ragged call, `BigVGAN.__call__(mel, lens=...)`, takes the lengths instead)."""
    groups = {}
    for b, s in enumerate(lengths):
        if s > 0:
            groups.setdefault(int(s), []).append(b)
    return groups


def _index_runs(members):
    """[(a, b)]: the sorted indices `members` as consecutive ranges a .. b - 1 (slices need no index tensor on the device)."""
    runs = []
    for i in members:
        if runs and runs[-1][1] == i:
            runs[-1][1] = i + 1
        else:
            runs.append([i, i + 1])
    return [tuple(r) for r in runs]


_VocoderCall = collections.namedtuple("_VocoderCall", "runs frames mel wave")


def _vocoder_seeds(vocoder, seeds):
    """{"seeds": seeds} for a vocoder that draws (HiFT), {} for one that does not (BigVGAN) or without seeds."""
    from .vocoder import HiFT
    return {"seeds": seeds} if seeds is not None and isinstance(vocoder, HiFT) else {}


def _vocode(vocoder, vc, S, ragged, what, hop=None, seeds=None, seed_kw=None, vocoder_kwargs=None, row_kwargs=None):
    """The vocoder calls of a batch: vc (n, C, Smax) as `_strip_prompt` gives it, S the n host lengths.  A batch of one
    length is one plain call on vc itself; one of several lengths is ONE `vocoder(vc, lens=S)` call with `ragged`, else one
    plain call per `group_by_length` group, its rows gathered as slices (`_index_runs`: no index tensor, no host-to-device
    copy).  A row without frames gets no call of its own.
    seeds (n integers) reach a call as `seed_kw(its rows' seeds)` (default: `_vocoder_seeds`, i.e. only a HiFT is given
    seeds); vocoder_kwargs describe all n rows and go to a call that covers them; row_kwargs ([dict of (1, ...) tensors] per
    row, HiFT's pinned draws) are concatenated in the order of a call's rows.  With `hop` a call that does not give
    frames x hop samples per row is a ValueError.
    -> [_VocoderCall(runs = row ranges [(a, b)], frames, mel = the mel passed (rows, C, frames), wave (rows, samples))]."""
    n, Smax = vc.size(0), vc.size(2)
    everyone = list(range(n))
    if len(set(S)) <= 1:
        todo = [(S[0], everyone, {})] if S and S[0] > 0 else []
    elif ragged:
        todo = [(Smax, everyone, {"lens": S})]
    else:
        todo = [(frames, members, {}) for frames, members in group_by_length(S).items()]
    calls = []
    for frames, members, kw in todo:
        runs = [(0, n)] if members is everyone else _index_runs(members)
        whole = members is everyone and frames == Smax
        if vocoder_kwargs:
            if not whole:
                raise ValueError(f"{what}: vocoder_kwargs describe the whole batch, a call per length needs them per row")
            kw.update(vocoder_kwargs)
        if row_kwargs:
            kw.update({key: torch.cat([row_kwargs[i][key] for i in members]) for key in row_kwargs[members[0]]})
        if seeds is not None:
            part = seeds if whole else [seeds[i] for i in members]
            kw.update(seed_kw(part) if seed_kw is not None else _vocoder_seeds(vocoder, part))
        m = vc if whole else torch.cat([vc[a:b, :, :frames] for a, b in runs]).contiguous()
        wave = vocoder(m, **kw).reshape(len(members), -1)
        if hop is not None and wave.size(1) != frames * hop:
            raise ValueError(f"{what}: the vocoder gave {wave.size(1)} samples per row, {frames * hop} expected (frames x hop)")
        calls.append(_VocoderCall(runs, frames, m, wave))
    return calls


def _row_views(vc, S, calls):
    """`_vocode`'s calls as one (mel (1, C, S_b), wave (1, S_b * hop)) pair of views per row; empty for a row without a call."""
    rows = [(vc[b:b + 1, :, :0], vc.new_zeros(1, 0)) if s == 0 else None for b, s in enumerate(S)]
    for call in calls:
        hop = call.wave.size(1) // call.frames
        for j, b in enumerate(b for run in call.runs for b in range(*run)):
            rows[b] = (call.mel[j:j + 1, :, :S[b]], call.wave[j:j + 1, :S[b] * hop])
    return rows


class _PoolFiles:
    """The files of a chunk pool behind their checks, stacked once: condition rows along time, prompts padded to Pmax, and the
    chunk table of `long_batch_plan`.  `what` names the entry point in errors."""

    def __init__(self, what, utterances, max_context_window, overlap_frame_len, hop, max_chunks):
        for u, (cond, pc, mel2, style2) in enumerate(utterances):
            if pc.size(1) != mel2.size(2):
                raise ValueError(f"{what}: utterance {u}: prompt_condition has {pc.size(1)} frames, mel2 {mel2.size(2)}")
        self.U = len(utterances)
        self.P = [int(t[2].size(2)) for t in utterances]
        self.n_src = [int(t[0].size(1)) for t in utterances]
        self.plan = long_batch_plan(self.n_src, self.P, max_context_window, overlap_frame_len, hop, max_chunks)
        self.dev = utterances[0][0].device
        self.utterances = utterances

    def stack(self):
        """The device tensors (called under the files' device, once there is a chunk to run)."""
        t0, dev = self.utterances[0], self.dev
        self.Dc, self.Cm = t0[0].size(2), t0[2].size(1)
        self.cond_all = torch.cat([_lib.f32c(t[0], dev)[0] for t in self.utterances])
        self.row_base = [sum(self.n_src[:u]) for u in range(self.U)]
        st = _stack_prompts([t[1:] for t in self.utterances], dev)
        self.pc_all, self.mel_all, self.style_all, self.Pmax = st["prompt_condition"], st["mel"], st["style"], st["Pmax"]

    def prompts_of(self, utt):
        """(mel, style) rows of the chunks whose files are `utt`."""
        if self.U > 1:
            idx = torch.tensor(utt, device=self.dev)
            return self.mel_all.index_select(0, idx), self.style_all.index_select(0, idx)
        return self.mel_all.expand(len(utt), -1, -1), self.style_all.expand(len(utt), -1)


def _pool_micro_batch(what, cfm, vocoder, files, mb, mel_rows, style_rows, waves, row0, n_timesteps, inference_cfg_rate, hop, noise_of,
                      kwargs_of, mb_seeds, seed_kw, ragged_vocoder, cfm_kwargs, file_settings):
    """One micro-batch of a chunk pool: `svc_chunks_gather_cond` -> one sampler call with per-row x_lens / prompt_lens ->
    `_strip_prompt` -> `_vocode` -> rows row0 .. of the chunk-wave buffer `waves`.  files: a stacked `_PoolFiles`; mb: the
    micro-batch's entries of its chunk table; mel_rows / style_rows: the chunks' prompt rows; noise_of(i, T) / kwargs_of(i, S):
    None, or the pinned sampler noise / vocoder draws of the micro-batch's chunk i."""
    i32, dev, P = _lib.i32_host, files.dev, files.P
    n = len(mb)
    S = [c[2] for c in mb]
    Pk = [P[c[0]] for c in mb]
    x_lens = [p + s for p, s in zip(Pk, S)]
    T = max(x_lens)
    mu = torch.empty(n, T, files.Dc, device=dev)
    _lib.check(_lib.lib().svc_chunks_gather_cond(_lib.ptr(files.pc_all), i32(P), files.U, files.Pmax, _lib.ptr(files.cond_all),
                                                 files.cond_all.size(0), i32([c[0] for c in mb]),
                                                 i32([files.row_base[c[0]] + c[1] for c in mb]), i32(S), n, files.Dc, T, _lib.ptr(mu),
                                                 _lib.stream_ptr()))
    z = None
    if noise_of is not None:
        z = torch.zeros(n, files.Cm, T, device=dev)
        for i, t_k in enumerate(x_lens):
            z[i, :, :t_k] = noise_of(i, t_k)[0]
    kws = [kwargs_of(i, s) for i, s in enumerate(S)] if kwargs_of is not None else None
    if file_settings is None:
        mel = cfm.inference(mu, x_lens, mel_rows, style_rows, None, n_timesteps, inference_cfg_rate=inference_cfg_rate,
                            z=z, prompt_lens=Pk, **_cfm_seeds(mb_seeds), **(cfm_kwargs or {}))
    else:
        mel = cfm.inference_rows(mu, x_lens, mel_rows, style_rows, [file_settings[c[0]] for c in mb],
                                 z=z, prompt_lens=Pk, **_cfm_seeds(mb_seeds))
    vc = _strip_prompt(mel, Pk, x_lens, max(S))
    for call in _vocode(vocoder, vc, S, ragged_vocoder, what, hop=hop, seeds=mb_seeds, seed_kw=seed_kw, row_kwargs=kws):
        j = 0
        for a, b in call.runs:       # rows of a call -> rows of the chunk wave buffer (slices: no synchronisation)
            waves[row0 + a:row0 + b, :call.frames * hop].copy_(call.wave[j:j + b - a])
            j += b - a


def _long_pool(cfm, vocoder, utterances, n_timesteps, inference_cfg_rate, hop, max_context_window, overlap_frame_len, noise_fn,
               vocoder_kwargs_fn, max_chunks, ragged_vocoder, seeds, seed_kw, cfm_kwargs=None, sampler=None):
    """The chunk pool of `HotPath.convert_long_batch` and of the timbre branch of `V2HotPath.convert_long_batch`, behind their
    argument checks: `long_batch_plan`, then per micro-batch `_pool_micro_batch` (`svc_chunks_gather_cond` -> one `cfm.inference`
    with per-row x_lens / prompt_lens -> `_strip_prompt` -> `_vocode` -> rows of one wave buffer), one `svc_chunks_assemble` and
    one host synchronisation at the end.  utterances, noise_fn, vocoder_kwargs_fn, ragged_vocoder (a bool here) and seeds (host
    integers or None) as `HotPath.convert_long_batch` documents them; seed_kw: `_vocode`'s; cfm_kwargs: further keywords of
    every sampler call (the v2 caller's `random_voice`); sampler: None, or per file a `cfm.sampler_setting` entry or None
    (checked by `_file_settings`): every chunk of a file then runs with its file's entry, the micro-batch in one
    `cfm.inference_rows` call."""
    U = len(utterances)
    if U == 0:
        return []
    file_settings = _file_settings("convert_long_batch", sampler, U, n_timesteps, inference_cfg_rate, **(cfm_kwargs or {}))
    files = _PoolFiles("convert_long_batch", utterances, max_context_window, overlap_frame_len, hop, max_chunks)
    plan = files.plan
    chunks, out_lens = plan["chunks"], plan["out_lens"]
    dev = files.dev
    ovw = overlap_frame_len * hop
    i32 = _lib.i32_host
    with torch.cuda.device(dev):
        out = torch.empty(sum(out_lens), device=dev, dtype=torch.float32)
        offs = [sum(out_lens[:u]) for u in range(U)]
        result = [out[o:o + n][None, :] for o, n in zip(offs, out_lens)]
        if not chunks:
            return result
        N = len(chunks)
        files.stack()
        utt = [c[0] for c in chunks]
        chunk_seeds = None
        if seeds is not None:       # chunk k of its file: the chunks are listed utterance-major
            first_of = {}
            for k, u in enumerate(utt):
                first_of.setdefault(u, k)
            chunk_seeds = [derive_seed(seeds[u], k - first_of[u]) for k, u in enumerate(utt)]
        mel_chunks, style_chunks = files.prompts_of(utt)
        fade_in, fade_out = (torch.from_numpy(w).to(dev) for w in _cos2_windows(ovw))
        stride = max(c[2] for c in chunks) * hop
        waves = torch.empty(N, stride, device=dev, dtype=torch.float32)      # row k: chunk k's waveform, lens[k] samples
        noise_of = (lambda i, t_k: noise_fn(t_k)) if noise_fn is not None else None
        kwargs_of = (lambda i, s: vocoder_kwargs_fn(s)) if vocoder_kwargs_fn is not None else None
        for k0, k1 in plan["micro_batches"]:
            _pool_micro_batch("convert_long_batch", cfm, vocoder, files, chunks[k0:k1], mel_chunks[k0:k1], style_chunks[k0:k1], waves, k0,
                              n_timesteps, inference_cfg_rate, hop, noise_of, kwargs_of,
                              chunk_seeds[k0:k1] if chunk_seeds is not None else None, seed_kw, ragged_vocoder, cfm_kwargs, file_settings)
        lens = [c[2] * hop for c in chunks]
        _lib.check(_lib.lib().svc_chunks_assemble(_lib.ptr(waves), C.c_longlong(stride), i32(lens), i32([int(c[3]) for c in chunks]),
                                                  i32([int(c[4]) for c in chunks]), N, _lib.ptr(fade_in), _lib.ptr(fade_out), ovw,
                                                  _lib.ptr(out), C.c_longlong(out.numel()), _lib.stream_ptr()))
        torch.cuda.current_stream(dev).synchronize()
    return result


# ------------------------------------------------------------------------ long-form streaming: emit, stage, hand out
class _StreamOut:
    """The delivery path of `convert_long_stream`: per micro-batch one `svc_chunks_emit` for the pieces the splicer released
    into a device staging buffer, one non-blocking copy into pinned host memory (to_host) and one event; `pop` waits for the
    oldest micro-batch's event -- never for the device or the stream -- and gives its `StreamPiece`s.  Pieces start at
    multiples of 4 samples of the staging buffer, so the 16-byte path of the kernel stays open to them."""

    def __init__(self, dev, ovw, pcm16, to_host):
        self.dev, self.ovw, self.pcm16, self.to_host = dev, ovw, pcm16, to_host
        self.fade_in, self.fade_out = (torch.from_numpy(w).to(dev) for w in _cos2_windows(ovw))
        self.pending = collections.deque()          # (event or None, [(piece, staging offset)], staging buffer, parts)
        self.carry = []

    def push(self, pieces, waves, rows, parts=None):
        """pieces: `_SplicePiece`s; waves (n_rows, stride): the chunk-wave buffer; rows[(file, chunk)] -> (row, samples it holds,
        first sample of the chunk it holds) for the chunks the pieces name.  Enqueues on the current stream."""
        if not pieces and not parts:
            return
        off, total = [], 0
        for p in pieces:
            off.append(total)
            total += -(-(p.end - p.begin) // 4) * 4
        buf = ev = None
        if total:
            i32 = _lib.i32_host
            a = dict(row=[], len=[], prev_row=[], prev_len=[], begin=[], end=[])
            for p in pieces:
                row, n, skip = rows[(p.file, p.chunk)] if p.chunk >= 0 else (0, 0, 0)
                prow, pn = -1, 0
                if p.prev_chunk >= 0 and p.begin < min(p.end, self.ovw):
                    prow, held, pskip = rows[(p.file, p.prev_chunk)]
                    pn = p.prev_len - pskip
                    assert held == pn and pn >= self.ovw
                assert n == p.len - skip and p.begin >= skip and (skip == 0 or prow < 0)      # a row that holds a tail only has no seam
                for key, v in zip(a, (row, n, prow, pn, p.begin - skip, p.end - skip)):
                    a[key].append(v)
            dev_f = torch.empty(total, device=self.dev, dtype=torch.float32)
            dev_p = torch.empty(total, device=self.dev, dtype=torch.int16) if self.pcm16 else None
            _lib.check(_lib.lib().svc_chunks_emit(_lib.ptr(waves), waves.stride(0), waves.size(0), i32(a["row"]), i32(a["len"]),
                                                  i32(a["prev_row"]), i32(a["prev_len"]), i32(a["begin"]), i32(a["end"]),
                                                  _lib.i64_host(off), len(pieces), _lib.ptr(self.fade_in), _lib.ptr(self.fade_out),
                                                  self.ovw, _lib.ptr(dev_f), _lib.ptr(dev_p), total, _lib.stream_ptr()))
            buf = dev_p if self.pcm16 else dev_f
            if self.to_host:
                host = torch.empty(total, dtype=buf.dtype, pin_memory=True)
                host.copy_(buf, non_blocking=True)
                buf = host
            ev = torch.cuda.Event()
            ev.record()
        self.pending.append((ev, list(zip(pieces, off)), buf, parts))

    def pop(self):
        """-> the `StreamPiece`s of the oldest pushed micro-batch, after its event; its parts ride on the first of them (parts of
        a micro-batch that released no piece wait for the next piece)."""
        ev, placed, buf, parts = self.pending.popleft()
        if ev is not None:
            ev.synchronize()
        dtype = torch.int16 if self.pcm16 else torch.float32
        empty = torch.empty(1, 0, dtype=dtype, device="cpu" if self.to_host else self.dev)
        out = []
        for p, o in placed:
            n = p.end - p.begin
            out.append(StreamPiece(p.file, p.offset, buf[o:o + n][None, :] if n else empty, p.final, None))
        if parts is not None:
            self.carry = self.carry + parts
        if out and self.carry:
            out[0] = out[0]._replace(parts=self.carry)
            self.carry = []
        return out


def _long_stream(what, cfm, vocoder, utterances, n_timesteps, inference_cfg_rate, hop, max_context_window, overlap_frame_len, noise_fn,
                 vocoder_kwargs_fn, max_chunks, first_chunks, growth, ragged_vocoder, seeds, seed_kw, pcm16, to_host, lookahead,
                 cfm_kwargs=None, sampler=None):
    """The generator behind `HotPath.convert_long_stream` and the timbre branch of `V2HotPath.convert_long_stream`, behind their
    argument checks: `long_batch_plan`'s chunks in `stream_schedule`'s order, per micro-batch `_pool_micro_batch` (the pool's
    body) into rows of one wave buffer in schedule order, then `_StreamOut.push` for the pieces `_StreamSplicer` released.
    Micro-batch m + lookahead is enqueued before micro-batch m's event is waited for."""
    U = len(utterances)
    if lookahead < 0:
        raise ValueError(f"{what}: lookahead = {lookahead}, a count of micro-batches enqueued ahead")
    if U == 0:
        return
    file_settings = _file_settings(what, sampler, U, n_timesteps, inference_cfg_rate, **(cfm_kwargs or {}))
    files = _PoolFiles(what, utterances, max_context_window, overlap_frame_len, hop, max_chunks)
    dev, ovw = files.dev, overlap_frame_len * hop
    by_file = [[c for c in files.plan["chunks"] if c[0] == u] for u in range(U)]
    sched = stream_schedule([len(c) for c in by_file], first_chunks, growth, max_chunks)
    order, micro = sched["order"], sched["micro_batches"]
    splicer = _StreamSplicer(U, [len(c) for c in by_file], ovw, keep_all=True)
    with torch.cuda.device(dev):
        out = _StreamOut(dev, ovw, pcm16, to_host)
        out.push(splicer.start(), None, {})
        if order:
            files.stack()
            chunks = [by_file[u][k] for u, k in order]
            rows = {uk: (i, chunks[i][2] * hop, 0) for i, uk in enumerate(order)}
            chunk_seeds = [derive_seed(seeds[u], k) for u, k in order] if seeds is not None else None
            waves = torch.empty(len(order), max(c[2] for c in chunks) * hop, device=dev, dtype=torch.float32)

    def enqueue(m):
        i0, i1 = micro[m]
        with torch.cuda.device(dev):
            mel_rows, style_rows = files.prompts_of([u for u, _ in order[i0:i1]])
            noise_of = (lambda i, T: noise_fn(*order[i0 + i], T)) if noise_fn is not None else None
            kwargs_of = (lambda i, S: vocoder_kwargs_fn(*order[i0 + i], S)) if vocoder_kwargs_fn is not None else None
            _pool_micro_batch(what, cfm, vocoder, files, chunks[i0:i1], mel_rows, style_rows, waves, i0, n_timesteps, inference_cfg_rate,
                              hop, noise_of, kwargs_of, chunk_seeds[i0:i1] if chunk_seeds is not None else None, seed_kw,
                              ragged_vocoder, cfm_kwargs, file_settings)
            pieces = [p for i in range(i0, i1) for p in splicer.complete(*order[i], chunks[i][2] * hop, chunks[i][4])]
            out.push(pieces, waves, rows)

    enqueued = 0
    while out.pending or enqueued < len(micro):
        # the first pending entry may be the empty files' pieces: micro-batches 0 .. lookahead are enqueued before it is handed out
        while enqueued < len(micro) and len(out.pending) <= lookahead:
            enqueue(enqueued)
            enqueued += 1
        if out.pending:
            yield from out.pop()


class HotPath:
    """cfm: seedvc_amd.cfm.CFM ; vocoder: seedvc_amd.vocoder.BigVGAN | HiFT."""

    def __init__(self, cfm, vocoder):
        self.cfm = cfm
        self.vocoder = vocoder

    def _vocoder_seeds(self, seeds):
        return _vocoder_seeds(self.vocoder, seeds)

    @torch.inference_mode()
    def convert_batch(self, mu, prompt, style, n_timesteps, inference_cfg_rate, z=None, x_lens=None,
                      prompt_lens=None, vocoder_kwargs=None, seeds=None):
        """B utterances (each an independent reference run): -> (mel (B,C,S), wave (B, S*hop)).  seeds: B integers in
        [0, 2^64), exclusive with z and with phase0 / noise in vocoder_kwargs: seeds[b] gives utterance b's sampler noise and,
        if the vocoder is a HiFT, its source draws, all made on the device (`CFM.inference`, `HiFT.__call__`)."""
        B, T = mu.size(0), mu.size(1)
        seeds = _seed_list("convert_batch", seeds, B, z, vocoder_kwargs)
        P = prompt.size(-1)
        lens = x_lens if x_lens is not None else torch.LongTensor([T] * B)
        mel = self.cfm.inference(mu, lens, prompt, style, None, n_timesteps, inference_cfg_rate=inference_cfg_rate,
                                 z=z, prompt_lens=prompt_lens, **_cfm_seeds(seeds))
        vc_target = mel[:, :, P:]                                   # inference.py:505
        wave = self.vocoder(vc_target.float(), **(vocoder_kwargs or {}), **self._vocoder_seeds(seeds))
        return vc_target, wave.reshape(B, -1)

    @torch.inference_mode()
    def convert_batch_ragged(self, mu, prompt, style, x_lens, prompt_lens, n_timesteps, inference_cfg_rate, z=None,
                             vocoder_kwargs=None):
        """B utterances of different lengths and prompts in one pass: mu (B, T, Dc), prompt (B, C, Pmax), style (B, Ds), x_lens /
        prompt_lens: B host integers each (prompt + output frames, prompt frames) -> list of B pairs (mel (1, C, S_b), wave
        (1, S_b * hop)), S_b = x_lens[b] - prompt_lens[b]: what `convert_batch` gives for each utterance alone.  The sampler with
        per-row lengths -> `_strip_prompt` -> `_vocode` with the ragged call, BigVGAN or HiFT (`svc_bigvgan_forward_ragged` /
        `svc_hift_forward_ragged`: no utterance sees its neighbour's padding).  vocoder_kwargs: HiFT's pinned f0 (B, Smax) /
        phase0 / noise (B, nh, Smax * up), row b being the draws of utterance b alone in its leading part (`convert_batch_ragged_seeded`: seeds instead of
        tensors).  Everything is enqueued from the host integers: no synchronisation."""
        return self._convert_batch_ragged(mu, prompt, style, x_lens, prompt_lens, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, None)

    @torch.inference_mode()
    def convert_batch_ragged_seeded(self, mu, prompt, style, x_lens, prompt_lens, n_timesteps, inference_cfg_rate, seeds,
                                    vocoder_kwargs=None):
        """`convert_batch_ragged` with seeds (B integers in [0, 2^64)) in place of z and of phase0 / noise in vocoder_kwargs
        (which may still pin HiFT's f0): utterance b's sampler noise and, if the vocoder is a HiFT, its source draws are those
        of seeds[b], made on the device, whatever its row, the padding and its neighbours -- bit for bit `convert_batch_ragged`
        fed `CFM.noise_draws` / `HiFT.noise_draws` of each seed.  (A method of its own: the parameter list of
        `convert_batch_ragged` is part of its contract.)"""
        if seeds is None:
            raise ValueError("convert_batch_ragged_seeded: seeds is None")
        return self._convert_batch_ragged(mu, prompt, style, x_lens, prompt_lens, n_timesteps, inference_cfg_rate, None, vocoder_kwargs,
                                          seeds)

    def _convert_batch_ragged(self, mu, prompt, style, x_lens, prompt_lens, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, seeds):
        B, T = mu.size(0), mu.size(1)
        seeds = _seed_list("convert_batch_ragged_seeded", seeds, B, z, vocoder_kwargs)
        x_lens, P = _lib.int_list(x_lens), _lib.int_list(prompt_lens)
        if len(x_lens) != B or len(P) != B:
            raise ValueError(f"convert_batch_ragged: {len(x_lens)} x_lens and {len(P)} prompt_lens for a batch of {B}")
        S = [t - p for t, p in zip(x_lens, P)]
        if min(S) < 0 or max(x_lens) > T or max(P) > prompt.size(-1) or min(P) < 0:
            raise ValueError("convert_batch_ragged: need 0 <= prompt_lens[b] <= x_lens[b] <= T and prompt_lens[b] <= prompt frames")
        with torch.cuda.device(mu.device):
            mel = self.cfm.inference(mu, x_lens, prompt, style, None, n_timesteps, inference_cfg_rate=inference_cfg_rate,
                                     z=z, prompt_lens=P, **_cfm_seeds(seeds))
            vc = _strip_prompt(mel, P, x_lens, max(max(S), 1))
            calls = _vocode(self.vocoder, vc, S, True, "convert_batch_ragged", seeds=seeds, seed_kw=self._vocoder_seeds,
                            vocoder_kwargs=vocoder_kwargs)
        return _row_views(vc, S, calls)

    @torch.inference_mode()
    def convert_long(self, cond, prompt_condition, mel2, style2, n_timesteps, inference_cfg_rate, hop,
                     max_context_window, overlap_frame_len=16, noise_fn=None, vocoder_kwargs_fn=None):
        """One long utterance, chunked exactly like the reference driver (inference.py:470-527): chunks of
        max_context_window - P source frames, advancing by S_chunk - 16, 16-frame cos^2 crossfade on the host.
        noise_fn(T) -> z (1,C,T) lets a caller pin the noise; vocoder_kwargs_fn(S) pins vocoder draws."""
        overlap_wave_len = overlap_frame_len * hop
        P = mel2.size(2)
        chunks, previous = [], None
        for p0, s_len, is_last in chunk_plan(cond.size(1), max_context_window - P, overlap_frame_len):
            cat_condition = torch.cat([prompt_condition, cond[:, p0:p0 + s_len]], dim=1)
            T = cat_condition.size(1)
            z = noise_fn(T) if noise_fn is not None else None
            vc_target = self.cfm.inference(cat_condition, torch.LongTensor([T]), mel2, style2, None, n_timesteps,
                                           inference_cfg_rate=inference_cfg_rate, z=z)[:, :, P:]
            kw = vocoder_kwargs_fn(vc_target.size(2)) if vocoder_kwargs_fn is not None else {}
            vc_wave = self.vocoder(vc_target.float(), **kw).reshape(1, -1)
            _, previous, _ = stream_wave_chunks(vc_wave, p0, vc_target.size(2), overlap_wave_len, overlap_frame_len, chunks,
                                                previous, is_last)
        return torch.tensor(np.concatenate(chunks))[None, :].float()

    @torch.inference_mode()
    def convert_long_device(self, cond, prompt_condition, mel2, style2, n_timesteps, inference_cfg_rate, hop,
                            max_context_window, overlap_frame_len=16, noise_fn=None, vocoder_kwargs_fn=None):
        """`convert_long` with everything kept on the device: same chunk boundaries, the cos^2
        crossfade done by `svc_crossfade` in the reference's float64 arithmetic (bit-identical), output assembled in one
        device buffer, and the vocoder of chunk k running on a second HIP stream beside the sampler of chunk k+1.
        One host synchronisation at the end instead of two `.cpu()` round trips per chunk."""
        dev = cond.device
        ovw = overlap_frame_len * hop
        P = mel2.size(2)
        plan = long_batch_plan([cond.size(1)], [P], max_context_window, overlap_frame_len, hop)     # one file: its chunks and samples
        out = torch.empty(plan["out_lens"][0], device=dev, dtype=torch.float32)
        fade_in, fade_out = (torch.from_numpy(w).to(dev) for w in _cos2_windows(ovw))
        s_main = torch.cuda.current_stream(dev)
        s_voc = Lanes._lane_stream(torch.device(dev), "vocoder")      # one per device for the process (see Lanes)
        s_voc.wait_stream(s_main)
        off, prev_tail, keep = 0, None, []
        for k, (_, p0, s_len, _, is_last) in enumerate(plan["chunks"]):
            cat_condition = torch.cat([prompt_condition, cond[:, p0:p0 + s_len]], dim=1)
            T = cat_condition.size(1)
            z = noise_fn(T) if noise_fn is not None else None
            vc_target = self.cfm.inference(cat_condition, torch.LongTensor([T]), mel2, style2, None, n_timesteps,
                                           inference_cfg_rate=inference_cfg_rate, z=z)[:, :, P:]
            kw = vocoder_kwargs_fn(vc_target.size(2)) if vocoder_kwargs_fn is not None else {}
            ready = torch.cuda.Event()
            ready.record(s_main)
            s_voc.wait_event(ready)
            with torch.cuda.stream(s_voc):
                wave = self.vocoder(vc_target.float(), **kw).reshape(-1)
                body = wave if is_last else wave[:-ovw]
                if k > 0:
                    n = min(body.numel(), ovw)
                    _lib.check(_lib.lib().svc_crossfade(_lib.ptr(body), _lib.ptr(prev_tail), _lib.ptr(fade_in),
                                                        _lib.ptr(fade_out), n, _lib.stream_ptr()))
                out[off:off + body.numel()].copy_(body)
                off += body.numel()
                prev_tail = None if is_last else wave[-ovw:]
                keep.append((vc_target, wave))          # alive until the side stream has consumed them
        s_main.wait_stream(s_voc)
        torch.cuda.current_stream(dev).synchronize()
        del keep
        return out[None, :]

    @torch.inference_mode()
    def convert_long_batch(self, utterances, n_timesteps, inference_cfg_rate, hop, max_context_window, overlap_frame_len=16,
                           noise_fn=None, vocoder_kwargs_fn=None, max_chunks=64, ragged_vocoder=None, seeds=None, *, sampler=None):
        """Long-form conversion of one or more files with every chunk in ONE pool: a chunk reads the source, its file's
        prompt and fresh noise, never its neighbour, so the chunks of all files go through the sampler and the vocoder as
        ragged batches of up to `max_chunks` chunks, and one launch cross-fades and concatenates them (`svc_chunks_assemble`:
        the reference's float64 arithmetic, bit for bit).

        utterances: list of (cond (1, n_src, Dc), prompt_condition (1, P, Dc), mel2 (1, C, P), style2 (1, Ds)), the
        arguments of `convert_long_device`, one tuple per file.  -> list of (1, L_u) tensors (views of one buffer); per
        file the chunk boundaries (`chunk_plan`), the cross-fade and the length of the drivers' loop run on it alone.  A file
        without source frames gives (1, 0).

        Per micro-batch (`long_batch_plan`, plan order = utterance-major): `svc_chunks_gather_cond` -> one `cfm.inference`
        with per-row x_lens / prompt_lens -> `_strip_prompt` -> `_vocode` -> rows of one wave buffer.  Seams are resolved
        once, after the last micro-batch, so a seam may cross micro-batches.
        ragged_vocoder (`_vocode`'s `ragged`): None = the ragged call if the vocoder is a `BigVGAN`, else one plain call per
        distinct chunk length (a file has at most two: full windows and its last chunk); True / False force it, for either
        vocoder (a caller who wants pinned draws in the ragged call wraps the vocoder).  vocoder_kwargs_fn(S) -> dict of
        tensors with a leading batch axis of 1 (pinned draws) is called once per chunk in plan order and concatenated per
        length group; it cannot be combined with the ragged call.
        noise_fn(T_k) -> (1, C, T_k) is called once per chunk in plan order with T_k = P_u + frames, the calls of the
        sequential loops.  With noise_fn=None the noise is one torch.randn per micro-batch: the same distribution, NOT the
        stream of draws the sequential loops consume.
        seeds: one integer in [0, 2^64) per file, exclusive with noise_fn and vocoder_kwargs_fn: chunk k of file u draws its
        sampler noise and, if the vocoder draws (`_vocoder_seeds`), its source draws from `derive_seed(seeds[u], k)`, on the
        device and inside the batched calls -- a file's audio is then a function of its own inputs and seed, whatever shares
        the pool.  The ragged call of such a vocoder is allowed with seeds (ragged_vocoder=True): there are no positional draws.
        sampler: per file a sampler setting -- a dict or (n_timesteps, inference_cfg_rate, temperature=1.0) as
        `CFM.inference_rows` takes it -- or None for the call's arguments; every chunk of a file uses its file's entry and a
        micro-batch is still one sampler call (`CFM.inference_rows`: files of one class share its launches).  sampler=None:
        every call is made with n_timesteps / inference_cfg_rate, as without the keyword.
        One host synchronisation, at the end."""
        if seeds is not None and (noise_fn is not None or vocoder_kwargs_fn is not None):
            raise ValueError("convert_long_batch: give seeds or noise_fn / vocoder_kwargs_fn, not both")
        seeds = _seed_list("convert_long_batch", seeds, len(utterances))
        if ragged_vocoder is None:
            from .vocoder import BigVGAN
            ragged_vocoder = isinstance(self.vocoder, BigVGAN)
        if ragged_vocoder and vocoder_kwargs_fn is not None:
            raise ValueError("convert_long_batch: vocoder_kwargs_fn pins per-chunk draws of a plain vocoder call; "
                             "it cannot be combined with the ragged vocoder call")
        return _long_pool(self.cfm, self.vocoder, utterances, n_timesteps, inference_cfg_rate, hop, max_context_window, overlap_frame_len,
                          noise_fn, vocoder_kwargs_fn, max_chunks, ragged_vocoder, seeds, self._vocoder_seeds, sampler=sampler)

    @torch.inference_mode()
    def convert_long_stream(self, utterances, n_timesteps, inference_cfg_rate, hop, max_context_window, overlap_frame_len=16, *,
                            seeds=None, noise_fn=None, vocoder_kwargs_fn=None, sampler=None, max_chunks=64, first_chunks=None, growth=4,
                            ragged_vocoder=None, pcm16=False, to_host=True, lookahead=1):
        """`convert_long_batch` as a generator of `StreamPiece(file, offset, wave, final)`: every file's audio is handed out
        as its chunks finish, in file order per file, instead of once at the end (the reference's streaming leg of
        `_stream_wave_chunks`, for many files at once).  `collect_stream(pieces, len(utterances))` gives what
        `convert_long_batch` returns; with exact stand-ins the two are bit-identical, whatever the schedule.

        The arguments are `convert_long_batch`'s, except: noise_fn(u, k, T) and vocoder_kwargs_fn(u, k, S) are keyed by file and
        chunk of the file (the order of the calls is the schedule's, not the sequential loop's); seeds still give chunk k of
        file u `derive_seed(seeds[u], k)`.  Schedule (`stream_schedule`): chunk-major over the files, micro-batches of
        min(max_chunks, ceil(first_chunks * growth ** m)) chunks, first_chunks None = one per file with chunks.
        wave: (1, n) float32, or int16 with pcm16 (`svc_chunks_emit`'s pcm plane: truncated toward zero, saturated); in pinned
        host memory with to_host, else a view of a device buffer that is valid on the current stream.

        Everything runs on the caller's current stream.  Per micro-batch: the pool's body (`_pool_micro_batch`), one
        `svc_chunks_emit` for the pieces `_StreamSplicer` released, one non-blocking copy into pinned memory, one event.
        Micro-batch m + lookahead is enqueued before the generator waits for the event of micro-batch m -- that event only,
        never the device or the stream -- so the device works while the consumer handles a piece.  Nothing further is enqueued
        until the consumer asks for the next piece (back-pressure); closing the generator early leaves the models usable.
        Argument errors are raised at the first next(), before anything is enqueued."""
        if seeds is not None and (noise_fn is not None or vocoder_kwargs_fn is not None):
            raise ValueError("convert_long_stream: give seeds or noise_fn / vocoder_kwargs_fn, not both")
        seeds = _seed_list("convert_long_stream", seeds, len(utterances))
        if ragged_vocoder is None:
            from .vocoder import BigVGAN
            ragged_vocoder = isinstance(self.vocoder, BigVGAN)
        if ragged_vocoder and vocoder_kwargs_fn is not None:
            raise ValueError("convert_long_stream: vocoder_kwargs_fn pins per-chunk draws of a plain vocoder call; "
                             "it cannot be combined with the ragged vocoder call")
        yield from _long_stream("convert_long_stream", self.cfm, self.vocoder, utterances, n_timesteps, inference_cfg_rate, hop,
                                max_context_window, overlap_frame_len, noise_fn, vocoder_kwargs_fn, max_chunks, first_chunks, growth,
                                ragged_vocoder, seeds, self._vocoder_seeds, pcm16, to_host, lookahead, sampler=sampler)


# ----------------------------------------------------------------------------------------- v2: tokens in, audio out
def v2_target_frames(frames_per_token, n_tokens):
    """Mel frames the CFM length regulator is asked for after the AR model produced `n_tokens` tokens.  The reference
    computes `int(source_mel_len / source_content_len * ar_out.size(1) * length_adjust)` in Python floats
    (modules/v2/vc_wrapper.py:636-712, quoted from memory: correct it here if the reference differs); the caller passes
    `frames_per_token = source_mel_len / source_content_len * length_adjust` and this is the one place that multiplies
    and truncates -- in double precision, like the reference."""
    return int(float(frames_per_token) * int(n_tokens))


def v2_ar_prompt(target_narrow, src_narrow):
    """The AR model's condition tokens: target then source narrow tokens along time (vc_wrapper.py:636-712, from memory)."""
    return torch.cat([target_narrow, src_narrow], dim=1)


def v2_chunk_plan(n_tokens, chunk_tokens):
    """Token ranges of the style branch of `convert_voice_with_streaming` (modules/v2/vc_wrapper.py, quoted from memory:
    correct it here if the reference differs): the reduced narrow tokens of the source are cut at `range(0, n, max_chunk_size)`
    into disjoint ranges, each generated by the AR model on its own, and the range that reaches the end is the last chunk.
    -> [(first token, tokens, is_last)], is_last = first + chunk_tokens >= n_tokens; no chunks for n_tokens == 0."""
    n, c = int(n_tokens), int(chunk_tokens)
    if c < 1:
        raise ValueError(f"v2_chunk_plan: chunk_tokens = {chunk_tokens}, a chunk needs at least one token")
    return [(i, min(c, n - i), i + c >= n) for i in range(0, n, c)]


def v2_seam_plan(chunk_files, wave_lens, is_last, overlap_wave_len, n_files):
    """Which chunk waveforms of the style branch are spliced, and how (host integers only).  chunk_files[k] / wave_lens[k] /
    is_last[k]: file, samples and `v2_chunk_plan` flag of chunk k, the chunks listed file-major; ov = overlap_wave_len.

    The AR model decides a chunk's length, and the reference's loop is only defined for long chunks: a chunk that is not the
    last and has fewer than ov samples is a numpy shape error there, and one of ov .. 2 ov - 1 samples would hand on a tail
    that already holds cross-faded samples, which `svc_chunks_assemble` (raw tails) does not do.  The rule here: a chunk is
    KEPT if it has at least 2 ov samples, or if it is the last chunk of its file; an empty chunk is never kept.  Chunks that
    are not kept contribute nothing.  `first` / `last` are taken over the kept chunks of a file, so a file whose final chunk
    is empty ends on its last kept chunk, which is emitted whole; a file without a kept chunk has no samples.  Over the kept
    chunks the result is `stream_wave_chunks` run on them in order, bit for bit.
    -> dict(kept, first, last: one bool per chunk (first / last False where not kept), out_lens: samples per file)."""
    N, ov = len(chunk_files), int(overlap_wave_len)
    if not (N == len(wave_lens) == len(is_last)):
        raise ValueError("v2_seam_plan: chunk_files, wave_lens and is_last must have one entry per chunk")
    kept = [n > 0 and (n >= 2 * ov or bool(l)) for n, l in zip(wave_lens, is_last)]
    first, last, out_lens = [False] * N, [False] * N, [0] * n_files
    for u in range(n_files):
        ks = [k for k in range(N) if chunk_files[k] == u and kept[k]]
        if ks:
            first[ks[0]], last[ks[-1]] = True, True
            out_lens[u] = sum(wave_lens[k] - (0 if last[k] else ov) for k in ks)
    return dict(kept=kept, first=first, last=last, out_lens=out_lens)


def v2_file_record(tokens_record, n_samples, hop, target, length_adjust=1.0):
    """One file of `V2HotPath.convert_long_batch` from one entry of `v2_content_tokens`: n_samples the source's samples at
    the mel rate (source_mel_len = n_samples // hop frames), target a record of `prepare_target`.  frames_per_token =
    source_mel_len / source_content_len * length_adjust with source_content_len the reduced narrow tokens (see
    `v2_target_frames`; 0.0 for a source without tokens), source_frames = int(source_mel_len * length_adjust)."""
    mel_len = int(n_samples) // int(hop)
    narrow = tokens_record["narrow_reduced"]
    return dict(target=target, src_narrow=narrow, src_tokens=tokens_record["wide"],
                frames_per_token=mel_len / narrow.size(1) * float(length_adjust) if narrow.size(1) else 0.0,
                source_frames=int(mel_len * float(length_adjust)))


@torch.inference_mode()
def v2_content_tokens(astral, waves_16k, lens, overlap_s=5.0):
    """The v2 model's content tokens of B clips (sources and targets together) from 16 kHz audio, on the device: ONE
    `AstralTokenizer.tokens_batch` call (HuBERT once per window, the wide head 0 and the narrow head 1 on the same rows) with the
    duration reduction of the narrow tokens in the same call, then one host synchronisation (the reduced counts).

    waves_16k (B, L), lens B host integers (`to_16k` gives both from audio at the file's rate) -> a list of B records dict(wide (1, R), narrow (1, R), narrow_reduced (1, n)) of int64
    device tensors.  The chain, for a source s and a target t of the list:

        tok = v2_content_tokens(astral, waves, lens)
        target = hot.prepare_target(target_narrow=tok[t]["narrow_reduced"], target_tokens=tok[t]["wide"], target_mel=mel, style=style)
        wave = hot.convert_batch(src_narrow=[tok[s]["narrow_reduced"]], targets=[target], ...)

    (vc_wrapper.py: the AR prompt is cat([target, source]) of the REDUCED narrow tokens, the CFM prompt condition comes from the
    target's wide tokens; `narrow` is kept for callers that skip the reduction)."""
    if astral.n_heads != 2:
        raise ValueError("v2_content_tokens: the tokenizer needs the wide (0) and the narrow (1) head")
    tok, rows, red, cnt = astral.tokens_batch(waves_16k, lens, overlap_s=overlap_s, reduce_head=1)
    counts = cnt.tolist()
    tok = tok.long()
    red = red.long()
    return [dict(wide=tok[0, b:b + 1, :r], narrow=tok[1, b:b + 1, :r], narrow_reduced=red[b:b + 1, :n]) for b, (r, n) in enumerate(zip(rows, counts))]


class V2HotPath:
    """The v2 chain as ONE call: narrow content tokens -> AR length regulator -> AR generate -> CFM length regulator ->
    cat([prompt_condition, cond]) -> CFM sampler (3-way CFG) -> strip the prompt frames -> BigVGAN
    (modules/v2/vc_wrapper.py:636-712, modules/v2/ar.py:382-422).  A batch is B independent runs of that chain.

    ar: seedvc_amd.ar.ARModel (setup_caches(max_batch_size=B) done by the caller); ar_lr / cfm_lr:
    seedvc_amd.length_regulator.InterpolateRegulator (v2_ar / v2_cfm); cfm: seedvc_amd.cfm.CFM (v2); vocoder: BigVGAN.
    ragged_vocoder: `_vocode`'s `ragged` -- a batch of several output lengths is one ragged vocoder call (True) or one plain
    call per length (False).
    cfm_timbre: None, or a second CFM (same weights and device) that samples the timbre branch -- `convert_long_batch` /
    `convert_long_stream` with convert_style=False -- instead of `cfm`.  The reference runs that branch's CFM in fp32
    (modules/v2/vc_wrapper.py:745) beside a fp16 style branch: CFM(..., precision="fp16x3") here reproduces it.  With None
    every call is the call it was."""

    def __init__(self, ar, ar_lr, cfm_lr, cfm, vocoder, ragged_vocoder=True, ar_prefill="slot", cfm_timbre=None):
        self.ar, self.ar_lr, self.cfm_lr, self.cfm, self.vocoder = ar, ar_lr, cfm_lr, cfm, vocoder
        if cfm_timbre is not None and (cfm_timbre.device != cfm.device or cfm_timbre.in_channels != cfm.in_channels):
            raise ValueError("V2HotPath: cfm_timbre must sit on cfm's device and have its in_channels")
        self.cfm_timbre = cfm_timbre
        self.ragged_vocoder = ragged_vocoder
        self.ar_prefill = ar_prefill           # "slot" | "ragged": how the AR prompts are prefilled (ARModel.generate_batch)
        self.device = cfm.device
        self._stacked = (None, None)
        self.marks = None           # a list: convert_batch appends (stage name, HIP event) at its stage boundaries (tools/v2_bench.py)

    def _mark(self, name):
        if self.marks is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.marks.append((name, ev))

    @torch.inference_mode()
    def prepare_target(self, target_narrow, target_tokens, target_mel, style):
        """Per-voice work done once: prompt_condition = cfm_lr(target_tokens, ylens=[P]) (vc_wrapper.py, the reference
        computes it per call).  target_narrow (1, Nn), target_tokens (1, Np), target_mel (1, C, P), style (1, Ds)."""
        dev = self.device
        P = int(target_mel.size(2))
        tok = target_tokens.to(dev).long()
        if P < 1 or tok.numel() < 1:
            raise ValueError("prepare_target: the target needs at least one content token and one mel frame")
        pc = self.cfm_lr(tok, ylens=torch.LongTensor([P]))[0]
        return dict(narrow=target_narrow.to(dev).long(), tokens=tok, mel=_lib.f32c(target_mel, dev), style=_lib.f32c(style, dev),
                    prompt_condition=pc, P=P)

    def _stack_targets(self, targets):
        """Padded batch tensors of the target records (kept while the same records come back in the same order)."""
        key = tuple(id(t) for t in targets)
        if self._stacked[0] == key:
            return self._stacked[1]
        st = dict(_stack_prompts([(t["prompt_condition"], t["mel"], t["style"]) for t in targets], self.device), keep=list(targets))
        self._stacked = (key, st)
        return st

    @torch.inference_mode()
    def convert_batch(self, src_narrow, targets, frames_per_token, n_timesteps, cfg_rates=(0.7, 0.7), top_p=0.7,
                      temperature=0.7, repetition_penalty=1.5, max_new=4001, seeds=None, exp_noise=None, z=None,
                      random_voice=False, noise_seeds=None):
        """src_narrow: list of B (1, Ns_b) token tensors; targets: list of B records of `prepare_target`;
        frames_per_token: list of B floats (see `v2_target_frames`); seeds | exp_noise: the AR draws (`ARModel.generate_batch`);
        z: the sampler's noise, a (B, C, >= T) tensor or a list of B (1, C, >= P_b + S_b) tensors (torch.randn when None);
        noise_seeds: B integers in [0, 2^64) instead of z -- utterance b's sampler noise is drawn on the device from
        noise_seeds[b] (`CFM.inference(seeds=)`; `seeds` keeps meaning the AR draws only).
        -> list of B dicts {tokens (1, n_b), mel (1, C, S_b), wave (1, S_b * hop)}.  One host synchronisation (the token
        counts); everything after it is enqueued from host integers."""
        B, dev = len(src_narrow), self.device
        if not (B == len(targets) == len(frames_per_token)):
            raise ValueError("convert_batch: src_narrow, targets and frames_per_token must have one entry per utterance")
        if seeds is not None and exp_noise is not None:
            raise ValueError("convert_batch: give seeds or exp_noise, not both")
        noise_seeds = _seed_list("convert_batch (noise_seeds)", noise_seeds, B, z)
        if B == 0:
            return []
        with torch.cuda.device(dev):
            self._mark("start")
            # AR condition: embedding-only regulator over cat([target_narrow, src_narrow]) of every utterance, one launch
            narrow = [v2_ar_prompt(t["narrow"], s.to(dev).long()) for t, s in zip(targets, src_narrow)]
            nlen = [int(x.size(1)) for x in narrow]
            tok_in = torch.zeros(B, max(nlen), dtype=torch.int64, device=dev)
            for b, x in enumerate(narrow):
                tok_in[b, :nlen[b]] = x[0]
            ar_cond = self.ar_lr(tok_in, in_lens=nlen)[0]
            toks, n = self.ar.generate_batch_raw([ar_cond[b:b + 1, :nlen[b]] for b in range(B)], [t["tokens"] for t in targets],
                                                 exp_noise, top_p, temperature, repetition_penalty, max_new, 16, seeds,
                                                 self.ar_prefill)
            self._mark("ar")
            # ---- the one synchronisation is behind us: n is a list of host integers
            ylens = [v2_target_frames(f, k) for f, k in zip(frames_per_token, n)]
            live = [b for b in range(B) if ylens[b] > 0]
            Cm = self.cfm.in_channels
            out = [dict(tokens=toks[b:b + 1, :n[b]].long(), mel=torch.zeros(1, Cm, 0, device=dev), wave=torch.zeros(1, 0, device=dev))
                   for b in range(B)]
            if not live:
                return out
            st = self._stack_targets([targets[b] for b in live])
            L, P = len(live), st["P"]
            S = [ylens[b] for b in live]
            nl = [n[b] for b in live]
            x_lens = [p + s for p, s in zip(P, S)]
            T = max(x_lens)
            # padded token rows hold zeros or an EOS: clamp so that every id is a row of the embedding
            idx = toks if L == B else toks[torch.tensor(live, device=dev)]
            tok = idx[:, :max(nl)].long().clamp_(max=self.cfm_lr.cfg["codebook_size"] - 1)
            cond = self.cfm_lr(tok, ylens=torch.LongTensor(S), in_lens=nl)[0]                     # (L, Smax, Dc), rows >= S_b zero
            mu = _assemble_cond(st["prompt_condition"], P, cond, S, T)
            self._mark("lr_assembly")
            if z is not None:
                zz = torch.zeros(L, Cm, T, device=dev)
                for i, b in enumerate(live):
                    if z[b].shape[-1] < x_lens[i]:
                        raise ValueError(f"convert_batch: z[{b}] has {z[b].shape[-1]} frames, the utterance needs {x_lens[i]}")
                    zz[i, :, :x_lens[i]] = _lib.f32c(z[b], dev).reshape(Cm, -1)[:, :x_lens[i]]
                z = zz
            mel = self.cfm.inference(mu, x_lens, st["mel"], st["style"], None, n_timesteps, inference_cfg_rate=list(cfg_rates),
                                     random_voice=random_voice, z=z, prompt_lens=P,
                                     **_cfm_seeds([noise_seeds[b] for b in live] if noise_seeds is not None else None))
            self._mark("cfm")
            vc = _strip_prompt(mel, P, x_lens, max(S))
            rows = _row_views(vc, S, _vocode(self.vocoder, vc, S, self.ragged_vocoder, "convert_batch"))
            for b, (mel_b, wave_b) in zip(live, rows):
                out[b]["mel"], out[b]["wave"] = mel_b, wave_b
            self._mark("strip_vocoder")
        return out

    def _style_chunks(self, what, files, ar_chunk_tokens, anonymization_only):
        """The style branch's chunk table, file-major: [(file, chunk of the file, first token, tokens, is_last)] (`v2_chunk_plan`
        per file).  ValueError for a chunk whose AR prompt does not fit the cache."""
        plan = [(u, j) + c for u, f in enumerate(files) for j, c in enumerate(v2_chunk_plan(f["src_narrow"].size(1), ar_chunk_tokens))]
        Lmax = self.ar.cfg["max_seq_len"]
        for u, j, p0, n, _ in plan:
            t = files[u]["target"]
            rows = n + 2 if anonymization_only else t["narrow"].size(1) + n + 2 + t["tokens"].size(1)
            if rows > Lmax:
                raise ValueError(f"{what}: file {u}, chunk {j}: an AR prompt of {rows} rows does not fit the cache "
                                 f"({Lmax} positions); use a smaller ar_chunk_tokens")
        return plan

    def _style_ar_requests(self, files, plan, anonymization_only, seeds, exp_noise_fn, ar_kw):
        """The AR side of the style branch's chunks: one ragged `ar_lr` call over the AR conditions of all chunks of `plan`
        (at least one), the chunks' seeds, and submit(sess, k): chunk k as one request of an `ARSession`.
        -> (chunk_seeds or None, submit); ar_kw: max_new, top_p, temperature, repetition_penalty of every request."""
        dev, K = self.device, len(plan)
        # AR condition of every chunk: one ragged regulator call over cat([target narrow, range]) (not assumed position-wise)
        narrow = []
        for u, j, p0, n, _ in plan:
            chunk = files[u]["src_narrow"][:, p0:p0 + n].to(dev).long()
            narrow.append(chunk if anonymization_only else v2_ar_prompt(files[u]["target"]["narrow"], chunk))
        nlen = [int(x.size(1)) for x in narrow]
        tok_in = torch.zeros(K, max(nlen), dtype=torch.int64, device=dev)
        for k, x in enumerate(narrow):
            tok_in[k, :nlen[k]] = x[0]
        ar_cond = self.ar_lr(tok_in, in_lens=nlen)[0]
        if seeds is not None:
            chunk_seeds = [derive_seed(seeds[u], j) for u, j, *_ in plan]
            ar_seeds = chunk_seeds
        else:
            chunk_seeds = None
            ar_seeds = torch.randint(0, 2 ** 62, (K,), dtype=torch.int64).tolist() if exp_noise_fn is None else None
        no_target = torch.zeros(1, 0, dtype=torch.int64, device=dev)

        def submit(sess, k):
            u, j = plan[k][:2]
            draws = dict(exp_noise=exp_noise_fn(u, j)) if exp_noise_fn is not None else dict(seed=ar_seeds[k])
            return sess.submit(ar_cond[k:k + 1, :nlen[k]], no_target if anonymization_only else files[u]["target"]["tokens"],
                               **ar_kw, **draws)
        return chunk_seeds, submit

    def _style_micro_batch(self, what, files, plan, ks, toks, ylens, st, mel_rows, style_rows, waves, row0, hop, n_timesteps, cfg_rates,
                           random_voice, noise_fn, chunk_seeds, file_settings):
        """One micro-batch of the style branch, the chunks `ks` of `plan` (all with ylen > 0): clamp the ids, one ragged `cfm_lr`
        call, `svc_chunks_gather_cond` over its output, one sampler call with per-row lengths, `_strip_prompt`, `_vocode`, rows
        row0 .. of the chunk-wave buffer `waves`.  toks / ylens: by chunk; st: `_stack_targets` of the files; mel_rows /
        style_rows: the chunks' prompt rows.  -> (vc, S, calls) as `_row_views` takes them."""
        dev, i32 = self.device, _lib.i32_host
        P, Pmax, pc_all = st["P"], st["Pmax"], st["prompt_condition"]
        Dc, Cm, U = pc_all.size(2), self.cfm.in_channels, len(files)
        top = self.cfm_lr.cfg["codebook_size"] - 1
        n = len(ks)
        S, nl = [ylens[k] for k in ks], [toks[k].size(1) for k in ks]
        Pk = [P[plan[k][0]] for k in ks]
        x_lens = [p + s for p, s in zip(Pk, S)]
        T, Smax = max(x_lens), max(S)
        tok = torch.zeros(n, max(nl), dtype=torch.int64, device=dev)
        for i, k in enumerate(ks):
            tok[i, :nl[i]] = toks[k][0]
        tok.clamp_(max=top)          # an id above the codebook (the AR vocabulary's EOS) is no row of the embedding
        cond = self.cfm_lr(tok, ylens=torch.LongTensor(S), in_lens=nl)[0]           # (n, Smax, Dc)
        mu = torch.empty(n, T, Dc, device=dev)
        _lib.check(_lib.lib().svc_chunks_gather_cond(_lib.ptr(pc_all), i32(P), U, Pmax, _lib.ptr(cond), n * Smax,
                                                     i32([plan[k][0] for k in ks]), i32([i * Smax for i in range(n)]), i32(S),
                                                     n, Dc, T, _lib.ptr(mu), _lib.stream_ptr()))
        self._mark("lr_assembly")
        z = None
        if noise_fn is not None:
            z = torch.zeros(n, Cm, T, device=dev)
            for i, k in enumerate(ks):
                z[i, :, :x_lens[i]] = _lib.f32c(noise_fn(plan[k][0], plan[k][1], x_lens[i]), dev)[0]
        mb_seeds = [chunk_seeds[k] for k in ks] if chunk_seeds is not None else None
        try:
            if file_settings is None:
                mel = self.cfm.inference(mu, x_lens, mel_rows, style_rows, None, n_timesteps,
                                         inference_cfg_rate=list(cfg_rates), random_voice=random_voice, z=z, prompt_lens=Pk,
                                         **_cfm_seeds(mb_seeds))
            else:
                mel = self.cfm.inference_rows(mu, x_lens, mel_rows, style_rows,
                                              [file_settings[plan[k][0]] for k in ks], z=z, prompt_lens=Pk,
                                              **_cfm_seeds(mb_seeds))
        except RuntimeError as e:
            i = max(range(n), key=lambda i: x_lens[i])
            raise RuntimeError(f"{what}: file {plan[ks[i]][0]}, chunk {plan[ks[i]][1]}: the sampler refused "
                               f"{x_lens[i]} frames (prompt {Pk[i]} + {S[i]} generated): {e}; use a smaller ar_chunk_tokens") from e
        self._mark("cfm")
        vc = _strip_prompt(mel, Pk, x_lens, Smax)
        calls = _vocode(self.vocoder, vc, S, self.ragged_vocoder, what, hop=hop)
        for call in calls:
            r = 0
            for a, b in call.runs:       # rows of a call -> rows of the chunk wave buffer (slices: no synchronisation)
                waves[row0 + a:row0 + b, :call.frames * hop].copy_(call.wave[r:r + b - a])
                r += b - a
        return vc, S, calls

    @torch.inference_mode()
    def convert_long_batch(self, files, n_timesteps, cfg_rates=(0.7, 0.7), *, max_context_window, hop, convert_style=True,
                           anonymization_only=False, random_voice=False, ar_chunk_tokens=1000, overlap_frame_len=16, top_p=0.7,
                           temperature=0.7, repetition_penalty=1.5, max_new=4001, seeds=None, exp_noise_fn=None, noise_fn=None,
                           max_chunks=64, steps_per_run=16, return_parts=False, sampler=None):
        """Whole files through the v2 chain, every chunk of every file in ONE pool: `convert_voice_with_streaming`
        (modules/v2/vc_wrapper.py, quoted from memory: correct it here if the reference differs).  The reference loops over
        chunks one after the other; its chunks read the same target, disjoint ranges of the source and fresh draws, never each
        other, so here they fill the AR batch and the sampler's batch together, and one launch splices them.

        files: list of dict(target = a `prepare_target` record, src_narrow (1, Ns) reduced narrow tokens, src_tokens (1, Nw)
        wide tokens, frames_per_token float, source_frames int) -- `v2_file_record` builds one.  max_context_window: frames of
        one sampler call, prompt included (the reference: 30 s); hop: samples per mel frame; overlap_frame_len: frames of the
        cos^2 cross-fade.  -> list of (1, L_u) waves, views of one buffer.

        convert_style=True (the style branch; reads src_narrow, frames_per_token): the reference cuts the source's narrow
        tokens into ranges of at most max_chunk_size (1000) tokens (`v2_chunk_plan`, ar_chunk_tokens), generates each with
        the AR model prompted by cat([target narrow, range]) and the target's wide tokens, runs CFM regulator -> sampler ->
        vocoder per chunk and splices the waves with `_stream_wave_chunks`.  Here, with the chunks listed file-major: one
        ragged `ar_lr` call over the AR conditions of all chunks; every chunk one request of an `ARSession(ar, steps_per_run)`
        (`ar.max_batch_size` slots, recycled as chunks finish), submitted in plan order and drained -- the token counts are the
        call's synchronisation point; ylen_k = v2_target_frames(frames_per_token_u, n_k); then per micro-batch of at most
        max_chunks chunks: clamp the ids, one ragged `cfm_lr` call, `svc_chunks_gather_cond` over its output, one
        `cfm.inference` with per-row lengths, `_strip_prompt`, `_vocode`, rows of one chunk-wave buffer; one
        `svc_chunks_assemble` at the end.  Seams: `v2_seam_plan` (a chunk shorter than two overlaps is dropped unless it ends
        its file).  anonymization_only: the AR condition is the range alone and the AR prompt has no target tokens; the CFM
        still uses the target record (or random_voice).  A chunk whose AR prompt does not fit the cache is a ValueError before
        anything is enqueued; a chunk the sampler refuses (prompt + ylen above its length limit) re-raises its error with the
        file and the chunk: use a smaller ar_chunk_tokens.

        convert_style=False (the timbre branch, the reference's default; reads src_tokens, source_frames): no AR.  One
        ragged `cfm_lr` call over the files' wide tokens with ylens = source_frames, then the pool of
        `HotPath.convert_long_batch` on its output (`_long_pool`): windows of max_context_window - P_u frames, the same seams.

        Draws.  seeds: one integer in [0, 2^64) per file; chunk k of file u uses derive_seed(seeds[u], k) for its AR draws and
        as its sampler-noise seed (the two Philox domains differ), so a file's audio is a function of its inputs and seed,
        whatever shares the pool and whichever slot a chunk gets.  exp_noise_fn(u, k) -> (>= max_new, vocab) Exp(1) draws and
        noise_fn(u, k, T) -> (1, C, T) pin the AR draws / the sampler noise of chunk k of file u (exclusive with seeds; the
        timbre branch has no AR draws).  With neither, the AR seeds come from torch's CPU generator as in `generate_batch` and
        the sampler noise is one torch.randn per micro-batch.

        sampler: per file a sampler setting -- a dict or (n_timesteps, inference_cfg_rate, temperature=1.0, random_voice=False),
        a rate being a float or the pair (intelligibility, similarity) -- or None for the call's n_timesteps / cfg_rates /
        random_voice; every chunk of a file uses its file's entry, in both branches, and a micro-batch stays one sampler call
        (`CFM.inference_rows`).  sampler=None: the calls made without the keyword.

        return_parts (style branch): -> (waves, parts), parts[u] a list with one dict(tokens (1, n), ylen, mel (1, C, ylen),
        wave (1, ylen * hop), kept) per chunk of file u."""
        U, dev = len(files), self.device
        if seeds is not None and (exp_noise_fn is not None or noise_fn is not None):
            raise ValueError("convert_long_batch: give seeds or exp_noise_fn / noise_fn, not both")
        seeds = _seed_list("convert_long_batch", seeds, U)
        if max_chunks < 1:
            raise ValueError(f"convert_long_batch: max_chunks = {max_chunks}, at least one chunk per micro-batch is needed")
        if not convert_style:
            if exp_noise_fn is not None or return_parts:
                raise ValueError("convert_long_batch: exp_noise_fn and return_parts belong to the style branch (convert_style=True)")
            return self._convert_long_timbre(files, n_timesteps, cfg_rates, random_voice, hop, max_context_window, overlap_frame_len,
                                             noise_fn, max_chunks, seeds, sampler)
        v2_chunk_plan(0, ar_chunk_tokens)          # its ValueError, with or without files
        file_settings = _file_settings("convert_long_batch", sampler, U, n_timesteps, list(cfg_rates), random_voice)
        if U == 0:
            return ([], []) if return_parts else []
        plan = self._style_chunks("convert_long_batch", files, ar_chunk_tokens, anonymization_only)
        K, ovw = len(plan), overlap_frame_len * hop
        Cm = self.cfm.in_channels
        i32 = _lib.i32_host
        with torch.cuda.device(dev):
            self._mark("start")
            toks = []
            if K:
                chunk_seeds, submit = self._style_ar_requests(files, plan, anonymization_only, seeds, exp_noise_fn,
                                                              dict(max_new=max_new, top_p=top_p, temperature=temperature,
                                                                   repetition_penalty=repetition_penalty))
                from .ar import ARSession
                sess = ARSession(self.ar, steps_per_run)
                try:
                    for k in range(K):
                        submit(sess, k)
                    done = dict(sess.drain())          # tickets count from 0 in submit order: ticket k is chunk k
                finally:
                    sess.close()
                toks = [done[k] for k in range(K)]
            self._mark("ar")
            # ---- the token counts are host integers from here on: everything below is enqueued from them
            ylens = [v2_target_frames(files[u]["frames_per_token"], toks[k].size(1)) for k, (u, *_) in enumerate(plan)]
            seam = v2_seam_plan([c[0] for c in plan], [y * hop for y in ylens], [c[4] for c in plan], ovw, U)
            out_lens = seam["out_lens"]
            out = torch.empty(sum(out_lens), device=dev, dtype=torch.float32)
            offs = [sum(out_lens[:u]) for u in range(U)]
            result = [out[o:o + n][None, :] for o, n in zip(offs, out_lens)]
            parts = [[] for _ in range(U)]
            if return_parts:
                for k, (u, *_) in enumerate(plan):
                    parts[u].append(dict(tokens=toks[k], ylen=ylens[k], mel=torch.zeros(1, Cm, 0, device=dev),
                                         wave=torch.zeros(1, 0, device=dev), kept=seam["kept"][k]))
            live = [k for k in range(K) if ylens[k] > 0]
            if live:
                st = self._stack_targets([f["target"] for f in files])
                if U > 1:
                    idx = torch.tensor([plan[k][0] for k in live], device=dev)
                    mel_chunks, style_chunks = st["mel"].index_select(0, idx), st["style"].index_select(0, idx)
                else:
                    mel_chunks, style_chunks = st["mel"].expand(len(live), -1, -1), st["style"].expand(len(live), -1)
                stride = max(ylens) * hop
                waves = torch.empty(len(live), stride, device=dev, dtype=torch.float32)     # row i: the wave of chunk live[i]
                for m0 in range(0, len(live), max_chunks):
                    ks = live[m0:m0 + max_chunks]
                    n = len(ks)
                    vc, S, calls = self._style_micro_batch("convert_long_batch", files, plan, ks, toks, ylens, st, mel_chunks[m0:m0 + n],
                                                           style_chunks[m0:m0 + n], waves, m0, hop, n_timesteps, cfg_rates, random_voice,
                                                           noise_fn, chunk_seeds, file_settings)
                    if return_parts:
                        for i, (k, (mel_k, _)) in enumerate(zip(ks, _row_views(vc, S, calls))):
                            part = parts[plan[k][0]][plan[k][1]]
                            part["mel"], part["wave"] = mel_k, waves[m0 + i:m0 + i + 1, :S[i] * hop]
                    self._mark("strip_vocoder")
                rows = [i for i, k in enumerate(live) if seam["kept"][k]]
                if rows:
                    kept_waves = waves if len(rows) == len(live) else torch.cat([waves[a:b] for a, b in _index_runs(rows)])
                    kept = [live[i] for i in rows]
                    fade_in, fade_out = (torch.from_numpy(w).to(dev) for w in _cos2_windows(ovw))
                    _lib.check(_lib.lib().svc_chunks_assemble(_lib.ptr(kept_waves), C.c_longlong(stride), i32([ylens[k] * hop for k in kept]),
                                                              i32([int(seam["first"][k]) for k in kept]), i32([int(seam["last"][k]) for k in kept]),
                                                              len(kept), _lib.ptr(fade_in), _lib.ptr(fade_out), ovw, _lib.ptr(out),
                                                              C.c_longlong(out.numel()), _lib.stream_ptr()))
                self._mark("assemble")
            torch.cuda.current_stream(dev).synchronize()
        return (result, parts) if return_parts else result

    def _timbre_utterances(self, files):
        """The timbre branch's files as utterances of `_long_pool` / `_long_stream`: one ragged `cfm_lr` call over the files'
        wide tokens with ylens = source_frames.  -> (utterances, frames per file); called under the device, with files."""
        U, dev = len(files), self.device
        frames = [int(f["source_frames"]) if f["src_tokens"].size(1) else 0 for f in files]
        live = [u for u in range(U) if frames[u] > 0]
        self._mark("start")
        if live:
            nw = [int(files[u]["src_tokens"].size(1)) for u in live]
            tok = torch.zeros(len(live), max(nw), dtype=torch.int64, device=dev)
            for i, u in enumerate(live):
                tok[i, :nw[i]] = files[u]["src_tokens"][0]
            cond = self.cfm_lr(tok, ylens=torch.LongTensor([frames[u] for u in live]), in_lens=nw)[0]
        self._mark("lr_assembly")
        none = torch.zeros(1, 0, self.cfm_lr.cfg["out_channels"], device=dev)
        conds = [none] * U
        for i, u in enumerate(live):
            conds[u] = cond[i:i + 1, :frames[u]]
        return [(conds[u], f["target"]["prompt_condition"], f["target"]["mel"], f["target"]["style"]) for u, f in enumerate(files)], frames

    def _convert_long_timbre(self, files, n_timesteps, cfg_rates, random_voice, hop, max_context_window, overlap_frame_len, noise_fn,
                             max_chunks, seeds, sampler=None):
        """The timbre branch of `convert_long_batch`: the CFM regulator over the files' wide tokens, then `_long_pool`."""
        if len(files) == 0:
            return []
        with torch.cuda.device(self.device):
            utterances, frames = self._timbre_utterances(files)
            pool_noise = None
            if noise_fn is not None:          # the pool asks per chunk in plan order: give each call its (file, chunk)
                order = long_batch_plan(frames, [f["target"]["P"] for f in files], max_context_window, overlap_frame_len, hop, max_chunks)
                first_of, uk = {}, []
                for k, c in enumerate(order["chunks"]):
                    uk.append((c[0], k - first_of.setdefault(c[0], k)))
                it = iter(uk)
                pool_noise = lambda T: noise_fn(*next(it), T)          # noqa: E731
            result = _long_pool(self.cfm_timbre or self.cfm, self.vocoder, utterances, n_timesteps, list(cfg_rates), hop, max_context_window, overlap_frame_len,
                                pool_noise, None, max_chunks, self.ragged_vocoder, seeds, lambda s: _vocoder_seeds(self.vocoder, s),
                                dict(random_voice=True) if random_voice else None, sampler=sampler)
            self._mark("pool")
        return result

    @torch.inference_mode()
    def convert_long_stream(self, files, n_timesteps, cfg_rates=(0.7, 0.7), *, max_context_window, hop, convert_style=True,
                            anonymization_only=False, random_voice=False, ar_chunk_tokens=1000, overlap_frame_len=16, top_p=0.7,
                            temperature=0.7, repetition_penalty=1.5, max_new=4001, seeds=None, exp_noise_fn=None, noise_fn=None,
                            max_chunks=64, steps_per_run=16, sampler=None, first_chunks=None, growth=4, pcm16=False, to_host=True,
                            lookahead=1, return_parts=False):
        """`convert_long_batch` as a generator of `StreamPiece(file, offset, wave, final, parts)`: every file's audio is handed
        out as its chunks finish (`convert_voice_with_streaming` hands each chunk's audio to its caller; here for many files
        at once).  The keywords are `convert_long_batch`'s plus `HotPath.convert_long_stream`'s first_chunks, growth, pcm16,
        to_host and lookahead; `collect_stream(pieces, len(files))` gives the waves `convert_long_batch` returns.  Everything
        runs on the current stream; argument errors are raised at the first next(), before anything is enqueued.

        convert_style=False (timbre branch): the ragged `cfm_lr` call, then the generator behind `HotPath.convert_long_stream`.

        convert_style=True (style branch): the chunks are submitted to the `ARSession` chunk-major (`stream_schedule`'s order:
        chunk 0 of every file first).  After every `sess.step()` the retired chunks join a ready list; micro-batch m of the
        ramp is launched once min(its size, chunks not yet dispatched) chunks are ready, lowest (chunk, file) first: regulator,
        sampler and vocoder (`_style_micro_batch`, the pool's body), then one `svc_chunks_emit` for the pieces the splicer
        released, one copy into pinned memory, one event.  AR steps and sampler work interleave on one stream; an AR step reads
        its token counts, so what was enqueued before it is finished when it returns and is handed out then.  A chunk's
        length is the AR model's decision: the splicer gets ylen * hop when the chunk is dispatched, and a chunk may complete
        before an earlier chunk of its file -- its wave is kept on the device until the file's pieces up to it are released.
        The session is closed in a `finally`: closing the generator early leaves the models usable.

        return_parts (style branch): pieces carry `parts`, a list of dict(file, chunk, tokens, ylen, mel, wave, kept) for the
        chunks dispatched since the previous piece that carried parts (None on the other pieces)."""
        what = "convert_long_stream"
        U, dev = len(files), self.device
        if seeds is not None and (exp_noise_fn is not None or noise_fn is not None):
            raise ValueError(f"{what}: give seeds or exp_noise_fn / noise_fn, not both")
        seeds = _seed_list(what, seeds, U)
        if max_chunks < 1:
            raise ValueError(f"{what}: max_chunks = {max_chunks}, at least one chunk per micro-batch is needed")
        if lookahead < 0:
            raise ValueError(f"{what}: lookahead = {lookahead}, a count of micro-batches enqueued ahead")
        if not convert_style:
            if exp_noise_fn is not None or return_parts:
                raise ValueError(f"{what}: exp_noise_fn and return_parts belong to the style branch (convert_style=True)")
            if U == 0:
                return
            with torch.cuda.device(dev):
                utterances, _ = self._timbre_utterances(files)
            yield from _long_stream(what, self.cfm_timbre or self.cfm, self.vocoder, utterances, n_timesteps, list(cfg_rates), hop, max_context_window,
                                    overlap_frame_len, noise_fn, None, max_chunks, first_chunks, growth, self.ragged_vocoder, seeds,
                                    lambda s: _vocoder_seeds(self.vocoder, s), pcm16, to_host, lookahead,
                                    dict(random_voice=True) if random_voice else None, sampler=sampler)
            return
        v2_chunk_plan(0, ar_chunk_tokens)          # its ValueError, with or without files
        file_settings = _file_settings(what, sampler, U, n_timesteps, list(cfg_rates), random_voice)
        plan = self._style_chunks(what, files, ar_chunk_tokens, anonymization_only)
        n_chunks = [sum(1 for c in plan if c[0] == u) for u in range(U)]
        ramp = _ramp_args(what, n_chunks, first_chunks, growth, max_chunks)
        if U == 0:
            return
        K, ovw, Cm = len(plan), overlap_frame_len * hop, self.cfm.in_channels
        index = {c[:2]: k for k, c in enumerate(plan)}
        submit_order = [index[uj] for uj in stream_schedule(n_chunks)["order"]]        # chunk-major; ticket t is chunk submit_order[t]
        splicer = _StreamSplicer(U, n_chunks, ovw)
        with torch.cuda.device(dev):
            out = _StreamOut(dev, ovw, pcm16, to_host)
            out.push(splicer.start(), None, {})
        if K == 0:
            while out.pending:
                yield from out.pop()
            return
        toks, ylens, old_waves = {}, {}, {}

        def launch(ks):
            """One micro-batch: the chunks ks (plan indices) -> sampler and vocoder for those with frames, emit for what the
            splicer releases."""
            live = [k for k in ks if ylens[k] > 0]
            pieces, parts = [], []
            for k in ks:
                u, j, _, _, is_last = plan[k]
                pieces += splicer.complete(u, j, ylens[k] * hop, is_last)
            # rows 0 .. of this micro-batch's buffer are its own chunks; behind them, what the pieces need of older chunks:
            # samples `skip` .. of a chunk delivered late, the last ovw samples of one that is only faded out
            rows = {plan[k][:2]: (i, ylens[k] * hop, 0) for i, k in enumerate(live)}
            skip = {}
            for p in pieces:
                if p.chunk >= 0 and (p.file, p.chunk) not in rows:
                    skip[(p.file, p.chunk)] = min(skip.get((p.file, p.chunk), p.begin), p.begin)
                if p.prev_chunk >= 0 and p.begin < min(p.end, ovw) and (p.file, p.prev_chunk) not in rows:
                    skip[(p.file, p.prev_chunk)] = min(skip.get((p.file, p.prev_chunk), p.prev_len - ovw), p.prev_len - ovw)
            for i, (uj, first) in enumerate(skip.items()):
                rows[uj] = (len(live) + i, old_waves[uj].size(1) - first, first)
            stride = max([1] + [r[1] for r in rows.values()])
            waves = torch.empty(len(rows), -(-stride // 4) * 4, device=dev, dtype=torch.float32)
            if live:
                st = self._stack_targets([f["target"] for f in files])
                if U > 1:
                    idx = torch.tensor([plan[k][0] for k in live], device=dev)
                    mel_rows, style_rows = st["mel"].index_select(0, idx), st["style"].index_select(0, idx)
                else:
                    mel_rows, style_rows = st["mel"].expand(len(live), -1, -1), st["style"].expand(len(live), -1)
                vc, S, calls = self._style_micro_batch(what, files, plan, live, toks, ylens, st, mel_rows, style_rows, waves, 0, hop,
                                                       n_timesteps, cfg_rates, random_voice, noise_fn, chunk_seeds, file_settings)
                mels = dict(zip(live, (m for m, _ in _row_views(vc, S, calls))))
                for i, k in enumerate(live):
                    old_waves[plan[k][:2]] = waves[i:i + 1, :ylens[k] * hop]
                self._mark("strip_vocoder")
            for uj, first in skip.items():
                waves[rows[uj][0], :rows[uj][1]].copy_(old_waves[uj][0, first:])
            if return_parts:
                for k in ks:
                    n, live_k = ylens[k] * hop, ylens[k] > 0
                    parts.append(dict(file=plan[k][0], chunk=plan[k][1], tokens=toks[k], ylen=ylens[k],
                                      mel=mels[k] if live_k else torch.zeros(1, Cm, 0, device=dev),
                                      wave=old_waves[plan[k][:2]] if live_k else torch.zeros(1, 0, device=dev),
                                      kept=n > 0 and (n >= 2 * ovw or bool(plan[k][4]))))
            out.push(pieces, waves, rows, parts if return_parts else None)
            self._mark("emit")
            for p in pieces:
                if p.final:          # the file is spliced: its chunk waves are not needed any more
                    for uj in [uj for uj in old_waves if uj[0] == p.file]:
                        del old_waves[uj]

        from .ar import ARSession
        with torch.cuda.device(dev):
            self._mark("start")
            chunk_seeds, submit = self._style_ar_requests(files, plan, anonymization_only, seeds, exp_noise_fn,
                                                          dict(max_new=max_new, top_p=top_p, temperature=temperature,
                                                               repetition_penalty=repetition_penalty))
            sess = ARSession(self.ar, steps_per_run)
        try:
            with torch.cuda.device(dev):
                for k in submit_order:
                    submit(sess, k)
            ready, dispatched, m = [], 0, 0
            while dispatched < K:
                size = min(_ramp_size(m, *ramp), K - dispatched)
                if len(ready) >= size:
                    ready.sort()
                    with torch.cuda.device(dev):
                        launch([k for _, _, k in ready[:size]])
                    del ready[:size]
                    dispatched, m = dispatched + size, m + 1
                    while len(out.pending) > lookahead:
                        yield from out.pop()
                    continue
                with torch.cuda.device(dev):
                    retired = sess.step()
                for t, tk in retired:
                    k = submit_order[t]
                    toks[k], ylens[k] = tk, v2_target_frames(files[plan[k][0]]["frames_per_token"], tk.size(1))
                    ready.append((plan[k][1], plan[k][0], k))
                while out.pending:          # the step read its token counts: everything enqueued before it is finished
                    yield from out.pop()
            while out.pending:
                yield from out.pop()
        finally:
            sess.close()


# ----------------------------------------------------------------------------------------- real-time sessions
def realtime_geometry(sr, hop, block_time, crossfade_time, extra_time, extra_time_right, ce_dit_difference):
    """The integer geometry of the reference GUI (real-time-gui.py: `start_vc` and `custom_infer`, quoted from memory:
    correct it here if the reference differs).  Every time is rounded to a multiple of zc = sr // 50 samples;
    Lb = min(crossfade_frame, 4 * zc), Ls = zc; skip_head / skip_tail / return_length count 20 ms units; the length
    regulator is asked for S = int((skip_head + return_length + skip_tail - int(ce_dit_difference * 50)) / 50 * sr // hop)
    mel frames and the GUI keeps `vc_wave[-(block + Lb + Ls) - tail : -tail]` of the S * hop samples, tail = skip_tail * sr // 50.
    -> dict(S, block, Lb, Ls, tail, start, n_inf, skip_head, skip_tail, return_length): the arguments of `RealtimeEngine`.
    ValueError where the S * hop samples do not hold n_inf + tail."""
    zc = sr // 50
    to_frame = lambda t: int(round(t * sr / zc)) * zc                                              # noqa: E731
    block, crossfade_frame = to_frame(block_time), to_frame(crossfade_time)
    Lb, Ls = min(crossfade_frame, 4 * zc), zc
    skip_head, skip_tail = to_frame(extra_time) // zc, to_frame(extra_time_right) // zc
    return_length = (block + Lb + Ls) // zc
    S = int((skip_head + return_length + skip_tail - int(ce_dit_difference * 50)) / 50 * sr // hop)
    tail = skip_tail * sr // 50
    n_inf = block + Lb + Ls
    if block < 1 or Lb < 1 or n_inf + tail > S * hop:
        raise ValueError(f"realtime_geometry: block {block}, sola buffer {Lb}, search {Ls} and tail {tail} samples do not fit "
                         f"the {S} x {hop} samples of a step")
    return dict(S=S, block=block, Lb=Lb, Ls=Ls, tail=tail, start=S * hop - tail - n_inf, n_inf=n_inf, skip_head=skip_head,
                skip_tail=skip_tail, return_length=return_length)


def realtime_input_geometry(sr, block_time, crossfade_time, extra_time_ce, extra_time_right, content_rate=16000):
    """The input side of the reference GUI's buffer arithmetic (real-time-gui.py: `start_vc`, quoted from memory: correct it
    here if the reference differs).  zc = sr // 50 and z16 = content_rate // 50 samples are 20 ms at the two rates; every time is
    rounded to a multiple of zc as in `realtime_geometry`; `input_wav` has extra_ce + crossfade + sola_search (zc) + block +
    extra_right samples and `input_wav_res` z16 * len(input_wav) // zc.
    -> dict(zc, z16, Lin (= block: the samples a block step takes), L16 (the content-rate context), hist (= 2 zc: the
    stream-rate samples kept between blocks), rows (L16 // z16 - 1: what a stride-z16 convolutional extractor with a
    z16 + z16 // 4 receptive field, wav2vec 2.0, yields for the context, and with it the ASTRAL tokenizer's token count for
    the context, `AstralTokenizer.tokens_fn`: min(frames, L16 // z16) over the same HuBERT extractor; Whisper yields
    L16 // z16 + 1)).
    ValueError where sr or content_rate is not a multiple of 50: a block must start at resampling phase 0."""
    sr, content_rate = int(sr), int(content_rate)
    if sr < 50 or content_rate < 50 or sr % 50 or content_rate % 50:
        raise ValueError(f"realtime_input_geometry: sr {sr} and content_rate {content_rate} must be multiples of 50 "
                         f"(20 ms must be a whole number of samples at both rates)")
    zc, z16 = sr // 50, content_rate // 50
    to_frame = lambda t: int(round(t * sr / zc)) * zc                                              # noqa: E731
    block = to_frame(block_time)
    total = to_frame(extra_time_ce) + to_frame(crossfade_time) + zc + block + to_frame(extra_time_right)
    L16 = z16 * total // zc
    if block < zc or L16 < (block // zc + 1) * z16:
        raise ValueError(f"realtime_input_geometry: a block of {block} samples does not fit a context of {L16}")
    return dict(zc=zc, z16=z16, Lin=block, L16=L16, hist=2 * zc, rows=L16 // z16 - 1)


def realtime_output_geometry(g, sr_model, sr_out):
    """The SOLA geometry of `realtime_geometry` (its dict `g`, or any dict with block, Lb, Ls) at another output rate: the GUI
    resamples `infer_wav` from the model's rate to the sound card's before SOLA (`resampler2`), so the splice runs in 20 ms
    units of zc_o = sr_out // 50 samples instead of zc_m = sr_model // 50.  -> dict(zc, block, Lb, Ls, n_inf) at the output
    rate.  ValueError where a rate is not a multiple of 50 or a length is not a multiple of zc_m."""
    sr_model, sr_out = int(sr_model), int(sr_out)
    if sr_model < 50 or sr_out < 50 or sr_model % 50 or sr_out % 50:
        raise ValueError(f"realtime_output_geometry: the rates {sr_model} and {sr_out} must be multiples of 50 "
                         f"(20 ms must be a whole number of samples at both rates)")
    zc_m, zc_o = sr_model // 50, sr_out // 50
    out = dict(zc=zc_o)
    for key in ("block", "Lb", "Ls"):
        v = int(g[key])
        if v % zc_m:
            raise ValueError(f"realtime_output_geometry: {key} = {v} is not a multiple of zc = {zc_m} samples")
        out[key] = v // zc_m * zc_o
    out["n_inf"] = out["block"] + out["Lb"] + out["Ls"]
    return out


def gate_power(threshold_db, zc):
    """The GUI's noise-gate threshold in dB (RMS re 1.0) as `svc_rt_push_gated` takes it: the energy of 4 zc samples at that RMS,
    float32(4 zc 10^(dB / 10)); None or at most -60 dB -> 0.0, the GUI's "off"."""
    if threshold_db is None or float(threshold_db) <= -60.0:
        return 0.0
    return float(np.float32(4.0 * zc * 10.0 ** (float(threshold_db) / 10.0)))


def gui_fade_windows(Lb):
    """(fade_in, fade_out) of the reference GUI: sin(0.5 pi linspace(0, 1, Lb))^2 and 1 - fade_in, float32, computed on the
    host.  The engine takes its windows as arrays because device and host `sin` differ in the last bit."""
    fade_in = torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, steps=Lb, dtype=torch.float32)) ** 2
    return fade_in, 1 - fade_in


class RealtimeEngine:
    """Block-by-block conversion of up to `max_streams` independent streams, one engine step per block: the reference GUI's
    `custom_infer` plus the SOLA splice of its `audio_callback` (real-time-gui.py, restated from memory: correct it here if
    the reference differs).  Per stream, given content features x (1, Tin, Din):

        cond  = length_regulator(x, ylens=[S], n_quantizers=3, f0=None)[0]
        mel   = cfm.inference(cat([prompt_condition, cond], 1), [P + S], mel2, style2, None, n_timesteps, cfg_rate)[:, :, P:]
        wave  = vocoder(mel).reshape(-1)                                    # S * hop samples
        infer = wave[start : start + n_inf]                                 # = vc_wave[-n_inf - tail : -tail]
        o*    = argmax_o <infer[o : o + Lb], sola_buffer> / sqrt(|infer[o : o + Lb]|^2 + 1e-8),  o = 0 .. Ls
        y     = infer[o*:];  y[:Lb] = y[:Lb] * fade_in + sola_buffer * fade_out
        sola_buffer = y[block : block + Lb];  output = y[:block]

    with n_inf = block + Lb + Ls and start = S * hop - tail - n_inf.  The geometry (host integers, `realtime_geometry`) is
    shared by the streams of an engine; each stream has its own reference (`open`) and its own SOLA buffer, a row of one
    device tensor.  A step is six enqueues -- length regulator, `svc_v2_assemble_cond` (ragged prompts), one `cfm.inference`
    with prompt_lens, `svc_mel_strip_prompt`, one plain vocoder call (every row has S frames), `svc_sola_step` -- from host
    integers only: nothing synchronises, and the data-dependent offset never leaves the device.

    length_regulator: seedvc_amd.length_regulator.InterpolateRegulator, v1 or the v2 model's discrete `v2_cfm`; cfm:
    seedvc_amd.cfm.CFM; vocoder: HiFT | BigVGAN with S * hop samples per row; fade_in / fade_out: (Lb,) float32 windows (default:
    `gui_fade_windows`).

    Token mode is the state of an engine whose regulator has `cfg["is_discrete"]`: the timbre branch of the v2
    wrapper (`convert_style=False`: wide content tokens -> `cfm_length_regulator` -> `cfm.inference` -> vocoder, no AR) block
    by block.  Per stream, given the wide tokens t (1, Tin) of the context, the first line above becomes

        cond  = length_regulator(t, ylens=[S])[0]

    and everything after it is the same step.  Such an engine steps with `step_tokens` (or `step_audio` after `attach_audio`
    with a tokenizer); `step` and `step_f0` are refused, as `step_tokens` is on a feature engine.  The wiring, with
    t = V2HotPath.prepare_target(...) of the reference:

        eng  = RealtimeEngine(hot.cfm_lr, hot.cfm, hot.vocoder, **geometry)
        slot = eng.open(t["prompt_condition"], t["mel"], t["style"])
        eng.attach_audio(astral, Resample(stream_rate, 16000), Lin, L16, ce_dit_difference)      # head 0: the wide tokens

    The v2 style branch (AR) has no real-time form: it changes durations and samples freely, so it has no block-aligned step."""

    def __init__(self, length_regulator, cfm, vocoder, S, hop, block, sola_buffer, sola_search, tail=0, max_streams=64,
                 fade_in=None, fade_out=None):
        S, hop, block, Lb, Ls, tail = (int(v) for v in (S, hop, block, sola_buffer, sola_search, tail))
        if block < 1 or Lb < 1 or Ls < 0 or tail < 0 or max_streams < 1:
            raise ValueError("RealtimeEngine: block, sola_buffer and max_streams must be at least 1, sola_search and tail at least 0")
        n_inf = block + Lb + Ls
        if n_inf + tail > S * hop:
            raise ValueError(f"RealtimeEngine: block + sola_buffer + sola_search + tail = {n_inf + tail} samples, a step gives "
                             f"{S} x {hop}")
        if (fade_in is None) != (fade_out is None):
            raise ValueError("RealtimeEngine: give both windows or neither")
        self.length_regulator, self.cfm, self.vocoder = length_regulator, cfm, vocoder
        self.S, self.hop, self.block, self.Lb, self.Ls, self.tail = S, hop, block, Lb, Ls, tail
        self.n_inf, self.start, self.max_streams = n_inf, S * hop - tail - n_inf, int(max_streams)
        self.device = cfm.device
        self.token_mode = bool((getattr(length_regulator, "cfg", None) or {}).get("is_discrete"))       # not an option: the regulator's kind
        if fade_in is None:
            fade_in, fade_out = gui_fade_windows(Lb)
        self.fade_in, self.fade_out = (_lib.f32c(torch.as_tensor(f), self.device).reshape(-1) for f in (fade_in, fade_out))
        if self.fade_in.numel() != Lb or self.fade_out.numel() != Lb:
            raise ValueError(f"RealtimeEngine: the windows must have sola_buffer = {Lb} entries")
        self.state = torch.zeros(self.max_streams, Lb, device=self.device, dtype=torch.float32)      # row = a stream's sola_buffer
        self._streams = {}                  # slot -> (prompt_condition, mel, style): a record of `_stack_prompts`
        self._stacked = (None, None)
        self._audio = None                  # `attach_audio`: the input side of `step_audio`
        self._out = None                    # `attach_output`: the splice at another rate than the model's
        self._speech = {}                   # slot -> the caller's VAD flag (`set_speech`)
        self._gate = {}                     # slot -> gate threshold as an energy of 4 zc samples (`set_gate`); absent: off
        self._vad = None                    # `attach_vad`: the device-resident VAD of `step_audio`
        self._sampler = {}                  # slot -> (n_timesteps, inference_cfg_rate, temperature, random_voice), None = the step call's (`set_sampler`)
        self._pitch = None                  # `attach_pitch`: the device-resident pitch track of `step_audio` (f0-conditioned models)

    def open(self, prompt_condition, mel2, style2):
        """A new stream on the reference (prompt_condition (1, P, Dc), mel2 (1, C, P), style2 (1, Ds)) -> its slot, the
        lowest free one; its SOLA buffer starts from zeros."""
        if prompt_condition.dim() != 3 or mel2.dim() != 3 or style2.dim() != 2 or prompt_condition.size(0) != 1 or \
                mel2.size(0) != 1 or style2.size(0) != 1 or prompt_condition.size(1) != mel2.size(2):
            raise ValueError(f"RealtimeEngine.open: prompt_condition {tuple(prompt_condition.shape)}, mel2 {tuple(mel2.shape)} and "
                             f"style2 {tuple(style2.shape)} are not (1, P, Dc), (1, C, P), (1, Ds)")
        for pc, mel, style in self._streams.values():
            if pc.size(2) != prompt_condition.size(2) or mel.size(1) != mel2.size(1) or style.size(1) != style2.size(1):
                raise ValueError("RealtimeEngine.open: Dc, C or Ds differ from the streams already open")
        slot = next((i for i in range(self.max_streams) if i not in self._streams), None)
        if slot is None:
            raise ValueError(f"RealtimeEngine.open: all {self.max_streams} slots are in use")
        self._streams[slot] = tuple(_lib.f32c(t, self.device) for t in (prompt_condition, mel2, style2))
        self._stacked = (None, None)
        self.state[slot].zero_()
        self._zero_audio(slot)
        self._speech[slot] = True
        self._gate.pop(slot, None)
        self._sampler.pop(slot, None)
        self._zero_vad(slot, on=False)
        self._zero_pitch(slot, forget=True)
        return slot

    def _check_slot(self, slot, what):
        if not 0 <= slot < self.max_streams:
            raise ValueError(f"RealtimeEngine.{what}: slot {slot!r} outside 0 .. {self.max_streams - 1}")
        if slot not in self._streams:
            raise ValueError(f"RealtimeEngine.{what}: slot {slot} is not open")

    def close(self, slot):
        self._check_slot(slot, "close")
        del self._streams[slot]
        self._stacked = (None, None)
        self._speech.pop(slot, None)
        self._gate.pop(slot, None)
        self._sampler.pop(slot, None)
        self._zero_vad(slot, on=False)
        self._zero_pitch(slot, forget=True)

    def reset(self, slot):
        """Zeroes the stream's SOLA buffer (the GUI does so when a stream restarts)."""
        self._check_slot(slot, "reset")
        self.state[slot].zero_()
        self._zero_audio(slot)
        self._speech[slot] = True
        if self._vad is not None:
            self._zero_vad(slot, on=slot in self._vad["on"])
        self._zero_pitch(slot, forget=False)

    # ------------------------------------------------------------------------------------------- live settings
    def attach_output(self, resample_out, fade_in=None, fade_out=None):
        """Output at another rate than the model's: resample_out is an `audio.Resample(model_rate, output_rate)`, both rates
        multiples of 50.  With zc_m and zc_o the 20 ms counts at the two rates, block, sola_buffer and sola_search must be
        multiples of zc_m and zc_m a multiple of the reduced model rate o (the GUI's geometry always is; `realtime_geometry` with
        the model's sr yields it).  The output geometry is the model's scaled by zc_o / zc_m (`realtime_output_geometry`); the
        SOLA state is reallocated as (max_streams, Lb_out) zeros and the windows default to `gui_fade_windows(Lb_out)`.  Allowed
        only while no stream is open.  After it every step method returns (n, block_out) at the output rate, and
        return_parts["infer"] is the (n, n_inf_out) row SOLA saw: one `svc_rt_out` resamples and splices."""
        if self._streams:
            raise ValueError("RealtimeEngine.attach_output: streams are open")
        if (fade_in is None) != (fade_out is None):
            raise ValueError("RealtimeEngine.attach_output: give both windows or neither")
        orig, new = int(resample_out.orig_freq), int(resample_out.new_freq)
        try:
            g = realtime_output_geometry(dict(block=self.block, Lb=self.Lb, Ls=self.Ls), orig, new)
        except ValueError as e:
            raise ValueError(f"RealtimeEngine.attach_output: {e}") from None
        o = orig // math.gcd(orig, new)
        if (orig // 50) % o:
            raise ValueError(f"RealtimeEngine.attach_output: 20 ms at the model rate ({orig // 50} samples) is not a multiple of "
                             f"the reduced rate o = {o}")
        if fade_in is None:
            fade_in, fade_out = gui_fade_windows(g["Lb"])
        fade_in, fade_out = (_lib.f32c(torch.as_tensor(f), self.device).reshape(-1) for f in (fade_in, fade_out))
        if fade_in.numel() != g["Lb"] or fade_out.numel() != g["Lb"]:
            raise ValueError(f"RealtimeEngine.attach_output: the windows must have {g['Lb']} entries at the output rate")
        self._out = dict(g, resample=resample_out, fade_in=fade_in, fade_out=fade_out)
        self.state = torch.zeros(self.max_streams, g["Lb"], device=self.device, dtype=torch.float32)

    def set_speech(self, slot, detected):
        """The GUI's `vad_speech_detected` for one stream, from whatever VAD the caller runs: True on `open` and `reset`; while
        False the stream's blocks are zeros before SOLA (the GUI's `infer_wav = zeros`).  The model still runs for the stream, so
        the batch stays one call."""
        self._check_slot(slot, "set_speech")
        self._speech[slot] = bool(detected)

    def set_gate(self, slot, threshold_db):
        """The GUI's input noise-gate threshold for one stream, in dB (RMS re 1.0): 20 ms frames whose last 80 ms lie below it are
        zeroed before they enter the history (`svc_rt_push_gated`).  None or at most -60: off, the default on `open`; kept across
        `reset`.  Needs `attach_audio`."""
        self._check_slot(slot, "set_gate")
        if self._audio is None:
            raise ValueError("RealtimeEngine.set_gate: attach_audio has not been called")
        p = gate_power(threshold_db, self._audio["zc"])
        if not p >= 0.0 or p == float("inf"):
            raise ValueError(f"RealtimeEngine.set_gate: threshold_db = {threshold_db!r}")
        if p == 0.0:
            self._gate.pop(slot, None)
            return
        if slot not in self._gate:          # energies are tracked only by gated pushes: a gate switched on starts from none
            self._audio["gate_e"][slot].zero_()
        self._gate[slot] = p

    def set_sampler(self, slot, n_timesteps=None, inference_cfg_rate=None, temperature=None, random_voice=None):
        """The GUI's `diffusion_steps` and `inference_cfg_rate` (and the sampler temperature) for one stream.  None: what the
        step call says (temperature: 1.0, random_voice: False), the default on `open`; kept across `reset`.  While no listed slot
        has an override a step is the one `cfm.inference` call it always was; otherwise it is one `cfm.inference_rows` call, in
        which streams of one class (same steps, guided or not) share every launch whatever their rates.  With a
        v2 sampler (`cfm.cfg["version"] == 2`) inference_cfg_rate may be the pair `CFM.inference` takes and random_voice the
        v2 wrapper's anonymisation flag for the stream (classes follow `CFM.rows_plan`); a v1 sampler refuses both."""
        self._check_slot(slot, "set_sampler")
        if n_timesteps is not None and int(n_timesteps) < 1:
            raise ValueError(f"RealtimeEngine.set_sampler: n_timesteps = {n_timesteps!r}")
        rate = inference_cfg_rate
        if isinstance(rate, (list, tuple)):
            if len(rate) != 2:
                raise ValueError(f"RealtimeEngine.set_sampler: a pair of rates has two entries, got {rate!r}")
            rate = (float(rate[0]), float(rate[1]))
        elif rate is not None:
            rate = float(rate)
        for name, v in (("inference_cfg_rate", rate), ("temperature", temperature)):
            if v is not None and not all(math.isfinite(float(x)) for x in (v if isinstance(v, tuple) else (v,))):
                raise ValueError(f"RealtimeEngine.set_sampler: {name} = {v!r}")
        if (isinstance(rate, tuple) or random_voice is not None) and (getattr(self.cfm, "cfg", None) or {}).get("version") != 2:
            raise ValueError("RealtimeEngine.set_sampler: a pair of rates and random_voice need a v2 sampler (cfm.cfg['version'] == 2)")
        if n_timesteps is None and rate is None and temperature is None and random_voice is None:
            self._sampler.pop(slot, None)
        else:
            self._sampler[slot] = (None if n_timesteps is None else int(n_timesteps), rate,
                                   None if temperature is None else float(temperature),
                                   None if random_voice is None else bool(random_voice))

    def attach_vad(self, vad):
        """A device-resident VAD (seedvc_amd.vad.FsmnVad) for `step_audio`: needs `attach_audio` with a 16 kHz
        content rate and a context that keeps the 960 samples of history `svc_vad_step` reads before a block's new ones.
        Allocates the per-slot VAD state and the mute flags (device int32, one per slot).  The VAD is off per slot until
        `set_vad(slot, True)`; a slot with its VAD off has its flag held at 1, so only `set_speech` mutes it."""
        a = self._audio
        if a is None:
            raise ValueError("RealtimeEngine.attach_vad: attach_audio has not been called")
        if a["z16"] != 320:
            raise ValueError(f"RealtimeEngine.attach_vad: the content rate is {a['z16'] * 50} Hz, the VAD takes 16000")
        n_new, end = a["Lin"] // a["zc"] * a["z16"], a["L16"] - a["z16"]
        if end - n_new < 960:
            raise ValueError(f"RealtimeEngine.attach_vad: the context keeps {end - n_new} samples before a block's {n_new} new ones, "
                             f"the VAD reads 960")
        if not callable(getattr(vad, "step", None)):
            raise ValueError("RealtimeEngine.attach_vad: vad has no step")
        from .vad import STATE_FLOATS
        self._vad = dict(vad=vad, n_new=n_new, end=end, on=set(), total={},
                         state=torch.zeros(self.max_streams, STATE_FLOATS, device=self.device, dtype=torch.float32),
                         flags=torch.ones(self.max_streams, device=self.device, dtype=torch.int32))

    def set_vad(self, slot, on):
        """Switches the attached VAD on or off for one stream.  On: the stream's VAD state starts fresh (flag 0: muted until a
        speech segment opens, the GUI's `vad_speech_detected = False`) from the next `step_audio` block.  Off (the default on
        `open`): the flag is held at 1.  Kept across `reset`, which restarts the state."""
        self._check_slot(slot, "set_vad")
        if self._vad is None:
            raise ValueError("RealtimeEngine.set_vad: attach_vad has not been called")
        if bool(on) != (slot in self._vad["on"]):
            self._zero_vad(slot, on=bool(on))

    def _zero_vad(self, slot, on):
        v = self._vad
        if v is None:
            return
        v["state"][slot].zero_()
        v["flags"][slot] = 0 if on else 1
        v["total"][slot] = 0
        (v["on"].add if on else v["on"].discard)(slot)

    def _stack_prompts(self, slots):
        """Padded batch tensors of the streams' references (kept while the same slots come back in the same order)."""
        key = tuple(slots)
        if self._stacked[0] == key:
            return self._stacked[1]
        st = _stack_prompts([self._streams[s] for s in slots], self.device)
        self._stacked = (key, st)
        return st

    @torch.inference_mode()
    def step(self, slots, content, n_timesteps, inference_cfg_rate, z=None, vocoder_kwargs=None, return_parts=False):
        """One block for the streams `slots` (a list of open slots, no slot twice); content (n, Tin, Din), row k for
        slots[k]; z: the sampler's noise (n, C, Pmax + S), torch.randn when None; vocoder_kwargs: passed to the vocoder call
        (HiFT's pinned draws); `step_seeded` takes seeds instead of the tensors.  -> (n, block) float32 on the device; with
        return_parts also dict(mel (n, C, S), infer (n, n_inf), offsets (n,) int32).  After `attach_output` block and n_inf
        are those of the output rate; a slot whose `set_speech` flag is False gets a row of zeros before SOLA."""
        self._check_mode("step", False)
        return self._step(slots, content, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, return_parts, None)

    @torch.inference_mode()
    def step_f0(self, slots, content, f0, f0_lens, n_timesteps, inference_cfg_rate, z=None, vocoder_kwargs=None, return_parts=False,
                seeds=None):
        """`step` for an f0-conditioned regulator with the caller's pitch track: f0 (n, Tf) in Hz, row k for slots[k], f0_lens n
        host frame counts (None: all Tf), handed to the regulator as `length_regulator(content, ylens=[S] * n, n_quantizers=3,
        f0=f0, f0_lens=f0_lens)`; seeds as `step_seeded` (then z is None).  `step_audio` after `attach_pitch` is this step on
        the track `svc_rt_pitch` wrote.  (A method of its own: the parameter list of `step` is part of its contract.)"""
        self._check_mode("step_f0", False)
        if f0 is None:
            raise ValueError("RealtimeEngine.step_f0: f0 is None")
        if f0.dim() != 2 or f0.size(0) != len(slots):
            raise ValueError(f"RealtimeEngine.step_f0: f0 {tuple(f0.shape)} is not (n = {len(slots)}, Tf)")
        if f0_lens is not None:
            f0_lens = _lib.int_list(f0_lens)
            if len(f0_lens) != len(slots) or not all(0 <= v <= f0.size(1) for v in f0_lens):
                raise ValueError(f"RealtimeEngine.step_f0: f0_lens {f0_lens} for {len(slots)} rows of {f0.size(1)} frames")
        return self._step(slots, content, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, return_parts, seeds, None, f0, f0_lens)

    @torch.inference_mode()
    def step_tokens(self, slots, tokens, n_timesteps, inference_cfg_rate, z=None, vocoder_kwargs=None, return_parts=False, seeds=None):
        """`step` of a token-mode engine (the v2 timbre branch): tokens (n, Tin) integer, row k the wide content
        tokens of slots[k]'s context; the regulator call is `length_regulator(tokens, ylens=[S] * n)[0]` and everything after it
        is `step` unchanged.  inference_cfg_rate: a float or the v2 sampler's pair, as `CFM.inference` takes it; seeds as
        `step_seeded` (then z is None).  (A method of its own: the parameter list of `step` is part of its contract.)"""
        self._check_mode("step_tokens", True)
        if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.size(0) != len(slots):
            raise ValueError(f"RealtimeEngine.step_tokens: tokens {tuple(getattr(tokens, 'shape', ()))} is not (n = {len(slots)}, Tin)")
        if tokens.is_floating_point() or tokens.is_complex() or tokens.dtype == torch.bool:
            raise ValueError(f"RealtimeEngine.step_tokens: tokens are {tokens.dtype}, an integer tensor is expected")
        return self._step(slots, tokens, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, return_parts, seeds)

    def _check_mode(self, what, tokens):
        if tokens != self.token_mode:
            raise ValueError(f"RealtimeEngine.{what}: the length regulator is discrete (token mode): use step_tokens" if self.token_mode
                             else f"RealtimeEngine.{what}: the length regulator is not discrete (cfg['is_discrete']): use step")

    def _regulate(self, content, n, f0, f0_lens):
        """The regulator call of a step.  Without a pitch track it is the call it always was; in token mode the v2 regulator's."""
        ylens = torch.LongTensor([self.S] * n)
        if self.token_mode:
            return self.length_regulator(content, ylens=ylens)[0]
        if f0 is None:
            return self.length_regulator(content, ylens=ylens, n_quantizers=3, f0=None)[0]
        return self.length_regulator(content, ylens=ylens, n_quantizers=3, f0=f0, f0_lens=f0_lens)[0]

    @torch.inference_mode()
    def step_seeded(self, slots, content, n_timesteps, inference_cfg_rate, seeds, vocoder_kwargs=None, return_parts=False):
        """`step` with seeds -- n integers in [0, 2^64) for THIS block, row k for slots[k] -- in place of z and of phase0 /
        noise in vocoder_kwargs (which may still pin HiFT's f0).  The caller derives them per block, e.g.
        `derive_seed(stream_seed, block_index)`; they give the sampler noise and, if the vocoder is a HiFT, its source draws,
        made on the device: bit for bit `step` fed `CFM.noise_draws` / `HiFT.noise_draws` of each seed.  (A method of its
        own: the parameter list of `step` is part of its contract.)"""
        if seeds is None:
            raise ValueError("RealtimeEngine.step_seeded: seeds is None")
        return self._step(slots, content, n_timesteps, inference_cfg_rate, None, vocoder_kwargs, return_parts, seeds)

    def _step(self, slots, content, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, return_parts, seeds, speech_dev=None,
              f0=None, f0_lens=None):
        slots = [int(s) for s in slots]
        seeds = _seed_list("RealtimeEngine.step_seeded", seeds, len(slots), z, vocoder_kwargs)
        for s in slots:
            self._check_slot(s, "step")
        if len(set(slots)) != len(slots):
            raise ValueError(f"RealtimeEngine.step: a slot appears twice in {slots}")
        n, dev, S = len(slots), self.device, self.S
        if content.dim() != (2 if self.token_mode else 3) or content.size(0) != n:
            raise ValueError(f"RealtimeEngine.step: content {tuple(content.shape)} is not (n = {n}, Tin" + ("" if self.token_mode else ", Din") + ")")
        live = self._out
        if n == 0:
            out = torch.zeros(0, live["block"] if live else self.block, device=dev)
            parts = dict(mel=torch.zeros(0, self.cfm.in_channels, S, device=dev),
                         infer=torch.zeros(0, live["n_inf"] if live else self.n_inf, device=dev),
                         offsets=torch.zeros(0, dtype=torch.int32, device=dev))
            return (out, parts) if return_parts else out
        with torch.cuda.device(dev):
            st = self._stack_prompts(slots)
            P = st["P"]
            cond = self._regulate(content, n, f0, f0_lens)                       # (n, S, Dc)
            if cond.size(1) != S:
                raise ValueError(f"RealtimeEngine.step: the length regulator gave {cond.size(1)} frames, {S} expected")
            mu = _assemble_cond(st["prompt_condition"], P, cond, [S] * n, st["Pmax"] + S)
            x_lens = [p + S for p in P]
            if not any(s in self._sampler for s in slots):
                mel = self.cfm.inference(mu, x_lens, st["mel"], st["style"], None, n_timesteps, inference_cfg_rate=inference_cfg_rate,
                                         z=z, prompt_lens=P, **_cfm_seeds(seeds))
            else:                                                                # per-slot sampler settings: still one call
                call = (n_timesteps, inference_cfg_rate, 1.0, False)
                settings = [tuple(c if o is None else o for o, c in zip(self._sampler.get(s, (None,) * 4), call)) for s in slots]
                mel = self.cfm.inference_rows(mu, x_lens, st["mel"], st["style"], settings, z=z, prompt_lens=P, **_cfm_seeds(seeds))
            vc = _strip_prompt(mel, P, x_lens, S)
            calls = _vocode(self.vocoder, vc, [S] * n, False, "RealtimeEngine.step", hop=self.hop, seeds=seeds,
                            vocoder_kwargs=vocoder_kwargs)                   # every row has S frames: one plain call
            wave = _lib.f32c(calls[0].wave, dev)
            offsets = torch.empty(n, dtype=torch.int32, device=dev) if return_parts else None
            speech = [1 if self._speech.get(s, True) else 0 for s in slots]
            if speech_dev is not None:                                           # a listed slot has its VAD on: device flags too
                g = live or dict(block=self.block, Lb=self.Lb, Ls=self.Ls, n_inf=self.n_inf, fade_in=self.fade_in, fade_out=self.fade_out)
                out = torch.empty(n, g["block"], device=dev)
                infer = torch.empty(n, g["n_inf"], device=dev)
                _lib.check(_lib.lib().svc_rt_out_dev(live["resample"]._h if live else None, _lib.ptr(wave), wave.size(1), self.start,
                                                     self.n_inf, n, _lib.ptr(self.state), self.max_streams, _lib.i32_host(slots),
                                                     None if all(speech) else _lib.i32_host(speech), _lib.ptr(speech_dev),
                                                     _lib.ptr(g["fade_in"]), _lib.ptr(g["fade_out"]), g["block"], g["Lb"], g["Ls"],
                                                     _lib.ptr(infer), _lib.ptr(out), _lib.ptr(offsets), _lib.stream_ptr()))
            elif live is None and all(speech):                                   # host state decides which entry splices
                out = torch.empty(n, self.block, device=dev)
                _lib.check(_lib.lib().svc_sola_step(_lib.ptr(wave), wave.size(1), self.start, n, _lib.ptr(self.state), self.max_streams,
                                                    _lib.i32_host(slots), _lib.ptr(self.fade_in), _lib.ptr(self.fade_out), self.block,
                                                    self.Lb, self.Ls, _lib.ptr(out), _lib.ptr(offsets), _lib.stream_ptr()))
                infer = wave[:, self.start:self.start + self.n_inf]
            else:
                g = live or dict(block=self.block, Lb=self.Lb, Ls=self.Ls, n_inf=self.n_inf, fade_in=self.fade_in, fade_out=self.fade_out)
                out = torch.empty(n, g["block"], device=dev)
                infer = torch.empty(n, g["n_inf"], device=dev)
                _lib.check(_lib.lib().svc_rt_out(live["resample"]._h if live else None, _lib.ptr(wave), wave.size(1), self.start,
                                                 self.n_inf, n, _lib.ptr(self.state), self.max_streams, _lib.i32_host(slots),
                                                 None if all(speech) else _lib.i32_host(speech), _lib.ptr(g["fade_in"]),
                                                 _lib.ptr(g["fade_out"]), g["block"], g["Lb"], g["Ls"], _lib.ptr(infer), _lib.ptr(out),
                                                 _lib.ptr(offsets), _lib.stream_ptr()))
        if return_parts:
            return out, dict(mel=vc, infer=infer, offsets=offsets)
        return out

    # ------------------------------------------------------------------------------------------- pitch
    def attach_pitch(self, rmvpe, lag_frames=8, warmup_frames=50, max_step_cents=100.0, thred=0.03):
        """Pitch for f0-conditioned (singing) models in `step_audio`: the offline drivers' `auto_f0_adjust` / `pitch_shift` for a
        stream.  rmvpe: anything with `f0_batch((n, L16) samples, thred=) -> (n, frames(L16))` and `frames(n_samples)`
        (seedvc_amd.rmvpe.RMVPE).  Per block the 16 kHz context goes through `rmvpe.f0_batch`, one `svc_rt_pitch` counts the
        2 Lin / zc frames the block renews -- those `lag_frames` before the end of the context -- into the slot's running
        voiced-pitch histogram and shifts the track by (reference median - running median), gliding by at most `max_step_cents`
        per block, and by the slot's semitones (`set_pitch`); the regulator takes the track from frame 2 ce on (a content row
        of 20 ms is two f0 frames).  Needs `attach_audio` with a 16 kHz content rate, a regulator with `f0_condition`,
        lag_frames >= 2 (the last z16 samples of a context are computed again by the next push),
        rmvpe.frames(L16) - lag_frames - 2 Lin / zc >= 0 and 2 ce < rmvpe.frames(L16).  Allocates the per-slot statistics and
        reference medians; `open` and `reset` zero a slot's statistics as they zero its SOLA buffer.  max_step_cents <= 0 or
        +inf means no limit: the shift goes to its target at once.  A second call replaces everything the first one allocated,
        so it is refused while a slot holds a reference median or a `set_pitch` setting; it also switches `set_pitch_window` and
        `set_pitch_memory` off again.

        The defaults are judgement, not measurements: 8 frames of lag keep the counted frames clear of the samples the next
        push recomputes and of RMVPE's view of the zero padding behind them; 50 voiced frames (0.5 s) before a median is
        trusted; 100 cents per block, so a settled shift of an octave arrives in about 2 s of 180 ms blocks."""
        a, old = self._audio, self._pitch
        if a is None:
            raise ValueError("RealtimeEngine.attach_pitch: attach_audio has not been called")
        if old is not None and (old["has_ref"] or old["auto"] or old["semis"]):
            raise ValueError(f"RealtimeEngine.attach_pitch: slots {sorted(old['has_ref'] | set(old['auto']) | set(old['semis']))} hold a "
                             f"reference median or pitch settings that a second attach would drop")
        if a["z16"] != 320:
            raise ValueError(f"RealtimeEngine.attach_pitch: the content rate is {a['z16'] * 50} Hz, RMVPE takes 16000")
        if not getattr(self.length_regulator, "cfg", {}).get("f0_condition"):
            raise ValueError("RealtimeEngine.attach_pitch: the length regulator is not f0-conditioned (cfg['f0_condition'])")
        if not callable(getattr(rmvpe, "f0_batch", None)) or not callable(getattr(rmvpe, "frames", None)):
            raise ValueError("RealtimeEngine.attach_pitch: rmvpe has no f0_batch / frames")
        lag, warmup, cents, thred = int(lag_frames), int(warmup_frames), float(max_step_cents), float(thred)
        if lag < 2:
            raise ValueError(f"RealtimeEngine.attach_pitch: lag_frames = {lag_frames!r}, at least 2 (the last 20 ms of a context are "
                             f"provisional)")
        if warmup < 0 or math.isnan(cents) or math.isnan(thred):
            raise ValueError(f"RealtimeEngine.attach_pitch: warmup_frames = {warmup_frames!r}, max_step_cents = {max_step_cents!r}, "
                             f"thred = {thred!r}")
        Tf, n_new = int(rmvpe.frames(a["L16"])), 2 * (a["Lin"] // a["zc"])
        if Tf - lag - n_new < 0:
            raise ValueError(f"RealtimeEngine.attach_pitch: the context has {Tf} f0 frames, a block counts {n_new} of them "
                             f"{lag} before its end")
        if 2 * a["ce"] >= Tf:
            raise ValueError(f"RealtimeEngine.attach_pitch: 2 ce = {2 * a['ce']} frames are dropped of a track of {Tf}")
        from . import rmvpe as _rmvpe
        max_step = cents * math.log(2.0) / 1200.0 if 0.0 < cents < float("inf") else 0.0       # cents -> natural-log units; 0: no limit
        self._pitch = dict(rmvpe=rmvpe, lag=lag, warmup=warmup, max_step=max_step, thred=thred, Tf=Tf, n_new=n_new,
                           state=torch.zeros(self.max_streams, _rmvpe.PITCH_STATE_WORDS, device=self.device, dtype=torch.int32),
                           ref_median=torch.zeros(self.max_streams, device=self.device, dtype=torch.float32),
                           has_ref=set(), auto={}, semis={},
                           win=None, memory=0, cache=None, ring=None)       # `set_pitch_window`, `set_pitch_memory`: off

    def set_reference_f0(self, slot, f0_ref, f0_ref_frames=None):
        """The pitch track of an open slot's reference (f0_ref (1, To) | (To,) in Hz, `rmvpe.f0_batch` of the reference clip;
        f0_ref_frames: its valid frames, default all): the slot's reference median -- torch's lower-middle median of
        log(f0 + 1e-5) over the voiced frames -- is written on the device from the `medians` output of `svc_f0_adjust` (column
        m_ori), with no synchronisation, and the automatic shift is switched on for the slot.  Until this call a slot has no
        automatic shift and `set_pitch(auto_adjust=True)` raises.  A reference without a voiced frame has the median 0.0, which
        the host cannot see without a synchronisation: `svc_rt_pitch` takes a median that is not positive as "no reference" and
        applies no automatic shift, as `svc_f0_adjust` applies none.  (A method of its own: the parameter list of `open` is
        part of its contract.)  Needs `attach_pitch`."""
        self._check_slot(slot, "set_reference_f0")
        p = self._pitch
        if p is None:
            raise ValueError("RealtimeEngine.set_reference_f0: attach_pitch has not been called")
        f = f0_ref.reshape(1, -1) if f0_ref.dim() == 1 else f0_ref
        if f.dim() != 2 or f.size(0) != 1 or f.size(1) < 1:
            raise ValueError(f"RealtimeEngine.set_reference_f0: f0_ref {tuple(f0_ref.shape)} is not (1, To)")
        To = f.size(1)
        frames = To if f0_ref_frames is None else int(f0_ref_frames)
        if not 1 <= frames <= To:
            raise ValueError(f"RealtimeEngine.set_reference_f0: f0_ref_frames = {f0_ref_frames!r} of {To}")
        from .rmvpe import f0_adjust
        f = _lib.f32c(f, self.device)
        _, med = f0_adjust(f, [frames], f, [frames], auto_f0_adjust=False, pitch_shift=0, return_medians=True)
        p["ref_median"][slot:slot + 1].copy_(med[:, 1])
        p["has_ref"].add(slot)
        p["auto"].setdefault(slot, True)

    def set_pitch(self, slot, semitones=None, auto_adjust=None):
        """The offline drivers' `pitch_shift` (semitones, any finite number) and `auto_f0_adjust` for one stream; None keeps
        what the slot has.  Defaults on `open`: 0 semitones, and the automatic shift on iff the slot has a reference median
        (`set_reference_f0`); kept across `reset`.  Switching the automatic shift lets the applied shift glide to its new
        target.  Needs `attach_pitch`."""
        self._check_slot(slot, "set_pitch")
        p = self._pitch
        if p is None:
            raise ValueError("RealtimeEngine.set_pitch: attach_pitch has not been called")
        if semitones is not None and not math.isfinite(float(semitones)):
            raise ValueError(f"RealtimeEngine.set_pitch: semitones = {semitones!r}")
        if auto_adjust and slot not in p["has_ref"]:
            raise ValueError(f"RealtimeEngine.set_pitch: slot {slot} has no reference median (set_reference_f0): no automatic shift")
        if semitones is not None:
            p["semis"][slot] = float(semitones)
        if auto_adjust is not None:
            p["auto"][slot] = bool(auto_adjust)

    def set_pitch_window(self, window_frames, guard_frames=None):
        """RMVPE on the context's tail: per block `rmvpe.f0_batch` sees only the last `window_frames` f0 frames of
        the context (160 samples each), not all Tf; the older frames of a slot's raw track stay in a per-slot device cache that
        moves with the stream, and one `svc_rt_pitch_win` updates it, counts and shifts.  The first `guard_frames` of a window
        are not trusted (they sit next to RMVPE's reflect padding): the cache keeps what an earlier block wrote there.
        Engine-wide (geometry and allocations are shared): needs `attach_pitch`, and is refused while any slot is open.
        `set_pitch_window(None)` switches it off again.  Requires window_frames - guard_frames >= 2 Lin / zc + lag_frames (a counted
        frame is one this block's window wrote), guard_frames >= 0, window_frames <= Tf <= 4096 and a window of at least
        `svc_rmvpe_min_len()` samples.  With the window on, return_parts["f0_raw"] is the slots' cache rows (n, Tf) and
        "f0_window" (n, window_frames) is RMVPE's track of the tail.

        No values are proposed: suitable ones depend on RMVPE's receptive field (how far a frame's estimate looks to either
        side), and the window's effect on the released checkpoint's accuracy is unmeasured here, because the checkpoint is
        absent.  Internally RMVPE pads a clip's frames to a multiple of 32 (RV_TMULT), so windows of 33 .. 64 frames cost the
        same network pass."""
        p = self._pitch_setting("set_pitch_window")
        if window_frames is None:
            p["win"] = None
            self._pitch_buffers()
            return
        if guard_frames is None:
            raise ValueError("RealtimeEngine.set_pitch_window: guard_frames is needed with window_frames (no default is proposed)")
        self._pitch_tf_limit("set_pitch_window")
        W, guard = int(window_frames), int(guard_frames)
        if guard < 0 or W > p["Tf"] or W - guard < p["n_new"] + p["lag"]:
            raise ValueError(f"RealtimeEngine.set_pitch_window: window_frames = {window_frames!r}, guard_frames = {guard_frames!r}: "
                             f"guard_frames >= 0, window_frames <= Tf = {p['Tf']} and window_frames - guard_frames >= "
                             f"{p['n_new']} + {p['lag']} (the frames a block counts lie lag_frames before the end) are required")
        n_win = self._audio["L16"] - _PITCH_HOP * (p["Tf"] - W)
        if n_win < int(_lib.lib().svc_rmvpe_min_len()):
            raise ValueError(f"RealtimeEngine.set_pitch_window: a window of {W} frames is {n_win} samples, RMVPE takes at least "
                             f"{int(_lib.lib().svc_rmvpe_min_len())}")
        p["win"] = (W, guard)
        self._pitch_buffers()

    def set_pitch_memory(self, memory_frames):
        """Statistics that forget: the running median of a slot is taken over its last `memory_frames` counted
        frames (10 ms each, voiced or not) instead of its whole past: a per-slot device ring holds their bins, and what a block
        pushes out of it leaves the histogram again.  A hard window, not a decay; when fewer than `warmup_frames` voiced frames
        remain the shift glides back to 0.  Engine-wide: needs `attach_pitch`, refused while any slot is open;
        `set_pitch_memory(None)` switches it off again.  memory_frames >= 2 Lin / zc.  No value is proposed.  With only the
        memory on the pitch step is `svc_rt_pitch_win` with the whole context as its window (window = Tf, guard = 0)."""
        p = self._pitch_setting("set_pitch_memory")
        if memory_frames is None:
            p["memory"] = 0
            self._pitch_buffers()
            return
        m = int(memory_frames)
        if m < p["n_new"]:
            raise ValueError(f"RealtimeEngine.set_pitch_memory: memory_frames = {memory_frames!r} is below the {p['n_new']} frames a "
                             f"block counts")
        self._pitch_tf_limit("set_pitch_memory")
        p["memory"] = m
        self._pitch_buffers()

    def _pitch_setting(self, what):
        if self._pitch is None:
            raise ValueError(f"RealtimeEngine.{what}: attach_pitch has not been called")
        if self._streams:
            raise ValueError(f"RealtimeEngine.{what}: streams are open")
        return self._pitch

    def _pitch_tf_limit(self, what):
        from .rmvpe import PITCH_WIN_MAX_TF
        if self._pitch["Tf"] > PITCH_WIN_MAX_TF:
            raise ValueError(f"RealtimeEngine.{what}: the context has {self._pitch['Tf']} f0 frames, svc_rt_pitch_win stages at most "
                             f"{PITCH_WIN_MAX_TF}")

    def _pitch_buffers(self):
        """The slots' cache rows and rings for the settings as they stand (no slot is open: everything starts fresh)."""
        from . import rmvpe as _rmvpe
        p = self._pitch
        on = p["win"] is not None or p["memory"] > 0
        p["cache"] = _rmvpe.rt_pitch_cache(self.max_streams, p["Tf"], self.device) if on else None
        p["ring"] = _rmvpe.rt_pitch_ring(self.max_streams, p["memory"], self.device) if on else None

    def _zero_pitch(self, slot, forget):
        """Fresh statistics for the slot; forget: also its reference median and settings (`open`, `close`)."""
        p = self._pitch
        if p is None:
            return
        p["state"][slot].zero_()
        for name in ("cache", "ring"):
            if p[name] is not None:
                p[name][slot].zero_()
        if forget:
            p["ref_median"][slot] = 0.0
            p["has_ref"].discard(slot)
            p["auto"].pop(slot, None)
            p["semis"].pop(slot, None)

    def _pitch_track(self, slots, ctx, return_parts):
        """The pitch stage of `step_audio`: ctx (n, L16) -> (f0 (n, Tf - 2 ce) for the regulator, f0_lens, parts | None)."""
        from . import rmvpe as _rmvpe
        p, ce2 = self._pitch, 2 * self._audio["ce"]
        if p["cache"] is not None:
            return self._pitch_track_win(slots, ctx, return_parts)
        raw = p["rmvpe"].f0_batch(ctx, thred=p["thred"])
        if raw.dim() != 2 or tuple(raw.shape) != (len(slots), p["Tf"]):
            raise ValueError(f"RealtimeEngine.step_audio: rmvpe.f0_batch gave {tuple(raw.shape)}, ({len(slots)}, {p['Tf']}) expected")
        res = _rmvpe.rt_pitch(raw, p["n_new"], p["lag"], slots, p["state"], p["ref_median"],
                              [1 if p["auto"].get(s, False) else 0 for s in slots], [p["semis"].get(s, 0.0) for s in slots],
                              warmup=p["warmup"], max_step=p["max_step"], return_shift=return_parts)
        f0, shift = res if return_parts else (res, None)
        parts = None
        if return_parts:
            # one device copy per slot, addressed by host integers: an index tensor would be a blocking host-to-device copy
            voiced = torch.stack([p["state"][s, _rmvpe.PITCH_BINS] for s in slots])
            parts = dict(f0_raw=raw, f0=f0, pitch_shift=shift, pitch_voiced=voiced)
        return f0[:, ce2:], [p["Tf"] - ce2] * len(slots), parts

    def _pitch_track_win(self, slots, ctx, return_parts):
        """`_pitch_track` with `set_pitch_window` or `set_pitch_memory` on: RMVPE on the context's tail, one `svc_rt_pitch_win`."""
        from . import rmvpe as _rmvpe
        p, ce2, n = self._pitch, 2 * self._audio["ce"], len(slots)
        Tf = p["Tf"]
        W, guard = p["win"] if p["win"] is not None else (Tf, 0)
        s0 = _PITCH_HOP * (Tf - W)
        # the slice starts on a frame centre, so its frame j is centred on context frame Tf - W + j and it has exactly W frames
        assert int(p["rmvpe"].frames(ctx.size(1) - s0)) == W, (ctx.size(1), s0, W)
        win = p["rmvpe"].f0_batch(ctx[:, s0:].contiguous(), thred=p["thred"])
        if win.dim() != 2 or tuple(win.shape) != (n, W):
            raise ValueError(f"RealtimeEngine.step_audio: rmvpe.f0_batch gave {tuple(win.shape)}, ({n}, {W}) expected")
        res = _rmvpe.rt_pitch_win(win, guard, p["n_new"], p["lag"], slots, p["cache"], p["ring"], p["state"], p["ref_median"],
                                  [1 if p["auto"].get(s, False) else 0 for s in slots], [p["semis"].get(s, 0.0) for s in slots],
                                  warmup=p["warmup"], max_step=p["max_step"], return_shift=return_parts, return_raw=return_parts)
        f0, shift, raw = res if return_parts else (res, None, None)
        parts = None
        if return_parts:
            voiced = torch.stack([p["state"][s, _rmvpe.PITCH_BINS] for s in slots])
            parts = dict(f0_raw=raw, f0=f0, pitch_shift=shift, pitch_voiced=voiced, f0_window=win)
        return f0[:, ce2:], [Tf - ce2] * n, parts

    # ------------------------------------------------------------------------------------------- audio in
    def attach_audio(self, content, resample, Lin, L16, ce_dit_difference):
        """The input side of a block step: after this call `step_audio` takes the microphone block itself.  content: anything
        with `semantic_fn((n, L16) samples) -> (n, T, D)` (Wav2Vec2Content, WhisperContent); on a token-mode engine anything
        with `tokens_fn((n, L16) samples, head=) -> (n, R) integer` and `codebook_size(head)` (AstralTokenizer), read at head 0,
        the wide tokens of the v2 timbre branch (`attach_tokens` names another head), whose codebook must fit the regulator's;
        resample: an
        `audio.Resample(stream_rate, content_rate)`, both rates multiples of 50; Lin: samples per block at the stream rate, a
        multiple of zc = stream_rate // 50; L16: the content-rate context per stream (`realtime_input_geometry`);
        ce_dit_difference: seconds of content dropped at the front (the GUI's `S_alt[:, int(ce_dit_difference * 50):]`).
        Allocates the per-slot history (max_streams, 2 zc) and the two-plane context ring of `svc_rt_push`, zeros; `open` and
        `reset` zero a slot's rows as they zero its SOLA buffer."""
        self._attach_audio(content, resample, Lin, L16, ce_dit_difference, 0)

    def attach_tokens(self, content, resample, Lin, L16, ce_dit_difference, head=0):
        """`attach_audio` of a token-mode engine with the tokenizer's head named: `step_audio` reads
        `content.tokens_fn(ctx, head=head)`.  (A method of its own: the parameter list of `attach_audio` is part of its
        contract.)  Refused on a feature engine."""
        if not self.token_mode:
            raise ValueError("RealtimeEngine.attach_audio: attach_tokens needs a discrete length regulator (cfg['is_discrete'])")
        self._attach_audio(content, resample, Lin, L16, ce_dit_difference, head)

    def _attach_audio(self, content, resample, Lin, L16, ce_dit_difference, head):
        orig, new = int(resample.orig_freq), int(resample.new_freq)
        Lin, L16 = int(Lin), int(L16)
        if orig < 50 or new < 50 or orig % 50 or new % 50:
            raise ValueError(f"RealtimeEngine.attach_audio: the rates {orig} and {new} must be multiples of 50")
        zc, z16 = orig // 50, new // 50
        if Lin < zc or Lin % zc:
            raise ValueError(f"RealtimeEngine.attach_audio: Lin = {Lin} is not a positive multiple of zc = {zc}")
        n_new = (Lin // zc + 1) * z16
        if L16 < n_new:
            raise ValueError(f"RealtimeEngine.attach_audio: L16 = {L16} is below the {n_new} samples a block renews")
        ce = int(float(ce_dit_difference) * 50)
        if ce < 0:
            raise ValueError("RealtimeEngine.attach_audio: ce_dit_difference is negative")
        head = int(head)
        if self.token_mode:
            if not callable(getattr(content, "tokens_fn", None)) or not callable(getattr(content, "codebook_size", None)):
                raise ValueError("RealtimeEngine.attach_audio: the length regulator is discrete (token mode): content needs tokens_fn "
                                 "and codebook_size (a tokenizer), a feature encoder does not fit")
            K, Kr = int(content.codebook_size(head)), int(self.length_regulator.cfg["codebook_size"])
            if K > Kr:
                raise ValueError(f"RealtimeEngine.attach_audio: head {head} has {K} codes, the length regulator's codebook_size is {Kr}")
        elif callable(getattr(content, "tokens_fn", None)):
            raise ValueError("RealtimeEngine.attach_audio: content is a tokenizer (tokens_fn), the length regulator is not discrete "
                             "(cfg['is_discrete'])")
        elif not callable(getattr(content, "semantic_fn", None)):
            raise ValueError("RealtimeEngine.attach_audio: content has no semantic_fn")
        ms, planes = self.max_streams, 2 * self.max_streams * L16
        ring = torch.zeros(int(_lib.lib().svc_rt_ring_floats(ms, L16)), device=self.device, dtype=torch.float32)
        self._audio = dict(content=content, head=head, resample=resample, Lin=Lin, L16=L16, zc=zc, z16=z16, ce=ce, ring=ring,
                           planes=ring[:planes].view(2, ms, L16), tickets=ring[planes:].view(torch.int64),
                           tiles=int(_lib.lib().svc_rt_push_tiles(L16)),
                           hist=torch.zeros(ms, 2 * zc, device=self.device, dtype=torch.float32),
                           gate_e=torch.zeros(ms, 3, device=self.device, dtype=torch.float32))
        self._gate = {}

    def _zero_audio(self, slot):
        if self._audio is not None:
            self._audio["planes"][:, slot].zero_()
            self._audio["hist"][slot].zero_()
            self._audio["gate_e"][slot].zero_()

    def audio_context(self, slot):
        """The content-rate context (L16,) of an open slot as the last `step_audio` left it (a copy; this call synchronises to
        read the slot's plane bit: it is for tests and tools, not for the block loop)."""
        self._check_slot(slot, "audio_context")
        if self._audio is None:
            raise ValueError("RealtimeEngine.audio_context: attach_audio has not been called")
        a = self._audio
        return a["planes"][(int(a["tickets"][slot]) // a["tiles"]) & 1, slot].clone()

    @torch.inference_mode()
    def step_audio(self, slots, audio, n_timesteps, inference_cfg_rate, z=None, vocoder_kwargs=None, return_parts=False):
        """One block from audio: audio (n, Lin) float32 at the stream rate, row k the new samples of slots[k].  One
        `svc_rt_push` (history, resampling, context shift and the dense batch), then
        `content.semantic_fn(ctx)[:, int(ce_dit_difference * 50):]`, then `step`.  -> as `step`; with return_parts the dict also
        carries ctx (n, L16) and content (n, T, D).  In token mode the middle is
        `content.tokens_fn(ctx, head=head)[:, int(ce_dit_difference * 50):]`, then `step_tokens`, inference_cfg_rate may be the
        v2 pair, and the dict carries ctx and tokens (n, R - ce) instead of content.  Lengths and slots are host integers:
        nothing synchronises.  Where a listed
        slot has a gate (`set_gate`) the push is `svc_rt_push_gated` and the dict also carries gate_mask (n, Lin / zc) int32.
        After `attach_pitch` the regulator also gets the streams' shifted pitch tracks (`rmvpe.f0_batch(ctx)`, one `svc_rt_pitch`;
        DESIGN.md 8q) and the dict carries f0_raw and f0 (n, Tf), pitch_shift (n,) and pitch_voiced (n,) int32.  With
        `set_pitch_window` or `set_pitch_memory` on, RMVPE runs on the context's tail and the step is one `svc_rt_pitch_win`
        (DESIGN.md 8r): f0_raw is the slots' cached track and the dict also carries f0_window (n, window_frames)."""
        return self._step_audio(slots, audio, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, return_parts, None)

    @torch.inference_mode()
    def step_audio_seeded(self, slots, audio, n_timesteps, inference_cfg_rate, seeds, vocoder_kwargs=None, return_parts=False):
        """`step_audio` with per-block seeds in place of z and the vocoder's draws, as `step_seeded`."""
        if seeds is None:
            raise ValueError("RealtimeEngine.step_audio_seeded: seeds is None")
        return self._step_audio(slots, audio, n_timesteps, inference_cfg_rate, None, vocoder_kwargs, return_parts, seeds)

    def _step_audio(self, slots, audio, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, return_parts, seeds):
        a = self._audio
        if a is None:
            raise ValueError("RealtimeEngine.step_audio: attach_audio has not been called")
        slots = [int(s) for s in slots]
        for s in slots:
            self._check_slot(s, "step_audio")
        if len(set(slots)) != len(slots):
            raise ValueError(f"RealtimeEngine.step_audio: a slot appears twice in {slots}")
        n = len(slots)
        if not 1 <= n <= 64:
            raise ValueError(f"RealtimeEngine.step_audio: {n} slots, 1 .. 64 per call")
        if audio.dim() != 2 or tuple(audio.shape) != (n, a["Lin"]):
            raise ValueError(f"RealtimeEngine.step_audio: audio {tuple(audio.shape)} is not (n = {n}, Lin = {a['Lin']})")
        with torch.cuda.device(self.device):
            block = _lib.f32c(audio, self.device)
            ctx = torch.empty(n, a["L16"], device=self.device, dtype=torch.float32)
            pows = [self._gate.get(s, 0.0) for s in slots]
            mask = None
            if not any(pows):                                                    # host state decides which entry pushes
                _lib.check(_lib.lib().svc_rt_push(a["resample"]._h, _lib.ptr(block), block.stride(0), a["Lin"], n, _lib.i32_host(slots),
                                                  self.max_streams, a["zc"], a["z16"], _lib.ptr(a["hist"]), _lib.ptr(a["ring"]), a["L16"],
                                                  _lib.ptr(ctx), _lib.stream_ptr()))
            else:
                mask = torch.empty(n, a["Lin"] // a["zc"], device=self.device, dtype=torch.int32) if return_parts else None
                _lib.check(_lib.lib().svc_rt_push_gated(a["resample"]._h, _lib.ptr(block), block.stride(0), a["Lin"], n,
                                                        _lib.i32_host(slots), self.max_streams, a["zc"], a["z16"], _lib.ptr(a["hist"]),
                                                        _lib.ptr(a["ring"]), a["L16"], _lib.ptr(ctx), (C.c_float * n)(*pows),
                                                        _lib.ptr(a["gate_e"]), _lib.ptr(mask), _lib.stream_ptr()))
            # the VAD runs on the samples of the context that no later push computes again (everything but its last z16): the
            # gated, resampled stream bit for bit, 20 ms behind the microphone
            v, vad_parts, speech_dev = self._vad, None, None
            rows = [k for k, s in enumerate(slots) if v is not None and s in v["on"]]
            if rows:
                x = ctx if len(rows) == n else torch.stack([ctx[k] for k in rows])      # device copies only: nothing synchronises
                on = [slots[k] for k in rows]
                vad_parts = v["vad"].step(x, v["end"], v["n_new"], [v["total"][s] for s in on], on, v["state"], v["flags"],
                                          return_parts=return_parts)
                for s in on:
                    v["total"][s] += v["n_new"]
                speech_dev = v["flags"]
            if self.token_mode:
                content = a["content"].tokens_fn(ctx, head=a["head"])[:, a["ce"]:]
            else:
                content = a["content"].semantic_fn(ctx)[:, a["ce"]:]
            f0, f0_lens, pitch_parts = self._pitch_track(slots, ctx, return_parts) if self._pitch is not None else (None, None, None)
        res = self._step(slots, content, n_timesteps, inference_cfg_rate, z, vocoder_kwargs, return_parts, seeds, speech_dev, f0, f0_lens)
        if return_parts:
            res[1].update(ctx=ctx, **({"tokens": content} if self.token_mode else {"content": content}))
            if pitch_parts is not None:
                res[1].update(pitch_parts)
            if vad_parts is not None:
                res[1]["vad"] = dict(vad_parts, slots=on, flags=speech_dev.clone())
            if mask is not None:
                res[1]["gate_mask"] = mask
        return res


# ----------------------------------------------------------------------------------------- multi-GPU sharding
def shard_range(n_items, rank, world_size):
    """Contiguous block partition of `n_items` utterances over ranks (first ranks take the remainder)."""
    base, rem = divmod(n_items, world_size)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


def gather_audio(local_wave, local_lens, n_items, group=None):
    """Gather per-rank output audio on rank 0.  local_wave (n_local, Lmax_local) float32, local_lens list[int].
    One length all-gather (ints) + one padded gather of audio; no collective is used inside the sampler or
    vocoder (utterances are independent).  Returns a list of 1-D tensors on rank 0, None elsewhere."""
    import torch.distributed as dist
    if not dist.is_initialized() or dist.get_world_size(group) == 1:
        return [local_wave[i, :local_lens[i]] for i in range(local_wave.size(0))]
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    dev = local_wave.device
    # lengths: every rank contributes a fixed-size vector (max shard size), -1 padded
    max_shard = (n_items + world - 1) // world
    lens = torch.full((max_shard,), -1, dtype=torch.int64, device=dev)
    lens[:len(local_lens)] = torch.tensor(local_lens, dtype=torch.int64, device=dev)
    all_lens = [torch.empty_like(lens) for _ in range(world)]
    dist.all_gather(all_lens, lens, group=group)
    all_lens = torch.stack(all_lens).cpu()          # one device -> host copy; the loops below index host memory
    Lmax = int(all_lens.max())
    buf = torch.zeros(max_shard, Lmax, dtype=torch.float32, device=dev)
    if local_wave.numel():
        buf[:local_wave.size(0), :local_wave.size(1)] = local_wave
    gathered = [torch.empty_like(buf) for _ in range(world)] if rank == 0 else None
    dist.gather(buf, gathered, dst=0, group=group)
    if rank != 0:
        return None
    out = []
    for r in range(world):
        for i in range(max_shard):
            n = int(all_lens[r][i])
            if n >= 0:
                out.append(gathered[r][i, :n])
    return out


class Lanes:
    """Several independent (sampler, vocoder) handle pairs on one GPU, each on its own HIP stream.

    The C ABI is re-entrant per (handle, stream) pair; utterances are independent, so a batch is split across lanes
    and the lanes' kernels overlap on the device (one lane's tail waves / small kernels run beside the other's
    GEMMs).  make_pair() -> (cfm, vocoder) is called once per lane."""

    # Lane streams are created once per device and shared by every Lanes object of the process: the runtime maps HIP
    # streams onto a few hardware queues as they are first used, and the streams of a SECOND Lanes object (a service that
    # rebuilds its models; bench.py's secondary workloads) were seen to land on one queue -- its lanes then run one after
    # the other (small B = 64: 40.6 k -> 38.4 k frames/s for whatever ran second in a process).
    _streams = {}

    @classmethod
    def _lane_stream(cls, device, i):
        key = (device.index if device.index is not None else torch.cuda.current_device(), i)
        if key not in cls._streams:
            cls._streams[key] = torch.cuda.Stream(device=device)
        return cls._streams[key]

    def __init__(self, make_pair, n_lanes=2, device="cuda:0"):
        self.device = torch.device(device)
        self.lanes = []
        for i in range(n_lanes):
            cfm, voc = make_pair()
            self.lanes.append((HotPath(cfm, voc), self._lane_stream(self.device, i)))

    @torch.inference_mode()
    def convert_batch(self, mu, prompt, style, n_timesteps, inference_cfg_rate, z=None, vocoder_kwargs=None):
        B = mu.size(0)
        n = len(self.lanes)
        cur = torch.cuda.current_stream(self.device)
        start = torch.cuda.Event()
        start.record(cur)
        outs, done = [], []
        for i, (hp, st) in enumerate(self.lanes):
            s, e = shard_range(B, i, n)
            if e == s:
                continue
            st.wait_event(start)
            with torch.cuda.stream(st):
                kw = {k: v[s:e] for k, v in (vocoder_kwargs or {}).items()}
                outs.append(hp.convert_batch(mu[s:e], prompt[s:e], style[s:e], n_timesteps, inference_cfg_rate,
                                             z=None if z is None else z[s:e], vocoder_kwargs=kw))
                ev = torch.cuda.Event()
                ev.record(st)
                done.append(ev)
        for ev in done:
            cur.wait_event(ev)
        return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
