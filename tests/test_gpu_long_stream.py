"""GPU side of long-form streaming: `svc_chunks_emit` bit for bit against `long_stream_cases.emit_model` (which
test_host_long_stream.py pins to the assemble and seam models) and against `svc_chunks_assemble` itself;
`HotPath.convert_long_stream` with the exact stand-ins against the reference's own loop over every schedule and lookahead, its
laziness, and with real models inside the pool's bound of the oracle; `V2HotPath.convert_long_stream` against
`convert_long_batch` and the host splice.  Models, inputs and oracles are those of test_gpu_long_batch.py and
test_gpu_v2_long.py, imported so that one suite run builds them once."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import ar_batch_cases as A
import cases
import long_batch_cases as LB
import long_stream_cases as LS
import test_gpu_long_batch as TB
import test_gpu_v2_long as TV
import v2_long_cases as L

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
OVW = cases.CHUNK_OVERLAP * cases.CHUNK_HOP
SENTINEL, PCM_SENTINEL = -7.0, 12345
i32 = lambda v: (C.c_int32 * len(v))(*[int(x) for x in v])      # noqa: E731
i64 = lambda v: (C.c_int64 * len(v))(*[int(x) for x in v])      # noqa: E731


# -------------------------------------------------------------------------------------------------------- svc_chunks_emit
def _emit_gpu(W, lens, pieces, ov, out_len, pcm=True, expect_error=None):
    """W (n_rows, stride) numpy, NaN past lens; pieces [(row, prev_row, begin, end, out_off)] -> (out, pcm) numpy; both planes hold
    their sentinel wherever no piece wrote."""
    from seedvc_amd import _lib
    fi, fo = (torch.from_numpy(f).to(DEV) for f in LB.fades(ov))
    dW = torch.from_numpy(W).to(DEV)
    out = torch.full((out_len,), SENTINEL, device=DEV)
    plane = torch.full((out_len,), PCM_SENTINEL, device=DEV, dtype=torch.int16) if pcm else None
    rc = _lib.lib().svc_chunks_emit(_lib.ptr(dW), W.shape[1], W.shape[0], i32([p[0] for p in pieces]), i32([lens[p[0]] for p in pieces]),
                                    i32([p[1] for p in pieces]), i32([lens[p[1]] if p[1] >= 0 else 0 for p in pieces]),
                                    i32([p[2] for p in pieces]), i32([p[3] for p in pieces]), i64([p[4] for p in pieces]), len(pieces),
                                    _lib.ptr(fi), _lib.ptr(fo), ov, _lib.ptr(out), _lib.ptr(plane), out_len, _lib.stream_ptr())
    torch.cuda.synchronize()
    if expect_error is not None:
        assert rc != 0 and expect_error in _lib.lib().svc_last_error()
    else:
        _lib.check(rc)
    return out.cpu().numpy(), plane.cpu().numpy() if pcm else None


def _seventy_pieces(ov, quantum):
    """71 chunks of 9 files under the style branch's seam rule, lengths multiples of `quantum`, in rows that are a random
    permutation of the chunks: one chunk dropped in the middle of a file (its neighbours' seam has a non-adjacent prev_row), one
    file whose last chunk is empty (a tail-flush piece), one whose last chunk is shorter than the overlap.  70 pieces, released
    by a shuffled completion order; files lie 4 * k samples apart in `out`, so there are samples no piece covers.
    -> (waves, lens by row, pieces of `emit_model`, out_len)."""
    rng = np.random.default_rng(ov)
    per = [9, 8, 8, 8, 8, 8, 8, 8, 6]
    q = lambda n: max(quantum, n // quantum * quantum)      # noqa: E731
    lens_of = {(u, k): q(int(rng.integers(2 * ov, 44))) for u, n in enumerate(per) for k in range(n)}
    lens_of[(1, 3)] = q(ov + 2)                     # below 2 ov, not last: dropped
    lens_of[(2, 7)] = 0                             # empty last chunk: chunk 6 ends the file, its tail is flushed
    lens_of[(3, 7)] = q(ov - 2) if quantum < ov - 2 else quantum       # a last chunk shorter than the overlap
    assert lens_of[(1, 3)] < 2 * ov and 0 < lens_of[(3, 7)] < ov
    keys = list(lens_of)
    rows = list(range(len(keys)))
    random.Random(ov).shuffle(rows)
    row_of = dict(zip(keys, rows))
    order = list(keys)
    random.Random(ov + 1).shuffle(order)
    pieces = LS.splice(per, lens_of, order, ov)
    per_file = LS.file_pieces(pieces, len(per))
    base, at = [], 4
    for ps in per_file:
        base.append(at)
        at += -(-sum(p.end - p.begin for p in ps) // 4) * 4 + 4 * (len(base) % 3)
    lens = [0] * len(keys)
    for uk, r in row_of.items():
        lens[r] = lens_of[uk]
    waves = [None] * len(keys)
    for r, n in enumerate(lens):
        w = rng.uniform(-1.2, 1.2, n).astype(np.float32)
        if n > 3:
            w[1], w[n - 2] = 1.0, -1.0              # where numpy's cast wraps and the kernel saturates
        waves[r] = w
    args = LS.emit_args(pieces, row_of, base)
    assert len(args) == 70 and any(b > 0 for _, _, b, _, _ in args) and any(p >= 0 and abs(p - r) > 1 for r, p, *_ in args)
    return waves, lens, args, at + 4


@pytest.mark.parametrize("ov, quantum, extra", [(8, 4, 4), (6, 1, 3)], ids=["16_byte_path", "4_byte_path"])
def test_emit_equals_the_model_and_writes_nothing_else(ov, quantum, extra):
    waves, lens, pieces, out_len = _seventy_pieces(ov, quantum)
    W = LB.padded_rows(waves, max(lens) + extra)
    got, pcm = _emit_gpu(W, lens, pieces, ov, out_len)
    want = LS.emit_model(W, lens, pieces, ov, out=np.full(out_len, SENTINEL, np.float32))
    covered = np.zeros(out_len, bool)
    for _, _, b, e, off in pieces:
        assert not covered[off:off + e - b].any()
        covered[off:off + e - b] = True
    assert not np.isnan(want).any() and (~covered).sum() >= 8
    assert np.array_equal(got, want)                                           # the pieces bit for bit, the sentinel elsewhere
    assert np.array_equal(got[~covered], np.full((~covered).sum(), SENTINEL, np.float32))
    assert np.array_equal(pcm[covered], LS.pcm_model(want[covered])) and (pcm[~covered] == PCM_SENTINEL).all()
    assert (pcm == 32767).any() and (pcm == -32768).any() and (want[covered] == 1.0).any() and (want[covered] == -1.0).any()
    without, _ = _emit_gpu(W, lens, pieces, ov, out_len, pcm=False)            # the float plane does not depend on the pcm plane
    assert np.array_equal(without, got)


def _assemble_gpu(W, lens, first, last, ov):
    from seedvc_amd import _lib
    fi, fo = (torch.from_numpy(f).to(DEV) for f in LB.fades(ov))
    dW = torch.from_numpy(W).to(DEV)
    n_out = sum(n - (0 if l else ov) for n, l in zip(lens, last))
    out = torch.full((n_out,), float("nan"), device=DEV)
    _lib.check(_lib.lib().svc_chunks_assemble(_lib.ptr(dW), C.c_longlong(W.shape[1]), i32(lens), i32(first), i32(last), len(lens),
                                              _lib.ptr(fi), _lib.ptr(fo), ov, _lib.ptr(out), C.c_longlong(n_out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("extra", [8, 5], ids=["stride_x4", "stride_odd"])
def test_emit_of_every_piece_equals_assemble(extra, golden):
    """The nine `chunkstream` and `chunkloop` utterances: their pieces, released in a shuffled order, give `svc_chunks_assemble`'s
    output and the reference's fixtures."""
    rows = [LB.chunkstream_rows(n) for n in cases.CHUNKSTREAM_CASES] + [LB.chunkloop_rows(n) for n in cases.CHUNKLOOP_CASES]
    keys = [f"chunkstream.{n}.out" for n in cases.CHUNKSTREAM_CASES] + [f"chunkloop.{n}.out" for n in cases.CHUNKLOOP_CASES]
    waves, lens, first, last = (sum((r[i] for r in rows), []) for i in range(4))
    W = LB.padded_rows(waves, max(lens) + extra)
    per = [len(r[1]) for r in rows]
    row_of, lens_of = {}, {}
    for u, n in enumerate(per):
        for k in range(n):
            row_of[(u, k)] = len(row_of)
            lens_of[(u, k)] = lens[row_of[(u, k)]]
    order = list(row_of)
    random.Random(3).shuffle(order)
    per_file = LS.file_pieces(LS.splice(per, lens_of, order, OVW, keep_all=True), len(per))
    base = np.cumsum([0] + [sum(p.end - p.begin for p in ps) for ps in per_file])
    want = _assemble_gpu(W, lens, first, last, OVW)
    assert base[-1] == want.numel()
    got, _ = _emit_gpu(W, lens, LS.emit_args([p for ps in per_file for p in ps], row_of, base), OVW, int(base[-1]))
    assert torch.equal(torch.from_numpy(got), want)
    assert torch.equal(want, torch.cat([torch.from_numpy(golden[k].astype(np.float32).reshape(-1)) for k in keys]))


@pytest.mark.parametrize("pieces, message", [([(1, 0, 0, 40, 0)], b"shorter than the overlap"),             # prev_len 4 < ov
                                             ([(2, -1, 0, 32, 0), (3, 2, 0, 40, 28)], b"overlap in out"),
                                             ([(2, -1, 0, 32, 0), (3, 2, 0, 40, 40)], b"outside out"),
                                             ([(2, -1, 0, 44, 0)], b"range outside"),
                                             ([(4, -1, 0, 8, 0)], b"row outside")])
def test_emit_refusals_launch_nothing(pieces, message):
    lens = [4, 40, 40, 40]
    W = LB.padded_rows([np.ones(n, np.float32) for n in lens], 44)
    got, pcm = _emit_gpu(W, lens + [8], pieces, 8, 76, expect_error=message)
    assert (got == SENTINEL).all() and (pcm == PCM_SENTINEL).all()


# -------------------------------------------------------------------------------- convert_long_stream with the exact fakes
NAMES = list(cases.CHUNKLOOP_CASES)
SCHEDULES = [(None, 2, 64), (1, 2, 64), (1, 1, 1), (2, 3, 4)]


def _want(golden, name):
    return torch.from_numpy(golden[f"chunkloop.{name}.out"].astype(np.float32).reshape(-1))


def _fake_hotpath(ragged):
    from seedvc_amd.pipeline import HotPath
    return HotPath(LB.BatchedFakeCFM(DEV), LB.FakeVocoder(ragged))


def _stream_kw(ragged, schedule=(None, 2, 64), **kw):
    first_chunks, growth, max_chunks = schedule
    return dict(overlap_frame_len=cases.CHUNK_OVERLAP, ragged_vocoder=ragged, first_chunks=first_chunks, growth=growth,
                max_chunks=max_chunks, **kw)


def _stream(hp, utts, **kw):
    return hp.convert_long_stream(utts, 10, 0.7, cases.CHUNK_HOP, cases.CHUNK_WINDOW, **kw)


@pytest.fixture(scope="module")
def loop_utts():
    return TB._loop_utts(NAMES)


@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "grouped"])
@pytest.mark.parametrize("lookahead", [0, 1, 2])
@pytest.mark.parametrize("schedule", SCHEDULES, ids=lambda s: "ramp_%s_%s_%s" % s)
def test_stream_equals_the_references_own_loop(schedule, lookahead, ragged, loop_utts, golden):
    from seedvc_amd.pipeline import collect_stream, stream_schedule
    hp = _fake_hotpath(ragged)
    pieces = list(_stream(hp, loop_utts, **_stream_kw(ragged, schedule, lookahead=lookahead)))
    sizes = [b - a for a, b in stream_schedule([1, 1, 2, 2, 4, 5], *schedule)["micro_batches"]]
    assert hp.cfm.batch_sizes == sizes
    assert all(p.wave.dtype == torch.float32 and p.wave.device.type == "cpu" and p.wave.is_pinned() for p in pieces if p.wave.numel())
    outs = collect_stream(pieces, len(NAMES))
    pool = hp.convert_long_batch(loop_utts, 10, 0.7, cases.CHUNK_HOP, cases.CHUNK_WINDOW, overlap_frame_len=cases.CHUNK_OVERLAP,
                                 ragged_vocoder=ragged)
    for n, o, b in zip(NAMES, outs, pool):
        assert o.shape == b.shape and torch.equal(o[0], _want(golden, n)), n
        assert torch.equal(o, b.cpu()), n


def test_stream_with_an_empty_utterance_pcm_and_device_pieces(loop_utts, golden):
    from seedvc_amd.pipeline import collect_stream
    hp = _fake_hotpath(True)
    utts = [loop_utts[2], (loop_utts[0][0][:, :0],) + loop_utts[0][1:], loop_utts[5]]
    asked = []

    def noise(u, k, T):
        asked.append((u, k, T))
        return torch.zeros(1, cases.CHUNK_C, T, device=DEV)
    pieces = list(_stream(hp, utts, **_stream_kw(True, noise_fn=noise)))
    assert asked == [(0, 0, 60), (2, 0, 60), (0, 1, 37), (2, 1, 60), (2, 2, 60), (2, 3, 60), (2, 4, 37)]        # chunk-major, by file and chunk
    assert [(p.file, p.offset, p.wave.shape, p.final) for p in pieces if p.file == 1] == [(1, 0, (1, 0), True)]
    outs = collect_stream(pieces, 3)
    assert torch.equal(outs[0][0], _want(golden, "loop2")) and torch.equal(outs[2][0], _want(golden, "loop5")) and outs[1].shape == (1, 0)
    # int16 pieces are the model applied to the float pieces
    pcm = list(_stream(hp, utts, **_stream_kw(True, pcm16=True)))
    assert [(p.file, p.offset, p.final) for p in pcm] == [(p.file, p.offset, p.final) for p in pieces]
    for a, b in zip(pcm, pieces):
        assert a.wave.dtype == torch.int16 and a.wave.shape == b.wave.shape
        assert np.array_equal(a.wave.numpy(), LS.pcm_model(b.wave.numpy()))
    assert any((a.wave.abs() > 300).any() for a in pcm)
    # device pieces hold the same values
    dev = list(_stream(hp, utts, **_stream_kw(True, to_host=False)))
    assert all(p.wave.device.type == "cuda" for p in dev)
    torch.cuda.synchronize()
    for a, b in zip(dev, pieces):
        assert (a.file, a.offset, a.final) == (b.file, b.offset, b.final) and torch.equal(a.wave.cpu(), b.wave)


def test_stream_argument_errors_come_at_the_first_next(loop_utts):
    hp = _fake_hotpath(True)
    for bad in (dict(seeds=[1] * 6, noise_fn=lambda u, k, T: None), dict(max_chunks=0), dict(first_chunks=0), dict(growth=0.5),
                dict(lookahead=-1), dict(seeds=[1, 2])):
        kw = _stream_kw(True)
        kw.update(bad)
        gen = _stream(hp, loop_utts, **kw)             # making the generator raises nothing
        with pytest.raises(ValueError):
            next(gen)
    assert hp.cfm.batch_sizes == []


# ---------------------------------------------------------------------------------------------------------- laziness
@pytest.mark.parametrize("lookahead", [0, 1, 2])
def test_stream_enqueues_no_more_than_it_is_asked_for(lookahead, loop_utts, golden):
    from seedvc_amd.pipeline import stream_schedule
    hp = _fake_hotpath(True)
    gen = _stream(hp, loop_utts, **_stream_kw(True, lookahead=lookahead))
    assert hp.cfm.batch_sizes == []
    first = next(gen)
    sizes = [b - a for a, b in stream_schedule([1, 1, 2, 2, 4, 5])["micro_batches"]]
    assert sizes == [6, 9]
    assert first.offset == 0 and len(hp.cfm.batch_sizes) <= 1 + lookahead and hp.cfm.batch_sizes == sizes[:1 + lookahead]
    rest = list(gen)
    assert hp.cfm.batch_sizes == sizes and len([p for p in [first] + rest if p.final]) == 6


def test_a_stream_closed_early_leaves_the_hot_path_usable(loop_utts, golden):
    hp = _fake_hotpath(True)
    for p in _stream(hp, loop_utts, **_stream_kw(True, (1, 1, 1))):
        break
    assert len(hp.cfm.batch_sizes) == 2                # lookahead 1: nothing further was enqueued
    gen = _stream(hp, loop_utts, **_stream_kw(True))
    next(gen)
    gen.close()
    pool = hp.convert_long_batch(loop_utts, 10, 0.7, cases.CHUNK_HOP, cases.CHUNK_WINDOW, overlap_frame_len=cases.CHUNK_OVERLAP)
    for n, o in zip(NAMES, pool):
        assert torch.equal(o[0].cpu(), _want(golden, n))


# -------------------------------------------------------------------------------------------------------- real models
def _real_stream(specs, **kw):
    from seedvc_amd.pipeline import HotPath, collect_stream
    m = TB._models()
    cfg = m["cfg"]
    hp = HotPath(m["cfm"], m["voc"])
    utts = [tuple(t.to(DEV) for t in TB._utt(cfg, S, P)) for S, P in specs]
    if "seeds" not in kw:
        kw["noise_fn"] = lambda u, k, T: TB._noise(cfg, T).to(DEV)
    outs = collect_stream(hp.convert_long_stream(utts, TB.STEPS, 0.7, TB.HOP, TB.WINDOW, overlap_frame_len=TB.OVERLAP, **kw), len(specs))
    return hp, utts, outs


def test_real_models_three_utterances_in_one_stream():
    """Each within waveform RMS 5e-3 of `O.chunked_convert`: the bound test_gpu_long_batch.py applies to the pool and to the
    sequential loop on these models and sizes."""
    specs = [(70, 16), (24, 16), (45, 11)]
    _, _, outs = _real_stream(specs)
    for (S_total, P), out in zip(specs, outs):
        ref = TB._oracle(S_total, P)
        assert out.shape == ref.shape
        rms = TB._rms(out, ref)
        print(f"S_total {S_total}, P {P}: streamed (3 utterances) vs oracle RMS {rms:.3e} (< 5e-3)")
        assert rms < 5e-3


def test_real_models_one_file_with_the_pools_partition_equals_the_pool():
    m = TB._models()
    hp, utts, outs = _real_stream([(70, 16)], first_chunks=64, growth=1)
    pool = hp.convert_long_batch(utts, TB.STEPS, 0.7, TB.HOP, TB.WINDOW, overlap_frame_len=TB.OVERLAP,
                                 noise_fn=lambda T: TB._noise(m["cfg"], T).to(DEV))
    assert torch.equal(outs[0], pool[0].cpu())
    assert TB._rms(outs[0], TB._oracle(70, 16)) < 5e-3


def test_real_models_a_seeded_file_does_not_depend_on_its_company():
    """With seeds a file's draws are its own (`derive_seed(seeds[u], k)`), so the file streamed alone and with two others
    differs only by the DiT's kernel forms: inside the 5e-3 that bounds either path against its oracle."""
    specs = [(70, 16), (24, 16), (45, 11)]
    _, _, together = _real_stream(specs, seeds=[31, 32, 33])
    for i, spec in enumerate(specs):
        _, _, alone = _real_stream([spec], seeds=[31 + i])
        assert alone[0].shape == together[i].shape and torch.isfinite(alone[0]).all()
        rms = TB._rms(alone[0], together[i])
        print(f"S_total {spec[0]}: seeded, alone vs in a stream of three RMS {rms:.3e} (< 5e-3), identical {torch.equal(alone[0], together[i])}")
        assert rms < 5e-3
    _, _, other = _real_stream([specs[0]], seeds=[99])
    assert not torch.equal(other[0], together[0])           # the seed does matter


# ----------------------------------------------------------------------------------------------------------------- v2
def _v2_stream(fs, **kw):
    args = dict(max_context_window=TV.WINDOW, hop=L.HOP, max_new=A.MAX_NEW)
    args.update(kw)
    return list(TV._hotpath().convert_long_stream([TV._record(f) for f in fs], L.N_STEPS, L.CFG_RATES, **args))


def test_v2_style_branch_streams_what_the_pool_assembles():
    from seedvc_amd.pipeline import collect_stream
    fs, seeds, ov = [0, 1, 2], [11, 2 ** 63 + 12, 13], 2
    assert all(f in L.qualified() for f in fs)
    kw = dict(ar_chunk_tokens=9, overlap_frame_len=ov, max_chunks=3, seeds=seeds)
    pieces = _v2_stream(fs, return_parts=True, **kw)
    _, pool_parts = TV._convert(fs, **kw)
    parts = [{} for _ in fs]
    for p in pieces:
        for d in p.parts or ():
            assert d["chunk"] not in parts[d["file"]]
            parts[d["file"]][d["chunk"]] = d
    assert [len(p) for p in parts] == [len(p) for p in pool_parts] == [3, 3, 4]
    for u, (mine, theirs) in enumerate(zip(parts, pool_parts)):
        for j, b in enumerate(theirs):
            a = mine[j]
            assert torch.equal(a["tokens"], b["tokens"]), f"file {u}, chunk {j}"
            assert a["ylen"] == b["ylen"] and a["kept"] == b["kept"] and a["mel"].shape == b["mel"].shape
            e_mel = (a["mel"] - b["mel"]).abs().mean().item()
            print(f"file {u}, chunk {j}: stream vs pool mel mean abs err {e_mel:.3e} (< 1e-3), identical {torch.equal(a['mel'], b['mel'])}")
            assert e_mel < 1e-3
    outs = collect_stream(pieces, len(fs))
    for u, out in enumerate(outs):
        want = TV._stream([parts[u][j] for j in sorted(parts[u])], ov)
        assert out.shape == (1, want.numel()) and want.numel() > 0 and torch.equal(out[0], want), u
    # without return_parts no piece carries parts, and the audio is the same call's audio
    plain = _v2_stream(fs, **kw)
    assert all(p.parts is None for p in plain)
    for a, b in zip(collect_stream(plain, len(fs)), outs):
        assert torch.equal(a, b)


def test_v2_short_chunks_give_one_final_piece():
    f, ov = 4, 16
    assert f in L.qualified()
    pieces = _v2_stream([f], ar_chunk_tokens=L.FILES[f][3], overlap_frame_len=ov, return_parts=True, **TV._pinned([f]))
    parts = sorted((d for p in pieces for d in p.parts or ()), key=lambda d: d["chunk"])
    assert [d["kept"] for d in parts] == [False] * (len(parts) - 1) + [True] and len(parts) == len(L.file_case(f)["chunks"])
    assert len(pieces) == 1 and pieces[0].final and pieces[0].offset == 0
    assert torch.equal(pieces[0].wave, parts[-1]["wave"].cpu())


def test_v2_timbre_branch_is_the_v1_stream():
    from seedvc_amd.pipeline import HotPath, collect_stream
    hp = TV._hotpath()
    fa, fb = L.qualified()[:2]
    ov, seeds = 2, [21, 22]
    recs = [dict(TV._record(fa), source_frames=30), dict(TV._record(fb), source_frames=9)]
    window = recs[0]["target"]["P"] + 12
    got = collect_stream(hp.convert_long_stream(recs, L.N_STEPS, L.CFG_RATES, convert_style=False, max_context_window=window, hop=L.HOP,
                                                overlap_frame_len=ov, seeds=seeds), 2)
    nw = [r["src_tokens"].size(1) for r in recs]
    tok = torch.zeros(2, max(nw), dtype=torch.int64, device=DEV)
    for i, r in enumerate(recs):
        tok[i, :nw[i]] = r["src_tokens"][0]
    cond = hp.cfm_lr(tok, ylens=torch.LongTensor([30, 9]), in_lens=nw)[0]
    utts = [(cond[i:i + 1, :n], r["target"]["prompt_condition"], r["target"]["mel"], r["target"]["style"])
            for i, (r, n) in enumerate(zip(recs, [30, 9]))]
    want = collect_stream(HotPath(hp.cfm, hp.vocoder).convert_long_stream(utts, L.N_STEPS, list(L.CFG_RATES), L.HOP, window,
                                                                          overlap_frame_len=ov, seeds=seeds, ragged_vocoder=True), 2)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.shape[1] > 0 and torch.isfinite(g).all() and torch.equal(g, w)
