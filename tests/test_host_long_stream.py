"""CPU side of long-form streaming (`svc_chunks_emit`, `pipeline.stream_schedule`, `pipeline._StreamSplicer`,
`pipeline.collect_stream`, `convert_long_stream`): the entry point is declared, exported and bound and refuses bad arguments
before anything touches a device; the schedule's order and ramp; the splicer against `long_batch_plan` and `v2_seam_plan`
over several completion orders; and the numpy model the GPU tests compare with, pinned to the assemble and seam models."""
import collections
import ctypes
import inspect
import os
import random
import re

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB
import long_stream_cases as LS
import v2_long_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)      # noqa: E731
ONE = ctypes.c_void_p(16)                           # never dereferenced: the checks come first
OVW = cases.CHUNK_OVERLAP * cases.CHUNK_HOP


def test_emit_is_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    assert "svc_chunks_emit" in set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    assert "svc_chunks_emit" in _lib.EXPORTS and hasattr(lib, "svc_chunks_emit")
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    for cls in (pipeline.HotPath, pipeline.V2HotPath):
        p = inspect.signature(cls.convert_long_stream).parameters
        assert inspect.isgeneratorfunction(inspect.unwrap(cls.convert_long_stream))
        assert (p["max_chunks"].default, p["pcm16"].default, p["to_host"].default, p["lookahead"].default) == (64, False, True, 1)
        q = inspect.signature(pipeline.stream_schedule).parameters
        assert (p["first_chunks"].default, p["growth"].default) == (q["first_chunks"].default, q["growth"].default)
    assert pipeline.StreamPiece._fields[:4] == ("file", "offset", "wave", "final")


# -------------------------------------------------------------------------------------- svc_chunks_emit: argument refusals
def _emit(row=(0, 1), length=(40, 40), prev_row=(-1, 0), prev_len=(0, 40), begin=(0, 0), end=(32, 40), out_off=(0, 32), ov=8,
          out_len=72, stride=48, n_rows=2, pcm=None):
    from seedvc_amd import _lib
    return _lib.lib().svc_chunks_emit(ONE, stride, n_rows, i32(*row), i32(*length), i32(*prev_row), i32(*prev_len), i32(*begin),
                                      i32(*end), i64(*out_off), len(row), ONE, ONE, ov, ONE, pcm, out_len, None)


@pytest.mark.parametrize("bad", [dict(row=(0, 2)), dict(row=(-1, 1)), dict(prev_row=(-1, 2)), dict(length=(40, 49)), dict(length=(40, -1)),
                                 dict(begin=(-4, 0)), dict(begin=(36, 0)), dict(end=(32, 44)), dict(prev_len=(0, 7)), dict(prev_len=(0, 49)),
                                 dict(out_off=(0, 28)), dict(out_off=(32, 0)), dict(out_len=68), dict(out_off=(-4, 32)), dict(ov=-1),
                                 dict(stride=-1), dict(n_rows=-1)],
                         ids=["row_above", "row_negative", "prev_row_above", "len_above_stride", "len_negative", "begin_negative",
                              "begin_above_end", "end_above_len", "prev_shorter_than_ov", "prev_len_above_stride", "overlap_by_4",
                              "overlap_reversed_order", "past_out_len", "out_off_negative", "ov_negative", "stride_negative",
                              "n_rows_negative"])
def test_emit_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _emit(**bad) != 0
    assert b"chunks_emit" in _lib.lib().svc_last_error()


def test_emit_of_nothing_is_not_an_error():
    from seedvc_amd import _lib
    lib = _lib.lib()
    assert lib.svc_chunks_emit(None, 0, 0, None, None, None, None, None, None, None, 0, None, None, 8, None, None, 0, None) == 0
    # pieces without samples need no buffers either
    assert _emit(row=(0,), length=(0,), prev_row=(-1,), prev_len=(0,), begin=(0,), end=(0,), out_off=(0,), out_len=0) == 0
    assert lib.svc_chunks_emit(None, 8, 1, None, None, None, None, None, None, None, 1, None, None, 8, None, None, 0, None) != 0


# ------------------------------------------------------------------------------------------------------ stream_schedule
def test_schedule_order_and_ramp():
    from seedvc_amd.pipeline import stream_schedule
    order = [(0, 0), (2, 0), (3, 0), (0, 1), (3, 1), (0, 2), (3, 2), (3, 3)]
    s = stream_schedule([3, 0, 1, 4])
    assert s["order"] == order and s["micro_batches"] == [(0, 3), (3, 8)]           # one chunk per file with chunks, then twice that
    s = stream_schedule([3, 0, 1, 4], first_chunks=1, growth=2, max_chunks=3)
    assert s["order"] == order and s["micro_batches"] == [(0, 1), (1, 3), (3, 6), (6, 8)]
    assert stream_schedule([3, 0, 1, 4], growth=1)["micro_batches"] == [(0, 3), (3, 6), (6, 8)]
    assert stream_schedule([3, 0, 1, 4], max_chunks=2)["micro_batches"] == [(0, 2), (2, 4), (4, 6), (6, 8)]      # the default is capped
    assert stream_schedule([], growth=1) == dict(order=[], micro_batches=[]) == stream_schedule([0, 0])
    assert stream_schedule([40], first_chunks=1, growth=1.5)["micro_batches"][:5] == [(0, 1), (1, 3), (3, 6), (6, 10), (10, 16)]


def test_schedule_of_one_file_can_equal_the_pools_partition():
    from seedvc_amd.pipeline import long_batch_plan, stream_schedule
    for n_src, max_chunks in ((113, 2), (113, 64), (1000, 7)):
        plan = long_batch_plan([n_src], [cases.CHUNK_P], cases.CHUNK_WINDOW, cases.CHUNK_OVERLAP, cases.CHUNK_HOP, max_chunks)
        s = stream_schedule([len(plan["chunks"])], first_chunks=max_chunks, growth=1, max_chunks=max_chunks)
        assert s["micro_batches"] == plan["micro_batches"] and s["order"] == [(0, k) for k in range(len(plan["chunks"]))]


@pytest.mark.parametrize("bad", [dict(first_chunks=0), dict(growth=0.5), dict(max_chunks=0)])
def test_schedule_argument_errors(bad):
    from seedvc_amd.pipeline import stream_schedule
    with pytest.raises(ValueError):
        stream_schedule([3, 1], **bad)


# ------------------------------------------------------------------------------- the splicer against `long_batch_plan`
def _loop_plan():
    from seedvc_amd.pipeline import long_batch_plan
    n_src = [v[0] for v in cases.CHUNKLOOP_CASES.values()]
    plan = long_batch_plan(n_src, [cases.CHUNK_P] * len(n_src), cases.CHUNK_WINDOW, cases.CHUNK_OVERLAP, cases.CHUNK_HOP)
    per = collections.Counter(c[0] for c in plan["chunks"])
    counts = [per[u] for u in range(len(n_src))]
    lens_of, row_of, at = {}, {}, collections.Counter()
    for row, c in enumerate(plan["chunks"]):
        lens_of[(c[0], at[c[0]])], row_of[(c[0], at[c[0]])] = c[2] * cases.CHUNK_HOP, row
        at[c[0]] += 1
    return plan, counts, lens_of, row_of


def _orders(keys):
    major = sorted(keys, key=lambda uk: (uk[1], uk[0]))
    shuffled = list(major)
    random.Random(7).shuffle(shuffled)
    return dict(chunk_major=major, reverse=major[::-1], shuffled=shuffled)


@pytest.mark.parametrize("order", ["chunk_major", "reverse", "shuffled"])
def test_splicer_tiles_every_file_of_a_v1_plan(order):
    plan, counts, lens_of, row_of = _loop_plan()
    assert len(plan["chunks"]) == 15 and len(counts) == 6
    pieces = LS.splice(counts, lens_of, _orders(lens_of)[order], OVW, keep_all=True)
    per = LS.file_pieces(pieces, 6)
    for u, ps in enumerate(per):
        assert sum(p.end - p.begin for p in ps) == plan["out_lens"][u]
        assert [p.chunk for p in ps] == list(range(counts[u]))                              # every chunk kept, in order, one piece each
        assert all(p.prev_chunk == p.chunk - 1 and (p.prev_chunk < 0 or p.prev_len == lens_of[(u, p.prev_chunk)]) for p in ps)
    if order == "chunk_major":          # nothing waits: a chunk's piece is released by its own completion
        assert [(p.file, p.chunk) for p in pieces] == _orders(lens_of)[order]


@pytest.mark.parametrize("order", ["chunk_major", "reverse", "shuffled"])
def test_emit_model_over_any_order_equals_the_assemble_model(order, golden):
    plan, counts, lens_of, row_of = _loop_plan()
    rows = [LB.chunkloop_rows(n) for n in cases.CHUNKLOOP_CASES]
    waves, lens, first, last = (sum((r[i] for r in rows), []) for i in range(4))
    W = LB.padded_rows(waves, max(lens) + 3)
    base = np.cumsum([0] + plan["out_lens"])
    pieces = LS.splice(counts, lens_of, _orders(lens_of)[order], OVW, keep_all=True)
    got = LS.emit_model(W, lens, LS.emit_args(pieces, row_of, base), OVW, out_len=int(base[-1]))
    assert np.array_equal(got, LB.assemble_model(W, lens, first, last, OVW))
    want = np.concatenate([golden[f"chunkloop.{n}.out"].astype(np.float32).reshape(-1) for n in cases.CHUNKLOOP_CASES])
    assert np.array_equal(got, want)                                                        # the reference's own loop


@pytest.mark.parametrize("name", list(cases.CHUNKSTREAM_CASES))
def test_v1_plans_keep_chunks_shorter_than_two_overlaps(name, golden):
    """The `chunkstream` cases drive the reference's state machine with chunks below 2 ov ("even": every chunk) and a last chunk
    below ov: a v1 plan keeps them all, and the pieces give the reference's output."""
    waves, lens, first, last = LB.chunkstream_rows(name)
    n = len(lens)
    keys = {(0, k): lens[k] for k in range(n)}
    W = LB.padded_rows(waves, max(lens) + 3)
    want = golden[f"chunkstream.{name}.out"].astype(np.float32).reshape(-1)
    for order in _orders(keys).values():
        pieces = LS.splice([n], keys, order, OVW, keep_all=True)
        (ps,) = LS.file_pieces(pieces, 1)
        assert [p.chunk for p in ps if p.end > p.begin] == [k for k in range(n) if lens[k] > (0 if last[k] else OVW)]
        got = LS.emit_model(W, lens, LS.emit_args(pieces, {(0, k): k for k in range(n)}, [0]), OVW, out_len=len(want))
        assert np.array_equal(got, want)
    if name == "even":          # every chunk is below 2 ov: the style branch's rule would keep the last one only
        assert all(x < 2 * OVW for x in lens)
        assert [p.chunk for p in LS.splice([n], keys, sorted(keys), OVW)] == [n - 1]


# --------------------------------------------------------------------------------- the splicer against `v2_seam_plan`
def _style_case(name):
    lens = LS.STYLE_PLANS[name]
    rng = np.random.default_rng(len(name))
    return lens, [rng.standard_normal(n).astype(np.float32) for n in lens]


@pytest.mark.parametrize("name", list(LS.STYLE_PLANS))
def test_splicer_and_emit_model_equal_the_seam_model(name):
    lens, waves = _style_case(name)
    n, ov = len(lens), LS.STYLE_OV
    want, plan = L.seam_model(waves, [0] * n, [k == n - 1 for k in range(n)], ov, 1)
    keys = {(0, k): lens[k] for k in range(n)}
    W = LB.padded_rows(waves, max(lens, default=0) + 3)
    for order in _orders(keys).values():
        pieces = LS.splice([n], keys, order, ov)
        (ps,) = LS.file_pieces(pieces, 1)
        assert sum(p.end - p.begin for p in ps) == plan["out_lens"][0]
        assert {p.chunk for p in ps if p.chunk >= 0} == {k for k in range(n) if plan["kept"][k]}
        got = LS.emit_model(W, lens, LS.emit_args(pieces, {(0, k): k for k in range(n)}, [0]), ov, out_len=plan["out_lens"][0])
        assert np.array_equal(got, want[0])


def test_splicer_pieces_of_the_named_plans():
    """What each synthetic plan is there for, spelled out: (chunk, prev_chunk, begin, end, final) per piece."""
    def pieces(name):
        lens = LS.STYLE_PLANS[name]
        keys = {(0, k): n for k, n in enumerate(lens)}
        return [(p.chunk, p.prev_chunk, p.begin, p.end, p.final) for p in LS.splice([len(lens)], keys, sorted(keys), LS.STYLE_OV)]
    assert pieces("all_kept") == [(0, -1, 0, 32, False), (1, 0, 0, 32, False), (2, 1, 0, 24, True)]
    assert pieces("middle_dropped") == [(0, -1, 0, 32, False), (2, 0, 0, 40, True)]
    assert pieces("last_empty") == [(0, -1, 0, 32, False), (1, 0, 0, 32, False), (1, 0, 32, 40, True)]
    assert pieces("only_last_kept") == [(2, -1, 0, 5, True)]
    assert pieces("one_empty_chunk") == pieces("no_chunks") == [(-1, -1, 0, 0, True)]
    assert pieces("last_shorter_than_ov") == [(0, -1, 0, 32, False), (1, 0, 0, 5, True)]


def test_splicer_holds_a_piece_until_its_predecessors_are_complete():
    from seedvc_amd.pipeline import _StreamSplicer
    sp = _StreamSplicer(2, [3, 0], 8)
    assert [(p.file, p.final, p.end) for p in sp.start()] == [(1, True, 0)]
    assert sp.complete(0, 2, 24, True) == [] and sp.complete(0, 1, 40, False) == []
    assert [(p.chunk, p.offset) for p in sp.complete(0, 0, 40, False)] == [(0, 0), (1, 32), (2, 64)]
    with pytest.raises(ValueError):
        sp.complete(0, 1, 40, False)            # twice
    with pytest.raises(ValueError):
        _StreamSplicer(1, [2], 8).complete(0, 0, 40, True)          # the plan's last chunk is the file's last


def test_pcm_model_truncates_and_saturates():
    x = np.array([0.0, 1.0, -1.0, 1.2, -1.2, 0.5, -0.5, 32767.9 / 32768, -32767.9 / 32768, 1e-6, -1e-6], np.float32)
    assert LS.pcm_model(x).tolist() == [0, 32767, -32768, 32767, -32768, 16384, -16384, 32767, -32767, 0, 0]
    inside = np.linspace(-0.999, 0.999, 1001).astype(np.float32)
    assert np.array_equal(LS.pcm_model(inside), (inside * 32768.0).astype(np.int16))        # the reference's line where it does not wrap


# -------------------------------------------------------------------------------------------------------- collect_stream
def test_collect_stream_checks_its_pieces():
    from seedvc_amd.pipeline import StreamPiece, collect_stream
    w = lambda n: torch.arange(n, dtype=torch.float32)[None, :]       # noqa: E731
    good = [StreamPiece(0, 0, w(3), False), StreamPiece(1, 0, w(0), True), StreamPiece(0, 3, w(2), True)]
    out = collect_stream(good, 2)
    assert out[0].tolist() == [[0, 1, 2, 0, 1]] and out[1].shape == (1, 0)
    for bad in ([StreamPiece(0, 0, w(3), False), StreamPiece(0, 4, w(2), True), good[1]],            # a gap
                [StreamPiece(0, 0, w(3), False), StreamPiece(0, 2, w(2), True), good[1]],            # an overlap
                [StreamPiece(0, 0, w(3), False), StreamPiece(0, 3, w(2), False), good[1]],           # no final
                good + [StreamPiece(0, 5, w(0), True)],                                              # a second final
                good[:1] + good[2:],                                                                 # a file without pieces
                [StreamPiece(0, 1, w(3), True), good[1]]):                                           # does not start at 0
        with pytest.raises(ValueError):
            collect_stream(bad, 2)
