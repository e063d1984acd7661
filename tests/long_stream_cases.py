"""Yardsticks of the long-form streaming tests (test_host_long_stream.py, test_gpu_long_stream.py).

`emit_model` is the numpy statement of `svc_chunks_emit`'s formula in include/seedvc_hip.h, float64 products and sum rounded
separately like `long_batch_cases.assemble_model`; the host test pins it to that model (and so to the reference-generated
fixtures of tests/golden/chunkloop.npz) and to `v2_long_cases.seam_model`.  `pcm_model` is the reference streaming leg's
`(wave * 32768.0).astype(np.int16)` with the one documented deviation, saturation instead of numpy's wrap.  `splice` drives
`pipeline._StreamSplicer` over a completion order and returns its pieces; `emit_args` turns pieces into the arrays of the
call."""
import numpy as np

import long_batch_cases as LB

STYLE_OV = 8
# synthetic chunk lengths of one file under the style branch's seam rule, ov = 8 (what each exercises: the issue's list)
STYLE_PLANS = {
    "all_kept": [40, 40, 24],
    "middle_dropped": [40, 10, 40],          # the seam joins chunks 0 and 2
    "last_empty": [40, 40, 0],               # chunk 1's tail is flushed as a raw final piece
    "only_last_kept": [10, 12, 5],           # emitted whole
    "one_empty_chunk": [0],
    "no_chunks": [],
    "last_shorter_than_ov": [40, 5],
}


def emit_model(waves, lens, pieces, ov, out=None, out_len=None):
    """waves (n_rows, stride) float32, anything past lens; pieces: [(row, prev_row, begin, end, out_off)] (prev_len = lens[prev_row])
    -> out, float32; samples no piece covers keep what `out` held (zeros for a fresh one)."""
    fi, fo = LB.fades(ov)
    if out is None:
        out = np.zeros(out_len if out_len is not None else max((o + e - b for _, _, b, e, o in pieces), default=0), np.float32)
    for row, prev_row, begin, end, off in pieces:
        i = np.arange(begin, end)
        v = waves[row, begin:end].astype(np.float64)
        if prev_row >= 0:
            s = i < ov
            tail = waves[prev_row, lens[prev_row] - ov + i[s]].astype(np.float64)
            v[s] = v[s] * fi[i[s]] + tail * fo[i[s]]
        out[off:off + end - begin] = v.astype(np.float32)
    return out


def pcm_model(x):
    """float32 -> int16: the exactly scaled float truncated toward zero, saturated to [-32768, 32767] (numpy would wrap +1.0)."""
    y = np.asarray(x, np.float32) * np.float32(32768.0)
    return np.clip(np.trunc(y), -32768, 32767).astype(np.int16)


def splice(chunks_per_file, lens_of, order, ov, keep_all=False):
    """Run `_StreamSplicer` over `order` [(file, chunk)]; lens_of[(file, chunk)] samples -> the released pieces, in release order
    (the empty pieces of files without chunks first).  keep_all: a v1 plan (every chunk kept), else the style branch's rule."""
    from seedvc_amd.pipeline import _StreamSplicer
    sp = _StreamSplicer(len(chunks_per_file), chunks_per_file, ov, keep_all)
    pieces = list(sp.start())
    for u, k in order:
        pieces += sp.complete(u, k, lens_of[(u, k)], k == chunks_per_file[u] - 1)
    return pieces


def file_pieces(pieces, n_files):
    """-> per file its pieces; asserts that they tile [0, total) in order and that exactly the last one is final."""
    per = [[p for p in pieces if p.file == u] for u in range(n_files)]
    for u, ps in enumerate(per):
        assert ps, f"file {u} has no piece"
        at = 0
        for p in ps:
            assert p.offset == at and 0 <= p.begin <= p.end <= p.len
            at += p.end - p.begin
        assert [p.final for p in ps] == [False] * (len(ps) - 1) + [True], u
    return per


def emit_args(pieces, row_of, file_base):
    """pieces -> [(row, prev_row, begin, end, out_off)] of `emit_model` with out_off = file_base[file] + offset; empty pieces
    (chunk -1) are left out."""
    return [(row_of[(p.file, p.chunk)], row_of[(p.file, p.prev_chunk)] if p.prev_chunk >= 0 else -1, p.begin, p.end,
             file_base[p.file] + p.offset) for p in pieces if p.chunk >= 0]
