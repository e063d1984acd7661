"""GPU tests of the device resampler (`svc_resample`, `audio.Resample`, `pipeline.to_16k` / `enrol_references_audio`) against
the dense float64 statement of torchaudio's operator (resample_cases.py).  The per-output bound is derived, not measured: the
textbook error of an fp32 dot product of ntaps terms, computed in float64 beside the yardstick."""
import ctypes as C

import pytest
import torch

import cases
import frontend_ragged_cases as R
import resample_cases as RC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
_handles = {}


def rs(pair):
    from seedvc_amd.audio import Resample
    if pair not in _handles:
        _handles[pair] = Resample(*pair, device=DEV)
    return _handles[pair]


def geometry(pair):
    """(o, n, width, ntaps) of a pair: the table's if it has the pair, else from the dense kernel."""
    if pair in RC.TABLE:
        return RC.TABLE[pair]
    o, n, width, K = RC.dense_kernel(*pair)
    return o, n, width, int((K != 0).sum(dim=1).max())


def long_len(r, extra=0):
    """An input length whose output is more than three workgroup tiles (+ extra tiles) plus an odd remainder."""
    want = (3 + extra) * r.tile + 37
    L = want * r.o // r.n + 1
    while r.out_len(L) < want or (r.out_len(L) - (3 + extra) * r.tile) % 2 == 0:
        L += 1
    return L


@pytest.mark.parametrize("pair", RC.GPU_PAIRS)
def test_parity_with_the_dense_statement(pair):
    r = rs(pair)
    o, n, width, ntaps = geometry(pair)
    assert (r.o, r.n) == (o, n) and r.tile > 0 and r.tile % n == 0
    worst = 0.0
    for L in (1, 5, o - 1, o, o + 1, 3 * o + 7, long_len(r)):
        x = RC.noise("parity", L, 2, L)
        got = r(x.to(DEV)).cpu()
        want = RC.resample_dense(*pair, x)
        bound = RC.fp32_bound(*pair, x, ntaps)
        assert got.shape == want.shape == (2, r.out_len(L)) and torch.isfinite(got).all()
        err = (got.double() - want).abs()
        ratio = (err / bound.clamp_min(1e-300)).max().item()
        worst = max(worst, ratio)
        print(f"{pair[0]} -> {pair[1]}: L {L} ({got.size(1)} outputs, tile {r.tile}): max |error| {err.max().item():.3e}, "
              f"largest error / bound {ratio:.3f}")
        assert (err <= bound).all()
    print(f"{pair[0]} -> {pair[1]}: largest error / bound over all lengths {worst:.3f}")


@pytest.mark.parametrize("pair", RC.GPU_PAIRS)
def test_prefix_property(pair):
    """Outputs whose taps lie wholly inside the shorter signal do not change when samples are appended: tile edges, the span staging
    and the phase arithmetic leave no trace in the bits."""
    from seedvc_amd.audio import sinc_resample_taps
    r = rs(pair)
    o, n, width, first, taps = sinc_resample_taps(*pair)
    L1, L2 = long_len(r), long_len(r, extra=1) + 2
    assert r.out_len(L1) > 3 * r.tile and L2 > L1
    x = RC.noise("prefix", 1, 1, L2)
    y1, y2 = r(x[:, :L1].to(DEV)).cpu(), r(x.to(DEV)).cpu()
    m = torch.arange(y1.size(1))
    last_sample = (m // n) * o + first.long()[m % n] + taps.size(1) - 1 - width
    inside = last_sample < L1
    assert int(inside.sum()) > 3 * r.tile - 64 and not bool(inside.all())
    assert torch.equal(y1[0, inside], y2[0, :y1.size(1)][inside])
    assert not torch.equal(y1[0, ~inside], y2[0, :y1.size(1)][~inside])          # and the signal's end does show in the others


@pytest.mark.parametrize("pair", RC.GPU_PAIRS)
def test_ragged_rows_equal_the_clip_alone(pair):
    r = rs(pair)
    L = long_len(r)
    lens = (L, 1, r.o + 1, L // 2 + 3)
    x = RC.noise("ragged", 2, 4, L)
    y = RC.ragged_batch(x, lens)                                                 # NaN above every clip's end
    out, out_lens = r(y.to(DEV), lens=lens)
    out = out.cpu()
    assert out.shape == (4, r.out_len(L)) and out_lens == [r.out_len(v) for v in lens]
    assert torch.isfinite(out).all()
    for b, v in enumerate(lens):
        alone = r(x[b:b + 1, :v].to(DEV)).cpu()
        assert torch.equal(out[b:b + 1, :out_lens[b]], alone)
        assert (out[b, out_lens[b]:] == 0).all()
    plain = r(x.to(DEV))
    same, same_lens = r(x.to(DEV), lens=(L,) * 4)
    assert torch.equal(plain, same) and same_lens == [r.out_len(L)] * 4
    assert r(x[0].to(DEV)).shape == (1, r.out_len(L)) and torch.equal(r(x[0].to(DEV)), plain[0:1])      # (L,) is a batch of one


def test_two_calls_and_two_handles():
    a, b = rs((22050, 16000)), rs((44100, 16000))
    L = long_len(a)
    x = RC.noise("det", 3, 2, L).to(DEV)
    y0 = a(x)
    other = b(x)
    y1 = a(x)
    assert torch.equal(y0, y1) and torch.equal(other, b(x))
    assert other.shape == (2, b.out_len(L)) and other.shape != y0.shape


def test_argument_errors_reach_no_device():
    from seedvc_amd import _lib
    r = rs((22050, 16000))
    lib, err = _lib.lib(), _lib.lib().svc_last_error
    B, L = 2, 900
    Lout = r.out_len(L)
    x = RC.noise("err", 4, B, L).to(DEV)
    buf = torch.full((B * Lout + 8,), 3.0, device=DEV)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)      # noqa: E731
    xp, op, st = _lib.ptr(x), _lib.ptr(buf), _lib.stream_ptr()

    def bad(rc, word):
        assert rc != 0 and word in err(), err()
        torch.cuda.synchronize()
        assert (buf == 3.0).all()

    call = lib.svc_resample
    bad(call(r._h, xp, i32(L, 0), B, L, op, Lout, st), b"lens")
    bad(call(r._h, xp, i32(L + 1, L), B, L, op, Lout, st), b"lens")
    bad(call(r._h, xp, None, 0, L, op, Lout, st), b"B outside")
    bad(call(r._h, xp, None, 65, L, op, Lout, st), b"B outside")
    bad(call(r._h, xp, None, B, L, op, Lout - 1, st), b"Lout")
    bad(call(r._h, xp, i32(L, L - 5), B, L, op, Lout - 1, st), b"Lout")            # the longest clip decides
    bad(call(r._h, None, None, B, L, op, Lout, st), b"x is NULL")
    bad(call(r._h, xp, None, B, L, None, Lout, st), b"out is NULL")
    inside = C.c_void_p(x.data_ptr() + 4 * (B * L - 1))                           # out begins at x's last sample
    bad(call(r._h, xp, None, B, L, inside, Lout, st), b"overlap")
    before = C.c_void_p(buf.data_ptr() + 4 * (B * Lout - 1))                      # x begins at out's last sample
    bad(call(r._h, before, None, B, L, op, Lout, st), b"overlap")
    # and the same arguments without the fault are fine
    assert call(r._h, xp, i32(L, L - 5), B, L, op, Lout, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:Lout], r(x[0:1])[0]) and (buf[B * Lout:] == 3.0).all()
    with pytest.raises(ValueError, match="lens"):
        r(x, lens=[L])


def test_wiring_to_16k_and_enrolment():
    from seedvc_amd.audio import MelSpectrogram, Resample
    from seedvc_amd.campplus import CAMPPlus
    from seedvc_amd.pipeline import enrol_references, enrol_references_audio, to_16k
    c, sd, _ = cases.campplus_case(R.CP_MODEL)
    cp = CAMPPlus(c, sd, DEV)
    cm, y, basis, lens = R.mel_batch("mel_22k")                                   # two clips at 22050 Hz, NaN above the shorter
    fe = MelSpectrogram(cm["n_fft"], cm["n_mels"], cm["sr"], cm["hop"], cm["n_fft"], cm["fmin"], cm["fmax"], center=False, mel_basis=basis)
    r = rs((cm["sr"], 16000))
    w = y.to(DEV)
    w16, l16 = to_16k(r, w, lens)
    assert l16 == [r.out_len(v) for v in lens] and w16.shape == (2, r.out_len(max(lens))) and torch.isfinite(w16).all()
    rec = enrol_references_audio(fe, cp, r, w, lens)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")               # a warm call enqueues from host integers only
    try:
        again = enrol_references_audio(fe, cp, r, w, lens)
        to_16k(r, w, lens)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    want = enrol_references(fe, cp, w, lens, w16, l16)
    assert sorted(rec) == sorted(want) == ["prompt", "prompt_lens", "style"]
    assert rec["prompt_lens"] == want["prompt_lens"]
    for key in ("prompt", "style"):
        assert torch.equal(rec[key], want[key]) and torch.equal(again[key], want[key]) and torch.isfinite(rec[key]).all()
    same = Resample(16000, 16000, device=DEV)
    z = same(w16)
    assert torch.equal(z, w16) and z.data_ptr() != w16.data_ptr() and same.out_len(777) == 777
    z, zl = same(w16, lens=l16)
    assert torch.equal(z, w16) and zl == l16
