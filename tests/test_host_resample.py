"""CPU side of the device resampler (`svc_resample`, `audio.Resample`, `pipeline.to_16k`): the taps table the library is given
is the dense float32 kernel bit for bit, the two length functions agree, the from-memory restatement of torchaudio's operator
that every GPU test is measured against does resample a sine, and the new symbols are declared, exported and bound."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

import resample_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

NAMES = ("svc_resampler_create", "svc_resampler_destroy", "svc_resample_len", "svc_resampler_tile", "svc_resample")


@pytest.mark.parametrize("pair", list(RC.TABLE))
def test_taps_table_is_the_dense_kernel(pair):
    from seedvc_amd.audio import sinc_resample_taps
    o, n, width, ntaps = RC.TABLE[pair]
    o_, n_, width_, first, taps = sinc_resample_taps(*pair)
    _, _, _, K = RC.dense_kernel(*pair)
    assert (o_, n_, width_) == (o, n, width) and taps.shape == (n, ntaps) and first.shape == (n,)
    assert taps.dtype == torch.float32 and first.dtype == torch.int32 and K.shape == (n, 2 * width + o)
    dense = torch.zeros(n, 2 * width + o + ntaps)                           # room for the 0.0 padding of the shorter runs
    cols = first.long()[:, None] + torch.arange(ntaps)[None, :]
    dense.scatter_(1, cols, taps)
    assert (dense[:, 2 * width + o:] == 0).all()
    dense = dense[:, :2 * width + o]
    live = K != 0
    # bit for bit where K is not zero; the dropped entries are K's exact zeros (of either sign: a product with one is +-0.0)
    assert torch.equal(dense.view(torch.int32)[live], K.view(torch.int32)[live]) and (dense[~live] == 0).all()
    runs = (K != 0).sum(dim=1)
    assert int(runs.max()) == ntaps and int(runs.min()) >= 1
    assert (taps[:, 0] != 0).all()                                            # first[j] is where the run starts


def test_lengths_agree():
    from seedvc_amd import _lib
    from seedvc_amd.audio import Resample
    lib = _lib.lib()
    for pair, (o, n, _, _) in RC.TABLE.items():
        r = Resample.__new__(Resample)                                        # out_len needs no handle and no GPU
        r.o, r.n, r._h = o, n, None
        for L in (1, 2, o - 1, o, o + 1, 2 ** 31 - 1, 64 * 26460000):
            if L < 1:
                continue
            want = -((-n * L) // o)
            assert r.out_len(L) == want and lib.svc_resample_len(o, n, L) == want, (pair, L)


@pytest.mark.parametrize("pair", RC.SINE_PAIRS)
def test_the_yardstick_is_a_resampler(pair):
    """A 1 kHz sine through the dense statement in float64 is the sine sampled at the new rate, within the 6-lobe Hann filter's
    pass-band ripple (4.4e-4, 4.0e-4, 4.0e-4, 1.5e-4, 1.5e-4, 6.9e-4 for the six pairs; the bound is about twice the largest)."""
    orig, new = pair
    L = orig // 2 + 37
    o, n, width, K32 = RC.dense_kernel(orig, new)
    g = math.gcd(orig, new)
    assert (o, n) == (orig // g, new // g)
    x = torch.sin(2 * math.pi * 1000.0 * torch.arange(L, dtype=torch.float64) / orig)[None]
    y = RC.resample_dense(orig, new, x)[0]                                    # the yardstick itself: float32 K, float64 arithmetic
    assert y.numel() == RC.out_len(o, n, L)
    want = torch.sin(2 * math.pi * 1000.0 * torch.arange(y.numel(), dtype=torch.float64) / new)
    e = (y - want)[40:-40].abs().max().item()
    print(f"{orig} -> {new}: 1 kHz sine, max |error| away from the ends {e:.2e}")
    assert e < 1.5e-3


def test_new_symbols_are_declared_exported_and_bound():
    from seedvc_amd import _lib, audio, pipeline
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert list(inspect.signature(audio.Resample.__call__).parameters) == ["self", "x", "lens"]
    assert list(inspect.signature(pipeline.to_16k).parameters) == ["resample", "waves", "lens"]
    assert list(inspect.signature(pipeline.enrol_references_audio).parameters) == ["mel_fn", "campplus", "resample", "waves", "lens"]
    # existing signatures stay
    assert list(inspect.signature(pipeline.enrol_references).parameters) == ["mel_fn", "campplus", "waves", "lens", "waves_16k", "lens_16k"]
    assert list(inspect.signature(pipeline.v2_content_tokens).parameters) == ["astral", "waves_16k", "lens", "overlap_s"]
