"""CPU side of the ragged BigVGAN call (`svc_bigvgan_forward_ragged`, `BigVGAN.__call__(mel, lens=...)`,
`V2HotPath(..., ragged_vocoder=...)`): the entry point is declared, exported and bound; its argument checks come before
anything is launched; the CPU model of the masking design equals the oracle run alone on every utterance (this keeps the
GPU tests' yardstick honest: the design itself loses nothing); and padding is no substitute for it, so a GPU test that
passes cannot be passing by padding."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import cases
import seedvc_oracle as O
import vocoder_ragged_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


def test_ragged_entry_point_is_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline, vocoder
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    name = "svc_bigvgan_forward_ragged"
    assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
    assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
    assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    p = inspect.signature(vocoder.BigVGAN.__call__).parameters
    assert "lens" in p and p["lens"].default is None
    p = inspect.signature(pipeline.V2HotPath.__init__).parameters
    assert "ragged_vocoder" in p and p["ragged_vocoder"].default is True
    assert callable(pipeline.group_by_length)


def test_ragged_argument_errors_need_no_gpu():
    """Lengths are checked on the host before the handle is touched or anything is launched."""
    from seedvc_amd import _lib
    lib = _lib.lib()
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks come first
    assert lib.svc_bigvgan_forward_ragged(one, one, i32(3, 5), 2, 4, one, None) != 0         # a length above S
    assert b"lens" in lib.svc_last_error()
    assert lib.svc_bigvgan_forward_ragged(one, one, i32(3, -1), 2, 4, one, None) != 0        # a negative length
    assert b"lens" in lib.svc_last_error()
    assert lib.svc_bigvgan_forward_ragged(one, one, None, 2, 4, one, None) != 0              # no lengths
    assert lib.svc_bigvgan_forward_ragged(one, one, i32(1), 0, 4, one, None) != 0            # B < 1
    assert lib.svc_bigvgan_forward_ragged(one, one, i32(0), 1, 0, one, None) != 0            # S < 1


@pytest.mark.parametrize("name", R.MODELS)
def test_masked_model_equals_oracle_alone(name):
    h, sd, _, _ = cases.bigvgan_case(name)
    lens = R.LENS
    up = R.total_up(h)
    mel = R.batch_mel(h, lens)                           # padding frames are NaN
    ref = R.ragged_reference(sd, h, mel, lens)
    got = R.masked_model(sd, h, mel, lens)
    assert got.shape == ref.shape == (len(lens), 1, max(lens) * up)
    assert torch.isfinite(got).all()
    for b, n in enumerate(lens):
        assert (got[b, 0, n * up:] == 0).all(), f"{name}: utterance {b} ({n} frames): tail not zero"
        if n:
            e = R.rms(got[b, 0, :n * up], ref[b, 0, :n * up])
            print(f"{name}: utterance {b} ({n} frames): masked model vs oracle alone RMS {e:.2e}")
            assert e < 1e-5


@pytest.mark.parametrize("name", R.MODELS)
def test_padding_is_not_a_substitute(name):
    """The oracle on a mel followed by floor-valued frames differs from the oracle on the mel alone, over the valid samples,
    by far more than any bound of the ragged tests (measured: RMS >= 2.8e-2)."""
    h, sd, _, _ = cases.bigvgan_case(name)
    up = R.total_up(h)
    for b, n in enumerate(R.LENS):
        if n == 0 or n == 430 and b:
            continue
        mel = R.utterance_mel(h, b, n)[None]
        padded = torch.cat([mel, torch.full((1, h["num_mels"], R.PAD_FRAMES), R.LOG_MEL_FLOOR)], dim=2)
        alone = O.bigvgan_forward(sd, h, mel).reshape(-1)
        with_pad = O.bigvgan_forward(sd, h, padded).reshape(-1)[:n * up]
        e = R.rms(with_pad, alone)
        print(f"{name}: {n} frames + {R.PAD_FRAMES} floor frames vs alone: RMS {e:.2e} over the valid samples")
        assert e > 1e-3
