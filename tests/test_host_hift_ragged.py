"""CPU side of the ragged HiFT call (`svc_hift_forward_ragged`, `HiFT.__call__(x, ..., lens=...)`,
`HotPath.convert_batch_ragged`): the entry point is declared, exported and bound; its argument checks come before anything is
launched; the CPU model of the design equals the oracle run alone on every utterance (this keeps the GPU tests' yardstick
honest: the design itself loses nothing); and padding is no substitute for it, so a GPU test that passes cannot be passing by
padding."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import cases
import hift_ragged_cases as R
import seedvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

# The masked model and the oracle alone run the same fp32 ops on the same values, but F.conv1d on a (B, C, 300) batch and on a
# (1, C, n) utterance may take different CPU algorithms (summation orders): ~1e-7 relative per conv, through ~60 convs of a
# signal of RMS ~0.1, and the float64 STFT / iSTFT are rounded to fp32 at the same places.  1e-5 is that with two orders of
# margin and a tenth of the GPU tests' bound (the ragged BigVGAN host test uses the same figure).
MODEL_RMS = 1e-5


def test_ragged_entry_point_is_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline, vocoder
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    name = "svc_hift_forward_ragged"
    assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
    assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
    assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    p = inspect.signature(vocoder.HiFT.__call__).parameters
    assert "lens" in p and p["lens"].default is None
    assert list(p)[:6] == ["self", "x", "f0", "phase0", "noise", "return_f0"]           # today's positional order stays
    p = inspect.signature(pipeline.HotPath.convert_batch_ragged).parameters
    assert list(p)[1:] == ["mu", "prompt", "style", "x_lens", "prompt_lens", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs"]


def test_ragged_argument_errors_need_no_gpu():
    """Lengths are checked on the host before the handle is touched or anything is launched."""
    from seedvc_amd import _lib
    fn = _lib.lib().svc_hift_forward_ragged
    err = _lib.lib().svc_last_error
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks come first
    assert fn(one, one, i32(3, 5), None, one, one, 2, 4, one, None, None) != 0         # a length above S
    assert b"lens" in err()
    assert fn(one, one, i32(3, -1), None, one, one, 2, 4, one, None, None) != 0        # a negative length
    assert b"lens" in err()
    assert fn(one, one, None, None, one, one, 2, 4, one, None, None) != 0              # no lengths
    assert fn(one, one, i32(1), None, one, one, 0, 4, one, None, None) != 0            # B < 1
    assert fn(one, one, i32(0), None, one, one, 1, 0, one, None, None) != 0            # S < 1


@pytest.fixture(scope="module")
def hift_r():
    c, sd, _, _, _, _ = cases.hift_case(R.MODEL)
    return c, sd, R.batch(c, sd, R.LENS)                 # NaN in every padding frame, f0 slot and noise sample


def test_masked_model_equals_oracle_alone(hift_r):
    c, sd, bt = hift_r
    lens, up = R.LENS, R.total_up(c)
    ref = R.ragged_reference(sd, c, bt, lens)
    got, f0 = R.masked_model(sd, c, bt, lens)
    assert got.shape == ref.shape == (len(lens), max(lens) * up)
    assert torch.isfinite(got).all() and torch.isfinite(f0).all()
    sig = ref[0].pow(2).mean().sqrt().item()
    assert sig > 1e-2 and ref.abs().max().item() < c["audio_limit"]          # a signal, and not a clamped one
    for b, n in enumerate(lens):
        assert (got[b, n * up:] == 0).all() and (f0[b, n:] == 0).all(), f"utterance {b} ({n} frames): tail not zero"
        if n:
            e = R.rms(got[b, :n * up], ref[b, :n * up])
            print(f"utterance {b} ({n} frames): masked model vs oracle alone RMS {e:.2e} (signal RMS {sig:.2e})")
            assert e < MODEL_RMS


def test_masked_f0_predictor_equals_oracle_alone(hift_r):
    c, sd, bt = hift_r
    f0 = R.masked_f0(sd, bt["mel"], R.LENS)
    for b, n in enumerate(R.LENS):
        if n:
            want = O.hift_f0_predictor(sd, bt["mel"][b:b + 1, :, :n])[0]
            rel = ((f0[b, :n] - want).abs() / want.abs().clamp_min(1.0)).max().item()
            print(f"utterance {b} ({n} frames): masked f0 predictor vs oracle alone, max rel {rel:.2e}")
            assert rel < 4e-6                            # five fp32 convs of K = 144: ~sqrt(144) * 6e-8 each; a fifth of the GPU bound
            assert not torch.isfinite(f0[b, n:]).any()   # the rows above are the poison, not values


def test_masked_model_with_its_own_f0_is_finite_and_zero_tailed(hift_r):
    c, sd, bt = hift_r
    up = R.total_up(c)
    got, f0 = R.masked_model(sd, c, bt, R.LENS, predicted_f0=True)
    assert torch.isfinite(got).all() and torch.isfinite(f0).all()
    for b, n in enumerate(R.LENS):
        assert (got[b, n * up:] == 0).all() and (f0[b, n:] == 0).all()


@pytest.mark.parametrize("fill", [R.LOG_MEL_FLOOR, 0.0], ids=["floor", "zeros"])
def test_padding_is_not_a_substitute(fill):
    """The oracle on an utterance inside a 300-frame row (pinned f0 and draws, the row's padding frames = `fill`, unvoiced f0
    and fresh noise above the end) differs from the oracle on the utterance alone, over the valid samples, by far more than
    any bound of the ragged tests."""
    c, sd, _, _, _, _ = cases.hift_case(R.MODEL)
    up, S = R.total_up(c), 300
    for b, n in ((3, 191), (4, 47), (7, 5)):
        mel, phase0, noise, f0 = R.utterance(c, sd, b, n)
        alone = O.hift_forward(sd, c, mel, phase0, noise, f0=f0)[0]
        row = torch.full((1, c["in_channels"], S), fill)
        row[:, :, :n] = mel
        f0_row = torch.zeros(1, S)
        f0_row[:, :n] = f0
        noise_row = cases.randn("hr.padnoise", b, 1, c["nb_harmonics"] + 1, S * up)
        noise_row[:, :, :n * up] = noise
        padded = O.hift_forward(sd, c, row, phase0, noise_row, f0=f0_row)[0, :n * up]
        e, e_hop = R.rms(padded, alone), R.rms(padded[-up:], alone[-up:])
        print(f"{n} frames in a {S}-frame row, padding {fill:+.2f}: RMS vs alone {e:.2e}, over the last hop {e_hop:.2e}")
        assert e > 1e-3
