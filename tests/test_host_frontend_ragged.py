"""CPU side of the ragged reference front-end (`svc_mel_forward_ragged`, `svc_kaldi_fbank_ragged`,
`svc_campplus_forward_ragged`; `MelSpectrogram.__call__(y, lens=...)`, `CAMPPlus.__call__(x, lens=...)`, `fbank_batch`,
`style_batch`, `pipeline.enrol_references`): the entry points are declared, exported and bound; their argument checks come
before anything is launched; the CPU statement of the design equals the oracle run alone on every clip (this keeps the GPU
tests' yardstick honest: the design itself loses nothing); and zero padding is no substitute for the lengths, so a GPU test
that passes cannot be passing by padding."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import cases
import frontend_ragged_cases as R
import seedvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

NAMES = ("svc_mel_forward_ragged", "svc_kaldi_fbank_ragged", "svc_campplus_forward_ragged")


def test_ragged_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, audio, campplus, pipeline
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
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    p = inspect.signature(audio.MelSpectrogram.__call__).parameters
    assert list(p) == ["self", "y", "lens", "pad_value"] and p["lens"].default is None and p["pad_value"].default == 0.0
    p = inspect.signature(campplus.CAMPPlus.__call__).parameters
    assert list(p) == ["self", "x", "x_lens", "lens"] and p["x_lens"].default is None and p["lens"].default is None
    p = inspect.signature(campplus.CAMPPlus.fbank_batch).parameters
    assert list(p) == ["self", "waves", "lens", "subtract_mean"] and p["subtract_mean"].default is False
    assert list(inspect.signature(campplus.CAMPPlus.style_batch).parameters) == ["self", "waves_16k", "lens"]
    assert list(inspect.signature(campplus.CAMPPlus.fbank).parameters) == ["self", "wave"]          # today's calls stay
    assert list(inspect.signature(campplus.CAMPPlus.style).parameters) == ["self", "wave_16k"]
    assert list(inspect.signature(pipeline.enrol_references).parameters) == ["mel_fn", "campplus", "waves", "lens", "waves_16k", "lens_16k"]


def test_ragged_argument_errors_need_no_gpu():
    """Lengths are checked on the host before the handle is touched or anything is launched, and the message names lens."""
    from seedvc_amd import _lib
    lib, err = _lib.lib(), _lib.lib().svc_last_error
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks come first

    def bad(rc):
        assert rc != 0 and b"lens" in err(), err()

    mel, fb, cp = lib.svc_mel_forward_ragged, lib.svc_kaldi_fbank_ragged, lib.svc_campplus_forward_ragged
    # mel: (m, y, lens, B, L, pad_value, out, stream)
    bad(mel(one, one, None, 2, 400, 0.0, one, None))                        # lens NULL
    bad(mel(one, one, i32(400, 401), 2, 400, 0.0, one, None))               # a length above L
    bad(mel(one, one, i32(400), 0, 400, 0.0, one, None))                    # B < 1
    # a length equal to the reflect padding (n_fft - hop) / 2: the one rule that needs the handle's n_fft and hop, so it cannot be
    # called without a GPU.  The rule itself is `svc_mel_min_len`, which the call compares lens[b] with: for mel_r (n_fft 64, hop
    # 16: pad 24) a length of 24 is below it, and the shortest legal clip is the 25 of frontend_ragged_cases.  The same call with a
    # real handle and lens = [400, 24] is in test_gpu_frontend_ragged.py (non-zero, names lens).
    assert lib.svc_mel_min_len(64, 16) == 25 == min(R.MEL_R_LENS) and 24 == (64 - 16) // 2
    assert lib.svc_mel_min_len(1024, 256) == 385                            # mel_22k: pad 384
    assert lib.svc_mel_min_len(64, 48) == 48                                # a hop above the pad: at least one hop
    # fbank: (m, wave, lens, B, L, subtract_mean, out, stream)
    bad(fb(one, one, None, 2, 5000, 0, one, None))
    bad(fb(one, one, i32(5000, 5001), 2, 5000, 0, one, None))
    bad(fb(one, one, i32(5000, 399), 2, 5000, 1, one, None))                # shorter than one 25 ms frame
    bad(fb(one, one, i32(5000), 0, 5000, 0, one, None))
    # CAMPPlus: (m, feat, lens, B, T, out, stream)
    bad(cp(one, one, None, 2, 260, one, None))
    bad(cp(one, one, i32(260, 261), 2, 260, one, None))
    bad(cp(one, one, i32(260, 7), 2, 260, one, None))                       # below the existing call's minimum of 8
    bad(cp(one, one, i32(260), 0, 260, one, None))


@pytest.fixture(scope="module")
def cp_r():
    c, sd, _ = cases.campplus_case(R.CP_MODEL)
    return c, sd, R.cp_batch(c)                          # NaN in every padding frame


def test_masked_campplus_equals_oracle_alone(cp_r):
    c, sd, feat = cp_r
    got = R.masked_campplus(sd, c, feat, R.CP_LENS)
    assert got.shape == (len(R.CP_LENS), c["embedding_size"]) and torch.isfinite(got).all()
    for b, n in enumerate(R.CP_LENS):
        want = O.campplus_forward(sd, c, feat[b:b + 1, :n])
        e = (got[b:b + 1] - want).abs().max().item()
        print(f"clip {b} ({n} frames, T2 {R.t2_of(n)}): masked model vs oracle alone, max |diff| {e:.2e} (|emb| mean {want.abs().mean():.3f})")
        assert e < 2e-5                                   # the project's CAMPPlus parity bound


def test_zero_padding_is_not_a_substitute(cp_r):
    """The oracle on a clip zero-padded to the batch's 260 frames differs from the oracle on the clip alone by far more than
    any bound of the ragged tests: the pooled statistics, every CAM layer's global-mean context and the convs' padding at the
    clip's end all see the padding."""
    c, sd, feat = cp_r
    for b, n in list(enumerate(R.CP_LENS))[1:]:
        alone = O.campplus_forward(sd, c, feat[b:b + 1, :n])
        row = torch.zeros(1, max(R.CP_LENS), c["feat_dim"])
        row[:, :n] = feat[b, :n]
        e = (O.campplus_forward(sd, c, row) - alone).abs().max().item()
        print(f"clip {b}: {n} frames zero-padded to {max(R.CP_LENS)}: embedding moves by {e:.2e}")
        assert e > 1e-2
