"""CPU side of the batched AR path: the C ABI, `_lib.EXPORTS` and the library agree on the new entry points, and the
sequences the GPU tests compare token for token are robust to the logit error the kernels are allowed."""
import ctypes
import os
import re

import pytest
import torch

import ar_batch_cases as A
import seedvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH_SYMBOLS = ("svc_ar_set_max_batch", "svc_ar_prefill_slot", "svc_ar_decode_step_batch", "svc_ar_generate_batch")
torch.set_grad_enabled(False)


def test_batch_abi_agrees():
    from seedvc_amd import _lib
    from seedvc_amd.ar import ARModel
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in BATCH_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1
    assert "#define SVC_ABI_VERSION 1" in header
    for name in ("generate_batch", "prefill_slot", "decode_step_batch"):
        assert callable(getattr(ARModel, name, None)), name


def test_argument_errors_need_no_gpu():
    """The batch limits are checked before anything touches the device."""
    from seedvc_amd import _lib
    lib = _lib.lib()
    assert lib.svc_ar_set_max_batch(None, 8, None) != 0
    assert lib.svc_last_error()


@pytest.mark.parametrize("b", A.ORDER)
def test_chosen_sequences_survive_the_allowed_logit_error(b, monkeypatch):
    """The probe that chose the sequences: the oracle on fp16-rounded matrices, with uniform noise of +- LOGIT_TOL x
    mean |logit| added to every logit vector, generates the oracle's tokens (10 trials)."""
    c, sd = A.model()
    text, target, noise, ref = A.sequence(b)
    assert ref.shape[1] == A.N_TOKENS[b]
    # boosting the winners does not move the oracle itself
    assert torch.equal(A.oracle_tokens(sd, text, target, noise), ref)
    sd16 = {k: (v.half().float() if v.dim() == 2 and ("layers." in k or k == "model.output.weight") else v) for k, v in sd.items()}
    plain_forward = O.ar_forward_generate
    gen = torch.Generator().manual_seed(1000 + b)

    def noisy_forward(*args, **kw):
        lg = plain_forward(*args, **kw)
        amp = A.LOGIT_TOL * max(lg.abs().mean().item(), 1.0)
        return lg + (torch.rand(lg.shape, generator=gen) * 2 - 1) * amp

    monkeypatch.setattr(O, "ar_forward_generate", noisy_forward)
    for trial in range(10):
        got = A.oracle_tokens(sd16, text, target, noise)
        assert got.shape == ref.shape and torch.equal(got, ref), f"sequence {b}, trial {trial}: {got.tolist()} vs {ref.tolist()}"
