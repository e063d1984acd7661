"""The DiT's full-precision mode (precision 2, fp16x3) without a GPU: the new entry points are declared, exported and bound,
precision names are checked before anything is loaded, refusals come before any allocation, and the error level of the split product
that the GPU bounds (test_gpu_dit_precision.py) are argued from."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dit_precision_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    for name in ("svc_dit_create_ex", "svc_dit_precision", "svc_op_attention_x3"):
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert hasattr(ops, "attention_x3")
    assert "3x the fp16 pack" in header        # the memory cost of a precision-2 handle is stated where it is created


@pytest.mark.parametrize("bad", [0, 3, -1, "fp32", "FP16", None, 2.0, True])
def test_estimator_rejects_unknown_precision_before_loading(bad):
    """The name is checked first: neither the state dict nor the device is looked at (both are unusable here)."""
    from seedvc_amd.cfm import CFM, Estimator

    class Untouchable(dict):
        def items(self):
            raise AssertionError("the state dict was read")

    for cls in (Estimator, CFM):
        with pytest.raises(ValueError, match="precision"):
            cls({"C": 80}, Untouchable(), "cuda:7", precision=bad)


def test_precision_names():
    from seedvc_amd.cfm import dit_precision
    assert [dit_precision(p) for p in (1, 2, "fp16", "fp16x3")] == [1, 2, 1, 2]


@pytest.mark.parametrize("precision", [0, 3, -1])
def test_create_refuses_other_precisions_before_any_allocation(precision):
    """Dummy weights and stream: the check comes before the first allocation, so no device is needed; *out stays NULL."""
    from seedvc_amd import _lib
    from seedvc_amd.cfm import _cfg_struct
    import cases
    cfg = cases.dit_case("tiny_r")[0]
    cs = _cfg_struct(cfg)
    out = ctypes.c_void_p()
    descs = (_lib.TensorDesc * 1)()
    rc = _lib.lib().svc_dit_create_ex(ctypes.byref(cs), descs, 0, precision, None, ctypes.byref(out))
    assert rc != 0 and out.value is None
    assert b"precision" in _lib.lib().svc_last_error()
    assert _lib.lib().svc_dit_precision(None) == 0


@pytest.mark.parametrize("K", P.X3_KS)
def test_split_product_error_level(K):
    """hi / lo split and the three-product sum on N(0, 1) operands against float64, beside a float32 product and a single fp16
    product.  The bound is the one the split's arithmetic gives (dit_precision_cases.X3_REL per product, plus the fp32
    accumulation both share); the measured ratio to float32's error is what DESIGN 8v quotes."""
    a, b = P.x3_operands(K)
    ref = a.astype(np.float64) @ b.astype(np.float64).T
    mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64).T          # sum_k |a_k b_k| per output
    e3 = np.abs(P.x3_matmul(a, b) - ref)
    e32 = np.abs((a @ b.T).astype(np.float64) - ref)
    ah, bh = P.split_hi_lo(a)[0], P.split_hi_lo(b)[0]
    e16 = np.abs((ah @ bh.T).astype(np.float64) - ref)
    print(f"K={K}: max err x3 {e3.max():.3e}  fp32 {e32.max():.3e}  fp16 operands {e16.max():.3e}  "
          f"x3/fp32 {e3.max() / e32.max():.2f}  fp16/x3 {e16.max() / e3.max():.0f}")
    # representation (worst case, every product) + three fp32 sums of K terms, summed pairwise by numpy or in order by the MFMA:
    # at most K roundings of a partial sum that never exceeds mag
    assert np.all(e3 <= P.X3_REL * mag + 3 * K * P.F32_EPS * mag)
    # the split recovers what a single fp16 rounding of both operands loses: 2 x 2^-11 per product against 3 x 2^-22, random signs
    assert e16.max() > 50 * e3.max()
    # and sits at float32's level: within 2^3 of a float32 product's own error on the same operands
    assert e3.max() <= 8 * e32.max()
    # hi + lo reproduces a float32 value to 2^-22 relative
    hi, lo = P.split_hi_lo(a)
    assert np.all(np.abs(a - (hi + lo)) <= 2.0 ** -22 * np.abs(a) + 2.0 ** -25)


def test_float64_yardstick_follows_the_oracle():
    """The float64 run is the oracle's own code: rounded to float32 it agrees with the oracle's float32 run to float32 noise, and the
    restated pieces are put back afterwards."""
    import cases
    import seedvc_oracle as O
    saved = O.timestep_embed, O.rope_table
    for name in ("tiny_r", "small_r", "v2_r"):
        cfg, sd, inp, meta, est64, smp64 = P.dit_reference(name)
        assert est64.dtype == torch.float64 and smp64.dtype == torch.float64
        T, Pl = meta["T"], meta["P"]
        prompt_x = torch.zeros(1, cfg["C"], T)
        prompt_x[..., :Pl] = inp["prompt"]
        y32 = O.dit_forward(sd, cfg, inp["x"], prompt_x, torch.LongTensor([T]), inp["t"], inp["style"], inp["mu"])
        d = (y32.double() - est64).abs().max().item()
        print(f"{name}: float32 oracle vs float64 yardstick, estimator max-abs {d:.3e}")
        assert d < 2e-4, (name, d)       # float32 noise of a 4-5 layer estimator with O(1) outputs; fp16 operands sit near 1e-2
    assert (O.timestep_embed, O.rope_table) == saved
