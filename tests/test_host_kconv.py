"""CPU side of the resident-tile conv's op-level suite (test_gpu_kconv.py): the seam is declared, exported and bound, and the
references of kconv_cases.py check themselves.  The GPU tests hold the fp16 + fp8-corrections kernel to `ref_p8` within
8 x n32 (the fp32 summation noise of that reference); these tests establish that such a bound separates a right kernel from a
subtly wrong one: 8 x n32 stays below a third of e_p8 (the distance of the mode from the truth), and every sabotage of the
restatement -- a dropped correction product, a scale off by a factor two, the two bytes swapped on one side -- moves the result
by more than 10 x e_p8."""
import ctypes
import os
import re

import pytest
import torch

import kconv_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

SABOTAGES = list(K.SABOTAGES.items())


def test_seam_is_declared_exported_and_bound():
    from seedvc_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    name = "svc_op_conv1d_ex"
    assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/seedvc_hip.h"
    assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(ops, "conv1d_cl_ex")
    # the ctypes mirror names the header's fields in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} svc_conv1d_ex_t;", header).group(1)
    fields = re.findall(r"\**\s*([A-Za-z_0-9]+)\s*[,;]", body)
    assert fields == [f[0] for f in _lib.Conv1dEx._fields_]


def test_seam_argument_errors_need_no_gpu():
    """The argument checks come before anything is allocated or launched."""
    from seedvc_amd import _lib
    fn, err = _lib.lib().svc_op_conv1d_ex, _lib.lib().svc_last_error

    def args(**kw):
        e = _lib.Conv1dEx()
        e.x = e.w = e.y = 16                     # never dereferenced: the checks come first
        e.B, e.L, e.Cin, e.Cout, e.k, e.dilation, e.Lout, e.dtype = 1, 200, 64, 64, 3, 1, 200, 2
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    for kw, word in [(dict(dtype=1), b"dtype"), (dict(bm=32), b"bm"), (dict(force_gemm=1, dtype=3), b"byte-pair"),
                     (dict(c_off=5), b"c_rows"), (dict(c_off=5, c_rows=204), b"c_rows"), (dict(post_a=16), b"Snake"),
                     (dict(next_p8=1), b"next_p8"), (dict(k=0), b"shape")]:
        assert fn(ctypes.byref(args(**kw)), None) != 0, kw
        assert word in err(), (kw, err())
    lens = (ctypes.c_int32 * 1)(201)
    assert fn(ctypes.byref(args(seq_len=ctypes.cast(lens, ctypes.POINTER(ctypes.c_int32)))), None) != 0
    assert b"seq_len" in err()


@pytest.mark.parametrize("Cin,k,dil", K.HOST_CASES)
def test_references_discriminate(Cin, k, dil):
    span = (k - 1) * dil
    x, w, b = K.make_case(Cin * 7 + k, 2, 257, Cin, 72, k)
    a = (x, w, dil, span // 2, 257)
    rp, rt, e_p8, n32, scale = K.p8_numbers(*a, bias=b)
    e_x3 = (K.ref_x3(*a, bias=b) - rt).abs().max().item() / scale
    e_f16 = (K.ref_f16(*a, bias=b) - rt).abs().max().item() / scale
    print(f"Cin {Cin} k {k} dil {dil}: n32 {n32:.2e}  e_p8 {e_p8:.2e}  e_x3 {e_x3:.2e}  e_f16 {e_f16:.2e}  w8_exp {K.w8_exp(w)}")
    assert 8 * n32 < e_p8 / 3
    assert e_x3 < e_p8 / 5 and e_p8 < e_f16 / 20       # the modes order as DESIGN.md says: fp16 >> p8 >> fp16x3
    assert e_x3 < 1e-5                                  # ... and the f16x3 restatement sits inside the bound f16x3 is held to
    for name, kw in SABOTAGES:
        d = (K.ref_p8(*a, bias=b, **kw) - rp).abs().max().item() / scale
        print(f"    {name}: {d:.2e}  ({d / e_p8:.0f} x e_p8)")
        assert d > 10 * e_p8, name


def test_p8_restatement_edges():
    """w8_exp at its upper clamp, at the largest weights fp16 holds and at an all-zero weight; amplitude 30 brings q8(a_hi) near its clamp without reaching it."""
    x, w, b = K.make_case(3, 1, 200, 64, 72, 3)
    assert K.w8_exp(w * 1e-5) == 24 and K.w8_exp(w * 1e12) == -24 and K.w8_exp(w * 0) == 0
    # the lower clamp is out of any real conv's reach: fp16 overflows first.  The largest weights w_hi can hold give -9.
    big = w * (6e4 / w.abs().max())
    assert K.w8_exp(big) == -9 and torch.isfinite(K.half(big)).all()
    assert 0 < K.w8_exp(w) < 24
    s = 2.0 ** K.w8_exp(w)
    assert 112 <= (w.abs().max() * s).item() <= 224
    assert torch.equal(K.ref_p8(x, w * 0, 1, 1, 200), torch.zeros(1, 200, 72, dtype=torch.float64))
    xa = 30 * x
    assert 100 < xa.abs().max().item() < 448
    _, _, e_p8, n32, _ = K.p8_numbers(xa, w, 1, 1, 200)
    assert 8 * n32 < e_p8 / 3
    # q8 is exact on what e4m3 holds, rounds to nearest even, keeps subnormals and saturates
    t = torch.tensor([0.0, 1.0, 448.0, 500.0, -1000.0, 2.0 ** -9, 2.0 ** -10 * 1.01, 2.0 ** -10, 17.0, 19.0])
    assert K.q8(t).tolist() == [0.0, 1.0, 448.0, 448.0, -448.0, 2.0 ** -9, 2.0 ** -9, 0.0, 16.0, 20.0]


def test_ref_modes_on_exact_operands():
    """operands that fp16 holds exactly: every mode's restatement equals the truth"""
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-8, 9, (2, 200, 64), generator=g).float() / 8
    w = torch.randint(-8, 9, (72, 64, 5), generator=g).float() / 64
    rt = K.ref_true(x, w, 3, 6, 200)
    assert torch.equal(K.ref_f16(x, w, 3, 6, 200), rt) and torch.equal(K.ref_x3(x, w, 3, 6, 200), rt)
    assert torch.equal(K.ref_p8(x, w, 3, 6, 200), rt)
    # and the zero padding is where the seam puts it: Lout = L - span with no pad is the valid conv
    assert torch.equal(K.ref_true(x, w, 3, 0, 188), rt[:, 6:194])


def test_snake_inputs_stay_clear_of_fp16_boundaries():
    """The fused-Snake test excuses elements whose float64 Snake lies within the fp32 Snake's own error of an fp16 rounding
    boundary; with the inputs it uses that is under 1 % of the elements (here on the reference's v, there on the kernel's)."""
    x, w, b, a, ib = K.snake_case()
    v = K.ref_true(x, w, 3, 9, 257, bias=b).float()
    err = K.snake_err(v, a, ib)
    sv = K.snake(v, a, ib)
    share = (K.f16_boundary_dist(sv) <= err).double().mean().item()
    print(f"snake error (4 x fp32 torch vs float64) {err:.2e}; share within it of an fp16 boundary {share:.4f}")
    assert err < 4e-6 and share < 0.01
    # the helpers: a boundary is half an ulp from a representable value, and ulp steps count across zero
    one = torch.tensor([1.0], dtype=torch.float64)
    assert abs(K.f16_boundary_dist(one).item() - 2.0 ** -12) < 1e-12       # below 1 the spacing halves
    bits = torch.tensor([1.0, -0.0, 6e-8], dtype=torch.float16).view(torch.int16)
    other = torch.tensor([1.0 + 2.0 ** -10, 0.0, -6e-8], dtype=torch.float16).view(torch.int16)
    assert K.f16_ulp_steps(bits, other).tolist() == [1, 0, 2]


def test_case_list_names_every_form_and_edge():
    cases = K.parity_cases()
    assert len(cases) == len(set(cases))
    forms = {(c[0],) + K.expected_form(c[1], c[2], c[4], c[9]) for c in cases}
    assert forms == {(m, bm, 128) for m in K.MODES for bm in (64, 128, 256)} | {(m, 256, 64) for m in K.MODES}
    col = lambda i: {c[i] for c in cases}      # noqa: E731
    assert col(3) == set(K.LS) and col(4) == {1, 3} and col(5) == set(K.CINS) and {(c[6], c[7]) for c in cases} == set(K.KD)
    assert {72, 130, 64} == col(2)
    for c in cases:
        mode, bm, Cout, L, B, Cin, k, dil, pad_left, Lout = c
        span = (k - 1) * dil
        assert span <= 64 and Lout >= K.KCONV_MIN_ROWS and pad_left in (0, span // 2, span) and Lout in (L, L - span)
        assert B * L <= 2000
    assert any(c[9] != c[3] for c in cases) and any(c[8] == 64 for c in cases)
