"""The epilogue of the resident-tile Conv1d (csrc/kconv.hip) and of the tap-GEMM's STORE form (csrc/kgemm_tile.h) through the
svc_op_conv1d_ex seam.  The epilogue requests its column vectors (bias, the Snake's a and 1 / b) once per lane and the res / res2
rows of every chunk of a pass before the first wait; these tests pin what that must not change.

Shapes: B = 2; L = 193 | 322 (one | two full 128-row tiles plus a short tail, above the L >= 192 selection rule); Cin = 64 | 128;
Cout = 128 | 72 (72: a partial count of 8-column groups and cout_pad > Cout, so the zero-plane rule runs); (k, dil) = (3, 1) |
(11, 5); operand modes p8 (dtype 3) and f16x3 (dtype 2).  Every test asserts from `took` that the kernel it means ran.

Bitwise tests need no tolerance: the tile forms share the epilogue and the K order.  test_epilogue_from_raw_sums restates the
epilogue in float64 from the kernel's OWN raw sums y0 (a second run with no epilogue term):
    y = ((act(y0 + bias) + res) * s) + res2,   s = 1/3,  act = none | leaky ReLU 0.1 | clamp 0.5
Each fp32 operation rounds once, by at most 2^-24 of its result (FMA contraction only removes roundings).  none and clamp give
four roundings.  Leaky ReLU has a fifth (v * slope) on its negative side, but the two roundings before `+ res` then pass through
`* s` = 1/3, so the sum stays below 2^-24 (|t1| / 30 + |t2| / 3 + |t3| / 3 + |t4| + |t5|) < 4 * 2^-24 max|t|.  Hence
    |y - ref| <= 4 * 2^-24 * max(1, largest intermediate magnitude)      per element.
The Snake planes and the tap-GEMM cases are held to what tests/test_gpu_kconv.py holds them to (kconv_cases.py).
"""
import itertools

import pytest
import torch

import kconv_cases as K

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CLAMP = 6       # KG_ACT_CLAMP (csrc/common.h)
B = 2
SHAPES = list(itertools.product(("p8", "f16x3"), (193, 322), (64, 128), (128, 72), ((3, 1), (11, 5))))
IDS = [f"{m}-L{L}-ci{ci}-co{co}-k{k}d{d}" for m, L, ci, co, (k, d) in SHAPES]
shapes = pytest.mark.parametrize("mode,L,Cin,Cout,kd", SHAPES, ids=IDS)
FULL = dict(act=K.LRELU, act_slope=0.1, out_scale=1.0 / 3.0)

_cases = {}


def case(L, Cin, Cout, k):
    """(x, w, bias, a, 1/b, res, res2) of a shape, on the CPU, made once"""
    key = (L, Cin, Cout, k)
    if key not in _cases:
        x, w, b, a, ib = K.snake_case(seed=L + 3 * Cin + 5 * Cout + 7 * k, B=B, L=L, Cin=Cin, Cout=Cout, k=k)
        g = torch.Generator().manual_seed(L + Cin + Cout + k)
        res, res2 = torch.randn(B, L, Cout, generator=g), torch.randn(B, L, Cout, generator=g)
        _cases[key] = (x, w, b, a, ib, res, res2)
    return _cases[key]


def run(x, w, b, mode, dil, pad, Lout, **kw):
    from seedvc_amd import ops
    kw = {n: (v.cuda() if torch.is_tensor(v) else v) for n, v in kw.items()}
    y, ph, pl, took = ops.conv1d_cl_ex(x.cuda(), w.cuda(), b.cuda() if b is not None else None, dilation=dil, pad_left=pad, Lout=Lout,
                                       dtype=mode, **kw)
    return y.cpu(), (ph.cpu() if ph is not None else None), (pl.cpu() if pl is not None else None), took


def assert_took(took, bm):
    assert took == {"kconv": True, "bm": bm, "bn": 128}, took


def same(a, b):
    """bit for bit (NaN patterns included)"""
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


# ------------------------------------------------------------------------------------------------ bitwise invariants
@shapes
def test_forms_and_ragged_bit_identical(mode, L, Cin, Cout, kd):
    """BM = 64 / 128 / 256 and the ragged form with seq_len = L: identical y and planes with the whole epilogue on"""
    (k, dil), pad = kd, (kd[0] - 1) * kd[1] // 2
    x, w, b, a, ib, res, res2 = case(L, Cin, Cout, k)
    for next_p8 in (False, True):
        kw = dict(res=res, res2=res2, post_a=a, post_ib=ib, next_p8=next_p8, **FULL)
        outs = []
        for bm, extra in ((64, {}), (128, {}), (256, {}), (128, dict(seq_len=[L] * B))):
            y, ph, pl, took = run(x, w, b, mode, dil, pad, L, bm=bm, **kw, **extra)
            assert_took(took, bm)
            assert torch.isfinite(y).all()
            outs.append((y, ph, pl))
        for o in outs[1:]:
            for t0, t1, name in zip(outs[0], o, ("y", "plane_hi", "plane_lo")):
                assert same(t0, t1), (next_p8, name)


@shapes
def test_in_place_equals_out_of_place(mode, L, Cin, Cout, kd):
    """res = y, then res2 = y: the kernel reads each element of the addend before it writes it, in every form (BM 256 runs the
    epilogue in two passes)"""
    (k, dil), pad = kd, (kd[0] - 1) * kd[1] // 2
    x, w, b, a, ib, res, res2 = case(L, Cin, Cout, k)
    kw = dict(post_a=a, post_ib=ib, next_p8=(mode == "p8"), **FULL)
    for bm in (64, 128, 256):
        want = run(x, w, b, mode, dil, pad, L, bm=bm, res=res, res2=res2, **kw)
        assert_took(want[3], bm)
        for name, args in (("res", dict(y_init=res, res="y", res2=res2)), ("res2", dict(y_init=res2, res=res, res2="y"))):
            got = run(x, w, b, mode, dil, pad, L, bm=bm, **args, **kw)
            assert_took(got[3], bm)
            for t0, t1, what in zip(want[:3], got[:3], ("y", "plane_hi", "plane_lo")):
                assert same(t0, t1), (bm, name, what)


@shapes
def test_rows_outside_the_window_are_kept(mode, L, Cin, Cout, kd):
    """c_rows > Lout, c_off > 0: y and the planes keep their sentinels outside [c_off, c_off + Lout); plane columns
    [Cout, cout_pad) of the written rows are zero words"""
    from seedvc_amd import ops
    (k, dil), pad = kd, (kd[0] - 1) * kd[1] // 2
    x, w, b, a, ib, res, res2 = case(L, Cin, Cout, k)
    c_off, c_rows, sentinel = 5, L + 9, -7777.0
    pad_rows = lambda t: torch.nn.functional.pad(t, (0, 0, c_off, c_rows - L - c_off))     # noqa: E731
    rows = slice(c_off, c_off + L)
    for bm in (64, 128, 256):
        y, ph, pl, took = run(x, w, b, mode, dil, pad, L, bm=bm, res=pad_rows(res), res2=pad_rows(res2), c_rows=c_rows, c_off=c_off,
                              y_fill=sentinel, post_a=a, post_ib=ib, next_p8=(mode == "p8"), **FULL)
        assert_took(took, bm)
        assert y.shape == (B, c_rows, Cout) and ph.shape == (B, c_rows, -(-Cout // 64) * 64) and pl.shape == ph.shape
        assert (y[:, :c_off] == sentinel).all() and (y[:, c_off + L:] == sentinel).all()
        assert torch.isfinite(y[:, rows]).all() and (y[:, rows] != sentinel).all()
        for pln in (ph, pl):
            assert (pln[:, :c_off] == ops.PLANE_FILL).all() and (pln[:, c_off + L:] == ops.PLANE_FILL).all()
            assert (pln[:, rows, Cout:] == 0).all()
            assert (pln[:, rows, :Cout] != ops.PLANE_FILL).all()
        # and the window holds what the same conv writes at c_off = 0
        y0, ph0, pl0, _ = run(x, w, b, mode, dil, pad, L, bm=bm, res=res, res2=res2, post_a=a, post_ib=ib, next_p8=(mode == "p8"), **FULL)
        assert same(y[:, rows].contiguous(), y0) and same(ph[:, rows].contiguous(), ph0) and same(pl[:, rows].contiguous(), pl0)


# ------------------------------------------------------------------------------------------------ the epilogue against its raw sums
@shapes
def test_epilogue_from_raw_sums(mode, L, Cin, Cout, kd):
    (k, dil), pad = kd, (kd[0] - 1) * kd[1] // 2
    x, w, b, a, ib, res, res2 = case(L, Cin, Cout, k)
    y0, _, _, took = run(x, w, None, mode, dil, pad, L, bm=128)
    assert_took(took, 128)
    assert torch.isfinite(y0).all()
    s = float(torch.tensor(1.0 / 3.0, dtype=torch.float32))
    for act, slope in ((0, 0.0), (K.LRELU, 0.1), (CLAMP, 0.5)):
        y, _, _, took = run(x, w, b, mode, dil, pad, L, bm=128, res=res, res2=res2, act=act, act_slope=slope, out_scale=1.0 / 3.0)
        assert_took(took, 128)
        sl = float(torch.tensor(slope, dtype=torch.float32))
        t1 = y0.double() + b.double()
        t2 = t1 if act == 0 else (torch.where(t1 > 0, t1, t1 * sl) if act == K.LRELU else t1.clamp(-sl, sl))
        t3 = t2 + res.double()
        t4 = t3 * s
        ref = t4 + res2.double()
        big = torch.stack([t.abs() for t in (t1, t2, t3, t4, ref)]).amax(0).clamp(min=1.0)
        d = ((y.double() - ref).abs() / big).max().item()
        print(f"act {act}: worst |y - ref| / max(1, intermediates) = {d / 2.0 ** -24:.2f} x 2^-24")
        assert d <= 4 * 2.0 ** -24, act
        if act == CLAMP:
            assert ((t1.abs() > sl).double().mean().item()) > 0.2       # the clamp does clamp


# ------------------------------------------------------------------------------------------------ Snake planes
def decode_pairs(pl):
    """int16 byte-pair plane -> (byte 0, byte 1) as float64"""
    by = pl.contiguous().view(torch.uint8)
    return by[..., 0::2].view(K.F8).double(), by[..., 1::2].view(K.F8).double()


def check_planes(label, y, ph, pl, a, ib, Cout, next_p8):
    """the planes against the Snake of the kernel's own fp32 v, as test_gpu_kconv.test_fused_snake_planes compares them"""
    sv = K.snake(y, a, ib)
    err = K.snake_err(y, a, ib)
    hi_bits = ph[..., :Cout]
    want = sv.float().half()
    near = K.f16_boundary_dist(sv) <= err
    steps = K.f16_ulp_steps(hi_bits, want.view(torch.int16))
    print(f"{label}: snake error {err:.2e}, {near.double().mean().item():.4f} near an fp16 boundary, {(steps != 0).sum().item()} differ")
    assert near.double().mean().item() <= 0.01
    assert (steps[~near] == 0).all()
    assert (steps[near] <= 1).all()
    assert (ph[..., Cout:] == 0).all() and (pl[..., Cout:] == 0).all()
    hi = hi_bits.contiguous().view(torch.float16).double()
    if not next_p8:
        lo = pl[..., :Cout].contiguous().view(torch.float16).double()
        assert (hi + lo - sv).abs().max().item() <= err
        return
    b0, b1 = decode_pairs(pl[..., :Cout])
    assert torch.equal(b0, K.q8(hi))
    resid = (hi + b1 / 2048.0 - sv).abs()
    allowed = 2.0 ** -4 * (sv - hi).abs() + 2.0 ** -20 + err
    assert (resid <= allowed).all()


def check_y(label, mode, y, x, w, dil, pad, L, extra=0.0, **epi):
    """y against the mode's reference at the mode's bound, as test_gpu_kconv.check has it"""
    assert torch.isfinite(y).all(), label
    y = y.double()
    if mode == "p8":
        rp, rt, e_p8, n32, scale = K.p8_numbers(x, w, dil, pad, L, **epi)
        d, dt = (y - rp).abs().max().item() / scale, (y - rt).abs().max().item() / scale
        print(f"{label}: kernel-ref_p8 {d:.2e} ({d / max(n32, 1e-30):.1f} x n32)  e_p8 {e_p8:.2e}")
        assert d <= 8 * n32 + extra / scale, label
        assert dt <= e_p8 + 8 * n32 + extra / scale, label
        return
    ref = K.REFS[mode](x, w, dil, pad, L, **epi)
    scale = max(1.0, ref.abs().max().item())
    d = (y - ref).abs().max().item() / scale
    print(f"{label}: kernel-ref {d:.2e}  scale {scale:.3g}")
    assert d < K.ABS_BOUND[mode] + extra / scale, label


@shapes
def test_snake_planes(mode, L, Cin, Cout, kd):
    (k, dil), pad = kd, (kd[0] - 1) * kd[1] // 2
    x, w, b, a, ib, _, _ = case(L, Cin, Cout, k)
    for next_p8 in ((True,) if mode == "p8" else (False, True)):
        y, ph, pl, took = run(x, w, b, mode, dil, pad, L, bm=128, post_a=a, post_ib=ib, next_p8=next_p8)
        assert_took(took, 128)
        if not next_p8 or mode == "p8":
            check_y(f"snake {mode}: y keeps the raw v", mode, y, x, w, dil, pad, L, bias=b)
        check_planes(f"snake {mode} next_p8={next_p8}", y, ph, pl, a, ib, Cout, next_p8)


# ------------------------------------------------------------------------------------------------ tap-GEMM STORE epilogue
@pytest.mark.parametrize("Cout", [128, 72])
def test_tap_gemm_same_operands(Cout):
    """the whole epilogue and the Snake through force_gemm: the mode's bound (plus the three fp32 roundings of the added terms, as
    test_epilogue_everything_on allows them), the planes as above, and within the bound of the resident-tile kernel's y"""
    mode, L, Cin, (k, dil) = "f16x3", 322, 128, (11, 5)
    pad = (k - 1) * dil // 2
    x, w, b, a, ib, res, res2 = case(L, Cin, Cout, k)
    kw = dict(res=res, res2=res2, post_a=a, post_ib=ib, **FULL)
    yg, ph, pl, took = run(x, w, b, mode, dil, pad, L, force_gemm=True, **kw)
    assert took["kconv"] is False
    v = K.ref_true(x, w, dil, pad, L, bias=b)
    big = v.abs().max().item() + res.abs().max().item() + res2.abs().max().item()
    check_y("tap-GEMM epilogue", mode, yg, x, w, dil, pad, L, extra=3 * 2.0 ** -24 * big, bias=b, res=res, res2=res2, **FULL)
    yk, _, _, took = run(x, w, b, mode, dil, pad, L, bm=128, **kw)
    assert_took(took, 128)
    assert (yg - yk).abs().max().item() < K.ABS_BOUND[mode] * max(1.0, yg.abs().max().item())
    # the planes on the case they are made for (bias only: |sv| stays where fp16 values are far apart)
    ys, phs, pls, took = run(x, w, b, mode, dil, pad, L, force_gemm=True, post_a=a, post_ib=ib)
    assert took["kconv"] is False
    check_planes("tap-GEMM planes", ys, phs, pls, a, ib, Cout, False)
    # in place on the tap-GEMM too
    for name, args in (("res", dict(y_init=res, res="y", res2=res2)), ("res2", dict(y_init=res2, res=res, res2="y"))):
        yi, phi, pli, took = run(x, w, b, mode, dil, pad, L, force_gemm=True, post_a=a, post_ib=ib, **args, **FULL)
        assert took["kconv"] is False
        assert same(yi, yg) and same(phi, ph) and same(pli, pl), name


@pytest.mark.parametrize("Cout", [128, 72])
def test_tap_gemm_one_tap_with_bias(Cout):
    from seedvc_amd import ops
    L, Cin = 322, 128
    x, w, b = K.make_case(5 + Cout, B, L, Cin, Cout, 1)
    for mode in ("f16", "f16x3"):
        y = ops.conv1d_cl(x.cuda(), w.cuda(), b.cuda(), pad_left=0, Lout=L, dtype=mode).cpu()
        assert ops.conv1d_last_took()["kconv"] is False
        ref = K.REFS[mode](x, w, 1, 0, L, bias=b)
        scale = max(1.0, ref.abs().max().item())
        d = (y.double() - ref).abs().max().item() / scale
        print(f"1-tap {mode} Cout{Cout}: kernel-ref {d:.2e}")
        assert d < K.ABS_BOUND[mode]
