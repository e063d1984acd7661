"""The resident-tile Conv1d (csrc/kconv.hip) at op level, through the svc_op_conv1d_ex seam: every operand mode (fp16, fp16x3,
fp16 + fp8 corrections), every tile form (BM 64 / 128 / 256 x BN 128, BM 256 x BN 64), the ragged form, the epilogue, the fused
Snake's operand planes and the routing of conv1d_run, against the float64 references of kconv_cases.py.  Every test first
asserts, from the seam's `took` word, that the kernel and the form it means to test are what ran.

Bounds.  fp16 is held to `ref_f16` and fp16x3 to the truth at the bounds of test_conv1d_channels_last (3e-5, 1e-5), times
max(1, |ref|max) as test_conv1d_fuzz has it.  The fp16 + fp8-corrections mode is held to its restatement `ref_p8` within
8 x n32, n32 being the fp32 summation noise of that restatement for the case at hand (the same convs evaluated in float32):
eight times, because the kernel sums chunk by chunk and tap by tap in another order than torch does.  test_host_kconv.py shows
that this is under a third of the mode's own distance from the truth (e_p8) and that a dropped correction product, a scale
exponent off by one or swapped bytes move the result by more than 10 x e_p8.
"""
import pytest
import torch

import kconv_cases as K

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def run(x, w, b, mode, dil, pad_left, Lout, **kw):
    from seedvc_amd import ops
    kw = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in kw.items()}
    if "planes" in kw:
        kw["planes"] = tuple(p.cuda() for p in kw["planes"])
    y, ph, pl, took = ops.conv1d_cl_ex(x.cuda(), w.cuda(), b.cuda() if b is not None else None, dilation=dil, pad_left=pad_left,
                                       Lout=Lout, dtype=mode, **kw)
    return y.cpu(), (ph.cpu() if ph is not None else None), (pl.cpu() if pl is not None else None), took


def assert_took(took, bm, bn):
    assert took == {"kconv": True, "bm": bm, "bn": bn}, took


def check(label, mode, y, x, w, dil, pad_left, Lout, floor=1.0, extra=0.0, fp8_sum_fallback=False, **epi):
    """y against the mode's reference at the mode's bound (module docstring); extra: absolute allowance for fp32 roundings of
    epilogue terms the bound does not know, already divided by nothing (it is scaled here)"""
    assert torch.isfinite(y).all(), label
    y = y.double()
    if mode == "p8":
        rp, rt, e_p8, n32, scale = K.p8_numbers(x, w, dil, pad_left, Lout, floor=floor, **epi)
        d, dt = (y - rp).abs().max().item() / scale, (y - rt).abs().max().item() / scale
        print(f"{label}: kernel-ref_p8 {d:.2e} ({d / max(n32, 1e-30):.1f} x n32)  n32 {n32:.2e}  e_p8 {e_p8:.2e}  kernel-true {dt:.2e}"
              f"  w8_exp {K.w8_exp(w)}  scale {scale:.3g}")
        # 8 x n32 is the bound the reference's own noise gives, and the bound of every case but one (fp8_sum_fallback, see
        # test_p8_scale_edges).  Measured on an MI355X over this file's other p8 cases: kernel-ref_p8 = 0.6 .. 3.3 x n32.
        bound = 8 * n32
        if fp8_sum_fallback:
            bound = min([e_p8 / 2] + [(K.ref_p8(x, w, dil, pad_left, Lout, **kw, **epi) - rp).abs().max().item() / scale / 10
                                      for kw in K.SABOTAGES.values()])
            print(f"    fall-back bound {bound:.2e} ({bound / n32:.0f} x n32)")
        assert d <= bound + extra / scale, label
        assert dt <= e_p8 + bound + extra / scale, label
        return d, n32, e_p8
    ref = K.REFS[mode](x, w, dil, pad_left, Lout, **epi)
    scale = max(floor, ref.abs().max().item())
    d = (y - ref).abs().max().item() / scale
    print(f"{label}: kernel-ref {d:.2e}  scale {scale:.3g}")
    assert d < K.ABS_BOUND[mode] + extra / scale, label
    return d


# ------------------------------------------------------------------------------------------------ parity of every form and mode
@pytest.mark.parametrize("mode,bm,Cout,L,B,Cin,k,dil,pad_left,Lout", K.parity_cases())
def test_parity(mode, bm, Cout, L, B, Cin, k, dil, pad_left, Lout):
    x, w, b = K.make_case(L * 7 + Cin * 3 + k * 11 + dil + Cout + pad_left, B, L, Cin, Cout, k)
    y, _, _, took = run(x, w, b, mode, dil, pad_left, Lout, bm=bm)
    assert_took(took, *K.expected_form(bm, Cout, B, Lout))
    assert y.shape == (B, Lout, Cout)
    check(f"{mode} bm{bm} Cout{Cout} L{L}->{Lout} B{B} Cin{Cin} k{k} d{dil} p{pad_left}", mode, y, x, w, dil, pad_left, Lout, bias=b)


def test_default_form_is_by_grid_size():
    """no override: BM = 64 while B * ceil(L / 256) * ceil(N / 128) <= 96, else 128 -- the form of any real batch"""
    x, w, b = K.make_case(12, 49, 192, 64, 130, 3)
    y, _, _, took = run(x[:48], w, b, "p8", 1, 1, 192)        # 48 * 1 * 2 = 96 tiles of 256 rows
    assert_took(took, 64, 128)
    y, _, _, took = run(x, w, b, "p8", 1, 1, 192)             # 98
    assert_took(took, 128, 128)
    check("default BM 128", "p8", y, x, w, 1, 1, 192, bias=b)


@pytest.mark.parametrize("what", ["tiny", "huge", "zero", "amp30"])
def test_p8_scale_edges(what):
    """w8_exp at its upper clamp (24), at the lowest value finite fp16 weights can give (-9: the lower clamp, -24, is beyond
    fp16's range), an all-zero weight (exponent 0) and activations whose fp8(hi) byte nears its clamp"""
    B, L, Cin, Cout, k, dil = 3, 257, 65, 72, 7, 3
    x, w, b = K.make_case(99, B, L, Cin, Cout, k, amp=30.0 if what == "amp30" else 1.0)
    floor = 1.0
    if what == "tiny":
        w, b, floor = w * 1e-5, None, 0.0
        assert K.w8_exp(w) == 24
    elif what == "huge":
        w, b = w * (6e4 / w.abs().max()), None
        assert K.w8_exp(w) == -9
    elif what == "zero":
        w = w * 0
    else:
        assert 100 < x.abs().max().item() < 448
    y, _, _, took = run(x, w, b, "p8", dil, 9, L, bm=128)
    assert_took(took, 128, 128)
    if what == "zero":
        assert torch.equal(y, b.expand(B, L, Cout))
        return
    # "tiny" takes the fall-back bound.  Its weights are fp16 subnormals (7 bits of w_hi at most), so the correction products are
    # 2 % of the output, not 2^-11 of it, and 2^11 s w_lo saturates: e_p8 = 1.4e-2.  Measured on an MI355X: kernel-ref_p8 =
    # 1.99e-6 = 22 x n32 (n32 = 9.0e-8), i.e. 1e-4 = 2^-13 of the correction sum.  That is the precision at which the fp8 MFMA
    # sums its 128 products (here of two magnitudes 2^8 apart); in every other case of this file the same 2^-13 sits on terms
    # 2^-11 of the output and stays inside 8 x n32.  The residual has no structure: over weight
    # scales 3e-5 .. 3e-6 and 3 / 7 taps it stays 0.8e-4 .. 1.2e-4 of the correction sum, the per-channel maxima lie within
    # 1.4x of each other and the rows at tile edges are not above the others (its mean is negative: the sum truncates).
    # The issue's fall-back for exactly this is e_p8 / 2, "closer to the restatement than the restatement is to the truth"; at this case's e_p8 that alone would let a dropped lo * w_hi product (1.9e-4)
    # through, so the bound is the smaller of e_p8 / 2 and a tenth of the nearest sabotaged restatement (kconv_cases.SABOTAGES):
    # 1.9e-5 here.  Both come from the references alone.
    check(f"p8 {what}", "p8", y, x, w, dil, 9, L, floor=floor, fp8_sum_fallback=(what == "tiny"), bias=b)


# ------------------------------------------------------------------------------------------------ forms agree bit for bit
@pytest.mark.parametrize("mode", K.MODES)
def test_forms_bit_identical(mode):
    """kconv_launch's claim: the summation order of an output element is the same in every form.  Two column tiles, two chunks,
    a tile edge inside every sequence; y and both fused-Snake planes.  The tap-GEMM is not claimed identical: the mode's bound."""
    B, L, Cin, Cout, k, dil, pad = 3, 321, 65, 130, 7, 3, 9
    x, w, b = K.make_case(2024, B, L, Cin, Cout, k)
    a, ib = K.snake_case(Cout=Cout)[3:]
    kw = dict(post_a=a, post_ib=ib, next_p8=(mode == "p8"))
    outs = {}
    for bm in (64, 128, 256):
        y, ph, pl, took = run(x, w, b, mode, dil, pad, L, bm=bm, **kw)
        assert_took(took, bm, 128)
        outs[bm] = (y, ph, pl)
    for bm in (128, 256):
        for t0, t1, name in zip(outs[64], outs[bm], ("y", "hi plane", "lo plane")):
            assert torch.equal(t0.view(torch.int32) if name == "y" else t0, t1.view(torch.int32) if name == "y" else t1), (bm, name)
    check(f"forms {mode}", mode, outs[64][0], x, w, dil, pad, L, bias=b)
    if mode == "p8":
        return      # the tap-GEMM reads no byte-pair planes
    yg, _, _, took = run(x, w, b, mode, dil, pad, L, force_gemm=True, post_a=a, post_ib=ib)
    assert took["kconv"] is False
    check(f"forms {mode} tap-GEMM", mode, yg, x, w, dil, pad, L, bias=b)
    scale = max(1.0, yg.abs().max().item())
    assert (yg - outs[64][0]).abs().max().item() < K.ABS_BOUND[mode] * scale


# ------------------------------------------------------------------------------------------------ ragged
RAGGED = [(128, 72, [321, 256, 193, 1]), (64, 130, [321, 320, 129, 64]), (256, 72, [321, 256, 193, 1]), (0, 64, [321, 257, 192, 1])]


@pytest.mark.parametrize("bm,Cout,lens", RAGGED)
@pytest.mark.parametrize("mode", K.MODES)
def test_ragged(mode, bm, Cout, lens):
    """Sequence b is x[b, :len_b] convolved alone.  The rows at and above len_b hold NaN: the kernel documents that it never
    loads them.  Nothing is asserted about output rows at and above len_b."""
    B, L, Cin, k, dil, pad = 4, 321, 65, 7, 3, 9
    x, w, b = K.make_case(700 + Cout, B, L, Cin, Cout, k)
    xn = x.clone()
    for i, n in enumerate(lens):
        xn[i, n:] = float("nan")
    y, _, _, took = run(xn, w, b, mode, dil, pad, L, bm=bm, seq_len=lens)
    assert_took(took, *K.expected_form(bm, Cout, B, L))
    # one reference over all valid rows (the bound's n32 and scale are the batch's), each sequence convolved alone
    valid = torch.cat([y[i, :n] for i, n in enumerate(lens)])[None]
    assert torch.isfinite(valid).all()
    refs = {name: torch.cat([fn(x[i:i + 1, :n], w, dil, pad, n, bias=b) for i, n in enumerate(lens)], 1)
            for name, fn in (("true", K.ref_true), ("mode", K.REFS[mode]))}
    scale = max(1.0, refs["true"].abs().max().item())
    d = (valid.double() - refs["mode"]).abs().max().item() / scale
    if mode == "p8":
        r32 = torch.cat([K.ref_p8(x[i:i + 1, :n], w, dil, pad, n, dt=torch.float32, bias=b) for i, n in enumerate(lens)], 1)
        n32 = (r32 - refs["mode"]).abs().max().item() / scale
        e_p8 = (refs["mode"] - refs["true"]).abs().max().item() / scale
        print(f"ragged p8 bm{bm} Cout{Cout}: kernel-ref_p8 {d:.2e} ({d / n32:.1f} x n32)  n32 {n32:.2e}  e_p8 {e_p8:.2e}")
        assert d <= 8 * n32
        assert (valid.double() - refs["true"]).abs().max().item() / scale <= e_p8 + 8 * n32
    else:
        print(f"ragged {mode} bm{bm} Cout{Cout}: kernel-ref {d:.2e}")
        assert d < K.ABS_BOUND[mode]
    # and bit for bit what the same sequence gives alone, wherever the sequence alone takes this kernel too
    for i, n in enumerate(lens):
        if n < K.KCONV_MIN_ROWS:
            continue
        ya, _, _, took = run(x[i:i + 1, :n].contiguous(), w, b, mode, dil, pad, n, bm=bm)
        assert_took(took, *K.expected_form(bm, Cout, 1, n))
        assert torch.equal(ya[0].view(torch.int32), y[i, :n].view(torch.int32)), (i, n)


# ------------------------------------------------------------------------------------------------ epilogue
@pytest.mark.parametrize("mode", K.MODES)
def test_epilogue_everything_on(mode):
    """bias, leaky ReLU, + res, * 1/3, + res2, written at row offset 5 of sequences of Lout + 9 rows; the other rows keep a
    sentinel.  The added terms each round once in fp32: half an ulp of the largest intermediate value, three times."""
    B, L, Cin, Cout, k, dil, pad = 3, 257, 64, 130, 5, 16, 32
    c_off, c_rows, sentinel = 5, L + 9, -7777.0
    x, w, b = K.make_case(31, B, L, Cin, Cout, k)
    g = torch.Generator().manual_seed(32)
    res, res2 = torch.randn(B, c_rows, Cout, generator=g), torch.randn(B, c_rows, Cout, generator=g)
    epi = dict(act=K.LRELU, act_slope=0.1, out_scale=1.0 / 3.0)
    y, _, _, took = run(x, w, b, mode, dil, pad, L, bm=128, res=res, res2=res2, c_rows=c_rows, c_off=c_off, y_fill=sentinel, **epi)
    assert_took(took, 128, 128)
    assert y.shape == (B, c_rows, Cout)
    assert (y[:, :c_off] == sentinel).all() and (y[:, c_off + L:] == sentinel).all()
    rows = slice(c_off, c_off + L)
    v = K.ref_true(x, w, dil, pad, L, bias=b)
    big = v.abs().max().item() + res.abs().max().item() + res2.abs().max().item()
    check(f"epilogue {mode}", mode, y[:, rows], x, w, dil, pad, L, extra=3 * 2.0 ** -24 * big, bias=b, res=res[:, rows],
          res2=res2[:, rows], **epi)


# ------------------------------------------------------------------------------------------------ fused Snake planes
def decode_pairs(pl):
    """int16 byte-pair plane -> (byte 0, byte 1) as float64"""
    by = pl.contiguous().view(torch.uint8)
    return by[..., 0::2].view(K.F8).double(), by[..., 1::2].view(K.F8).double()


@pytest.mark.parametrize("mode,next_p8", [("f16", False), ("f16x3", False), ("p8", True), ("f16x3", True)])
def test_fused_snake_planes(mode, next_p8):
    from seedvc_amd import ops
    L, Cout, dil, pad = 257, 72, 3, 9
    x, w, b, a, ib = K.snake_case()
    y, ph, pl, took = run(x, w, b, mode, dil, pad, L, bm=128, post_a=a, post_ib=ib, next_p8=next_p8)
    assert_took(took, 128, 128)
    assert ph.shape == (3, L, 128) and pl.shape == ph.shape
    check(f"snake {mode}: y keeps the raw v", mode, y, x, w, dil, pad, L, bias=b)
    # pad columns: the next conv reads all cin_pad channels of these planes (the seam pre-fills them with a non-zero pattern)
    assert ops.PLANE_FILL != 0
    assert (ph[..., Cout:] == 0).all() and (pl[..., Cout:] == 0).all()
    sv = K.snake(y, a, ib)                       # float64, on the kernel's own fp32 v
    err = K.snake_err(y, a, ib)
    hi_bits = ph[..., :Cout]
    want = sv.float().half()                     # float64 -> fp32 -> fp16 double-rounds only next to a boundary: excused below
    near = K.f16_boundary_dist(sv) <= err
    steps = K.f16_ulp_steps(hi_bits, want.view(torch.int16))
    print(f"snake {mode} next_p8={next_p8}: snake error {err:.2e}, {near.double().mean().item():.4f} of the elements near an fp16 boundary, "
          f"{(steps != 0).sum().item()} differ")
    assert near.double().mean().item() <= 0.01
    assert (steps[~near] == 0).all()
    assert (steps[near] <= 1).all()
    hi = hi_bits.contiguous().view(torch.float16).double()
    if not next_p8:
        lo = pl[..., :Cout].contiguous().view(torch.float16).double()
        d = (hi + lo - sv).abs().max().item()
        print(f"    hi + lo - sv: {d:.2e}")
        assert d <= err
        return
    b0, b1 = decode_pairs(pl[..., :Cout])
    assert torch.equal(b0, K.q8(hi))
    resid = (hi + b1 / 2048.0 - sv).abs()
    allowed = 2.0 ** -4 * (sv - hi).abs() + 2.0 ** -20 + err
    print(f"    byte-pair residual / allowance, worst: {(resid / allowed).max().item():.3f}")
    assert (resid <= allowed).all()


def test_snake_to_p8_conv_chain():
    """What the model does: conv A writes the operand planes of conv B through its fused Snake (byte pairs), conv B runs in the
    fp16 + fp8-corrections mode on them.  B is held to ref_p8 evaluated on the planes as decoded from A: the producer and the
    consumer agree on the format, byte order and pad columns included (B reads all 128 channels of A's 72)."""
    L, dil, pad = 257, 3, 9
    x, w, b, a, ib = K.snake_case()
    _, ph, pl, took = run(x, w, b, "p8", dil, pad, L, bm=128, post_a=a, post_ib=ib, next_p8=True)
    assert_took(took, 128, 128)
    xb, wb, bb = K.make_case(77, 3, L, 72, 130, 3)            # xb gives B its shape only
    yb, _, _, took = run(xb, wb, bb, "p8", 5, 5, L, bm=64, planes=(ph, pl))
    assert_took(took, 64, 128)
    hi = ph[..., :72].contiguous().view(torch.float16).double()
    b0, b1 = decode_pairs(pl[..., :72])
    rp = K.ref_p8(None, wb, 5, 5, L, planes=(hi, b0, b1), bias=bb)
    r32 = K.ref_p8(None, wb, 5, 5, L, planes=(hi, b0, b1), dt=torch.float32, bias=bb)
    scale = max(1.0, rp.abs().max().item())
    n32 = (r32 - rp).abs().max().item() / scale
    d = (yb.double() - rp).abs().max().item() / scale
    print(f"chain: kernel-ref_p8 {d:.2e} ({d / n32:.1f} x n32)  n32 {n32:.2e}")
    assert torch.isfinite(yb).all() and d <= 8 * n32


# ------------------------------------------------------------------------------------------------ routing
def test_routing_table():
    """conv1d_run's choice, pinned on both sides of every condition a shape can cross."""
    from seedvc_amd import ops

    def took(L=192, k=3, dil=1, Cin=64, Cout=64, mode="f16x3"):
        x, w, b = K.make_case(1, 1, L, Cin, Cout, k)
        span = (k - 1) * dil
        y, _, _, t = run(x, w, b, mode, dil, span // 2, L)
        check(f"routing L{L} k{k} d{dil} Cin{Cin} Cout{Cout}", mode, y, x, w, dil, span // 2, L, bias=b)
        return t["kconv"]
    assert took() is True
    assert took(L=191) is False                       # KCONV_MIN_ROWS
    assert took(k=5, dil=16) is True                  # span 64
    assert took(k=6, dil=13) is False                 # span 65
    assert took(k=1) is False
    assert took(Cin=18) is True                       # cin_pad 64 (pad channels)
    assert took(Cout=18) is True                      # cout_pad 64
    assert took(mode="f16") is True and took(mode="f16", L=191) is False
    # stride and pad mode exist in the first seam only; it shares the second's body and leaves the same word behind
    x, w, b = K.make_case(2, 1, 400, 64, 64, 3)
    xc, wc, bc = x.cuda(), w.cuda(), b.cuda()
    for kw, want in [(dict(), True), (dict(stride=2, Lout=200), False), (dict(pad_mode=1), False), (dict(dtype="f32"), False)]:
        kw = {"dtype": "f16x3", "Lout": 400, **kw}
        ops.conv1d_cl(xc, wc, bc, pad_left=1, **kw)
        assert ops.conv1d_last_took()["kconv"] is want, kw


def test_p8_on_a_shape_the_kernel_does_not_take_fails_cleanly():
    from seedvc_amd import _lib
    x, w, b = K.make_case(1, 1, 191, 64, 64, 3)
    with pytest.raises(RuntimeError, match="resident-tile"):
        run(x, w, b, "p8", 1, 1, 191)
    assert b"fp8-pair" in _lib.lib().svc_last_error()
    with pytest.raises(RuntimeError, match="resident-tile"):        # ... nor may a tap-GEMM conv be asked for byte pairs
        a, ib = K.snake_case(Cout=64)[3:]
        run(x, w, b, "f16x3", 1, 1, 191, post_a=a, post_ib=ib, next_p8=True)
    x, w, b = K.make_case(1, 1, 192, 64, 64, 3)                     # the neighbour runs
    y, _, _, took = run(x, w, b, "p8", 1, 1, 192)
    assert_took(took, 256, 64)
