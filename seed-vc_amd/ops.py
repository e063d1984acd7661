"""Op-level wrappers over the C ABI (parity tests and the anti-aliased activation seam)."""
import torch

from . import _lib


def anti_alias_activation_forward(inputs, up_ftr, down_ftr, alpha, beta):
    """Drop-in for `anti_alias_activation_cuda.forward(inputs, up_ftr, down_ftr, alpha, beta)`
    (reference: modules/bigvgan/alias_free_activation/cuda/activation1d.py:23-25): (B,C,L) in -> (B,C,L) out,
    same dtype (fp32 / fp16 / bf16); alpha/beta are log-scale, exp() is applied in the kernel."""
    assert inputs.is_cuda and inputs.dim() == 3
    x = inputs.contiguous()
    dt = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[x.dtype]
    y = torch.empty_like(x)
    with torch.cuda.device(x.device):
        up = _lib.f32c(up_ftr, x.device).reshape(-1)
        dn = _lib.f32c(down_ftr, x.device).reshape(-1)
        al = _lib.f32c(alpha, x.device).reshape(-1)
        be = _lib.f32c(beta, x.device).reshape(-1)
        B, Cc, L = x.shape
        _lib.check(_lib.lib().svc_anti_alias_act_fwd(_lib.ptr(x), _lib.ptr(y), _lib.ptr(up), _lib.ptr(dn), _lib.ptr(al),
                                                     _lib.ptr(be), B, Cc, L, dt, _lib.stream_ptr()))
    return y


def linear(a, w, bias=None, dtype="f16", act=0):
    M, K = a.shape
    N = w.shape[0]
    dev = a.device
    with torch.cuda.device(dev):
        a, w = _lib.f32c(a), _lib.f32c(w)
        b = _lib.f32c(bias) if bias is not None else None
        c = torch.empty(M, N, device=dev)
        _lib.check(_lib.lib().svc_op_linear(_lib.ptr(a), _lib.ptr(w), _lib.ptr(b), _lib.ptr(c), M, N, K,
                                            0 if dtype == "f16" else 1, act, _lib.stream_ptr()))
    return c


def conv1d_cl(x, w, bias, dilation=1, stride=1, pad_left=0, Lout=None, pad_mode=0, dtype="f32"):
    """x (B, L, Cin) channels-last, w (Cout, Cin, k) torch layout -> (B, Lout, Cout)."""
    B, L, Cin = x.shape
    Cout, _, k = w.shape
    dev = x.device
    if Lout is None:
        Lout = L
    with torch.cuda.device(dev):
        x, w = _lib.f32c(x), _lib.f32c(w)
        b = _lib.f32c(bias) if bias is not None else None
        y = torch.empty(B, Lout, Cout, device=dev)
        _lib.check(_lib.lib().svc_op_conv1d(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B, L, Cin, Cout, k,
                                            dilation, stride, pad_left, Lout, pad_mode, {"f16": 0, "f32": 1, "f16x3": 2}[dtype],
                                            _lib.stream_ptr()))
    return y


CONV_DTYPES_EX = {"f16": 0, "f16x3": 2, "p8": 3}
PLANE_FILL = 0x7E7E      # what conv1d_cl_ex's planes hold where the conv did not write (an fp16 / fp8 NaN pattern, never zero)


def conv1d_cl_ex(x, w, bias=None, dilation=1, pad_left=0, Lout=None, dtype="f16x3", seq_len=None, res=None, res2=None,
                 out_scale=0.0, act=0, act_slope=0.0, c_rows=0, c_off=0, y_fill=None, post_a=None, post_ib=None, next_p8=False,
                 bm=0, force_gemm=False, planes=None, y_init=None):
    """Test aid over svc_op_conv1d_ex (include/seedvc_hip.h): one stride-1 zero-padded channels-last conv with the epilogue, the
    fused Snake, the ragged form, the fp16 + fp8-corrections mode ("p8") and a tile-form override.
    x (B, L, Cin) fp32, or planes = (hi, lo) int16 (B, L, cin_pad) as a fused Snake returned them (x then only gives the shape).
    Returns (y (B, c_rows, Cout), plane_hi, plane_lo, took): the planes are int16 (B, c_rows, cout_pad) or None without a Snake,
    took = dict(kconv=bool, bm=int, bn=int).  Rows of y the conv does not write hold y_fill, or y_init's (B, c_rows, Cout) where
    given.  res / res2 = "y" passes y itself as that addend (the conv runs in place on what y_init put there)."""
    import ctypes as C
    B, L, Cin = x.shape
    Cout, _, k = w.shape
    dev = x.device
    if Lout is None:
        Lout = L
    rows = c_rows if c_rows else Lout
    cin_pad, cout_pad = -(-Cin // 64) * 64, -(-Cout // 64) * 64
    with torch.cuda.device(dev):
        e = _lib.Conv1dEx()
        keep = [_lib.f32c(w)]
        e.w = keep[0].data_ptr()
        if planes is not None:
            hi, lo = (p.contiguous() for p in planes)
            assert hi.shape == (B, L, cin_pad) and lo.shape == hi.shape and hi.dtype == torch.int16 and lo.dtype == torch.int16
            keep += [hi, lo]
            e.a_hi, e.a_lo = hi.data_ptr(), lo.data_ptr()
        else:
            keep.append(_lib.f32c(x))
            e.x = keep[-1].data_ptr()
        for name, t, shape in (("bias", bias, (Cout,)), ("res", res, (B, rows, Cout)), ("res2", res2, (B, rows, Cout)),
                               ("post_a", post_a, (Cout,)), ("post_ib", post_ib, (Cout,))):
            if t is not None and not isinstance(t, str):
                assert tuple(t.shape) == shape, name
                keep.append(_lib.f32c(t))
                setattr(e, name, keep[-1].data_ptr())
        e.B, e.L, e.Cin, e.Cout, e.k, e.dilation, e.pad_left, e.Lout = B, L, Cin, Cout, k, dilation, pad_left, Lout
        e.dtype = CONV_DTYPES_EX[dtype]
        if seq_len is not None:
            assert len(seq_len) == B
            lens = (C.c_int32 * B)(*[int(v) for v in seq_len])
            e.seq_len = C.cast(lens, C.POINTER(C.c_int32))
        e.out_scale, e.act, e.act_slope, e.c_rows, e.c_off = out_scale, act, act_slope, c_rows, c_off
        e.next_p8, e.bm, e.force_gemm = int(next_p8), bm, int(force_gemm)
        if y_init is not None:
            assert tuple(y_init.shape) == (B, rows, Cout)
            y = _lib.f32c(y_init).clone()
        else:
            y = torch.full((B, rows, Cout), float("nan") if y_fill is None else y_fill, device=dev)
        e.y = y.data_ptr()
        for name, t in (("res", res), ("res2", res2)):
            if isinstance(t, str):
                assert t == "y" and y_init is not None, name
                setattr(e, name, e.y)
        p_hi = p_lo = None
        if post_a is not None:
            p_hi = torch.full((B, rows, cout_pad), PLANE_FILL, dtype=torch.int16, device=dev)
            p_lo = torch.full((B, rows, cout_pad), PLANE_FILL, dtype=torch.int16, device=dev)
            e.plane_hi, e.plane_lo = p_hi.data_ptr(), p_lo.data_ptr()
        _lib.check(_lib.lib().svc_op_conv1d_ex(C.byref(e), _lib.stream_ptr()))
    return y, p_hi, p_lo, _took(e.took)


def _took(word):
    return {"kconv": bool(word & 1), "bm": (word >> 8) & 0xFFF, "bn": word >> 20}


def conv1d_last_took():
    """which kernel this thread's last conv1d_cl / conv1d_cl_ex call ran: dict(kconv=bool, bm=int, bn=int) (test aid)"""
    return _took(_lib.lib().svc_op_conv1d_last_took())


_PANEL_F32 = ("wo", "w1", "w3", "w2", "wskip", "wqkv", "w_merge", "head_wa", "head_w2", "gate_a", "gate_f", "g_ffn", "w_f", "b_f", "g_attn",
              "w_a", "b_a", "bskip", "g_fin", "w_fin", "b_fin", "head_b0", "head_b2", "tok_time", "tok_style", "st_term", "rope")
_PANEL_F16 = ("ao", "skip_in", "x16")
_PANEL_INT = ("D", "I", "gated", "tm", "M", "Lout", "seq_rows", "row_off", "n_seq", "add_one", "do_post", "do_skip", "do_qkv", "do_final",
              "seam", "ldw", "C", "vt_mode", "ldv", "head_C", "npre", "time_first", "T")


def dit_panel(a, device="cuda:0", fill16=0x6A5A, fill32=-777.25):
    """Test aid over svc_op_dit_panel (include/seedvc_hip.h): ONE launch of the fused DiT row-panel kernel on unpacked weights.
    `a` maps the fields of svc_dit_panel_t to ints / floats and CPU or device tensors (fp32 weights, vectors, x, st_term and
    rope; fp16 ao, skip_in, x16; None = absent), plus want_c16.  Every activation buffer has n_seq * seq_rows rows.
    Returns {name: device tensor} of every output buffer handed to the kernel, whether the launch writes it or not: x (a copy
    of a["x"], run in place), c16 (with want_c16), n16 (with do_final, the head seam included), qk and vt (n_seq, D, vt_ld) (with
    do_qkv), v32 (rows, ldv) (with the head seam).  Where the kernel does not write, fp16 buffers hold the bit pattern fill16
    and v32 holds fill32."""
    import ctypes as C
    dev = torch.device(device)
    D, n_rows = int(a["D"]), int(a["n_seq"]) * int(a["seq_rows"])
    with torch.cuda.device(dev):
        e = _lib.DitPanel()
        keep = []
        for name in _PANEL_INT:
            setattr(e, name, int(a.get(name) or 0))
        e.eps, e.q_scale = float(a["eps"]), float(a.get("q_scale") or 0.0)
        for names, dt in ((_PANEL_F32, torch.float32), (_PANEL_F16, torch.float16)):
            for name in names:
                t = a.get(name)
                if t is not None:
                    assert t.dtype == dt, name
                    keep.append(t.to(dev).contiguous())
                    setattr(e, name, keep[-1].data_ptr())
        for name, rows in (("ao", n_rows), ("skip_in", n_rows), ("st_term", n_rows)):
            assert a.get(name) is None or tuple(a[name].shape) == (rows, D), name
        assert a.get("x16") is None or tuple(a["x16"].shape) == (n_rows, 128)
        assert a.get("rope") is None or (a["rope"].shape[0] >= e.row_off + e.Lout and tuple(a["rope"].shape[1:]) == (32, 2))
        assert a.get("tok_style") is None or tuple(a["tok_style"].shape) == (e.n_seq, D)
        assert tuple(a["x"].shape) == (n_rows, D) and a["x"].dtype == torch.float32
        out = {"x": a["x"].to(dev).contiguous().clone()}
        e.x = out["x"].data_ptr()
        f16 = lambda *shape: torch.full(shape, fill16, dtype=torch.int16, device=dev).view(torch.float16)     # noqa: E731
        if a.get("want_c16"):
            out["c16"] = f16(n_rows, D)
            e.c16 = out["c16"].data_ptr()
        if e.do_final:
            out["n16"] = f16(n_rows, D)
            e.n16 = out["n16"].data_ptr()
        if e.do_qkv:
            vt_ld = int(a["vt_ld"])
            out["qk"] = f16(n_rows, 2 * D)
            out["vt"] = f16(e.n_seq, D, vt_ld)
            e.qk, e.vt, e.vt_ld, e.vt_seq_stride = out["qk"].data_ptr(), out["vt"].data_ptr(), vt_ld, D * vt_ld
        if e.seam == 2:
            out["v32"] = torch.full((n_rows, max(e.ldv, 1)), fill32, dtype=torch.float32, device=dev)
            e.v32 = out["v32"].data_ptr()
        _lib.check(_lib.lib().svc_op_dit_panel(C.byref(e), _lib.stream_ptr()))
    return out


def conv_transpose1d_cl(x, w, bias, stride, dtype="f32"):
    """x (B, L, Cin), w (Cin, Cout, k = 2*stride) -> (B, L*stride, Cout); padding = stride // 2."""
    B, L, Cin = x.shape
    _, Cout, k = w.shape
    dev = x.device
    with torch.cuda.device(dev):
        x, w = _lib.f32c(x), _lib.f32c(w)
        b = _lib.f32c(bias) if bias is not None else None
        y = torch.empty(B, L * stride, Cout, device=dev)
        _lib.check(_lib.lib().svc_op_conv_transpose1d(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), B, L, Cin, Cout,
                                                      k, stride, {"f16": 0, "f32": 1, "f16x3": 2}[dtype], _lib.stream_ptr()))
    return y


def attention(q, k, v, kv_lens=None):
    """q,k,v (N, T, H, 64) fp32 -> softmax(q k^T / 8, keys < kv_len) v."""
    N, T, H, hd = q.shape
    assert hd == 64
    dev = q.device
    with torch.cuda.device(dev):
        q, k, v = _lib.f32c(q), _lib.f32c(k), _lib.f32c(v)
        out = torch.empty_like(q)
        lens = _lib.i64_host(kv_lens)
        _lib.check(_lib.lib().svc_op_attention(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), N, T, H, lens,
                                               _lib.stream_ptr()))
    return out


def attention_x3(q, k, v, kv_lens, Tq=None, q_start=0, out=None):
    """Mirror of svc_op_attention_x3 (include/seedvc_hip.h): the split-precision (fp16x3) attention of the DiT's precision 2.
    q, k, v (n_seq, seq_rows, H, 64) fp32, RoPE already applied -> softmax(q k^T / 8, keys < kv_lens[seq]) v for the query rows
    [q_start, Tq) of every sequence; the other rows of `out` (given, or NaN-filled) are left as they are."""
    n_seq, seq_rows, H, hd = q.shape
    assert hd == 64 and k.shape == q.shape and v.shape == q.shape
    dev = q.device
    with torch.cuda.device(dev):
        q, k, v = _lib.f32c(q), _lib.f32c(k), _lib.f32c(v)
        if out is None:
            out = torch.full_like(q, float("nan"))
        lens = _lib.i64_host([int(x) for x in kv_lens])
        _lib.check(_lib.lib().svc_op_attention_x3(_lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(out), n_seq, seq_rows, H,
                                                  seq_rows if Tq is None else int(Tq), int(q_start), lens, _lib.stream_ptr()))
    return out


def attention_ex(a, device="cuda:0", fill16=0x6A5A, fill32=-777.25):
    """Test aid over svc_op_attention_ex (include/seedvc_hip.h): ONE attention launch on buffers already in the kernels' layout.
    `a` maps the fields of svc_attention_t to ints and fp16 CPU or device tensors, taken exactly as given: either qk
    (n_seq * seq_rows, ld_qk) with q at column q_col (default 0) and k at column k_col (default H * 64), or q and k
    (n_seq * seq_rows, ld_qk) each; vt (n_seq, H * 64, vt_ld); kv_len a list of n_seq ints or None (then kv_len_const);
    out32 truthy for the fp32 output; ld_out (default H * 64).  Returns the whole output buffer (n_seq * seq_rows, ld_out): fp16
    filled with the bit pattern fill16, or fp32 filled with fill32, wherever the launch does not write."""
    import ctypes as C
    dev = torch.device(device)
    H, n_rows = int(a["H"]), int(a["n_seq"]) * int(a["seq_rows"])
    with torch.cuda.device(dev):
        e = _lib.Attention()
        put = lambda t: t.to(dev).contiguous()     # noqa: E731
        if a.get("qk") is not None:
            qk = put(a["qk"])
            keep = [qk]
            assert qk.dtype == torch.float16 and qk.dim() == 2 and qk.shape[0] == n_rows
            e.ld_qk = qk.shape[1]
            e.q = qk.data_ptr() + 2 * int(a.get("q_col", 0))
            e.k = qk.data_ptr() + 2 * int(a.get("k_col", H * 64))
        else:
            q, k = put(a["q"]), put(a["k"])
            keep = [q, k]
            assert q.dtype == torch.float16 and k.dtype == torch.float16 and q.shape == k.shape and q.dim() == 2 and q.shape[0] == n_rows
            e.ld_qk, e.q, e.k = q.shape[1], q.data_ptr(), k.data_ptr()
        vt = put(a["vt"])
        keep.append(vt)
        assert vt.dtype == torch.float16 and vt.dim() == 3 and vt.shape[0] == int(a["n_seq"])
        e.vt, e.vt_ld, e.vt_seq_stride = vt.data_ptr(), vt.shape[2], vt.shape[1] * vt.shape[2]
        for name in ("n_seq", "H", "seq_rows", "Tq", "q_start", "kv_len_const", "vt_perm", "qt_form"):
            setattr(e, name, int(a.get(name) or 0))
        lens = _lib.i64_host(a.get("kv_len"))
        if lens is not None:
            assert len(lens) == e.n_seq
            e.kv_len = C.cast(lens, C.POINTER(C.c_int64))
        e.ld_out = int(a.get("ld_out") or H * 64)
        if a.get("out32"):
            out = torch.full((n_rows, e.ld_out), fill32, dtype=torch.float32, device=dev)
            e.out32 = out.data_ptr()
        else:
            out = torch.full((n_rows, e.ld_out), fill16, dtype=torch.int16, device=dev).view(torch.float16)
            e.out = out.data_ptr()
        _lib.check(_lib.lib().svc_op_attention_ex(C.byref(e), _lib.stream_ptr()))
    return out


def _i32_field(values, n, what):
    """list of n ints (or None) -> (HOST int32 array kept alive by the caller, pointer for a struct field)"""
    import ctypes as C
    if values is None:
        return None, None
    assert len(values) == n, what
    arr = _lib.i32_host([int(v) for v in values])
    return arr, C.cast(arr, C.POINTER(C.c_int32))


def act_cl(x, C, ldy, taps=None, a=None, inv_b=None, out="f32", lo=None, mode=0, slope=0.0, lens=None, device="cuda:0", guard=8,
           fill16=0x6A5A, fill32=-777.25):
    """Test aid over svc_op_act_cl (include/seedvc_hip.h): ONE act_cl_launch, every argument as given.
    x (B, L, ldx) fp32 (it may hold NaN wherever the kernel must not read); C channels; taps (12,), a, inv_b (C,) fp32 or None;
    out "f32" | "f16"; lo None | "f16" | "p8" (the fp16 residual or the fp8 byte pair); lens a list of B ints or None.
    x sits between `guard` rows of NaN on the device.  Returns (hi, lo, guard): the WHOLE plane buffers (guard + B * L + guard,
    ldy), fp32 or int16 words, guard rows in front and behind included, holding fill32 / the bit pattern fill16 wherever the launch
    did not write; lo is None when not asked for."""
    import ctypes as Ct
    dev = torch.device(device)
    B, L, ldx = x.shape
    assert x.dtype == torch.float32 and out in ("f32", "f16") and lo in (None, "f16", "p8") and (guard * ldx) % 2 == 0
    with torch.cuda.device(dev):
        e = _lib.ActCl()
        xg = torch.full((guard + B * L + guard, ldx), float("nan"), dtype=torch.float32, device=dev)
        xg[guard:guard + B * L] = x.reshape(B * L, ldx).to(dev)
        keep = [xg]
        e.x = xg.data_ptr() + 4 * guard * ldx

        def plane():
            if out == "f32":
                return torch.full((guard + B * L + guard, ldy), fill32, dtype=torch.float32, device=dev)
            return torch.full((guard + B * L + guard, ldy), fill16, dtype=torch.int16, device=dev)
        esz = 4 if out == "f32" else 2
        hi = plane()
        e.y_hi = hi.data_ptr() + esz * guard * ldy
        p_lo = None
        if lo is not None:
            p_lo = plane()
            e.y_lo = p_lo.data_ptr() + esz * guard * ldy
        e.ldx, e.ldy, e.out_f16, e.lo_fmt = ldx, ldy, int(out == "f16"), int(lo == "p8")
        if taps is not None:
            e.taps = (Ct.c_float * 12)(*[float(v) for v in taps.reshape(12).tolist()])
        for name, t in (("a", a), ("inv_b", inv_b)):
            if t is not None:
                assert tuple(t.shape) == (C,) and t.dtype == torch.float32, name
                keep.append(t.to(dev).contiguous())
                setattr(e, name, keep[-1].data_ptr())
        e.B, e.C, e.L, e.mode, e.slope = B, C, L, mode, slope
        arr, p = _i32_field(lens, B, "lens")
        if p is not None:
            e.lens = p
        _lib.check(_lib.lib().svc_op_act_cl(Ct.byref(e), _lib.stream_ptr()))
    return hi, p_lo, guard


_HIFT_SCALARS_I = ("stage", "B", "n_utt", "NH", "up", "S", "S_in", "F", "Lw", "ld", "C", "vd", "mode")
_HIFT_SCALARS_F = ("sr", "sine_amp", "noise_std", "voiced_thr", "limit", "slope")


def hift_signal(a, device="cuda:0", fill16=0x6A5A, fill32=-777.25):
    """Test aid over svc_op_hift_signal (include/seedvc_hip.h): ONE HiFT signal stage through the model's launcher.
    `a` maps the fields of svc_hift_signal_t: ints and floats; `in`, phase0, noise, lin_w, lin_b as fp32 CPU or device tensors
    (None = absent), taken as given; src, len, lw, nf as lists of B ints or None.  The output buffer is allocated here in the
    stage's shape (1: (B, S up), 2: (B, F, ld), 3: (B F, 16), 4: (n_utt, Lw), 5: (B, S, ld), 6: (B S, ld)), fp32 holding fill32 or,
    for the fp16 forms of stages 5 and 6 (vd != 1), int16 words holding the bit pattern fill16.  Returns (out, out_lo): the whole
    buffers; out_lo only for vd 2 | 3, else None."""
    import ctypes as C
    dev = torch.device(device)
    with torch.cuda.device(dev):
        e = _lib.HiftSignal()
        for name in _HIFT_SCALARS_I:
            setattr(e, name, int(a.get(name) or 0))
        for name in _HIFT_SCALARS_F:
            setattr(e, name, float(a.get(name) or 0.0))
        keep = []
        for name in ("in", "phase0", "noise", "lin_w", "lin_b"):
            t = a.get(name)
            if t is not None:
                assert t.dtype == torch.float32, name
                keep.append(t.to(dev).contiguous())
                setattr(e, name, keep[-1].data_ptr())
        for name in ("src", "len", "lw", "nf"):
            arr, p = _i32_field(a.get(name), e.B, name)
            if p is not None:
                keep.append(arr)
                setattr(e, name, p)
        shape = {1: (e.B, e.S * e.up), 2: (e.B, e.F, e.ld), 3: (e.B * e.F, 16), 4: (e.n_utt, e.Lw), 5: (e.B, e.S, e.ld),
                 6: (e.B * e.S, e.ld)}[e.stage]
        half_out = e.stage >= 5 and e.vd != 1
        new = lambda: (torch.full(shape, fill16, dtype=torch.int16, device=dev) if half_out     # noqa: E731
                       else torch.full(shape, fill32, dtype=torch.float32, device=dev))
        out, out_lo = new(), None
        e.out = out.data_ptr()
        if half_out and e.vd in (2, 3):
            out_lo = new()
            e.out_lo = out_lo.data_ptr()
        _lib.check(_lib.lib().svc_op_hift_signal(C.byref(e), _lib.stream_ptr()))
    return out, out_lo


_AR_SLOT_I = ("cnt", "done", "max_new", "min_before_eos", "eos", "has_noise")
_AR_SLOT_F = ("temperature", "top_p", "rep_pen")


def ar_sampler(a, device="cuda:0", guard=2, fill32=-777.25, fill_tok=-7777):
    """Test aid over svc_op_ar_sampler (include/seedvc_hip.h): ONE launch of the AR sampler, in the form a["form"].
    form 0: logits (V,), prev (list of ints or None), suppress, rep_pen, temperature, top_p, exp_noise (V,) or None with seed and
            step, probs (bool).  Returns dict(idx, probs).
    form 1: logits (V,), toks (max_new,) int32, noise (max_new, V) or None, emb (V, D), pos [input, kv], and the scalars cnt,
            min_before_eos, eos, temperature, top_p, rep_pen, seed; probs (bool).  Returns dict(cnt, pos, toks, next_x, probs).
    form 2: logits (B, V), toks (B, max_new) int32, noise (B, max_new, V) or None, emb (V, D), pos [[input] * B, [kv] * B], Lmax
            and lists of B values: cnt, done, max_new, min_before_eos, eos, has_noise, temperature, top_p, rep_pen, seed.
            Returns dict(cnt, done, pos, toks, next_x).
    Every returned buffer is the WHOLE device buffer with `guard` canary rows in front and behind (probs, next_x: fill32; toks:
    fill_tok); next_x of form 2 has Bp = B rounded up to 16 rows between the guards, all holding fill32 before the launch."""
    import ctypes as C
    dev = torch.device(device)
    form = int(a["form"])
    with torch.cuda.device(dev):
        e = _lib.ArSampler()
        keep = []

        def put(t, dtype):
            keep.append(t.to(dev, dtype).contiguous())
            return keep[-1]

        def guarded(rows, cols, fill, dtype):
            keep.append(torch.full((guard + rows + guard, cols), fill, dtype=dtype, device=dev))
            return keep[-1]

        lg = a["logits"]
        V = lg.shape[-1]
        e.form, e.V = form, V
        B = lg.shape[0] if form == 2 else 1
        Bp = (B + 15) // 16 * 16
        if form == 2:
            rows = torch.full((Bp, V), float("nan"), dtype=torch.float32)
            rows[:B] = lg
            lg = rows
        e.logits = put(lg, torch.float32).data_ptr()
        out = {}
        if form != 2 and a.get("probs"):
            out["probs"] = guarded(1, V, fill32, torch.float32)
            e.probs_out = out["probs"].data_ptr() + 4 * guard * V
        if form == 0:
            prev = a.get("prev")
            if prev is not None and len(prev):
                e.prev = put(torch.tensor([int(v) for v in prev], dtype=torch.int32), torch.int32).data_ptr()
                e.n_prev = len(prev)
            sup = a.get("suppress")
            e.suppress = -1 if sup is None else int(sup)
            e.rep_pen, e.temperature, e.top_p = float(a["rep_pen"]), float(a["temperature"]), float(a["top_p"])
            if a.get("exp_noise") is not None:
                e.exp_noise = put(a["exp_noise"], torch.float32).data_ptr()
            e.seed, e.step = int(a.get("seed") or 0), int(a.get("step") or 0)
            idx = torch.full((1,), fill_tok, dtype=torch.int32, device=dev)
            e.idx_out = idx.data_ptr()
        else:
            emb = put(a["emb"], torch.float32)
            D = emb.shape[1]
            toks_in = a["toks"].reshape(B, -1)
            max_new = toks_in.shape[1]
            e.D, e.B, e.max_new, e.Lmax = D, B, max_new, int(a.get("Lmax") or 0)
            e.emb = emb.data_ptr()
            toks = guarded(B, max_new, fill_tok, torch.int32)
            toks[guard:guard + B] = toks_in.to(dev, torch.int32)
            e.toks = toks.data_ptr() + 4 * guard * max_new
            next_x = guarded(Bp if form == 2 else 1, D, fill32, torch.float32)
            e.next_x = next_x.data_ptr() + 4 * guard * D
            if a.get("noise") is not None:
                e.noise = put(a["noise"], torch.float32).data_ptr()
            host = {}
            slot = lambda name: a[name] if form == 2 else [a.get(name) or 0]      # noqa: E731
            for name in _AR_SLOT_I:
                host[name] = _lib.i32_host([int(v) for v in slot(name)])
                setattr(e, "s_" + name, C.cast(host[name], C.POINTER(C.c_int32)))
            for name in _AR_SLOT_F:
                host[name] = (C.c_float * B)(*[float(v) for v in slot(name)])
                setattr(e, "s_" + name, C.cast(host[name], C.POINTER(C.c_float)))
            host["seed"] = (C.c_uint64 * B)(*[int(v) for v in slot("seed")])
            e.s_seed = C.cast(host["seed"], C.POINTER(C.c_uint64))
            p = a["pos"] if form == 2 else [[a["pos"][0]], [a["pos"][1]]]
            host["pos"] = _lib.i32_host([int(v) for v in list(p[0]) + list(p[1])])
            e.pos = C.cast(host["pos"], C.POINTER(C.c_int32))
        _lib.check(_lib.lib().svc_op_ar_sampler(C.byref(e), _lib.stream_ptr()))
        if form == 0:
            out["idx"] = int(idx.item())
        else:
            out["toks"], out["next_x"] = toks, next_x
            cnt, pos = list(host["cnt"]), [list(host["pos"])[:B], list(host["pos"])[B:]]
            if form == 2:
                out.update(cnt=cnt, done=list(host["done"]), pos=pos)
            else:
                out.update(cnt=cnt[0], pos=[pos[0][0], pos[1][0]])
    out["guard"] = guard
    return out


class _ArOpBuffers:
    """The device buffers of one ar_attn / ar_linear call: inputs as given, outputs and caches with canary guard rows."""

    def __init__(self, dev, guard, fill32, fill16):
        self.dev, self.guard, self.fill32, self.fill16, self.keep = dev, guard, fill32, fill16, []

    def put(self, t, dtype=torch.float32):
        self.keep.append(t.to(self.dev, dtype).contiguous())
        return self.keep[-1].data_ptr()

    def padded(self, t, rows, pad, dtype=torch.float32):
        """t (r, cols) in the first rows of a (rows, cols) buffer whose other rows hold `pad`"""
        buf = torch.full((rows, t.shape[1]), pad, dtype=dtype)
        buf[:t.shape[0]] = t.to(dtype)
        return self.put(buf, dtype)

    def guarded(self, rows, cols, dtype=torch.float32, init=None):
        """(guard + rows + guard, cols) holding the fill (rows [guard, guard + len(init)) = init); returns (tensor, pointer to row guard)"""
        g = self.guard
        t = torch.full((g + rows + g, cols), self.fill16 if dtype == torch.float16 else self.fill32, dtype=dtype, device=self.dev)
        if init is not None:
            t[g:g + init.shape[0]] = init.to(self.dev, dtype)
        self.keep.append(t)
        return t, t.data_ptr() + g * cols * t.element_size()

    def caches(self, a):
        """kc, vc (n_slots, Hkv, Lmax, 64) -> guarded (guard + n_slots Hkv Lmax + guard, 64) buffers"""
        kc, pk = self.guarded(a["kc"].numel() // 64, 64, init=a["kc"].reshape(-1, 64))
        vc, pv = self.guarded(a["vc"].numel() // 64, 64, init=a["vc"].reshape(-1, 64))
        return kc, pk, vc, pv


def ar_attn(a, device="cuda:0", guard=2, fill32=-777.25, fill16=-777.0):
    """Test aid over svc_op_ar_attn (include/seedvc_hip.h): ONE launch of a cache-touching AR kernel, a["kind"] = 0 ar_attn, 1
    dec_attn2, 2 battn, 3 ar_prefill_attn, 4 ar_rope_cache, 5 ar_rope_cache_ragged.  a: H, Hkv, Lmax; x (rows, cols) fp32 (q |
    qkv_raw (1, D + 2 kvd) | qkv); kc, vc (n_slots, Hkv, Lmax, 64) fp32; rope (Lmax, 32, 2); slots (list); seq_S (list, kinds 3
    and 5); pos [[input_pos ...], [kv_pos ...]]; kind 1: hres (D,), eps, wo (D, D) fp16; kind 2: pad = what the rows n .. Bp - 1 of
    q hold (NaN).  Returns dict(y16 | q_out | part, kc, vc, guard): the WHOLE device buffers, `guard` canary rows in front and
    behind (fp32: fill32, fp16: fill16); y16 of kind 2 has Bp rows between the guards; kc, vc are (guard + n_slots Hkv Lmax +
    guard, 64)."""
    import ctypes as C
    dev = torch.device(device)
    kind = int(a["kind"])
    with torch.cuda.device(dev):
        b = _ArOpBuffers(dev, guard, fill32, fill16)
        e = _lib.ArAttn()
        e.kind, e.H, e.Hkv, e.Lmax = kind, int(a["H"]), int(a["Hkv"]), int(a["Lmax"])
        D = 64 * e.H
        x = a["x"]
        pos = a["pos"]
        R = len(pos[0])
        e.n_slots = a["kc"].shape[0]
        e.n = len(a["slots"]) if kind in (2, 3, 5) else R
        rows = (e.n + 15) // 16 * 16 if kind == 2 else R
        e.x = b.padded(x, rows, a.get("pad", float("nan"))) if kind == 2 else b.put(x)
        e.ldq = x.shape[1]
        out = {"guard": guard}
        out["kc"], e.kc, out["vc"], e.vc = b.caches(a)
        if a.get("rope") is not None:
            e.rope = b.put(a["rope"])
        host = [_lib.i32_host([int(v) for v in a["slots"]]), _lib.i32_host([int(v) for v in list(pos[0]) + list(pos[1])])]
        e.slots, e.pos = C.cast(host[0], C.POINTER(C.c_int32)), C.cast(host[1], C.POINTER(C.c_int32))
        if a.get("seq_S") is not None:
            host.append(_lib.i32_host([int(v) for v in a["seq_S"]]))
            e.seq_S = C.cast(host[-1], C.POINTER(C.c_int32))
        if kind in (0, 2, 3):
            out["y16"], e.y16 = b.guarded(rows, D, torch.float16)
        if kind in (4, 5):
            out["q_out"], e.q_out = b.guarded(rows, D)
        if kind == 1:
            e.hres, e.eps, e.wo = b.put(a["hres"]), float(a["eps"]), b.put(a["wo"], torch.float16)
            out["part"], e.part = b.guarded(e.H, D)
        _lib.check(_lib.lib().svc_op_ar_attn(C.byref(e), _lib.stream_ptr()))
    return out


_AR_ROLES = {"qkv": 0, "wo": 1, "w13": 2, "w2": 3, "head": 4}


def ar_linear(a, device="cuda:0", guard=2, fill32=-777.25, fill16=-777.0, w_pad=0.5):
    """Test aid over svc_op_ar_linear (include/seedvc_hip.h): ONE launch of a skinny AR linear.  a: path (0 GEMV pair, 1 batched, 2
    the B = 1 decode step), role ("qkv", "wo", "w13", "w2", "head"), D, I, H, Hkv, V; x (rows, K) fp32 or fp16 as the role takes it;
    W (N, K) fp16 (packed here into N rounded up to 128 rows, the others holding w_pad); gamma, eps; res (rows, D) and inplace (the
    output buffer starts as res and res points at it); path 2: W2, part (H, D); the qkv role of paths 0 and 1: kc, vc, rope, slots,
    pos, Lmax as in ar_attn.  Path 1 pads x and res to Bp = rows rounded up to 16 with a["pad"] (NaN).  Returns dict(out32 | out16 |
    out2 | q_out, kc, vc, guard): the WHOLE buffers with `guard` canary rows in front and behind; path 1 outputs have Bp rows."""
    import ctypes as C
    dev = torch.device(device)
    path, role = int(a["path"]), _AR_ROLES[a["role"]]
    with torch.cuda.device(dev):
        b = _ArOpBuffers(dev, guard, fill32, fill16)
        e = _lib.ArLinear()
        e.path, e.role = path, role
        for n in ("D", "I", "H", "Hkv", "V"):
            setattr(e, n, int(a[n]))
        D, I, V = e.D, e.I, e.V
        Nqkv = D + 128 * e.Hkv
        x = a["x"].reshape(-1, a["x"].shape[-1])
        S = x.shape[0]
        e.rows = S
        rows = (S + 15) // 16 * 16 if path == 1 else S
        pad = a.get("pad", float("nan"))
        e.x = b.padded(x, rows, pad, x.dtype)

        def packed(w):
            buf = torch.full(((w.shape[0] + 127) // 128 * 128, w.shape[1]), w_pad, dtype=torch.float16)
            buf[:w.shape[0]] = w
            return b.put(buf, torch.float16)
        e.W = packed(a["W"])
        if a.get("W2") is not None:
            e.W2 = packed(a["W2"])
        if a.get("gamma") is not None:
            e.gamma, e.eps = b.put(a["gamma"]), float(a["eps"])
        out = {"guard": guard}
        host = []
        if role == 0 and path != 2:
            e.Lmax, e.n_slots = int(a["Lmax"]), a["kc"].shape[0]
            out["kc"], e.kc, out["vc"], e.vc = b.caches(a)
            e.rope = b.put(a["rope"])
            host = [_lib.i32_host([int(v) for v in a["slots"]]), _lib.i32_host([int(v) for v in list(a["pos"][0]) + list(a["pos"][1])])]
            e.slots, e.pos = C.cast(host[0], C.POINTER(C.c_int32)), C.cast(host[1], C.POINTER(C.c_int32))
            out["q_out"], e.q_out = b.guarded(rows, D)
        else:
            cols = {0: Nqkv, 1: D, 3: D, 4: V}.get(role)
            res = a.get("res")
            if res is not None:
                res = res.reshape(-1, D)
                if path == 1:
                    res = torch.cat([res, torch.full((rows - S, D), pad)])
            if role == 2:
                out["out16"], e.out16 = b.guarded(rows, I, torch.float16)
            elif a.get("inplace"):
                out["out32"], e.out32 = b.guarded(rows, cols, init=res)
                e.res = e.out32
            else:
                out["out32"], e.out32 = b.guarded(rows, cols)
                if res is not None:
                    e.res = b.put(res)
            if path == 2 and role in (1, 2):
                out["out2"], e.out2 = b.guarded(1, Nqkv if role == 1 else D)
            if a.get("part") is not None:
                e.part = b.put(a["part"])
        _lib.check(_lib.lib().svc_op_ar_linear(C.byref(e), _lib.stream_ptr()))
    return out


_KGEMM_INT = ("dtype", "epi", "form", "M", "N", "Lout", "a_seq_rows", "a_off", "a_stride", "a_len", "pad_mode", "reflect_min", "c_seq_rows",
              "c_off", "post_n", "act", "post_relu", "vec_ok", "rope_D", "vt_mode", "check_only")
_KGEMM_F32 = ("out_scale", "act_slope", "q_scale")


def kgemm(a, device="cuda:0", guard=2, fill32=-777.25, fill16=0x6A5A, w_pad=0.5):
    """Test aid over svc_op_kgemm (include/seedvc_hip.h): ONE kgemm_launch on unpacked fp32 operands.  `a` maps the scalars of
    svc_kgemm_t to ints / floats, plus: src (list of up to 4 (rows, K) tensors), taps (list of (source index, shift)), W (N, sum
    of the taps' K; packed into N rounded up to 256 rows, the others holding w_pad), bias (N,), rowvec and gate ((N,) = ld 0, or
    (nseq, N)), res and res2 ((c_rows, ldc), or "c32": the output itself, which then starts as a["c_init"]), post_a and post_ib
    (post_n,), rope (rows, 32, 2), seq_len and a_seq_map (lists), ldc, c_rows (default nseq * c_seq_rows), vt_ld, and want_c32 /
    want_c16 / want_c16_lo.  Returns dict(c32 | c16 | c16_lo (guard + c_rows + guard, ldc), vt (guard + nseq rope_D + guard,
    vt_ld), guard): the WHOLE device buffers, fp32 holding fill32 and the 16-bit ones (returned as float16) the bit pattern
    fill16 wherever the launch did not write."""
    import ctypes as C
    dev = torch.device(device)
    with torch.cuda.device(dev):
        b = _ArOpBuffers(dev, guard, fill32, fill16)
        e = _lib.KGemm()
        for n in _KGEMM_INT:
            setattr(e, n, int(a.get(n) or 0))
        for n in _KGEMM_F32:
            setattr(e, n, float(a.get(n) or 0.0))
        src = a["src"]
        assert 1 <= len(src) <= 4 and 1 <= len(a["taps"]) <= 48
        e.n_src = len(src)
        for i, t in enumerate(src[:4]):
            assert t.dim() == 2 and t.dtype == torch.float32
            e.a_src[i], e.a_rows[i], e.a_K[i] = b.put(t), t.shape[0], t.shape[1]
        e.n_taps = len(a["taps"])
        for t, (i, shift) in enumerate(a["taps"][:48]):
            e.tap_src[t], e.tap_shift[t], e.tap_K[t] = int(i), int(shift), src[i].shape[1] if 0 <= i < len(src) else 0
        W = a["W"]
        assert W.dim() == 2 and W.shape[0] == e.N and W.dtype == torch.float32
        # the entry point strides W by the sum of the taps' K and takes the vectors' sizes on trust: they are held here
        assert W.shape[1] == sum(src[i].shape[1] for i, _ in a["taps"] if 0 <= i < len(src)), "W has the taps' K columns"
        assert a.get("bias") is None or a["bias"].numel() >= e.N, "bias has N entries"
        for n in ("post_a", "post_ib"):
            assert a.get(n) is None or a[n].numel() >= e.post_n, n + " has post_n entries"
        wbuf = torch.full(((e.N + 255) // 256 * 256, W.shape[1]), w_pad, dtype=torch.float32)
        wbuf[:e.N] = W
        e.w, e.w_rows = b.put(wbuf), wbuf.shape[0]
        nseq = -(-e.M // max(e.Lout, 1))
        host = []
        for n in ("seq_len", "a_seq_map"):
            if a.get(n) is not None:
                assert len(a[n]) == nseq, n
                host.append(_lib.i32_host([int(v) for v in a[n]]))
                setattr(e, n, C.cast(host[-1], C.POINTER(C.c_int32)))
        e.ldc = ldc = int(a["ldc"])
        e.c_rows = c_rows = int(a.get("c_rows") or nseq * e.c_seq_rows)
        for n in ("bias", "post_a", "post_ib"):
            if a.get(n) is not None:
                setattr(e, n, b.put(a[n]))
        for n in ("rowvec", "gate"):
            t = a.get(n)
            if t is not None:
                assert tuple(t.shape) in ((e.N,), (nseq, e.N)), n
                setattr(e, n, b.put(t))
                setattr(e, "ld_" + n, 0 if t.dim() == 1 else e.N)
        out = {"guard": guard}

        def plane():
            t = torch.full((guard + c_rows + guard, ldc), fill16, dtype=torch.int16, device=dev).view(torch.float16)
            b.keep.append(t)
            return t, t.data_ptr() + guard * ldc * 2
        if a.get("want_c32"):
            init = a.get("c_init")
            assert init is None or tuple(init.shape) == (c_rows, ldc)
            out["c32"], e.c32 = b.guarded(c_rows, ldc, init=init)
        if a.get("want_c16"):
            out["c16"], e.c16 = plane()
        if a.get("want_c16_lo"):
            out["c16_lo"], e.c16_lo = plane()
        for n in ("res", "res2"):
            t = a.get(n)
            if isinstance(t, str):
                assert t == "c32" and a.get("want_c32") and a.get("c_init") is not None, n
                setattr(e, n, e.c32)
            elif t is not None:
                assert tuple(t.shape) == (c_rows, ldc), n
                setattr(e, n, b.put(t))
        if a.get("rope") is not None:
            assert tuple(a["rope"].shape[1:]) == (32, 2) and a["rope"].dtype == torch.float32
            e.rope, e.rope_rows = b.put(a["rope"]), a["rope"].shape[0]
        if e.epi == 3:
            e.vt_ld = vt_ld = int(a["vt_ld"])
            rows = nseq * e.rope_D
            t = torch.full((guard + rows + guard, vt_ld), fill16, dtype=torch.int16, device=dev).view(torch.float16)
            b.keep.append(t)
            out["vt"], e.vt = t, t.data_ptr() + guard * vt_ld * 2
        _lib.check(_lib.lib().svc_op_kgemm(C.byref(e), _lib.stream_ptr()))
    return out


def permute_vt(vt, mode):
    """Test aid over svc_op_permute_vt: a copy of the natural-order V^T buffer vt (rows, vt_ld) fp16 on the device, its columns
    permuted in place into order `mode` by attention_permute_vt."""
    assert vt.is_cuda and vt.dtype == torch.float16 and vt.dim() == 2
    out = vt.contiguous().clone()
    with torch.cuda.device(vt.device):
        _lib.check(_lib.lib().svc_op_permute_vt(out.data_ptr(), out.shape[0], out.shape[1], int(mode), _lib.stream_ptr()))
    return out


LR_STAGES = {"gather": 0, "gn_stats": 1, "gn_mish": 2, "mask_copy": 3}
LR_GN_PARTS = 32          # lr.hip's LR_GN_PARTS: the partials of the GroupNorm statistics per utterance


def lr_stage(a, device="cuda:0", guard=2, fill32=-777.25):
    """Test aid over svc_op_lr (include/seedvc_hip.h): ONE launch of one length-regulator kernel.  a: stage (a key of LR_STAGES),
    tout_max, C, ld, ylens (list; B = its length), plus
      gather     feat (B, tin_max, ld_feat) fp32 | tokens (B, tin_max) int64 + emb (codebook, C); in_lens (list), interpolate;
                 f0_emb (n_bins, C) with f0 (B, tf0_max) + f0_lens (list), or with f0_mask (C,)
      gn_stats   x (B, tout_max, ld)
      gn_mish    x (B, tout_max, ld), stats (B, 32, 2) float64, gamma (C,), beta (C,), eps
      mask_copy  x (B, tout_max, ld), N, ld_out
    Returns dict(guard, inputs = {name: the device buffer of every tensor the kernel only reads, AFTER the launch}, and the
    written buffer WHOLE, `guard` canary rows in front and behind holding fill32: x (guard + B tout_max + guard, ld) for gather
    and gn_mish (in place on a copy of a["x"]), stats (guard + 32 B + guard, 2) float64, out (guard + B tout_max + guard, ld_out))."""
    import ctypes as C
    dev = torch.device(device)
    with torch.cuda.device(dev):
        b = _ArOpBuffers(dev, guard, fill32, 0)
        e = _lib.LrOp()
        stage = a["stage"]
        e.stage = LR_STAGES[stage] if stage in LR_STAGES else int(stage)
        ylens = [int(v) for v in a["ylens"]]
        B = len(ylens)
        e.B, e.tout_max, e.C, e.ld = B, int(a["tout_max"]), int(a.get("C") or 0), int(a["ld"])
        rows = B * e.tout_max
        host = [_lib.i32_host(ylens)]
        e.ylens = C.cast(host[0], C.POINTER(C.c_int32))
        e.check_only = int(a.get("check_only") or 0)
        out, inputs = {"guard": guard}, {}

        def read_only(name, t, dtype=torch.float32):
            ptr = b.put(t, dtype)
            inputs[name] = b.keep[-1]
            return ptr

        def lens(name):
            assert len(a[name]) == B, name
            host.append(_lib.i32_host([int(v) for v in a[name]]))
            return C.cast(host[-1], C.POINTER(C.c_int32))
        if stage == "gather":
            if a.get("tokens") is not None:
                tok = a["tokens"]
                assert tok.dim() == 2 and tok.shape[0] == B and tuple(a["emb"].shape[1:]) == (e.C,)
                assert 0 <= int(tok.min()) and int(tok.max()) < a["emb"].shape[0], "tokens lie inside the table"
                e.tokens, e.emb, e.tin_max = read_only("tokens", tok, torch.int64), read_only("emb", a["emb"]), tok.shape[1]
            else:
                feat = a["feat"]
                assert feat.dim() == 3 and feat.shape[0] == B
                e.feat, e.ld_feat, e.tin_max = read_only("feat", feat), feat.shape[2], feat.shape[1]
            e.in_lens, e.interpolate = lens("in_lens"), int(a["interpolate"])
            if a.get("f0_emb") is not None:
                assert a["f0_emb"].dim() == 2 and a["f0_emb"].shape[1] == e.C
                e.f0_emb, e.n_bins = read_only("f0_emb", a["f0_emb"]), a["f0_emb"].shape[0]
                if a.get("f0_mask") is not None:
                    assert a["f0_mask"].numel() == e.C
                    e.f0_mask = read_only("f0_mask", a["f0_mask"])
            if a.get("f0") is not None:
                assert a["f0"].dim() == 2 and a["f0"].shape[0] == B
                e.f0, e.tf0_max, e.f0_lens = read_only("f0", a["f0"]), a["f0"].shape[1], lens("f0_lens")
            out["x"], e.x = b.guarded(rows, e.ld)
        else:
            x = a["x"]
            assert tuple(x.shape) == (B, e.tout_max, e.ld) and x.dtype == torch.float32
            if stage == "gn_mish":
                out["x"], e.x = b.guarded(rows, e.ld, init=x.reshape(rows, e.ld))
            else:
                e.x = read_only("x", x)
            if stage == "gn_stats":
                out["stats"], e.stats = b.guarded(LR_GN_PARTS * B, 2, dtype=torch.float64)
            elif stage == "gn_mish":
                assert tuple(a["stats"].shape) == (B, LR_GN_PARTS, 2) and a["gamma"].numel() == e.C and a["beta"].numel() == e.C
                e.stats = read_only("stats", a["stats"], torch.float64)
                e.gamma, e.beta, e.eps = read_only("gamma", a["gamma"]), read_only("beta", a["beta"]), float(a["eps"])
            elif stage == "mask_copy":
                e.N, e.ld_out = int(a["N"]), int(a["ld_out"])
                out["out"], e.out = b.guarded(rows, e.ld_out)
        _lib.check(_lib.lib().svc_op_lr(C.byref(e), _lib.stream_ptr()))
        out["inputs"] = inputs
    return out


def rmsnorm(x, gamma, w=None, b=None, add_one=False):
    rows, D = x.shape
    dev = x.device
    with torch.cuda.device(dev):
        x, gamma = _lib.f32c(x), _lib.f32c(gamma)
        w = _lib.f32c(w) if w is not None else None
        b = _lib.f32c(b) if b is not None else None
        y = torch.empty_like(x)
        _lib.check(_lib.lib().svc_op_rmsnorm(_lib.ptr(x), _lib.ptr(gamma), _lib.ptr(w), _lib.ptr(b), int(add_one),
                                             _lib.ptr(y), rows, D, _lib.stream_ptr()))
    return y


CENSUS_COUNTS = ("n", "n_hi_clamp", "n_hi_sub", "n_lo_flush", "n_lo_clamp")
CENSUS_SUMS = ("s_hi2", "s_hi_err2", "s_lo2", "s_lo_err2")


def census_dict(c):
    """svc_census_t -> dict (counts as ints, max_hi and the four sums as floats)."""
    d = {k: int(getattr(c, k)) for k in CENSUS_COUNTS}
    d["max_hi"] = float(c.max_hi)
    d.update({k: float(getattr(c, k)) for k in CENSUS_SUMS})
    return d


def range_census(hi, lo, C, lens=None, device="cuda:0"):
    """Test aid over svc_op_range_census (include/seedvc_hip.h): ONE range census of the fp16 operand planes hi, lo (B, L, ld)
    (they may hold NaN in rows at and above lens[b]); C live channels; lens a list of B ints or None.  Returns the record as a
    dict (census_dict)."""
    import ctypes as Ct
    dev = torch.device(device)
    B, L, ld = hi.shape
    assert hi.dtype == lo.dtype == torch.float16 and hi.shape == lo.shape
    with torch.cuda.device(dev):
        h, l = hi.to(dev).contiguous(), lo.to(dev).contiguous()
        e, out = _lib.RangeCensus(), _lib.Census()
        e.hi, e.lo, e.B, e.L, e.C, e.ld = h.data_ptr(), l.data_ptr(), B, L, C, ld
        arr, p = _i32_field(lens, B, "lens")
        if p is not None:
            e.lens = p
        e.out = Ct.pointer(out)
        _lib.check(_lib.lib().svc_op_range_census(Ct.byref(e), _lib.stream_ptr()))
    return census_dict(out)


def weight_census(w, device="cuda:0"):
    """Test aid over svc_op_weight_census: w (Cout, Cin, k) fp32 packed as an fp16p8 model packs it -> (sums (Cout, 4) float64:
    sum w_hi^2, sum (w_hi - dq)^2, sum w_lo^2, sum (w_lo - dq)^2 per output channel, w8_exp)."""
    import ctypes as Ct
    dev = torch.device(device)
    Cout, Cin, k = w.shape
    with torch.cuda.device(dev):
        wd = _lib.f32c(w, dev)
        out = (Ct.c_double * (Cout * 4))()
        ex = Ct.c_int(0)
        _lib.check(_lib.lib().svc_op_weight_census(_lib.ptr(wd), Cout, Cin, k, out, Ct.byref(ex), _lib.stream_ptr()))
    return torch.tensor(list(out), dtype=torch.float64).reshape(Cout, 4), ex.value
