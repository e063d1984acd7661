"""Float64 restatement of ONE launch of the fused DiT row-panel kernel (csrc/fused.hip) at op level, shared by test_host_panel.py
(which checks that the restatement can tell a right kernel from a subtly wrong one, and ties it to the oracle's blocks) and
test_gpu_panel.py (which holds the kernel to it through svc_op_dit_panel).  CPU only, plain torch ops.

A launch is described by a dict of arguments (`make_args`): the fields of svc_dit_panel_t, with CPU tensors for the operands.
ref_panel(args, dt) returns, for every output buffer the launch writes, the PRE-ROUNDING values in dt and the mask of written
elements.  Every sum is in dt; values are rounded to fp16 exactly where the kernel rounds (its MFMA operands) and nowhere else:
  P1     x1 = x + [gate_a *] half(Wo) ao
  norm   rs = rsqrt(mean(x^2) + eps); A = g (add_one + w) or g; n = half(x rs A + b)
  MLP    h = half(silu(half(W1) n) (half(W3) n)); x2 = x1 + [gate_f *] half(W2) h
  c16    half(x2), taken before the skip
  skip   x3 = bskip + half(Wskip[:, :D]) half(x2) + half(Wskip[:, D:]) skip_in
  final  n16 = half(norm_fin(x))
  head   v = half(W2h) half(silu(half(Wa) n16 + b0)) + b2 on columns < head_C; n16 is not written.  x is scratch behind the head:
         the gated form parks x1 there (the MLP accumulators need the registers), the ungated form leaves it alone
  QKV    n = half(attn_norm(x)); q = half(rope(half(Wq) n) q_scale); k = half(rope(half(Wk) n)); v = half(half(Wv) n) stored at
         vt[seq][d][vt_pos(pos, mode)]; RoPE on interleaved pairs with table row row_off + m % Lout
  merge  x[seq][pos] = token (pos < npre) | st_term + half(Wm[:, :C]) x16[seq][pos - npre] (data rows) | 0 (pad rows), then QKV
Local row m is buffer row (m // Lout) seq_rows + row_off + m % Lout.

The bound (see `bounds` and `excess`): with r the float64 pre-rounding value and e = 4 max(noise32) over that output of that
case, an fp32 output passes if |y - r| <= e and an fp16 output if |float(y) - r| <= ulp16(r) / 2 + e.  noise32 is the distance of
a float32 evaluation of this restatement from the float64 one: the kernel is an fp32-accumulate evaluation of the same rounded
operands, and what dominates either is an fp16 intermediate (n, h, half(x2)) landing on the other side of a rounding boundary.
Which intermediates do so depends on the summation order, so `noise32` does not rely on the flips one float32 run happens to
make: it rounds every intermediate that lies within its own fp32 noise of a boundary the other way as well (see there).
"""
import random

import torch

SEAM_NONE, SEAM_MERGE, SEAM_HEAD = 0, 1, 2
MERGE_K = 128                       # PANEL_MERGE_K: the width of an x16 row
MARGIN = 4.0                        # the project's margin for a bound made of a reference's own fp32 noise (kconv_cases.snake_err)
F16_OUTPUTS = ("c16", "n16", "qk", "vt")
F32_OUTPUTS = ("x", "v32")
OUTPUTS = ("x", "c16", "n16", "qk", "vt", "v32")
CANARY16 = 0x6A5A                   # a finite fp16 (3252.0) no output takes
CANARY32 = -777.25


def half(t):
    """fp16 rounding, returned in t's dtype"""
    return t.to(torch.float32).half().to(t.dtype)


def ulp16(r):
    """spacing of the fp16 values around |r| (float64): 2^(floor(log2 |r|) - 10), 2^-24 in the subnormal range and at zero"""
    a = r.double().abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10.0)


def vt_perm_pos(pos):
    """common.h: inside every group of 32 keys, key 16 h + 4 f + r -> position 8 f + 4 h + r"""
    return (pos & ~31) | (((pos >> 2) & 3) << 3) | (((pos >> 4) & 1) << 2) | (pos & 3)


def vt_perm_pos16(pos):
    """common.h: inside every group of 16 keys, key 8 a + 4 f + r -> position 8 f + 4 a + r (bits 2 and 3 swapped)"""
    return (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1)


def vt_pos(pos, mode):
    return vt_perm_pos16(pos) if mode == 2 else (vt_perm_pos(pos) if mode == 1 else pos)


def rope_table(n_pos, head_dim=64, base=10000.0):
    """oracle.rope_table (fp32 table), restated here so that this module needs no import path"""
    inv = 1.0 / (base ** (torch.arange(0, head_dim, 2).float() / head_dim))
    ang = torch.outer(torch.arange(n_pos).float(), inv)
    return torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1)


# ------------------------------------------------------------------------------------------------ the restatement
# Sabotages: what a subtly wrong kernel, packer or launcher would compute.  name -> when a case can show it.
SABOTAGES = {
    "w1 and w3 swapped": lambda a: a["do_post"],
    "gate_a left out": lambda a: a["do_post"] and a["gated"],
    "gate_f left out": lambda a: a["do_post"] and a["gated"],
    "add_one ignored": lambda a: a["add_one"] and a["mod"],
    # unit rows hide eps = 1e-5; the small rows (make_args) reach a norm directly unless a skip linear rebuilds them first
    "eps left out": lambda a: a["do_post"] or not a["do_skip"],
    "ungated residual added twice": lambda a: a["do_post"] and not a["gated"],
    "rope sin sign flipped": lambda a: a["do_qkv"],
    "rope without row_off": lambda a: a["do_qkv"] and a["row_off"] > 0,
    "rope on tile-shifted positions": lambda a: a["do_qkv"] and a["M"] > 16,
    "q_scale on k as well": lambda a: a["do_qkv"],
    "wskip halves swapped": lambda a: a["do_skip"],
    "c16 taken after the skip": lambda a: a["do_skip"] and a["want_c16"],
    "final norm with the attention-norm vectors": lambda a: a["do_final"],
    "head b0 after the silu": lambda a: a["seam"] == SEAM_HEAD,
    "merge data rows offset by one": lambda a: a["seam"] == SEAM_MERGE and a["npre"] > 0 and a["T"] > 1,
    "pad row keeps st_term": lambda a: a["seam"] == SEAM_MERGE and a["npre"] + a["T"] < a["Lout"],
    "vt_pos mode 1 for mode 2": lambda a: a["do_qkv"] and a["vt_mode"] == 2 and a["row_off"] + a["Lout"] > 4,
    "one mlp output tile dropped": lambda a: a["do_post"],
}


def rows_of(a):
    """buffer row, sequence and position of every local row"""
    m = torch.arange(a["M"])
    seq, l = m // a["Lout"], m % a["Lout"]
    return seq * a["seq_rows"] + a["row_off"] + l, seq, a["row_off"] + l


def _lin(w, v, dt):
    return v @ half(w.to(dt)).T


def _norm(x, g, w, b, a, dt, sab):
    eps = 0.0 if sab == "eps left out" else a["eps"]
    one = 0.0 if sab == "add_one ignored" else float(a["add_one"])
    rs = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + torch.tensor(eps, dtype=torch.float32).to(dt))
    A = torch.zeros(x.shape[-1], dtype=dt) if g is None else (g.to(dt) * (one + w.to(dt)) if w is not None else g.to(dt))
    return x * rs * A + (b.to(dt) if b is not None else 0.0)


def _silu(t):
    return t * torch.sigmoid(t)


def _rope(v, tab, pos, dt, flip):
    """v (M, D) as heads of 64 with interleaved pairs; tab (n_pos, 32, 2) fp32"""
    M, D = v.shape
    p = v.reshape(M, D // 64, 32, 2)
    c = tab[pos, :, 0].to(dt)[:, None, :]
    s = tab[pos, :, 1].to(dt)[:, None, :] * (-1.0 if flip else 1.0)
    return torch.stack([p[..., 0] * c - p[..., 1] * s, p[..., 1] * c + p[..., 0] * s], dim=-1).reshape(M, D)


STAGES = ("n_ffn", "h", "x2h", "n_fin", "s_head", "n_attn")      # the fp16 intermediates: MFMA operands built in registers


def flip_near_boundary(t, tol):
    """half(t), except that an element within tol of the midpoint of two fp16 values takes the one on the other side"""
    h = half(t)
    inf = torch.tensor(float("inf"), dtype=torch.float16)
    up = torch.nextafter(h.to(torch.float16), inf).to(t.dtype)
    dn = torch.nextafter(h.to(torch.float16), -inf).to(t.dtype)
    other = torch.where(t >= h, up, dn)
    return torch.where(((h + other) / 2 - t).abs() <= tol, other, h)


def ref_panel(a, dt=torch.float64, sab=None, flip=None, taps=None, force=None):
    """{output: (pre-rounding values in dt over the whole buffer, bool mask of the elements the launch writes)}
    taps: a dict that receives (pre-rounding values, rounded values) of every fp16 intermediate (STAGES).
    force: {stage: rounded values} used in place of this run's own (so that a float32 run shows each stage's local noise).
    flip = (stage, tol): that intermediate is rounded the other way wherever it lies within tol of a rounding boundary."""
    D, M = a["D"], a["M"]

    def rnd(stage, t):
        if force is not None and stage in force:
            h = force[stage].to(dt)
        else:
            h = flip_near_boundary(t, flip[1]) if flip is not None and flip[0] == stage else half(t)
        if taps is not None:
            taps[stage] = (t, h)
        return h
    rows, seq, pos = rows_of(a)
    n_rows = a["n_seq"] * a["seq_rows"]
    out = {}

    def put(name, vals, width, cols=None):
        buf = torch.zeros(n_rows, width, dtype=dt)
        mask = torch.zeros(n_rows, width, dtype=torch.bool)
        c = slice(0, width) if cols is None else cols
        buf[rows, c] = vals
        mask[rows, c] = True
        out[name] = (buf, mask)

    f16 = lambda t: t.to(dt)       # noqa: E731  fp16 operands hold their values exactly
    gated = bool(a["gated"])
    if a["seam"] == SEAM_MERGE:
        t = pos - a["npre"]
        is_data = (t >= 0) & (t < a["T"])
        tc = t.clamp(0, a["T"] - 1)
        if sab == "merge data rows offset by one":
            tc = pos.clamp(0, a["T"] - 1)
        x16 = f16(a["x16"]).reshape(a["n_seq"], a["seq_rows"], MERGE_K)[seq, tc][:, :a["C"]]
        st = a["st_term"].to(dt).reshape(a["n_seq"], a["seq_rows"], D)
        data = st[seq, a["npre"] + tc] + _lin(a["w_merge"][:, :a["C"]], x16, dt)
        x = torch.zeros(M, D, dtype=dt)
        if a["npre"] > 0:
            tok = a["tok_style"].to(dt)[seq] if a["tok_style"] is not None else torch.zeros(M, D, dtype=dt)
            if a["time_first"]:
                tok = torch.where((pos == 0)[:, None], a["tok_time"].to(dt)[None, :], tok)
            x = torch.where((t < 0)[:, None], tok, x)
        if sab == "pad row keeps st_term":
            x = torch.where((t >= a["T"])[:, None], st[seq, pos], x)
        x = torch.where(is_data[:, None], data, x)
        put("x", x, D)
    else:
        x = a["x"].to(dt)[rows]

    if a["do_post"]:
        p1 = _lin(a["wo"], f16(a["ao"])[rows], dt)
        if gated and a["gate_a"] is not None and sab != "gate_a left out":
            p1 = a["gate_a"].to(dt) * p1
        x1 = x + p1
        if sab == "ungated residual added twice":
            x1 = x1 + x
        n = rnd("n_ffn", _norm(x1, a["g_ffn"], a["w_f"], a["b_f"], a, dt, sab))
        w1, w3 = (a["w3"], a["w1"]) if sab == "w1 and w3 swapped" else (a["w1"], a["w3"])
        h = rnd("h", _silu(_lin(w1, n, dt)) * _lin(w3, n, dt))
        mlp = _lin(a["w2"], h, dt)
        if sab == "one mlp output tile dropped":
            mlp[:, D - 32:D - 16] = 0.0
        if gated and a["gate_f"] is not None and sab != "gate_f left out":
            mlp = a["gate_f"].to(dt) * mlp
        x = x1 + mlp
        if a["seam"] == SEAM_HEAD:
            if gated:
                put("x", x1, D)
        elif not a["do_skip"]:
            put("x", x, D)
        if a["want_c16"] and sab != "c16 taken after the skip":
            put("c16", x, D)
    if a["do_skip"]:
        ws = a["wskip"]
        wa, wb = (ws[:, D:], ws[:, :D]) if sab == "wskip halves swapped" else (ws[:, :D], ws[:, D:])
        x = _lin(wa, rnd("x2h", x), dt) + _lin(wb, f16(a["skip_in"])[rows], dt) + (a["bskip"].to(dt) if a["bskip"] is not None else 0.0)
        put("x", x, D)
        if a["want_c16"] and sab == "c16 taken after the skip":
            put("c16", x, D)
    if a["do_final"]:
        fin = (a["g_fin"], a["w_fin"], a["b_fin"])
        if sab == "final norm with the attention-norm vectors":
            # what the kernel keeps in those two LDS vectors: the attention norm's, or behind the head seam the head's biases
            if a["seam"] == SEAM_HEAD:
                fin = (a["head_b0"], None, torch.cat([a["head_b2"], torch.zeros(D - a["head_C"])]))
            else:
                fin = (a["g_attn"], a["w_a"], a["b_a"]) if a["do_qkv"] else (None, None, None)
        nf = _norm(x, *fin, a, dt, sab)
        if a["seam"] == SEAM_HEAD:
            b0 = a["head_b0"].to(dt)
            hin = _lin(a["head_wa"], rnd("n_fin", nf), dt)
            s = _silu(hin) + b0 if sab == "head b0 after the silu" else _silu(hin + b0)
            put("v32", _lin(a["head_w2"], rnd("s_head", s), dt) + a["head_b2"].to(dt), a["ldv"], slice(0, a["head_C"]))
        else:
            put("n16", nf, D)
    if a["do_qkv"]:
        n = rnd("n_attn", _norm(x, a["g_attn"], a["w_a"], a["b_a"], a, dt, sab))
        qkv = _lin(a["wqkv"], n, dt)
        rp = pos
        if sab == "rope without row_off":
            rp = pos - a["row_off"]
        if sab == "rope on tile-shifted positions":
            m = (torch.arange(M) + 16).clamp_max(M - 1)
            rp = a["row_off"] + m % a["Lout"]
        flip = sab == "rope sin sign flipped"
        qs = torch.tensor(a["q_scale"], dtype=torch.float32).to(dt)
        q = _rope(qkv[:, :D], a["rope"], rp, dt, flip) * qs
        k = _rope(qkv[:, D:2 * D], a["rope"], rp, dt, flip)
        if sab == "q_scale on k as well":
            k = k * qs
        put("qk", torch.cat([q, k], dim=1), 2 * D)
        mode = a["vt_mode"] if a["vt_mode"] else 1          # the kernel treats 0 as 1
        if sab == "vt_pos mode 1 for mode 2":
            mode = 1
        vt = torch.zeros(a["n_seq"], D, a["vt_ld"], dtype=dt)
        mask = torch.zeros(a["n_seq"], D, a["vt_ld"], dtype=torch.bool)
        col = torch.tensor([vt_pos(int(p_), mode) for p_ in pos])
        vt[seq, :, col] = qkv[:, 2 * D:]
        mask[seq, :, col] = True
        out["vt"] = (vt, mask)
    return out


def noise32(a):
    """{output: elementwise distance of a float32 evaluation of the restatement from the float64 one, on the pre-rounding values}.
    A float32 evaluation is not unique: another summation order (the kernel's MFMA k order, torch's blocked one) moves every fp16
    intermediate by its own fp32 noise, and an intermediate that lies that close to a rounding boundary then lands on either
    side.  One float32 run realises one random subset of these flips -- in a 4-row launch often none, and then its distance from
    the float64 run is pure summation noise (~1e-6) while a right kernel that flips one element of n or h is off by
    ulp16 x |w| (~1e-4).  So the flips are modelled, not sampled: for every intermediate, every element within
    MARGIN x (its own fp32 noise: the distance of a float32 evaluation of that element from the float64 one on the same rounded
    inputs, not below the intermediate's median relative and median absolute distance) of a boundary is rounded the other way
    and the restatement re-evaluated in float64; the noise of an element is the largest of all these distances and the float32
    run's.  All candidates of an intermediate flip at once (rows are independent, a row holds a few), which errs on the wide
    side by the sum of a row's flips instead of the largest."""
    t64, t32 = {}, {}
    r64 = ref_panel(a, taps=t64)
    r32 = ref_panel(a, torch.float32)
    out = {k: (r32[k][0].double() - r64[k][0]).abs() for k in r64}
    # each intermediate's own fp32 noise: a float32 run fed the float64 run's rounded intermediates
    ref_panel(a, torch.float32, taps=t32, force={k: v[1] for k, v in t64.items()})
    for stage in t64:
        t = t64[stage][0]
        d = (t32[stage][0].double() - t).abs()
        if d.max().item() == 0.0:
            continue          # an input passed through (half(x) in front of a skip linear without the post phase): nothing to flip
        # an element's own noise: what the float32 run shows on it, not below the stage's typical relative and absolute levels
        tol = MARGIN * torch.maximum(d, torch.maximum(t.abs() * (d / t.abs().clamp_min(1e-30)).median(), d.median()))
        rf = ref_panel(a, flip=(stage, tol))
        for k in out:
            out[k] = torch.maximum(out[k], (rf[k][0] - r64[k][0]).abs())
    return out


def bounds(a):
    """{output: (r, mask, e)} with e = MARGIN x max(noise32) over the written elements of that output"""
    r64 = ref_panel(a)
    n = noise32(a)
    return {k: (r, mask, MARGIN * n[k][mask].max().item()) for k, (r, mask) in r64.items()}


def excess(name, y, r, mask, e):
    """How far y (float64 values of what the kernel stored, or of a pre-rounding restatement for an fp32 output) is from the
    reference, in units of the bound's e: fp32 outputs |y - r| / e, fp16 outputs (|y - r| - ulp16(r) / 2) / e.  <= 1 passes."""
    d = (y.double() - r).abs()
    if name in F16_OUTPUTS:
        d = d - ulp16(r) / 2
    d = torch.nan_to_num(d[mask], nan=float("inf"))
    if e == 0.0:
        return 0.0 if (d <= 0).all() else float("inf")
    return (d.max() / e).item()


def as_stored(name, pre):
    """what a kernel computing `pre` stores: rounded to the output's format, as float64"""
    return half(pre).double() if name in F16_OUTPUTS else pre.to(torch.float32).double()


# ------------------------------------------------------------------------------------------------ inputs
def make_args(c):
    """The arguments of one launch from a case dict (see `case`).  Seeded randn: x, ao, skip_in, x16 of unit scale except every
    fourth row, which is 250 x smaller (so that eps = 1e-5 weighs in a norm); weights randn / sqrt(fan_in); gammas 1 +- 0.2,
    modulations w, b +- 0.5 (the AdaLN projections of the checkpoints give +- 0.1 .. 1), gates 0.3 +- 0.5, biases +- 0.5."""
    g = torch.Generator().manual_seed(c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    D, I = c["D"], c["I"]
    n_seq, Lout, seq_rows, row_off = c["n_seq"], c["Lout"], c["seq_rows"], c["row_off"]
    n_rows = n_seq * seq_rows
    a = dict(c)
    a["M"] = n_seq * Lout
    a["eps"] = 1e-5
    a["q_scale"] = 0.125 * 1.4426950408889634
    scale = torch.where(torch.arange(n_rows) % 4 == 1, 0.004, 1.0)[:, None]
    a["x"] = rn(n_rows, D) * scale
    vec = lambda amp, mean=0.0: mean + amp * rn(D)     # noqa: E731
    mod = c["mod"]
    for name in ("wo", "w1", "w3", "w2", "wskip", "wqkv", "w_merge", "head_wa", "head_w2", "gate_a", "gate_f", "g_ffn", "w_f", "b_f",
                 "g_attn", "w_a", "b_a", "bskip", "g_fin", "w_fin", "b_fin", "head_b0", "head_b2", "tok_time", "tok_style", "ao",
                 "skip_in", "x16", "st_term", "rope"):
        a[name] = None
    if c["do_post"]:
        a["wo"] = rn(D, D) / D ** 0.5
        a["w1"], a["w3"] = rn(I, D) / D ** 0.5, rn(I, D) / D ** 0.5
        a["w2"] = rn(D, I) / I ** 0.5
        a["ao"] = (rn(n_rows, D) * scale).half()
        a["g_ffn"] = vec(0.2, 1.0)
        if mod:
            a["w_f"], a["b_f"] = vec(0.5), vec(0.5)
        if c["gated"]:
            a["gate_a"], a["gate_f"] = vec(0.5, 0.3), vec(0.5, 0.3)
    if c["do_skip"]:
        a["wskip"] = rn(D, 2 * D) / (2 * D) ** 0.5
        a["skip_in"] = rn(n_rows, D).half()
        a["bskip"] = vec(0.5)
    if c["do_qkv"]:
        a["wqkv"] = rn(3 * D, D) / D ** 0.5
        a["g_attn"] = vec(0.2, 1.0)
        if mod:
            a["w_a"], a["b_a"] = vec(0.5), vec(0.5)
        a["rope"] = rope_table(seq_rows)
        a["vt_ld"] = -(-seq_rows // 32) * 32 + c["vt_extra"]
    else:
        a["vt_ld"] = 0
    if c["do_final"]:
        a["g_fin"] = vec(0.2, 1.0)
        if mod:
            a["w_fin"], a["b_fin"] = vec(0.5), vec(0.5)
    if c["seam"] == SEAM_MERGE:
        C = c["C"]
        a["ldw"] = C + 24                                   # the merge linear's other input blocks lie behind the x block
        a["w_merge"] = rn(D, a["ldw"]) / a["ldw"] ** 0.5
        # x16 row t belongs to position npre + t: it shares that row's scale; columns >= C: finite junk that meets zero weights
        a["x16"] = (rn(n_rows, MERGE_K) * torch.roll(scale, -c["npre"], 0)).half()
        a["st_term"] = rn(n_rows, D) * scale
        a["tok_time"], a["tok_style"] = rn(D), rn(n_seq, D)
    if c["seam"] == SEAM_HEAD:
        a["head_wa"] = rn(D, D) / D ** 0.5
        a["head_w2"] = rn(c["head_C"], D) / D ** 0.5
        a["head_b0"], a["head_b2"] = vec(0.5), 0.5 * rn(c["head_C"])
        a["ldv"] = c["head_C"] + c["ldv_extra"]
    else:
        a["ldv"] = 0
    return a


LAYOUTS = {            # name -> (n_seq, Lout, seq_rows, row_off)
    "m4": (1, 4, 4, 0),                  # one 4-row group; 124 clamped lanes
    "m128": (1, 128, 128, 0),            # one full panel
    "3x44": (3, 44, 44, 0),              # panel 0 straddles all three sequences; panel 1 has 4 rows
    "window": (2, 52, 72, 20),           # the last layer's tail_only window
    "5x52": (5, 52, 52, 0),              # three panels; every wave's rows cross a sequence edge somewhere
}
# phase mixes: name -> (do_post, want_c16, do_skip, do_qkv, do_final, seam)
MIXES = {
    "qkv": (0, 0, 0, 1, 0, SEAM_NONE),
    "merge+qkv": (0, 0, 0, 1, 0, SEAM_MERGE),
    "post+qkv": (1, 0, 0, 1, 0, SEAM_NONE),
    "post+c16+qkv": (1, 1, 0, 1, 0, SEAM_NONE),
    "post+skip+qkv": (1, 0, 1, 1, 0, SEAM_NONE),
    "post+c16+skip+qkv": (1, 1, 1, 1, 0, SEAM_NONE),
    "post+final": (1, 0, 0, 0, 1, SEAM_NONE),
    "post+final+head": (1, 0, 0, 0, 1, SEAM_HEAD),
    "skip+qkv": (0, 0, 1, 1, 0, SEAM_NONE),
}
CKPT_I = {384: 1024, 512: 1536}        # specs.ffn_dim


def case(D, gated, tm, I, layout, mix, seed, add_one=None, mod=True, vt_mode=1, vt_extra=0, npre=1, time_first=1, T=None, C=80,
         head_C=80, ldv_extra=0):
    """layout: a name of LAYOUTS or (n_seq, Lout, seq_rows, row_off)"""
    n_seq, Lout, seq_rows, row_off = LAYOUTS[layout] if isinstance(layout, str) else layout
    do_post, want_c16, do_skip, do_qkv, do_final, seam = MIXES[mix]
    if T is None:
        T = max(1, Lout - npre - 5)        # pad rows behind the data rows wherever the sequence is long enough
    T = max(1, min(T, Lout - npre))
    return dict(D=D, gated=gated, tm=tm, I=I, layout=layout, mix=mix, seed=seed, n_seq=n_seq, Lout=Lout, seq_rows=seq_rows,
                row_off=row_off, do_post=do_post, want_c16=want_c16, do_skip=do_skip, do_qkv=do_qkv, do_final=do_final, seam=seam,
                add_one=int(gated) if add_one is None else add_one, mod=mod, vt_mode=vt_mode, vt_extra=vt_extra, npre=npre,
                time_first=time_first, T=T, C=C, head_C=head_C, ldv_extra=ldv_extra)


def case_id(c):
    s = f"D{c['D']}-g{c['gated']}-tm{c['tm']}-I{c['I']}-{c['layout']}-{c['mix']}"
    if c["seam"] == SEAM_MERGE:
        s += f"-npre{c['npre']}tf{c['time_first']}T{c['T']}C{c['C']}"
    if c["seam"] == SEAM_HEAD:
        s += f"-hC{c['head_C']}+{c['ldv_extra']}"
    if c["do_qkv"]:
        s += f"-vt{c['vt_mode']}+{c['vt_extra']}"
    return s + f"-a{c['add_one']}m{int(c['mod'])}-s{c['seed']}"


def parity_cases():
    """the named edges first, then a seeded sample of the product"""
    out = []
    seed = [1000]

    def add(*a, **kw):
        seed[0] += 1
        out.append(case(*a, seed=seed[0], **kw))

    mixes = list(MIXES)
    layouts = list(LAYOUTS)
    # every (D, gated, tm) with every phase mix once -- all 20 instantiations (the merge seam has no gated form of its own) -- on
    # layouts, FFN widths and V^T forms that rotate
    i = 0
    for D in (384, 512):
        for gated in (0, 1):
            for tm in (1, 2):
                for mix in mixes:
                    lay = layouts[i % 5]
                    if MIXES[mix][5] == SEAM_MERGE and lay == "window":
                        lay = "3x44"
                    add(D, gated, tm, (32, 96)[i % 2], lay, mix, vt_mode=1 + (i // 2) % 2, vt_extra=32 * ((i // 3) % 2),
                        head_C=(16, 80, 128)[i % 3], ldv_extra=16 * ((i // 2) % 2), npre=i % 3, time_first=(i // 3) % 2,
                        C=(80, 128)[i % 2])
                    i += 1
    # the checkpoints' own FFN width, M = 132
    for D in (384, 512):
        add(D, int(D == 512), 0, CKPT_I[D], "3x44", "post+qkv")
    # the merge seam's edges: T = 1, no prefix, a prefix without the time token, both widths
    for D, tm in ((384, 2), (512, 1)):
        add(D, 0, tm, 32, "3x44", "merge+qkv", npre=2, time_first=1, T=1, C=128)
        add(D, 0, tm, 32, "5x52", "merge+qkv", npre=0, time_first=0, C=80)
        add(D, 0, tm, 32, "m128", "merge+qkv", npre=2, time_first=0, T=100, C=80)
        add(D, 0, tm, 32, "m4", "merge+qkv", npre=1, time_first=1, T=1, C=128)
    # the window with the final norm and with the head; every head width with both strides
    for D, gated, tm in ((384, 0, 2), (512, 1, 1), (512, 1, 2)):
        add(D, gated, tm, 96, "window", "post+final")
        for head_C in (16, 80, 128):
            for extra in (0, 16):
                add(D, gated, tm, 32, ("window", "3x44")[extra // 16], "post+final+head", head_C=head_C, ldv_extra=extra)
    # add_one with and without the modulation vectors (null pointers), crossed with the form
    for D, gated in ((384, 0), (512, 1)):
        for add_one in (0, 1):
            for mod in (False, True):
                add(D, gated, 0, 32, "3x44", "post+c16+skip+qkv", add_one=add_one, mod=mod)
    rng = random.Random(20250311)
    for _ in range(16):
        mix = rng.choice(mixes)
        lay = rng.choice([l for l in layouts if not (MIXES[mix][5] == SEAM_MERGE and l == "window")])
        add(rng.choice([384, 512]), rng.choice([0, 1]), rng.choice([1, 2]), rng.choice([32, 96]), lay, mix,
            add_one=rng.choice([0, 1]), mod=rng.random() < 0.7, vt_mode=rng.choice([1, 2]), vt_extra=rng.choice([0, 32]),
            npre=rng.choice([0, 1, 2]), time_first=rng.choice([0, 1]), C=rng.choice([80, 128]), head_C=rng.choice([16, 80, 128]),
            ldv_extra=rng.choice([0, 16]))
    return out


def instantiation(c):
    """(D, gated, tm, seam) of the template instantiation a case launches"""
    tm = c["tm"] if c["tm"] else (2 if c["D"] == 384 else 1)
    return c["D"], 0 if c["seam"] == SEAM_MERGE else c["gated"], tm, c["seam"]
