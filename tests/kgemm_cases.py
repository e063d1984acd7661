"""The tap-GEMM (csrc/kgemm_tile.h, kgemm.hip, kgemm_big.hip) at op level: the float64 reference, the derived error bound, the
cases, an fp32 emulation and the named sabotages.  test_host_kgemm.py pins the reference to torch and the oracle and shows that
every sabotage is caught; test_gpu_kgemm.py runs the kernel (ops.kgemm: ONE kgemm_launch per call).

REFERENCE.  Plain float64 torch on exactly the operands the kernel gets (A and W rounded to fp16 for dtype 0, fp32 for dtype 1).
  row map     m = s Lout + pos, q0 = pos a_stride + shift_t, len = seq_len[s] (or a_len).  ZERO: q0 outside [0, len) contributes
              nothing.  CLAMP: q = clamp(q0, 0, len - 1).  REFLECT: lenx = max(len, reflect_min); q0 < 0 -> -q0, q0 >= lenx ->
              2 (lenx - 1) - q0; a result still outside [0, len) contributes nothing.  Source row = (a_seq_map[s] or s) a_seq_rows +
              a_off + q; output row = s c_seq_rows + c_off + pos.
  STORE       v = acc + bias + rowvec[s], act, * gate[s], + res, * out_scale (0 = 1), + res2, relu if post_relu.  c32 = v.  With the
              Snake t = v + post_ib sin^2(post_a v) below post_n and 0 at and above it: c16 = fp16(t), c16_lo = fp16(t - fp16(t));
              otherwise c16 = fp16(v).
  SWIGLU      out[j] = silu(v[2j]) v[2j+1];  TANHSIG  out[j] = tanh(v[2j]) sigmoid(v[2j+1]);  v = acc + bias + rowvec[s]
  QKV_ROPE    pair (2i, 2i+1) of every 64-wide head of q and k rotated with rope[pos][i], q scaled by q_scale, both to fp16;
              V to vt[s][d][vt_pos(pos, vt_mode)] (vt_pos restated below from common.h).  No bias, no rowvec (refused).

BOUND (absolute, per output element; u = 2^-24; nothing fitted to the kernel's output).  First-order terms, as ar_step_cases.py
and panel_cases.py state them; the fp32 emulation is held to HALF the bound.
  dot(n)      fp32 sum of n products in ANY order: (n + 2) u sum|terms|, n = the padded K summed over the taps   [Higham 3.5]
  added term  one rounding, u |result|, for bias, rowvec, gate, res, out_scale, res2 each; relu, abs and clamp are exact
  exp, rcp    __expf / v_exp_f32 relative 2 u (|x| + 1); v_rcp_f32 1 ulp (2 u); a / b 2.5 ulp (5 u)      [ar_step_cases.py]
  silu        1.1 E + |silu| (2 u (|v| + 1) + 7 u);  sigmoid  0.25 E + sig (2 u (|v| + 1) + 7 u);  lrelu  max(1, |slope|) E + u |f|
  SWIGLU      1.1 |b| E_a + |silu a| E_b + |silu(a) b| (2 u (|a| + 1) + 7 u)                                [ar_step_cases.py]
  TANHSIG     th = 1 - 2 rcp(1 + exp2(2 a log2 e)): the exp error reaches th through (1 - th^2) / 2, the add and the rcp through
              r = 1 - th:  e_th = (1 - th^2) u (2 |a| + 1) ... written out in `tanhsig`; sig as above; the product u |o|
  rotation    dot(2) of (a c, b s), contracted into an fma or not: 4 u (|a c| + |b s|); the q scale u |o|   [ar_step_cases.py]
  Snake       (1 + |post_ib post_a|) E + 2^-22 (|v| + |post_ib|) + 2^-23 |post_a v| |post_ib|           [vocoder_pointwise_cases.py]
  fp16 out    + half an fp16 ulp at |ref| + E (the format's own step: the error / bound RATIO of an fp16 output is that of the
              excess over the half step to E, the assertion is |got - ref| <= E + half step)
  c16_lo      |hi + lo - t| <= E_t + 2^-22 |t| + 2^-25                                                  [vocoder_pointwise_cases.py]
  erff, expm1f, tanhf (act_apply)   the ROCm install carries no OCML accuracy table, so each function's own error was measured once
              on an MI355X on its activation-only case (one k-tile, W a 0 / 1 selection matrix: the pre-activation is exact)
              against float64, and TWICE the measured value is the constant (the factor covers arguments the case did not sample):
                gelu (erff)   |err| <= K_GELU u |v|        measured 1.552 u |v| (8320 arguments in [-20, 20]),  K_GELU  = 3.104
                elu (expm1f)  |err| <= K_EXPM1 u |f|       measured 1.121 u |f|,                                K_EXPM1 = 2.242
                tanh (tanhf)  |err| <= K_TANH u |f|        measured 1.405 u |f|,                                K_TANH  = 2.810
              (test_gpu_kgemm.py::test_activation_function_constants prints the three figures of the run and holds them to the
              constants.)  Through an activation E becomes L E + that, L the Lipschitz constant (gelu 1.13).

SABOTAGES of the reference, each caught by at least one case (test_host_kgemm.py names which): see SABOTAGES.
"""
import math

import torch

U = 2.0 ** -24
GUARD = 2
F32_FILL, F16_FILL = -777.25, 0x6A5A
LOG2E = 1.4426950408889634
# measured on an MI355X, in units of u (see the docstring); the constants are twice these
MEASURED_GELU, MEASURED_EXPM1, MEASURED_TANH = 1.552, 1.121, 1.405
K_GELU, K_EXPM1, K_TANH = 2 * MEASURED_GELU, 2 * MEASURED_EXPM1, 2 * MEASURED_TANH

PAD_ZERO, PAD_REFLECT, PAD_CLAMP = 0, 1, 2
ACT = dict(none=0, silu=1, elu=2, lrelu=3, tanh=4, abs=5, clamp=6, sigmoid=7, gelu=8)
EPI = dict(store=0, swiglu=1, tanhsig=2, qkv=3)
FORMS = (0x10, 0x20, 0x80, 0xB0, 0x90, 0x50, 0x70, 0x40)      # the forms the bit-identity tests of test_gpu_ops.py run

SABOTAGES = ("pair_swapped", "pair_over_row", "q_scale_on_k", "vt_wrong_mode", "v_pos_plus_1", "gate_before_act", "scale_before_res",
             "res2_before_scale", "relu_before_res", "reflect_no_min", "reflect_off_by_one", "clamp_for_zero", "neighbour_seq_len",
             "seq_map_ignored", "c_off_ignored", "taps_reversed", "tap_k_offset", "bias_n_plus_8", "snake_above_post_n", "lo_of_unrounded")


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).float()


def ulp16(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def half_ulp16(ref, E):
    return 0.5 * ulp16(ref.abs() + E)


def rope_unit(g, rows):
    """unit (cos, sin) pairs, different for every (position, pair)"""
    ang = torch.rand(rows, 32, generator=g, dtype=torch.float64) * 2 * math.pi
    return torch.stack([ang.cos(), ang.sin()], -1).float()


def vt_pos(pos, mode):
    """common.h: vt_perm_pos (mode 1), vt_perm_pos16 (mode 2), natural (mode 0)"""
    if mode == 1:
        return (pos & ~31) | (((pos >> 2) & 3) << 3) | (((pos >> 4) & 1) << 2) | (pos & 3)
    if mode == 2:
        return (pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1)
    return pos


def ktile(dtype):
    return 64 if dtype == 0 else 32


def nseq_of(c):
    return -(-c["M"] // c["Lout"])


# ------------------------------------------------------------------------------------------------------------ row map
def map_row(c, s, pos, shift, sab=None):
    """the row of its sequence that (s, pos, shift) reads, or None where it contributes nothing"""
    lens = c.get("seq_len")
    if lens is not None:
        ln = lens[(s + 1) % len(lens)] if sab == "neighbour_seq_len" else lens[s]
    else:
        ln = c["a_len"]
    q = pos * c["a_stride"] + shift
    mode = c["pad_mode"]
    if sab == "clamp_for_zero" and mode == PAD_ZERO:
        mode = PAD_CLAMP
        if ln < 1:
            return None
    if 0 <= q < ln:
        return q
    if mode == PAD_ZERO:
        return None
    if mode == PAD_CLAMP:
        return min(max(q, 0), ln - 1)
    lenx = ln if sab == "reflect_no_min" else max(ln, c["reflect_min"])
    if q < 0:
        q = -q - (1 if sab == "reflect_off_by_one" else 0)
    elif q >= lenx:
        q = 2 * (lenx - 1) - q + (1 if sab == "reflect_off_by_one" else 0)
    return q if 0 <= q < ln else None


def source_rows(c, sab=None):
    """[tap] -> LongTensor (M,) of absolute source rows, -1 where nothing is read"""
    M, Lout = c["M"], c["Lout"]
    out = []
    for (_, shift) in c["taps"]:
        idx = torch.full((M,), -1, dtype=torch.long)
        for m in range(M):
            s, pos = divmod(m, Lout)
            q = map_row(c, s, pos, shift, sab)
            if q is not None:
                sm = c["a_seq_map"][s] if (c.get("a_seq_map") is not None and sab != "seq_map_ignored") else s
                idx[m] = sm * c["a_seq_rows"] + c["a_off"] + q
        out.append(idx)
    return out


def host_ranges(c):
    """svc_op_kgemm's range computation restated: {(s, tap): (lowest, highest) absolute source row}, only where a row is read"""
    out = {}
    for s in range(nseq_of(c)):
        ln = c["seq_len"][s] if c.get("seq_len") is not None else c["a_len"]
        base = (c["a_seq_map"][s] if c.get("a_seq_map") is not None else s) * c["a_seq_rows"] + c["a_off"]
        npos = min(c["Lout"], c["M"] - s * c["Lout"])
        for t, (_, shift) in enumerate(c["taps"]):
            lo = hi = None
            for pos in range(npos):
                q0 = pos * c["a_stride"] + shift
                if 0 <= q0 < ln:
                    q = q0
                elif c["pad_mode"] == PAD_ZERO:
                    continue
                elif c["pad_mode"] == PAD_CLAMP:
                    q = 0 if q0 < 0 else ln - 1
                else:
                    lenx = max(ln, c["reflect_min"])
                    q = -q0 if q0 < 0 else (2 * (lenx - 1) - q0 if q0 >= lenx else q0)
                    if not 0 <= q < ln:
                        continue
                lo = q if lo is None else min(lo, q)
                hi = q if hi is None else max(hi, q)
            if lo is not None:
                out[(s, t)] = (base + lo, base + hi)
    return out


# ------------------------------------------------------------------------------------------------------------ reference
def operand(t, dtype):
    return (t.half() if dtype == 0 else t.float()).double()


def accumulate(c, src, sab=None):
    """(acc, sum |terms|, padded K) in float64 over the row map"""
    dt = c["dtype"]
    W = operand(c["W"], dt)
    taps = list(c["taps"])
    rows = source_rows(c, sab)
    Ks = [src[i].shape[1] for i, _ in taps]
    koff = [sum(Ks[:t]) for t in range(len(taps))]
    if sab == "taps_reversed":
        koff = koff[::-1]
    acc = torch.zeros(c["M"], c["N"], dtype=torch.float64)
    ab = torch.zeros_like(acc)
    kt = ktile(dt)
    for t, (i, _) in enumerate(taps):
        idx = rows[t]
        a = operand(src[i], dt)
        a = a[idx.clamp_min(0) % a.shape[0]]                  # (a sabotaged map may leave the buffer: it wraps)
        a = torch.where((idx >= 0)[:, None], a, torch.zeros_like(a))
        k0 = koff[t]
        if sab == "tap_k_offset" and t > 0:
            k0 = k0 + kt
        if sab is not None:
            k0 = k0 % max(W.shape[1] - Ks[t] + 1, 1)
        w = W[:, k0:k0 + Ks[t]]
        acc += a @ w.T
        ab += a.abs() @ w.abs().T
    return acc, ab, sum(-(-k // kt) * kt for k in Ks)


def act_apply(v, E, act, slope):
    s = float(torch.tensor(slope, dtype=torch.float32))
    if act == ACT["silu"]:
        f = v * torch.sigmoid(v)
        return f, 1.1 * E + f.abs() * (2 * U * (v.abs() + 1) + 7 * U) + 1e-38
    if act == ACT["sigmoid"]:
        f = torch.sigmoid(v)
        return f, 0.25 * E + f * (2 * U * (v.abs() + 1) + 7 * U) + 1e-38
    if act == ACT["elu"]:
        f = torch.where(v > 0, v, torch.expm1(v))
        return f, E + torch.where(v > 0, torch.zeros_like(v), K_EXPM1 * U * f.abs())
    if act == ACT["lrelu"]:
        f = torch.where(v > 0, v, v * s)
        return f, max(1.0, abs(s)) * E + U * f.abs()
    if act == ACT["tanh"]:
        f = torch.tanh(v)
        return f, E + K_TANH * U * f.abs()
    if act == ACT["abs"]:
        return v.abs(), E
    if act == ACT["clamp"]:
        return v.clamp(-s, s), E
    if act == ACT["gelu"]:
        return 0.5 * v * (1 + torch.erf(v / math.sqrt(2.0))), 1.13 * E + K_GELU * U * v.abs()
    return v, E


def seq_vec(c, name):
    """rowvec / gate as (M, N) float64, or None"""
    t = c.get(name)
    if t is None:
        return None
    t = t.double()
    if t.dim() == 1:
        return t[None].expand(c["M"], -1)
    return t[torch.arange(c["M"]) // c["Lout"]]


def tanhsig(a, b, Ea, Eb):
    th, sg = torch.tanh(a), torch.sigmoid(b)
    r = 1 - th
    e_th = (1 - th * th) * U * (2 * a.abs() + 1) + r * 3 * U + U * th.abs() + Ea
    e_sg = sg * ((1 - sg) * 2 * U * (b.abs() + 1) + 3 * U) + 0.25 * Eb
    o = th * sg
    return o, sg * e_th + th.abs() * e_sg + U * o.abs() + 1e-38


def swiglu(a, b, Ea, Eb):
    sl = a * torch.sigmoid(a)
    o = sl * b
    return o, 1.1 * b.abs() * Ea + sl.abs() * Eb + o.abs() * (2 * U * (a.abs() + 1) + 7 * U) + 1e-38


def out_rows(c, sab=None):
    m = torch.arange(c["M"])
    s, pos = m // c["Lout"], m % c["Lout"]
    return s * c["c_seq_rows"] + (0 if sab == "c_off_ignored" else c["c_off"]) + pos


def c_rows_of(c):
    return c.get("c_rows") or nseq_of(c) * c["c_seq_rows"]


def reference(c, sab=None, src=None):
    """{output: dict(ref, E, mask, kind)} over the WHOLE buffers between the guards: (c_rows, ldc), vt (nseq rope_D, vt_ld).
    mask = written by the launch; elsewhere the buffer keeps its fill.  kind: "f32", "f16" or "lo" (ref = t, judged on hi + lo)."""
    src = c["src"] if src is None else src
    M, N, epi = c["M"], c["N"], c["epi"]
    nseq = nseq_of(c)
    acc, ab, Kp = accumulate(c, src, sab)
    E = (Kp + 2) * U * ab
    v = acc

    def add(t):
        nonlocal v, E
        v = v + t
        E = E + U * v.abs()
    if c.get("bias") is not None:
        bias = c["bias"].double()
        if sab == "bias_n_plus_8":
            bias = torch.roll(bias, -8)
        add(bias[None])
    rv = seq_vec(c, "rowvec")
    if rv is not None:
        add(rv)
    orow = out_rows(c, sab)
    rows, ldc = c_rows_of(c), c["ldc"]
    out = {}

    def put(name, ref, Eo, kind, cols=None):
        cols = ref.shape[1] if cols is None else cols
        R = torch.zeros(rows, ldc, dtype=torch.float64)
        B = torch.zeros(rows, ldc, dtype=torch.float64)
        Mk = torch.zeros(rows, ldc, dtype=torch.bool)
        R[orow, :cols], B[orow, :cols], Mk[orow, :cols] = ref, Eo, True
        out[name] = dict(ref=R, E=B, mask=Mk, kind=kind)

    if epi == EPI["store"]:
        gate = seq_vec(c, "gate")
        if sab == "gate_before_act" and gate is not None:
            v = v * gate
        v, E = act_apply(v, E, c.get("act") or 0, c.get("act_slope") or 0.0)
        if gate is not None and sab != "gate_before_act":
            v = v * gate
            E = E * gate.abs() + U * v.abs()
        res = c.get("res")
        if isinstance(res, str):
            res = c["c_init"]
        res2 = c.get("res2")
        if isinstance(res2, str):
            res2 = c["c_init"]
        sc = float(torch.tensor(c.get("out_scale") or 0.0, dtype=torch.float32)) or 1.0
        r1 = res.double()[orow, :N] if res is not None else None
        r2 = res2.double()[orow, :N] if res2 is not None else None
        relu = bool(c.get("post_relu"))
        if sab == "relu_before_res" and relu:
            v = v.clamp_min(0)
        if sab == "scale_before_res":
            v, E = v * sc, E * abs(sc)
        if sab == "res2_before_scale" and r2 is not None:
            add(r2)
        if r1 is not None:
            add(r1)
        if sab != "scale_before_res" and sc != 1.0:
            v = v * sc
            E = E * abs(sc) + U * v.abs()
        if r2 is not None and sab != "res2_before_scale":
            add(r2)
        if relu and sab != "relu_before_res":
            v = v.clamp_min(0)
        if c.get("want_c32"):
            put("c32", v, E, "f32")
        t, Et = v, E
        if c.get("post_a") is not None:
            pn = c["post_n"]
            pa = torch.zeros(N, dtype=torch.float64)
            pib = torch.zeros(N, dtype=torch.float64)
            k = min(pn, N)
            pa[:k], pib[:k] = c["post_a"].double()[:k], c["post_ib"].double()[:k]
            if sab == "snake_above_post_n":
                pa[k:], pib[k:] = c["post_a"].double()[k - 1], c["post_ib"].double()[k - 1]
            t = v + pib * torch.sin(pa * v) ** 2
            Et = (1 + (pib * pa).abs()) * E + 2.0 ** -22 * (v.abs() + pib.abs()) + 2.0 ** -23 * (pa * v).abs() * pib.abs()
            live = (torch.arange(N) < pn)[None].expand_as(t)
            if sab != "snake_above_post_n":
                t, Et = torch.where(live, t, torch.zeros_like(t)), torch.where(live, Et, torch.zeros_like(Et))
            if c.get("want_c16_lo"):
                tl = t.half().double() if sab == "lo_of_unrounded" else t
                put("c16_lo", tl, Et + 2.0 ** -22 * t.abs() + 2.0 ** -25, "lo")
        if c.get("want_c16"):
            put("c16", t, Et, "f16")
        return out

    if epi in (EPI["swiglu"], EPI["tanhsig"]):
        a, b, Ea, Eb = v[:, 0::2], v[:, 1::2], E[:, 0::2], E[:, 1::2]
        if sab == "pair_swapped":
            a, b, Ea, Eb = b, a, Eb, Ea
        o, Eo = (swiglu if epi == EPI["swiglu"] else tanhsig)(a, b, Ea, Eb)
        if c.get("want_c32"):
            put("c32", o, Eo, "f32")
        if c.get("want_c16"):
            put("c16", o, Eo, "f16")
        return out

    # QKV_ROPE
    D = c["rope_D"]
    tab = c["rope"].double()
    m = torch.arange(M)
    pos = m % c["Lout"]
    n = torch.arange(2 * D)
    if sab == "pair_over_row":          # the pair index counted over the whole row, not per 64-wide head
        flat = tab.reshape(-1, 2)
        cs = flat[(pos[:, None] * 32 + (n // 2)[None]) % flat.shape[0]]
    else:
        cs = tab[pos][:, (n // 2) % 32]                          # (M, 2D, 2)
    x = v[:, :2 * D]
    Ex = E[:, :2 * D]
    part = torch.empty_like(x)
    part[:, 0::2], part[:, 1::2] = x[:, 1::2], x[:, 0::2]
    Ep = torch.empty_like(Ex)
    Ep[:, 0::2], Ep[:, 1::2] = Ex[:, 1::2], Ex[:, 0::2]
    sign = torch.where(n % 2 == 0, -1.0, 1.0).double()[None]
    co, si = cs[..., 0], cs[..., 1]
    o = x * co + sign * part * si
    Eo = co.abs() * Ex + si.abs() * Ep + 4 * U * ((x * co).abs() + (part * si).abs())
    qs = float(torch.tensor(c["q_scale"], dtype=torch.float32))
    scale = torch.where(n < D, qs, 1.0).double()[None] if sab != "q_scale_on_k" else torch.where(n < D, 1.0, qs).double()[None]
    o = o * scale
    Eo = Eo * scale.abs() + U * o.abs()
    put("c16", o, Eo, "f16")
    vt_ld = c["vt_ld"]
    mode = c["vt_mode"] if sab != "vt_wrong_mode" else (c["vt_mode"] + 1) % 3
    R = torch.zeros(nseq * D, vt_ld, dtype=torch.float64)
    B = torch.zeros_like(R)
    Mk = torch.zeros(nseq * D, vt_ld, dtype=torch.bool)
    for mi in range(M):
        s, p = divmod(mi, c["Lout"])
        col = vt_pos(p + 1 if sab == "v_pos_plus_1" else p, mode)
        if col < vt_ld:
            R[s * D:(s + 1) * D, col], B[s * D:(s + 1) * D, col], Mk[s * D:(s + 1) * D, col] = v[mi, 2 * D:], E[mi, 2 * D:], True
    out["vt"] = dict(ref=R, E=B, mask=Mk, kind="f16")
    return out


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def sin_sq32(x):
    n = torch.round(x * 0.318309886183790672)
    r = x + n * -3.140625
    r = r + n * -9.67502593994140625e-4
    r = r + n * -1.509957990978376e-7
    r2 = r * r
    p = r2 * 2.6348154733568663e-06 + -0.00019822761532850564
    p = p * r2 + 0.008333242498338223
    p = p * r2 + -0.1666666567325592
    sn = p * r2 * r + r
    return sn * sn


def emulate(c):
    """the kernel's arithmetic in fp32 torch ops: fp32 accumulation k-tile by k-tile in tap order, the epilogue in the kernel's
    order.  Returns {output: values (float64 of what the kernel would store) over the written elements' buffers}"""
    f = torch.float32
    dt = c["dtype"]
    M, N, epi = c["M"], c["N"], c["epi"]
    W = operand(c["W"], dt).to(f)
    rows = source_rows(c)
    acc = torch.zeros(M, N, dtype=f)
    k0 = 0
    kt = ktile(dt) // (2 if dt == 0 else 1)
    for t, (i, _) in enumerate(c["taps"]):
        idx = rows[t]
        a = operand(c["src"][i], dt).to(f)[idx.clamp_min(0)]
        a = torch.where((idx >= 0)[:, None], a, torch.zeros_like(a))
        K = a.shape[1]
        for k in range(0, K, kt):
            acc = acc + a[:, k:k + kt] @ W[:, k0 + k:k0 + min(k + kt, K)].T
        k0 += K
    v = acc
    if c.get("bias") is not None:
        v = v + c["bias"].to(f)[None]
    rv = seq_vec(c, "rowvec")
    if rv is not None:
        v = v + rv.to(f)
    orow = out_rows(c)
    rows_c, ldc = c_rows_of(c), c["ldc"]
    out = {}

    def put(name, val):
        R = torch.zeros(rows_c, ldc, dtype=torch.float64)
        R[orow, :val.shape[1]] = val.double()
        out[name] = R
    if epi == EPI["store"]:
        act, s = c.get("act") or 0, torch.tensor(c.get("act_slope") or 0.0, dtype=f)
        if act == ACT["silu"]:
            v = v / (1 + torch.exp(-v))
        elif act == ACT["sigmoid"]:
            v = 1 / (1 + torch.exp(-v))
        elif act == ACT["elu"]:
            v = torch.where(v > 0, v, torch.expm1(v))
        elif act == ACT["lrelu"]:
            v = torch.where(v > 0, v, v * s)
        elif act == ACT["tanh"]:
            v = torch.tanh(v)
        elif act == ACT["abs"]:
            v = v.abs()
        elif act == ACT["clamp"]:
            v = torch.minimum(torch.maximum(v, -s), s)
        elif act == ACT["gelu"]:
            v = 0.5 * v * (1 + torch.erf(v * 0.70710678118654752))
        g = seq_vec(c, "gate")
        if g is not None:
            v = v * g.to(f)
        for name in ("res", "sc", "res2"):
            if name == "sc":
                if c.get("out_scale"):
                    v = v * torch.tensor(c["out_scale"], dtype=f)
                continue
            r = c.get(name)
            if isinstance(r, str):
                r = c["c_init"]
            if r is not None:
                v = v + r.to(f)[orow, :N]
        if c.get("post_relu"):
            v = v.clamp_min(0)
        if c.get("want_c32"):
            put("c32", v)
        t = v
        if c.get("post_a") is not None:
            pn = min(c["post_n"], N)
            pa, pib = torch.zeros(N, dtype=f), torch.zeros(N, dtype=f)
            pa[:pn], pib[:pn] = c["post_a"][:pn], c["post_ib"][:pn]
            t = v + pib * sin_sq32(pa * v)
            t = torch.where((torch.arange(N) < c["post_n"])[None], t, torch.zeros_like(t))
            if c.get("want_c16_lo"):
                put("c16_lo", t.half().double() + (t - t.half().to(f)).half().double())       # hi + lo, as the check reads it
        if c.get("want_c16"):
            put("c16", t.half())
        return out
    if epi in (EPI["swiglu"], EPI["tanhsig"]):
        a, b = v[:, 0::2], v[:, 1::2]
        l2 = torch.tensor(LOG2E, dtype=f)
        if epi == EPI["swiglu"]:
            o = a * (1 / (1 + torch.exp2(-a * l2))) * b
        else:
            th = 1 - 2 * (1 / (1 + torch.exp2(2 * l2 * a)))
            o = th * (1 / (1 + torch.exp2(-b * l2)))
        if c.get("want_c32"):
            put("c32", o)
        if c.get("want_c16"):
            put("c16", o.half())
        return out
    D = c["rope_D"]
    pos = torch.arange(M) % c["Lout"]
    n = torch.arange(2 * D)
    cs = c["rope"].to(f)[pos][:, (n // 2) % 32]
    x = v[:, :2 * D]
    part = torch.empty_like(x)
    part[:, 0::2], part[:, 1::2] = x[:, 1::2], x[:, 0::2]
    sign = torch.where(n % 2 == 0, -1.0, 1.0).to(f)[None]
    o = (x * cs[..., 0] + sign * (part * cs[..., 1])) * torch.where(n < D, torch.tensor(c["q_scale"], dtype=f), torch.tensor(1.0, dtype=f))[None]
    put("c16", o.half())
    R = torch.zeros(nseq_of(c) * D, c["vt_ld"], dtype=torch.float64)
    for mi in range(M):
        s, p = divmod(mi, c["Lout"])
        R[s * D:(s + 1) * D, vt_pos(p, c["vt_mode"])] = v[mi, 2 * D:].half().double()
    out["vt"] = R
    return out


# ------------------------------------------------------------------------------------------------------------ judging
def judge(exp, vals, scale=1.0):
    """vals {output: float64 values over the whole buffer between the guards} against `exp` on the written elements -> (list of
    outputs with an element out of bound, worst error / bound).  fp16 outputs: |err| <= scale E + half step, ratio = the excess
    over the half step to E."""
    bad, worst = [], 0.0
    for name, e in exp.items():
        got, mk = vals[name], e["mask"]
        err = (got - e["ref"]).abs()[mk]
        E = e["E"][mk]
        ok_nan = not bool(torch.isnan(got[mk]).any())
        if e["kind"] == "f16":
            hs = half_ulp16(e["ref"], e["E"])[mk]
            exc = (err - hs).clamp_min(0)
        else:
            exc = err
        ratio = exc / E.clamp_min(1e-300)
        ratio = torch.where((exc == 0), torch.zeros_like(ratio), ratio)
        r = float(ratio.max()) if ratio.numel() else 0.0
        if not ok_nan:
            r = float("inf")
        if r > scale:
            bad.append(name)
        worst = max(worst, r)
    return bad, worst


def differs(c, sab):
    """where the sabotaged reference leaves the bound of the true one: list of (output, count of elements)"""
    a, b = reference(c, src=c["src_clean"]), reference(c, sab, src=c["src_clean"])      # finite everywhere: a sabotaged map reads other rows
    hits = []
    for name, e in a.items():
        s = b[name]
        n = int((e["mask"] != s["mask"]).sum())
        both = e["mask"] & s["mask"]
        lim = e["E"] + (half_ulp16(e["ref"], e["E"]) if e["kind"] == "f16" else 0.0)
        # a kernel that did what the sabotage does would be off by this much from the true reference (its own rounding aside)
        n += int((((e["ref"] - s["ref"]).abs() > 2 * lim) & both).sum())
        if n:
            hits.append((name, n))
    return hits


# ------------------------------------------------------------------------------------------------------------ cases
def forms_of(c):
    """the tile-form overrides that admit the case (launch_wide is reached: DIRECT epilogues, or STORE wider than 64 columns)"""
    if c["epi"] == EPI["store"] and c["N"] <= 64:
        return ()
    out = []
    for f in FORMS:
        if f == 0x90 and not (c["dtype"] == 0 and c["N"] % 256 == 0 and (c["epi"] != EPI["qkv"] or (2 * c["rope_D"]) % 256 == 0)):
            continue
        if f == 0x90 and c.get("act") == ACT["gelu"]:          # kgemm_big_launch has no GELU instantiation: it refuses the launch
            continue
        out.append(f)
    return tuple(out)


def build(name, group, seed=1, dtype=0, epi=0, nseq=1, Lout=8, M=None, N=64, K=(64,), taps=((0, 0),), a_len=None, seq_len=None,
          a_seq_map=None, a_off=0, a_stride=1, a_seq_rows=None, pad_mode=PAD_ZERO, reflect_min=0, c_off=0, c_seq_rows=None, ldc=None,
          vec_ok=None, terms=(), act=0, act_slope=0.0, amp=1.0, out_scale=0.0, post_n=None, form=0, rope_D=0, vt_mode=0, q_scale=0.0,
          want=("c32",), select=False, n_phys=None):
    g = gen(seed)
    M = nseq * Lout if M is None else M
    a_len = Lout * a_stride if a_len is None else a_len
    lens = list(seq_len) if seq_len is not None else None
    longest = max(lens) if lens else a_len
    a_seq_rows = longest + 2 * a_off if a_seq_rows is None else a_seq_rows
    if n_phys is None:
        n_phys = (max(a_seq_map) + 1) if a_seq_map is not None else nseq
    c_seq_rows = Lout + c_off if c_seq_rows is None else c_seq_rows
    paired, qkv = epi in (1, 2), epi == 3
    width = N // 2 if paired else (2 * rope_D if qkv else N)
    if vec_ok is None:
        vec_ok = int(N % 8 == 0)
    if ldc is None:
        ldc = (width + 7) // 8 * 8 + (8 if vec_ok or paired or qkv else 3)      # canary columns behind the written width
    c = dict(name=name, group=group, dtype=dtype, epi=epi, form=form, M=M, N=N, Lout=Lout, a_seq_rows=a_seq_rows, a_off=a_off,
             a_stride=a_stride, a_len=a_len, pad_mode=pad_mode, reflect_min=reflect_min, c_seq_rows=c_seq_rows, c_off=c_off, ldc=ldc,
             vec_ok=vec_ok, act=act, act_slope=act_slope, out_scale=out_scale, post_relu=int("relu" in terms), taps=list(taps),
             seq_len=lens, a_seq_map=list(a_seq_map) if a_seq_map is not None else None, rope_D=rope_D, vt_mode=vt_mode, q_scale=q_scale,
             want_c32=int("c32" in want), want_c16=int("c16" in want or qkv), want_c16_lo=int("c16_lo" in want))
    if qkv:
        c["want_c32"] = 0
    Ks = [K[i] for i, _ in taps]
    Ktot = sum(Ks)
    if select:       # activation-only: one k-tile, W a 0 / 1 selection matrix, A values exact in fp16
        assert len(K) == 1 and len(taps) == 1 and N <= K[0]
        W = torch.zeros(N, K[0])
        W[torch.arange(N), torch.arange(N)] = 1.0
        clean = [(torch.linspace(-amp, amp, n_phys * a_seq_rows * K[0]).reshape(-1, K[0])[torch.randperm(n_phys * a_seq_rows, generator=g)]).half().float()]
    else:
        W = randn(g, N, Ktot, scale=amp / math.sqrt(Ktot))
        clean = [randn(g, n_phys * a_seq_rows, k) for k in K]
    c["W"] = W
    c["src_clean"] = clean
    # NaN in every source row the row map must not read: rows above seq_len, below a_off, of skipped sequences, behind strides
    c["src"] = clean
    read = [torch.zeros(t.shape[0], dtype=torch.bool) for t in clean]
    for t, idx in enumerate(source_rows(c)):
        read[taps[t][0]][idx[idx >= 0]] = True
    c["src"] = [torch.where(r[:, None], t, torch.full_like(t, float("nan"))) for t, r in zip(clean, read)]
    rows = c_rows_of(c)
    if "bias" in terms:
        b = randn(g, N)
        b[0::2] += 1.5           # a different bias for even and odd columns: a swapped pair shows
        b[1::2] -= 1.0
        c["bias"] = b
    if "rowvec0" in terms:
        c["rowvec"] = randn(g, N)
    if "rowvecN" in terms:
        c["rowvec"] = randn(g, nseq, N)
    if "gate0" in terms:
        c["gate"] = randn(g, N) + 0.5
    if "gateN" in terms:
        c["gate"] = randn(g, nseq, N) + 0.5
    if "res" in terms:
        c["res"] = randn(g, rows, ldc) - (2.0 if "relu" in terms else 0.0)      # a negative residual in front of the relu
    if "res2" in terms:
        c["res2"] = randn(g, rows, ldc)
    if "res_c32" in terms:
        c["c_init"] = randn(g, rows, ldc)
        c["res"] = "c32"
    if "res2_c32" in terms:
        c["c_init"] = randn(g, rows, ldc)
        c["res2"] = "c32"
    if "snake" in terms:
        c["post_n"] = N if post_n is None else post_n
        c["post_a"] = randn(g, max(c["post_n"], 1)).abs() + 0.5
        c["post_ib"] = randn(g, max(c["post_n"], 1)).abs() + 0.25
    if qkv:
        c["rope"] = rope_unit(g, Lout)
        c["vt_ld"] = (Lout + 63) // 64 * 64
    return c


ALL_TERMS = ("bias", "rowvecN", "gateN", "res", "res2", "relu", "snake")


def conv_taps(k, d, centred):
    left = ((k - 1) * d) // 2 if centred else (k - 1) * d
    return [(0, t * d - left) for t in range(k)]


_CASES = None


def all_cases():
    global _CASES
    if _CASES is not None:
        return _CASES
    cs = []
    S, W, T, Q = EPI["store"], EPI["swiglu"], EPI["tanhsig"], EPI["qkv"]
    # ---- tiles and ring
    for M in (1, 63, 64, 65, 129, 257):
        for N in (8, 24, 64, 72, 136):
            cs.append(build(f"tile-M{M}-N{N}", "tiles", seed=M + N, Lout=M, N=N, K=(64,), terms=("bias",), want=("c32", "c16")))
    for dtype in (0, 1):
        for form in (0x40, 0x10):
            for K in (32, 64, 200, 328):
                cs.append(build(f"ring-{'f16' if dtype == 0 else 'f32'}-form{form:02x}-K{K}", "tiles", seed=K + form + dtype, dtype=dtype, Lout=65, N=72,
                                K=(K,), form=form, terms=("bias",)))
    cs.append(build("group-M130-N576-form50", "tiles", seed=5, Lout=130, N=576, K=(64,), form=0x50, terms=("bias",)))
    cs.append(build("grid9-M129-N136-K200", "tiles", seed=6, Lout=129, N=136, K=(200,), terms=("bias",)))
    # ---- scalar epilogue: every STORE term at once
    for N in (1, 5, 18, 33):
        cs.append(build(f"scalar-N{N}", "scalar", seed=10 + N, nseq=2, Lout=37, N=N, K=(40,), vec_ok=0, terms=ALL_TERMS, act=ACT["silu"],
                        out_scale=0.75, post_n=max(N - 3, 1), want=("c32", "c16", "c16_lo")))
    cs.append(build("scalar-N24-vec0", "scalar", seed=15, nseq=2, Lout=9, N=24, K=(64,), vec_ok=0, terms=ALL_TERMS, act=ACT["lrelu"], act_slope=0.1,
                    out_scale=1.5, post_n=13, want=("c32", "c16", "c16_lo")))
    # the scalar epilogue under the launch_wide forms: wider than 64 columns, an ldc that is no multiple of 8
    cs.append(build("scalar-N72-vec0", "scalar", seed=16, nseq=2, Lout=35, N=72, K=(64,), vec_ok=0, ldc=77, terms=ALL_TERMS, act=ACT["silu"], out_scale=0.75,
                    post_n=67, want=("c32", "c16", "c16_lo")))
    cs.append(build("scalar-N130-vec0", "scalar", seed=17, nseq=2, Lout=70, N=130, K=(96,), vec_ok=0, terms=("bias", "rowvecN", "res", "relu"), want=("c32", "c16")))
    # ---- STORE terms, vec_ok = 1
    for i, terms in enumerate((("bias",), ("rowvec0",), ("rowvecN",), ("gate0",), ("gateN",), ("res",), ("res2",), ("res", "res2"), ("res", "relu"),
                               ("res_c32",), ("res2_c32",), ("snake",), ALL_TERMS)):
        sc = 0.6 if ("res" in terms and "res2" in terms) else 0.0
        cs.append(build("store-" + "+".join(terms), "store", seed=20 + i, nseq=3, Lout=23, N=72, K=(96,), terms=terms, out_scale=sc,
                        act=ACT["silu"] if terms == ALL_TERMS or terms[0].startswith("gate") else 0, post_n=61 if terms == ALL_TERMS else None,
                        want=("c32", "c16", "c16_lo") if "snake" in terms else ("c32", "c16")))
    cs.append(build("store-snake-N136-post100", "store", seed=40, nseq=2, Lout=70, N=136, K=(64,), terms=("bias", "snake"), post_n=100,
                    want=("c32", "c16", "c16_lo")))
    # whole 256-column tiles: the 256 x 256 form (0x90) admits these STORE launches
    cs.append(build("store-N256-all", "store", seed=41, nseq=2, Lout=133, N=256, K=(128,), terms=ALL_TERMS, act=ACT["silu"], out_scale=0.6, post_n=250,
                    want=("c32", "c16", "c16_lo")))
    cs.append(build("gelu-N256", "act", seed=93, nseq=1, Lout=130, N=256, K=(64,), act=ACT["gelu"], amp=4.0, terms=("bias", "res"), want=("c32", "c16")))
    for name, code in ACT.items():
        if name == "none":
            continue
        slope = {"clamp": 3.0, "lrelu": 0.0}.get(name, 0.0)
        cs.append(build(f"act-{name}", "act", seed=50 + code, Lout=70, N=72, K=(64,), act=code, act_slope=slope, amp=6.0, terms=("bias",), want=("c32", "c16")))
        cs.append(build(f"actonly-{name}", "actonly", seed=70 + code, Lout=130, N=64, K=(64,), act=code, act_slope=slope, amp=20.0, select=True))
    cs.append(build("act-lrelu-slope0.2", "act", seed=90, Lout=33, N=72, K=(64,), act=ACT["lrelu"], act_slope=0.2, amp=6.0))
    for want in (("c32",), ("c16",), ("c32", "c16")):
        cs.append(build("gelu-" + "+".join(want), "act", seed=91, dtype=0, Lout=70, N=136, K=(64,), act=ACT["gelu"], amp=4.0, terms=("bias", "res"), want=want))
    cs.append(build("gelu-f32", "act", seed=92, dtype=1, Lout=70, N=24, K=(40,), act=ACT["gelu"], amp=4.0, terms=("bias",)))
    # ---- row maps
    for Lout in (1, 5, 13, 64):
        for st in (1, 2, 5):
            ln = Lout * st
            cs.append(build(f"map-L{Lout}-stride{st}", "rowmap", seed=100 + Lout + st, nseq=3, Lout=Lout, N=24, K=(64,), a_stride=st, a_off=1,
                            a_len=ln, a_seq_rows=ln + 2, taps=conv_taps(3, 1, True), terms=("bias",)))
    for k in (1, 3, 7, 16):
        for d in (1, 3):
            for centred in (False, True):
                cs.append(build(f"taps-k{k}-d{d}-{'centred' if centred else 'causal'}", "rowmap", seed=120 + k + d, nseq=2, Lout=19, N=24, K=(32,),
                                taps=conv_taps(k, d, centred), terms=("bias",)))
    cs.append(build("taps-48", "rowmap", seed=130, nseq=2, Lout=21, N=72, K=(64,), taps=[(0, t - 24) for t in range(48)]))
    cs.append(build("concat-2src", "rowmap", seed=131, nseq=2, Lout=17, N=72, K=(64, 40), taps=[(0, 0), (1, 0)], terms=("bias",)))
    cs.append(build("concat-3src", "rowmap", seed=132, nseq=2, Lout=17, N=72, K=(72, 64, 24), taps=[(0, 0), (1, -1), (2, 1)], terms=("bias",), want=("c32", "c16")))
    for mode, nm in ((PAD_ZERO, "zero"), (PAD_REFLECT, "reflect")):
        cs.append(build(f"ragged-{nm}", "rowmap", seed=133 + mode, nseq=3, Lout=11, N=24, K=(64,), seq_len=[11, 1, 0], a_seq_rows=11,
                        pad_mode=mode, taps=conv_taps(3, 1, True), terms=("bias",)))
    cs.append(build("reflect-min0", "rowmap", seed=140, nseq=2, Lout=12, N=24, K=(64,), pad_mode=PAD_REFLECT, taps=conv_taps(5, 2, True)))
    pad = 4                                                       # k = 5, dilation 2: left = right = 4
    for ln in (1, 2, pad, pad + 1):
        cs.append(build(f"reflect-min-len{ln}", "rowmap", seed=141 + ln, nseq=3, Lout=6, N=24, K=(64,), pad_mode=PAD_REFLECT, reflect_min=pad + 1,
                        seq_len=[ln, 6, ln], a_seq_rows=6, taps=conv_taps(5, 2, True), terms=("bias",)))
    for ln in (1, 3):
        cs.append(build(f"clamp-len{ln}", "rowmap", seed=150 + ln, nseq=2, Lout=9, N=24, K=(64,), pad_mode=PAD_CLAMP, seq_len=[ln, 9], a_seq_rows=9,
                        taps=[(0, -12), (0, -1), (0, 0), (0, 2), (0, 12)]))
    cs.append(build("seqmap-gather", "rowmap", seed=160, nseq=4, Lout=7, N=24, K=(64,), a_seq_map=[2, 0, 0, 1], n_phys=4, taps=conv_taps(3, 1, True), terms=("bias",)))       # sequence 3 of the source is skipped
    cs.append(build("c_off3", "rowmap", seed=161, nseq=3, Lout=10, N=72, K=(64,), c_off=3, c_seq_rows=15, terms=("bias",), want=("c32", "c16")))
    cs.append(build("window", "rowmap", seed=162, nseq=2, Lout=6, N=72, K=(64,), a_off=5, c_off=5, a_len=6, a_seq_rows=11, c_seq_rows=11,
                    terms=("bias", "res")))
    # ---- SWIGLU / TANHSIG
    for epi, nm in ((W, "swiglu"), (T, "tanhsig")):
        for N in (32, 64, 160, 256):
            for M in (1, 65, 130):
                cs.append(build(f"{nm}-N{N}-M{M}", "paired", seed=200 + N + M + epi, epi=epi, Lout=M, N=N, K=(64,), terms=("bias",), amp=2.0, want=("c16",)))
        cs.append(build(f"{nm}-rowvec0", "paired", seed=230 + epi, epi=epi, nseq=3, Lout=21, N=64, K=(64,), terms=("bias", "rowvec0"), want=("c16", "c32")))
        cs.append(build(f"{nm}-rowvecN", "paired", seed=232 + epi, epi=epi, nseq=3, Lout=21, N=160, K=(96,), terms=("rowvecN",), want=("c16",)))
        cs.append(build(f"{nm}-sat30", "paired", seed=234 + epi, epi=epi, Lout=66, N=64, K=(64,), terms=("bias",), amp=10.0, want=("c16", "c32")))
    cs.append(build("tanhsig-f32", "paired", seed=240, dtype=1, epi=T, nseq=2, Lout=33, N=64, K=(40,), terms=("bias", "rowvec0"), amp=2.0, want=("c16", "c32")))
    cs.append(build("tanhsig-reflect", "paired", seed=241, epi=T, nseq=3, Lout=9, N=32, K=(64,), pad_mode=PAD_REFLECT, reflect_min=3, seq_len=[9, 2, 5],
                    a_seq_rows=9, taps=conv_taps(5, 1, True), terms=("rowvec0",), want=("c16",)))
    # ---- QKV_ROPE
    qs = 0.125 * LOG2E
    for D in (128, 256):
        for Lout, nseq in ((1, 1), (5, 3), (7, 3), (64, 1), (70, 1), (70, 3) if D == 128 else (5, 1)):
            for mode in (0, 1, 2):
                cs.append(build(f"qkv-D{D}-L{Lout}x{nseq}-vt{mode}", "qkv", seed=300 + D + Lout + nseq + mode, epi=Q, nseq=nseq, Lout=Lout, N=3 * D, K=(64,),
                                rope_D=D, vt_mode=mode, q_scale=qs))
    cs.append(build("qkv-D128-L7-M19", "qkv", seed=330, epi=Q, nseq=3, Lout=7, M=19, N=384, K=(128,), rope_D=128, vt_mode=1, q_scale=qs))
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    _CASES = cs
    return cs


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


GROUPS = ("tiles", "scalar", "store", "act", "actonly", "rowmap", "paired", "qkv")
