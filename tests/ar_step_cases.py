"""The AR step kernels at op level (csrc/ar_prefill.h, ar_decode1.h, ar_batch.h, ar_prefill_attn.h): the float64 reference, the
derived error bound, the cases, an fp32 emulation and the named sabotages.  test_host_ar_step.py pins the reference to the
oracle and shows that every sabotage is caught; test_gpu_ar_step.py runs the kernels (ops.ar_attn, ops.ar_linear).

REFERENCE.  Plain float64 torch on exactly the operands the kernel gets (fp32 inputs, fp16 weights widened):
  attention   y[h] = softmax(q[h] . k / 8 over cache rows 0 .. kv_pos of KV head h // (H / Hkv)) . v
  rope        pair (2 i, 2 i + 1) of every 64-wide head of q and k rotated with table entry (input_pos, i); k, v -> row kv_pos
  dec_attn2   q, k, v = qkv_raw / rms(hres); rotation; attention INCLUDING the new key (used for row kv_pos whatever the cache
              holds there); y rounded to fp16; part[h][n] = sum_d wo[n][64 h + d] y[d]
  linears     RMSNorm (x rsqrt(mean x^2 + eps) gamma), W x, SwiGLU on interleaved (w1_j, w3_j) rows, + residual

BOUND (absolute, per output element; u = 2^-24, nothing fitted to a kernel's output).  First-order terms; every relative term
is below 1e-3, so the neglected products are below 1e-3 of the bound, and the fp32 emulation is held to HALF the bound.
  dot(n)      fp32 sum of n products in ANY order: (n + 2) u sum|terms|                                       [Higham 3.5]
  exp         __expf(x) = v_exp_f32(x log2 e): the subtraction and the scaling round the argument (2 u |x|), the instruction is
              good to 1 ulp (2 u)  ->  relative 2 u (|x| + 1); expf is no worse
  rsqrt, div  v_rsq_f32 1 ulp (2 u); a / b without correctly-rounded division 2.5 ulp (5 u)
  rstd        mean of n squares (n + 2) u + the add and divide 2 u, halved by the root, + the instruction:  e_r = (n + 4) u / 2 + 2 u
              (dec_attn2: n = the depth of its fixed lane-then-tree sum, D / 64 + 7, since its y meets an fp16 rounding)
  softmax     the result is invariant to the shift m, so only each score's own error d_j (dot(64) at its own |q|.|k| / 8, plus
              input errors) and the exp errors count: weight j is off by e_j = d_j + (n_r + 1) (2 u (spread + 1) + u), spread =
              max s - min s of the case, n_r = the kernel's rescale steps (chunks or batches + merge stages).
              y = sum p v / sum p:  E = (max e_j + (n + 2) u) (sum w |v| + |y|) + 5 u |y|
  fp16 out    + half an fp16 ulp at |ref| + E.  That half step is the format's, not an estimate, and a correctly rounded result
              reaches it by itself; the error / bound RATIO of an fp16 output is therefore that of the excess over the half
              step to E, while the assertion is |got - ref| <= E + half step on every element
  rotation    dot(2) of (a c, b s), contracted into an fma or not: 4 u (|a c| + |b s|)
  dec_attn2   q, k carry (e_r + 5 u) (|a c| + |b s|) from the scale and the rotation, v carries (e_r + u) |v|.  The kernel rounds
              y to fp16 and so does the reference: the two fp16 values are EQUAL unless the reference y lies within E of a
              midpoint between two fp16 neighbours, where they may be one step apart (fp16_flip).  part carries that step
              through |wo|, + dot(64) -- so a y that is not rounded, or rounded elsewhere, shows
  bgemm NORM  x gamma is rounded to fp16 before the MFMA: 2^-11 |x gamma| (or 2^-25 absolute below the normal range) through
              |w| rstd; rstd is applied after the sum
  SwiGLU      silu'(a) <= 1.1:  1.1 |b| E_a + |silu a| E_b + |silu(a) b| (2 u (|a| + 1) + 7 u), then fp16
"""
import math

import torch

U = 2.0 ** -24
GUARD = 2
F32_FILL, F16_FILL = -777.25, -777.0
NAMES = ("qkv", "wo", "w13", "w2", "head")


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).float()


def ulp16(x):
    """the spacing of fp16 at |x| (float64 tensor), subnormal spacing below 2^-14"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 10)


def rope_unit(g, Lmax):
    """unit (cos, sin) pairs, different for every (position, pair)"""
    ang = torch.rand(Lmax, 32, generator=g, dtype=torch.float64) * 2 * math.pi
    return torch.stack([ang.cos(), ang.sin()], -1).float()


def rope_bf16(Lmax, base=10000.0):
    """the model's table (svc_ar_create): bf16-rounded cos / sin"""
    inv = 1.0 / (base ** (torch.arange(0, 64, 2).float() / 64))
    ang = torch.outer(torch.arange(Lmax).float(), inv)
    return torch.stack([ang.cos(), ang.sin()], -1).to(torch.bfloat16).float()


def caches(g, n_slots, Hkv, Lmax, scale=0.5):
    """seeded finite NON-ZERO values in every row"""
    def one():
        t = randn(g, n_slots, Hkv, Lmax, 64, scale=scale)
        return torch.where(t == 0, torch.full_like(t, 0.25), t)
    return one(), one()


# ------------------------------------------------------------------------------------------------------------ reference
def ref_rotate(x, rope, ip, heads, sab=None):
    """x (..., heads * 64) float64, rotated per head with rope[ip]; returns (rotated, |a||c| + |b||s| per element)"""
    tab = rope.double()
    xr = x.reshape(heads, 32, 2)
    if sab == "pair_over_row":          # the pair index counted over the whole row, not per head
        flat = tab.reshape(-1, 2)
        idx = (ip * 32 + torch.arange(heads * 32)) % flat.shape[0]
        cs = flat[idx].reshape(heads, 32, 2)
    else:
        cs = tab[ip][None].expand(heads, 32, 2)
    c, s = cs[..., 0], cs[..., 1]
    a, b = xr[..., 0], xr[..., 1]
    o = torch.stack([a * c - b * s, b * c + a * s], -1).reshape(-1)
    ab = torch.stack([a.abs() * c.abs() + b.abs() * s.abs(), b.abs() * c.abs() + a.abs() * s.abs()], -1).reshape(-1)
    return o, ab


def ref_rope_cache(qkv, rope, ip, kp, H, Hkv, sab=None):
    """one row: (q_out (D,), k_row (kvd,), v_row (kvd,), cache row index, abs companions of q and k)"""
    D, kvd = 64 * H, 64 * Hkv
    x = qkv.double()
    rp = kp if sab == "rot_kv_pos" else ip
    q, qa = ref_rotate(x[:D], rope, rp, H, sab)
    k, ka = ref_rotate(x[D:D + kvd], rope, rp, Hkv, sab)
    v = x[D + kvd:D + 2 * kvd]
    if sab == "v_rotated":
        v = ref_rotate(v, rope, rp, Hkv)[0]
    return dict(q=q, k=k, v=v, row=kp + 1 if sab == "row_plus_1" else kp, qa=qa, ka=ka)


def ref_attn_head(q, K, V, n, sab=None):
    """q (64,), K, V (L, 64) float64, n valid keys -> y (64,) and what the bound needs"""
    if sab == "keys_plus_1":
        n = min(n + 1, K.shape[0])
    if sab == "keys_minus_1":
        n = max(n - 1, 1)
    idx = torch.arange(n)
    if sab == "seam_256" and n > 256:
        idx = idx[idx != 256]
    if sab == "seam_512" and n > 512:
        idx = idx[idx != 512]
    if sab == "merge_row_lost" and n > 62:       # the 16-lane row of key slots 62, 63 (keys j = 62, 63 mod 64)
        idx = idx[(idx % 64) < 62]
    k, v = K[idx], V[idx]
    s = (k @ q) * (1.0 if sab == "no_scale" else 0.125)
    if sab == "no_rescale":                      # chunks of 32 keys; the accumulators keep their old scale when the maximum moves
        m, l, acc = None, 0.0, torch.zeros(64, dtype=torch.float64)
        for c0 in range(0, len(idx), 32):
            sc = s[c0:c0 + 32]
            m = sc.max() if m is None else torch.maximum(m, sc.max())
            p = (sc - m).exp()
            l, acc = l + p.sum(), acc + p @ v[c0:c0 + 32]
        y, w = acc / l, torch.softmax(s, 0)
    else:
        w = torch.softmax(s, 0)
        y = w @ v
    return dict(y=y, absv=w @ v.abs(), sabs=(k.abs() @ q.abs()) * 0.125, spread=float(s.max() - s.min()), n=len(idx), w=w, idx=idx)


def kv_head(h, H, Hkv, sab=None):
    return h % Hkv if sab == "kv_head_mod" else h // (H // Hkv)


def ref_attn_row(q, kc, vc, kp, H, Hkv, sab=None):
    """q (D,), kc, vc (Hkv, Lmax, 64) of the row's slot -> list of per-head dicts"""
    return [ref_attn_head(q.double()[64 * h:64 * h + 64], kc[kv_head(h, H, Hkv, sab)].double(), vc[kv_head(h, H, Hkv, sab)].double(), kp + 1, sab)
            for h in range(H)]


def attn_bound(r, n_resc, e_score_in=None, extra=None):
    """E before the output rounding, for one head's dict; e_score_in: per-key absolute score error from inexact inputs"""
    d = 66 * U * r["sabs"] + (e_score_in if e_score_in is not None else 0.0)
    e = float(d.max()) + (n_resc + 1) * (2 * U * (r["spread"] + 1) + U)
    E = (e + (r["n"] + 2) * U) * (r["absv"] + r["y"].abs()) + 5 * U * r["y"].abs()
    return E + (extra if extra is not None else 0.0)


def half_ulp16(ref, E):
    """the rounding of an fp16 output: half a step at the largest magnitude the computed value can have"""
    return 0.5 * ulp16(ref.abs() + E)


N_RESC = {0: lambda n: 0, 1: lambda n: -(-n // 256) + 2, 2: lambda n: -(-n // 512), 3: lambda n: -(-n // 32)}


def ref_attention(kind, q, kc, vc, kp, H, Hkv, sab=None):
    """kinds 0, 2, 3 for one row: (y (D,), arithmetic bound E (D,), the fp16 output's half step (D,))"""
    heads = ref_attn_row(q, kc, vc, kp, H, Hkv, sab)
    y = torch.cat([r["y"] for r in heads])
    E = torch.cat([attn_bound(r, N_RESC[kind](kp + 1)) for r in heads])
    return y, E, half_ulp16(y, E)


def fp16_flip(y, E):
    """how far the kernel's fp16(y) can be from fp16(ref y), per element: 0 unless the reference lies within E of a midpoint
    between two fp16 neighbours -- there the computed value may round to the other one, a whole step away"""
    y16 = y.half()
    b = y16.view(torch.int16)
    nb = [(b + 1).view(torch.float16).double(), (b - 1).view(torch.float16).double()]
    y16 = y16.double()
    near = torch.zeros_like(y, dtype=torch.bool)
    step = torch.zeros_like(y)
    for n in nb:
        near |= ((y - (y16 + n) / 2).abs() <= E) | (y16 == 0)
        step = torch.maximum(step, torch.where(y16 == 0, torch.full_like(y, 2.0 ** -24), (n - y16).abs()))
    return torch.where(near, step, torch.zeros_like(y))


def e_rstd(n):
    return (n + 4) * U / 2 + 2 * U


def ref_dec_attn2(c, sab=None):
    """kind 1 -> dict(part (H, D), k (kvd,), v (kvd,), row, and their bounds)"""
    H, Hkv, D = c["H"], c["Hkv"], 64 * c["H"]
    kvd = 64 * Hkv
    ip, kp = c["pos"][0][0], c["pos"][1][0]
    x = c["x"][0].double()
    hres = c["hres"].double()
    n_rms = D + 64 if sab == "rstd_length" else D
    rstd = 1.0 / torch.sqrt((hres * hres).sum() / n_rms + c["eps"])
    rc = ref_rope_cache(x * rstd, c["rope"], ip, kp, H, Hkv, sab)
    # 1 / rms in dec_attn2: a lane squares and adds its D / 64 <= 16 elements, then one tree over the wave (4 DPP steps + 3 adds);
    # positive terms, so the sum is good to (its depth) u whatever the values.  No other order exists in the kernel (no fast-math)
    er = e_rstd(D // 64 + 7)
    kc, vc = c["kc"][c["slots"][0]].double().clone(), c["vc"][c["slots"][0]].double().clone()
    if sab != "cache_row_read":
        kc[:, kp] = rc["k"].reshape(Hkv, 64)
        vc[:, kp] = rc["v"].reshape(Hkv, 64)
    wo = c["wo"].double()
    part, Ep = torch.zeros(H, D, dtype=torch.float64), torch.zeros(H, D, dtype=torch.float64)
    rows_per = -(-D // 8)
    for h in range(H):
        hk = kv_head(h, H, Hkv, sab)
        q = rc["q"][64 * h:64 * h + 64]
        r = ref_attn_head(q, kc[hk], vc[hk], kp + 1, sab)
        qa = rc["qa"][64 * h:64 * h + 64]
        e_in = (er + 5 * U) * (kc[hk][r["idx"]].abs() @ qa) * 0.125
        new = (r["idx"] == kp).nonzero().reshape(-1)
        extra = 0.0
        if len(new):
            e_in[new] += (er + 5 * U) * (rc["ka"][64 * hk:64 * hk + 64] @ q.abs()) * 0.125
            extra = r["w"][new] * (er + U) * rc["v"][64 * hk:64 * hk + 64].abs()
        E = attn_bound(r, N_RESC[1](kp + 1), e_in, extra)
        y16 = r["y"] if sab == "y_not_rounded" else r["y"].half().double()
        wh = wo[:, 64 * h:64 * h + 64]
        if sab == "wo_slice_shift":
            wh = torch.roll(wh, -rows_per, 0)
        part[h] = wh @ y16
        Ep[h] = wh.abs() @ fp16_flip(r["y"], E) + 66 * U * (wh.abs() @ y16.abs())
    return dict(part=part, E_part=Ep, k=rc["k"], v=rc["v"], row=rc["row"], E_k=(er + 5 * U) * rc["ka"], E_v=(er + U) * rc["v"].abs())


def ref_linear(c, sab=None):
    """one linear of c["role"] on c["path"] -> dict(out (rows, N) float64, E (rows, N)); qkv roles of paths 0, 1: out is the
    unrotated projection's rotation: dict(q, k, v, E_q, E_k, E_v) per row in lists; path 2 roles 1, 2 add out2 / E2"""
    path, role, D, I = c["path"], c["role"], c["D"], c["I"]
    x = c["x"].double()
    W = c["W"].double()
    K = W.shape[1]
    norm = role in ("qkv", "w13", "head") and not (path == 2 and role == "qkv")
    Ex_rel, xin_abs = 0.0, None
    if path == 2 and role == "w13":              # h = h_in + sum of the head partials, summed in fp32: (H + 1) u sum|terms|
        hsum_abs = x.abs() + c["part"].double().abs().sum(0)
        x = x + c["part"].double().sum(0)
        E_h = (c["H"] + 1) * U * hsum_abs
        xin_abs = E_h
    out2 = E2 = None
    if norm:
        n_rms = K + 64 if sab == "rstd_length" else K
        rstd = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / n_rms + c["eps"])
        g = c["gamma"].double()
        xn = x * rstd * ((1 + g) if sab == "gamma_added" else g)
        er = e_rstd(K)
        if path == 1:                            # fp16(x gamma) into the MFMA, rstd after the sum
            xg = (x * g).abs()
            T = (torch.maximum(2.0 ** -11 * xg, torch.full_like(xg, 2.0 ** -25)) * rstd) @ W.abs().T + (er + U) * (xn.abs() @ W.abs().T)
        else:
            T = (er + 2 * U) * (xn.abs() @ W.abs().T)
        if xin_abs is not None:
            # the error of h goes through the weights, and moves rstd by at most |E_h|_2 / |h|_2 (Cauchy-Schwarz on sum h dh / sum h^2)
            T = T + (xin_abs * rstd * g.abs()) @ W.abs().T + float(xin_abs.norm() / x.norm()) * (xn.abs() @ W.abs().T)
    else:
        xn, T = x, 0.0
    if path == 2 and role == "wo":               # dec_w2qkv: rows [0, D) h_out = h_mid + w2 ff; rows [D, D + Nqkv) qkv_raw = wc [ff | h_mid]
        W2 = c["W2"].double()
        hm = c["res"].double()
        both = torch.cat([x, hm], -1)
        out = hm + x @ W2.T
        E = (I + 2) * U * (x.abs() @ W2.abs().T) + U * out.abs()
        out2 = both @ W.T
        E2 = (I + D + 4) * U * (both.abs() @ W.abs().T)
    else:
        acc = xn @ W.T
        E = T + (K + 2) * U * (xn.abs() @ W.abs().T)
        out = acc
    if role in ("wo", "w2") and not (path == 2 and role == "wo"):
        res = c["res"].double()
        out = out + res * (2 if sab == "residual_twice" else 1)
        E = E + U * out.abs()
    if sab == "last_row_doubled" and out.shape[1] % 2:
        out = out.clone()                        # the odd last row has no partner: its sum taken twice
        out[:, -1] = 2 * out[:, -1]
    if role == "w13":
        if sab == "glu_halves":
            a, b = out[:, :I], out[:, I:]
            Ea, Eb = E[:, :I], E[:, I:]
        else:
            a, b = out[:, 0::2], out[:, 1::2]
            Ea, Eb = E[:, 0::2], E[:, 1::2]
        sl = a / (1 + (-a).exp())
        o = sl * b
        Eo = 1.1 * b.abs() * Ea + sl.abs() * Eb + o.abs() * (2 * U * (a.abs() + 1) + 7 * U)
        r = dict(out=o, E=Eo, half=half_ulp16(o, Eo))
        if path == 2:
            r.update(out2=x, E2=E_h)
        return r
    if role == "qkv" and path != 2:
        rows = []
        for s in range(out.shape[0]):
            rc = ref_rope_cache(out[s], c["rope"], c["pos"][0][s], c["pos"][1][s], c["H"], c["Hkv"], sab)
            # the rotation of an inexact projection: |c| E_a + |s| E_b, and its own two roundings
            Er = ref_rotate(E[s][:D + 64 * c["Hkv"]], c["rope"], c["pos"][0][s], c["H"] + c["Hkv"])[1]
            rc["E_q"] = Er[:D] + 4 * U * rc["qa"]
            rc["E_k"] = Er[D:] + 4 * U * rc["ka"]
            rc["E_v"] = E[s][D + 64 * c["Hkv"]:]
            rows.append(rc)
        return dict(rows=rows)
    r = dict(out=out, E=E)
    if out2 is not None:
        r.update(out2=out2, E2=E2)
    return r


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def emu_attn_head(q, K, V, n, streams, chunk):
    """fp32, the structure of the kernels: `streams` interleaved key streams (key j -> stream j % streams), each an online softmax
    in chunks of `chunk` of its keys with one rescale per chunk, merged in stream order with exp(m_i - M)"""
    q, K, V = q.float(), K.float()[:n], V.float()[:n]
    s = (K * (q * 0.125)).sum(-1, dtype=torch.float32)
    ms, ls, accs = [], [], []
    for st in range(min(streams, n)):
        ss, vv = s[st::streams], V[st::streams]
        m, l, acc = torch.tensor(-1e30), torch.tensor(0.0), torch.zeros(64)
        step = chunk if chunk else len(ss)
        for c0 in range(0, len(ss), step):
            sc = ss[c0:c0 + step]
            mn = torch.maximum(m, sc.max())
            scale = (m - mn).exp()
            p = (sc - mn).exp()
            l = l * scale + p.sum(dtype=torch.float32)
            acc = acc * scale + (p[:, None] * vv[c0:c0 + step]).sum(0, dtype=torch.float32)
            m = mn
        ms.append(m), ls.append(l), accs.append(acc)
    M = torch.stack(ms).max()
    w = (torch.stack(ms) - M).exp()
    num = (torch.stack(accs) * w[:, None]).sum(0, dtype=torch.float32)
    return num / (torch.stack(ls) * w).sum(dtype=torch.float32)


EMU_SHAPE = {0: (1, 0), 1: (64, 4), 2: (1, 512), 3: (4, 8)}      # kind -> (streams, keys of a stream per chunk)


def emu_attention(kind, q, kc, vc, kp, H, Hkv):
    st, ch = EMU_SHAPE[kind]
    return torch.cat([emu_attn_head(q[64 * h:64 * h + 64], kc[h // (H // Hkv)], vc[h // (H // Hkv)], kp + 1, st, ch) for h in range(H)]).half()


def emu_rotate(x, rope, ip, heads):
    xr = x.float().reshape(heads, 32, 2)
    c, s = rope[ip][None, :, 0], rope[ip][None, :, 1]
    return torch.stack([xr[..., 0] * c - xr[..., 1] * s, xr[..., 1] * c + xr[..., 0] * s], -1).reshape(-1)


def emu_dec_attn2(c):
    H, Hkv, D = c["H"], c["Hkv"], 64 * c["H"]
    kvd = 64 * Hkv
    ip, kp = c["pos"][0][0], c["pos"][1][0]
    h = c["hres"].float()
    rstd = torch.rsqrt((h * h).sum(dtype=torch.float32) / D + torch.tensor(c["eps"]))
    x = c["x"][0].float() * rstd
    q, k, v = emu_rotate(x[:D], c["rope"], ip, H), emu_rotate(x[D:D + kvd], c["rope"], ip, Hkv), x[D + kvd:]
    kc, vc = c["kc"][c["slots"][0]].clone(), c["vc"][c["slots"][0]].clone()
    kc[:, kp], vc[:, kp] = k.reshape(Hkv, 64), v.reshape(Hkv, 64)
    part = torch.zeros(H, D)
    for hh in range(H):
        y = emu_attn_head(q[64 * hh:64 * hh + 64], kc[hh // (H // Hkv)], vc[hh // (H // Hkv)], kp + 1, 64, 4).half().float()
        part[hh] = (c["wo"].float()[:, 64 * hh:64 * hh + 64] * y).sum(-1, dtype=torch.float32)
    return dict(part=part, k=k, v=v)


def emu_dot(xn, W, lanes, quarters=1):
    """fp32 products summed per lane (a lane owns the 8-element chunks lane, lane + lanes, ...), the lanes summed, the K quarters
    of the batched kernel in wave order"""
    K = W.shape[1]
    per = -(-(K // 32) // quarters) * 32
    rows = []
    for x in xn:
        out = None
        for qd in range(quarters):
            k0, k1 = qd * per, min(K, (qd + 1) * per)
            if k0 >= k1:
                p = torch.zeros(W.shape[0])
            else:
                prod = x[None, k0:k1] * W[:, k0:k1]
                n8 = (k1 - k0) // 8
                pad = -(-n8 // lanes) * lanes - n8
                prod = torch.nn.functional.pad(prod, (0, 8 * pad)).reshape(W.shape[0], -1, lanes, 8)
                p = prod.permute(0, 2, 1, 3).reshape(W.shape[0], lanes, -1).sum(-1, dtype=torch.float32).sum(-1, dtype=torch.float32)
            out = p if out is None else out + p
        rows.append(out)
    return torch.stack(rows)


def emu_linear(c):
    path, role, D, I = c["path"], c["role"], c["D"], c["I"]
    x, W = c["x"].float(), c["W"].float()
    K = W.shape[1]
    norm = role in ("qkv", "w13", "head") and not (path == 2 and role == "qkv")
    r = {}
    if path == 2 and role == "w13":
        for p in c["part"].float():
            x = x + p
        r["out2"] = x
    rstd = None
    if norm:
        rstd = torch.rsqrt((x * x).sum(-1, keepdim=True, dtype=torch.float32) / K + torch.tensor(c["eps"]))
        g = c["gamma"].float()
        xn = (x * g).half().float() if path == 1 else x * rstd * g
    else:
        xn = x
    if path == 2 and role == "wo":
        hm = c["res"].float()
        r["out"] = hm + emu_dot(x, c["W2"].float(), 64)
        r["out2"] = emu_dot(x, W[:, :I], 64) + emu_dot(hm, W[:, I:], 64)
        return r
    out = emu_dot(xn, W, 64 if path != 1 else 4, 4 if path == 1 else 1)
    if path == 1 and norm:
        out = out * rstd
    if role in ("wo", "w2"):
        out = out + c["res"].float()
    if role == "w13":
        a, b = out[:, 0::2], out[:, 1::2]
        out = ((a / (1 + (-a).exp())) * b).half()
    if role == "qkv" and path != 2:
        kvd = 64 * c["Hkv"]
        r["rows"] = [dict(q=emu_rotate(out[s][:D], c["rope"], c["pos"][0][s], c["H"]), k=emu_rotate(out[s][D:D + kvd], c["rope"], c["pos"][0][s], c["Hkv"]),
                          v=out[s][D + kvd:]) for s in range(out.shape[0])]
        return r
    r["out"] = out
    return r


# ------------------------------------------------------------------------------------------------------------ cases
HEADS = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 2), (9, 3), (12, 2), (16, 4)]
HEADS_PREFILL = HEADS + [(14, 2), (8, 1)]


def plant(c, g, slot, hk, kp, mode):
    """late dominant key: the last valid cache row of (slot, hk) lines up with every head's q, so the running maximum moves at the
    end; `maxima`: a key every 61 rows grows with its index, so maxima differ across key slots, rows and waves"""
    H, Hkv = c["H"], c["Hkv"]
    qh = c["qrow"].reshape(H, 64)[hk * (H // Hkv)]
    unit = qh / qh.norm()
    if mode == "late" and kp >= 1:
        c["kc"][slot, hk, kp - 1 if c["kind"] == 1 else kp] = unit * 48.0 / max(float(qh.norm()), 1e-3)
    if mode == "maxima":
        for i, j in enumerate(range(0, kp + 1, 61)):
            c["kc"][slot, hk, j] = unit * (8.0 + 0.5 * i) / max(float(qh.norm()), 1e-3)


def kp_tag(kps):
    kps = list(kps)
    return "_".join(map(str, kps[:3])) + (f"+{len(kps) - 3}" if len(kps) > 3 else "")


def attn_case(kind, H, Hkv, Lmax, kps, seed, n_slots=None, plant_mode=None, bf16=False, seq_S=None, slots=None):
    """kinds 0, 2: one row per kv_pos in kps (kind 2: one slot each); kind 1: kps = [kv_pos]; kind 3: sequences seq_S starting at
    kv_pos kps[i]"""
    g = gen(seed)
    D = 64 * H
    if kind == 3:
        kp = [k0 + s for k0, S in zip(kps, seq_S) for s in range(S)]
    else:
        kp = list(kps)
    R = len(kp)
    n_slots = n_slots or (R if kind == 2 else len(seq_S) if kind == 3 else 1)
    if slots is None:
        slots = list(range(n_slots))[::-1][:R if kind == 2 else len(seq_S) if kind == 3 else 1]      # non-ascending
    kc, vc = caches(g, n_slots, Hkv, Lmax)
    ip = [int(v) for v in torch.randint(0, Lmax, (R,), generator=g)]
    ip = [(p + 1) % Lmax if p == k else p for p, k in zip(ip, kp)]          # input_pos != kv_pos
    c = dict(kind=kind, H=H, Hkv=Hkv, Lmax=Lmax, kc=kc, vc=vc, slots=slots, pos=[ip, kp], seq_S=seq_S,
             name=f"k{kind}-H{H}x{Hkv}-L{Lmax}-kp{kp_tag(kps)}" + (f"-{plant_mode}" if plant_mode else "") + ("-bf16" if bf16 else ""))
    if kind == 1:
        c.update(x=randn(g, 1, D + 128 * Hkv, scale=0.6), hres=randn(g, D, scale=1.3), eps=1e-5, wo=randn(g, D, D, scale=0.05).half(),
                 rope=rope_bf16(Lmax) if bf16 else rope_unit(g, Lmax))
        rstd = 1.0 / math.sqrt(float((c["hres"].double() ** 2).mean()) + 1e-5)
        c["qrow"] = ref_rope_cache(c["x"][0].double() * rstd, c["rope"], ip[0], kp[0], H, Hkv)["q"].float()
    else:
        c["x"] = randn(g, R, D, scale=0.35)
        c["qrow"] = c["x"][-1]
    if plant_mode:
        row_slot = slots[0] if kind in (0, 1) else slots[-1]
        for hk in range(Hkv):
            plant(c, g, row_slot, hk, kp[-1], plant_mode)
    return c


def row_slot(c, r):
    """slot of row r of a kind 0 / 2 / 3 case"""
    if c["kind"] == 0:
        return c["slots"][0]
    if c["kind"] == 2:
        return c["slots"][r]
    acc = 0
    for i, S in enumerate(c["seq_S"]):
        acc += S
        if r < acc:
            return c["slots"][i]


def dec_attn2_cases():
    out = []
    for i, (H, Hkv) in enumerate(HEADS):
        out.append(attn_case(1, H, Hkv, 1030, [(0, 1, 7, 63, 255, 256, 257, 511, 512)[i]], 100 + i))
    for i, kp in enumerate((513, 767, 768, 1023, 1024, 1029)):
        out.append(attn_case(1, 2, 1, 1030, [kp], 120 + i))
    out.append(attn_case(1, 1, 1, 8, [7], 130))
    out.append(attn_case(1, 2, 1, 8, [0], 131))
    out.append(attn_case(1, 2, 1, 4096, [4095], 132))
    out.append(attn_case(1, 2, 1, 8192, [8191], 133))
    out.append(attn_case(1, 12, 2, 8192, [4097], 134))
    out.append(attn_case(1, 12, 2, 1030, [700], 135, plant_mode="late"))
    out.append(attn_case(1, 6, 2, 1030, [1029], 136, plant_mode="maxima"))
    out.append(attn_case(1, 4, 1, 1030, [300], 137, bf16=True))
    return out


BATTN_POS = [0, 31, 32, 510, 511, 512, 513, 1023, 1024, 1025]


def battn_cases():
    out = []
    for i, (B, (H, Hkv), Lmax) in enumerate([(1, (1, 1), 8), (16, (3, 1), 1030), (17, (4, 1), 1030), (33, (5, 1), 1030), (64, (2, 1), 1030),
                                             (17, (12, 2), 1030), (3, (6, 2), 8192), (2, (9, 3), 1030), (2, (16, 4), 1030)]):
        pool = [p for p in BATTN_POS if p < Lmax] + [Lmax - 1]
        kps = [pool[(b + i) % len(pool)] for b in range(B)]
        kps[0] = Lmax - 1 if Lmax == 8192 else kps[0]
        out.append(attn_case(2, H, Hkv, Lmax, kps, 200 + i))
    out.append(attn_case(2, 12, 2, 1030, [5, 1029, 600], 220, plant_mode="late"))
    out.append(attn_case(2, 6, 2, 1030, [700, 1029], 221, plant_mode="maxima"))
    out.append(attn_case(2, 2, 1, 8, [7, 0], 222))
    return out


def ar_attn_cases():
    pool = [0, 15, 16, 1022, 1023, 1024, 1025, 2047, 2048, 2049]
    out = [attn_case(0, 1, 1, 8, [7], 300), attn_case(0, 2, 1, 8, [0, 3, 7], 301)]
    for i, (S, (H, Hkv)) in enumerate([(3, (3, 1)), (8, (4, 1)), (17, (5, 1)), (3, (6, 2)), (1, (9, 3)), (3, (12, 2)), (1, (16, 4))]):
        out.append(attn_case(0, H, Hkv, 2050, [pool[(s + 3 * i) % len(pool)] for s in range(S)], 310 + i))
    out.append(attn_case(0, 2, 1, 8192, [8191, 4096], 320))
    out.append(attn_case(0, 12, 2, 2050, [2049], 321, plant_mode="late"))
    out.append(attn_case(0, 6, 2, 2050, [2049], 322, plant_mode="maxima"))
    return out


def prefill_attn_cases():
    out = []
    # tile maxima: 0 | 15, 30 | 31;  31, 32 | 16, 32, 33;  15, 31, 47, 63 | 54;  47, 63, 64 | 46, 47 | 63
    shapes = [([1, 31, 16], [0, 0, 16]), ([17, 33], [16, 1]), ([64, 15], [0, 40]), ([33, 17, 1], [32, 31, 63])]
    for i, (H, Hkv) in enumerate(HEADS_PREFILL):
        S, start = shapes[i % len(shapes)]
        out.append(attn_case(3, H, Hkv, 128, start, 400 + i, n_slots=len(S) + 1, seq_S=S))
    out.append(attn_case(3, 12, 2, 128, [31], 420, seq_S=[33], plant_mode="late"))
    out.append(attn_case(3, 6, 2, 128, [0], 421, seq_S=[64], plant_mode="maxima"))
    return out


def rope_case(kind, H, Hkv, Lmax, kps, seed, seq_S=None, n_slots=1, bf16=False, ld_extra=0):
    g = gen(seed)
    D, kvd = 64 * H, 64 * Hkv
    if kind == 5:
        kp = [k0 + s for k0, S in zip(kps, seq_S) for s in range(S)]
        slots = list(range(n_slots))[::-1][:len(seq_S)]
    else:
        kp, slots = list(kps), [n_slots - 1]
    R = len(kp)
    kc, vc = caches(g, n_slots, Hkv, Lmax)
    ip = [int(v) for v in torch.randint(0, Lmax, (R,), generator=g)]
    ip = [(p + 1) % Lmax if p == k else p for p, k in zip(ip, kp)]
    return dict(kind=kind, H=H, Hkv=Hkv, Lmax=Lmax, kc=kc, vc=vc, slots=slots, pos=[ip, kp], seq_S=seq_S, x=randn(g, R, D + 2 * kvd + ld_extra),
                rope=rope_bf16(Lmax) if bf16 else rope_unit(g, Lmax), name=f"k{kind}-H{H}x{Hkv}-L{Lmax}-kp{kp_tag(kps)}")


def rope_cases():
    out = [rope_case(4, 1, 1, 8, [0, 7, 3, 4], 500), rope_case(4, 12, 2, 1030, [0, 1029, 500, 501], 501, n_slots=2),
           rope_case(4, 9, 3, 64, [10, 11, 63], 502, bf16=True, ld_extra=8), rope_case(4, 16, 4, 8192, [8190, 8191, 0], 503),
           rope_case(5, 2, 1, 64, [0, 31, 62], 510, seq_S=[1, 16, 2], n_slots=4), rope_case(5, 12, 2, 128, [0, 100], 511, seq_S=[17, 28], n_slots=3),
           rope_case(5, 5, 1, 8, [0, 4], 512, seq_S=[4, 4], n_slots=2)]
    return out


SIZES = [(64, 64), (128, 256), (192, 320), (320, 192), (768, 2304), (1024, 2560)]
HKV = {64: 1, 128: 1, 192: 1, 320: 1, 768: 2, 1024: 4}


def linear_case(path, role, D, I, V, rows, seed, inplace=False, Lmax=64):
    g = gen(seed)
    H, Hkv = D // 64, HKV[D]
    Nqkv = D + 128 * Hkv
    c = dict(path=path, role=role, D=D, I=I, H=H, Hkv=Hkv, V=V, rows=rows, eps=1e-5, inplace=inplace,
             name=f"p{path}-{role}-D{D}-I{I}-V{V}-r{rows}" + ("-inplace" if inplace else ""))
    N, K = {"qkv": (Nqkv, D), "wo": (D, D), "w13": (2 * I, D), "w2": (D, I), "head": (V, D)}[role]
    rows_x = 1 if path == 2 else rows
    if path == 2 and role == "wo":               # dec_w2qkv: x = ff (I) fp16, res = h_mid, W2 = w2, W = wc [Nqkv][I + D]
        c.update(x=randn(g, 1, I).half(), res=randn(g, 1, D), W2=randn(g, D, I, scale=0.05).half(), W=randn(g, Nqkv, I + D, scale=0.05).half())
        return c
    fp16_in = role in ("wo", "w2")
    c["x"] = randn(g, rows_x, K).half() if fp16_in else randn(g, rows_x, K, scale=1.5)
    c["W"] = randn(g, N, K, scale=0.05).half()
    if role in ("qkv", "w13", "head"):
        c["gamma"] = randn(g, K, scale=0.3) + 1.0
    if fp16_in:
        c["res"] = randn(g, rows_x, D)
    if path == 2 and role == "w13":
        c["part"] = randn(g, H, D, scale=0.3)
    if role == "qkv" and path != 2:
        n_slots = rows if path == 1 else 2
        c["kc"], c["vc"] = caches(g, n_slots, Hkv, Lmax)
        c["rope"] = rope_unit(g, Lmax)
        c["Lmax"] = Lmax
        c["slots"] = list(range(n_slots))[::-1][:rows if path == 1 else 1]
        edge = [0, Lmax - 1, Lmax // 2, Lmax // 2 + 1]
        kp = [edge[s % 4] if path == 0 else int(torch.randint(0, Lmax, (1,), generator=g)) for s in range(rows)]
        if path == 0 and rows > 4:
            kp = edge + list(range(5, 5 + rows - 4))
        ip = [(k + 3) % Lmax for k in kp]
        c["pos"] = [ip, kp]
    return c


def linear_cases():
    out, seed = [], 600
    vs = [17, 33, 65, 1024, 4093]
    for i, (D, I) in enumerate(SIZES):
        for path in (0, 1, 2):
            rows = {0: (1, 5, 8)[i % 3], 1: (1, 16, 17, 48, 49, 64)[i], 2: 1}[path]
            for role in NAMES:
                seed += 1
                out.append(linear_case(path, role, D, I, vs[i % 5], rows, seed, inplace=role in ("wo", "w2") and not (path == 2 and role == "wo")))
    out.append(linear_case(0, "w13", 128, 2624, 17, 3, 700))
    out.append(linear_case(0, "w2", 128, 2624, 17, 3, 701))
    out.append(linear_case(1, "head", 128, 256, 4093, 17, 702))
    out.append(linear_case(0, "head", 128, 256, 65, 8, 703))
    out.append(linear_case(2, "head", 128, 256, 4093, 1, 704))
    out.append(linear_case(1, "wo", 128, 256, 17, 17, 705, inplace=False))
    return out


# ------------------------------------------------------------------------------------------------------------ checks
def cache_after(c, writes):
    """(kc, vc, E_k, E_v) after the call, all of the caches' shape: `writes` = (slot, row, k, v, E_k, E_v) with (kvd,) vectors.  E is
    zero -- bit equality -- everywhere but in the written rows"""
    kc, vc = c["kc"].double().clone(), c["vc"].double().clone()
    Ek, Ev = torch.zeros_like(kc), torch.zeros_like(vc)
    for sl, row, k, v, ek, ev in writes:
        if row < c["Lmax"]:
            kc[sl, :, row], vc[sl, :, row] = k.reshape(-1, 64), v.reshape(-1, 64)
            Ek[sl, :, row], Ev[sl, :, row] = ek.reshape(-1, 64), ev.reshape(-1, 64)
    return [("kc", kc, Ek, None), ("vc", vc, Ev, None)]


def seq_slots(c):
    """slot of every row of a kind 4 / 5 case or of a qkv-role linear"""
    if c.get("seq_S"):
        return [sl for sl, S in zip(c["slots"], c["seq_S"]) for _ in range(S)]
    R = len(c["pos"][1])
    return list(c["slots"]) if len(c["slots"]) == R else [c["slots"][0]] * R


def expected(c, sab=None):
    """what the call must leave: a list of (buffer name, float64 reference, bound), every element of every output and cache"""
    if "path" in c:
        r = ref_linear(c, sab)
        if "rows" in r:
            sl = seq_slots(c)
            return [("q_out", torch.stack([x["q"] for x in r["rows"]]), torch.stack([x["E_q"] for x in r["rows"]]), None)] + \
                cache_after(c, [(sl[i], x["row"], x["k"], x["v"], x["E_k"], x["E_v"]) for i, x in enumerate(r["rows"])])
        name = "out16" if c["role"] == "w13" else "out32"
        out = [(name, r["out"], r["E"], r.get("half"))]
        if "out2" in r:
            out.append(("out2", r["out2"], r["E2"], None))
        return out
    kind = c["kind"]
    if kind in (0, 2, 3):
        rows = [ref_attention(kind, c["x"][r], c["kc"][row_slot(c, r)], c["vc"][row_slot(c, r)], kp, c["H"], c["Hkv"], sab)
                for r, kp in enumerate(c["pos"][1])]
        return [("y16",) + tuple(torch.stack([x[i] for x in rows]) for i in range(3))]
    if kind == 1:
        r = ref_dec_attn2(c, sab)
        return [("part", r["part"], r["E_part"], None)] + cache_after(c, [(c["slots"][0], r["row"], r["k"], r["v"], r["E_k"], r["E_v"])])
    sl = seq_slots(c)
    rows = [ref_rope_cache(c["x"][i][:64 * c["H"] + 128 * c["Hkv"]], c["rope"], c["pos"][0][i], c["pos"][1][i], c["H"], c["Hkv"], sab) for i in range(len(sl))]
    # the rotation is dot(2): (2 + 2) u (|a c| + |b s|), contracted into an fma or not; v is a copy
    return [("q_out", torch.stack([x["q"] for x in rows]), torch.stack([4 * U * x["qa"] for x in rows]), None)] + \
        cache_after(c, [(sl[i], x["row"], x["k"], x["v"], 4 * U * x["ka"], torch.zeros_like(x["v"])) for i, x in enumerate(rows)])


def emulated(c):
    """the fp32 emulation of the call, the buffers of expected() in the same order"""
    def cache(writes):
        kc, vc = c["kc"].clone(), c["vc"].clone()
        for sl, row, k, v in writes:
            kc[sl, :, row], vc[sl, :, row] = k.reshape(-1, 64), v.reshape(-1, 64)
        return [kc, vc]
    if "path" in c:
        r = emu_linear(c)
        if "rows" in r:
            sl = seq_slots(c)
            return [torch.stack([x["q"] for x in r["rows"]])] + cache([(sl[i], c["pos"][1][i], x["k"], x["v"]) for i, x in enumerate(r["rows"])])
        return [r["out"]] + ([r["out2"]] if "out2" in r else [])
    kind = c["kind"]
    if kind in (0, 2, 3):
        return [torch.stack([emu_attention(kind, c["x"][r], c["kc"][row_slot(c, r)], c["vc"][row_slot(c, r)], kp, c["H"], c["Hkv"])
                             for r, kp in enumerate(c["pos"][1])])]
    if kind == 1:
        r = emu_dec_attn2(c)
        return [r["part"]] + cache([(c["slots"][0], c["pos"][1][0], r["k"], r["v"])])
    sl, D, kvd = seq_slots(c), 64 * c["H"], 64 * c["Hkv"]
    qs, ws = [], []
    for i in range(len(sl)):
        x, ip = c["x"][i], c["pos"][0][i]
        qs.append(emu_rotate(x[:D], c["rope"], ip, c["H"]))
        ws.append((sl[i], c["pos"][1][i], emu_rotate(x[D:D + kvd], c["rope"], ip, c["Hkv"]), x[D + kvd:D + 2 * kvd]))
    return [torch.stack(qs)] + cache(ws)


def within(got, ref, E, half=None):
    """EVERY element: bit-equal to the reference where E == 0, else |got - ref| <= E (+ the half step of an fp16 output, which is
    the format's and no estimate).  Returns (ok, worst ratio where E > 0); for an fp16 output the ratio is that of the EXCESS over
    the half step to E, since a correctly rounded result alone reaches the half step"""
    d = (got.double() - ref).abs()
    h = half if half is not None else torch.zeros_like(E)
    loose = E > 0
    ok = bool((d[~loose] == 0).all()) and bool((d[loose] <= (E + h)[loose]).all()) and bool(torch.isfinite(got.double()).all())
    return ok, (float(((d - h).clamp_min(0)[loose] / E[loose]).max()) if loose.any() else 0.0)


def compare(c, gots, sab=None):
    """(names of the buffers with an element out of bound, worst ratio)"""
    bad, worst = [], 0.0
    for (name, ref, E, half), got in zip(expected(c, sab), gots):
        assert got.shape == ref.shape, (c["name"], name, got.shape, ref.shape)
        ok, r = within(got, ref, E, half)
        if not ok:
            bad.append(name)
        worst = max(worst, r)
    return bad, worst


def kernel_of(c):
    if "path" in c:
        return ("gemv_pair", "bgemm", "dec")[c["path"]] + " " + c["role"]
    return ("ar_attn", "dec_attn2", "battn", "ar_prefill_attn", "ar_rope_cache", "ar_rope_cache_ragged")[c["kind"]]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = ar_attn_cases() + dec_attn2_cases() + battn_cases() + prefill_attn_cases() + rope_cases() + linear_cases()
        assert len({c["name"] for c in _ALL}) == len(_ALL)
    return _ALL


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def _attn(c):
    return c.get("kind") in (0, 1, 2, 3)


def _cache_writer(c):
    return c.get("kind") in (1, 4, 5) or (c.get("role") == "qkv" and c.get("path") in (0, 1))


# name -> the cases that must catch it
SABOTAGES = {
    "keys_plus_1": lambda c: _attn(c) and all(k < c["Lmax"] - 1 for k in c["pos"][1]),
    "keys_minus_1": lambda c: _attn(c) and any(k >= 1 for k in c["pos"][1]),
    "seam_256": lambda c: _attn(c) and max(c["pos"][1]) > 256,
    "seam_512": lambda c: _attn(c) and max(c["pos"][1]) > 512,
    "kv_head_mod": lambda c: _attn(c) and c["Hkv"] > 1 and c["H"] // c["Hkv"] > 1,
    "no_scale": lambda c: _attn(c) and any(k >= 1 for k in c["pos"][1]),
    "no_rescale": lambda c: _attn(c) and c["name"].endswith("-late"),
    "merge_row_lost": lambda c: c.get("kind") == 1 and c["pos"][1][0] >= 63,
    "rot_kv_pos": _cache_writer,
    "pair_over_row": lambda c: _cache_writer(c) and c["H"] > 1 and (c.get("kind") != 1 or c["Hkv"] > 1 or c["pos"][1][0] >= 1),
    "v_rotated": _cache_writer,
    "row_plus_1": _cache_writer,
    "cache_row_read": lambda c: c.get("kind") == 1,
    "y_not_rounded": lambda c: c.get("kind") == 1 and c["pos"][1][0] <= 63,      # beyond, E of a long sum reaches the fp16 step
    "wo_slice_shift": lambda c: c.get("kind") == 1,
    "rstd_length": lambda c: c.get("kind") == 1 or (c.get("role") in ("qkv", "w13", "head") and not (c["path"] == 2 and c["role"] == "qkv")),
    "gamma_added": lambda c: c.get("role") in ("qkv", "w13", "head") and not (c["path"] == 2 and c["role"] == "qkv"),
    "glu_halves": lambda c: c.get("role") == "w13",
    "residual_twice": lambda c: c.get("role") in ("wo", "w2") and not (c["path"] == 2 and c["role"] == "wo"),
    "last_row_doubled": lambda c: c.get("role") == "head" and c["V"] % 2 == 1,
}
