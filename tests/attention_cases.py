"""The attention kernels (csrc/attention.hip) at op level: the cases, the float64 reference, the bound and a CPU emulation of
the kernels' numerics, shared by test_host_attention.py (which shows that the checks separate a right kernel from a subtly
wrong one) and test_gpu_attention.py (which holds all twelve launched instantiations to them through svc_op_attention_ex).
CPU only, plain torch ops.  Nothing here calls the library.

A launch is a dict `a` (`build`): the fields of svc_attention_t with CPU fp16 tensors already in the kernels' layout, as
ops.attention_ex takes them, plus the logical operands the reference reads.

Layout (`layout`; from attention.hip's header and the prose of common.h, not from the library's code)
  qk [n_seq * seq_rows][ld_qk]   row seq * seq_rows + pos; q of head h at columns [64 h, 64 h + 64), k at [D + 64 h, ...), D = 64 H;
                                 ld_qk = 2 D, or 3 D with a third block the kernels never read; q is pre-scaled by log2(e) / 8 and
                                 rounded to fp16, so the softmax is 2^(q . k)
  vt [n_seq][D][vt_ld]           key p of a sequence at column vt_pos(p, vt_perm): mode 0 natural; mode 1: key 16 h + 4 f + r of
                                 every 32-group at 8 f + 4 h + r; mode 2: key 8 a + 4 f + r of every 16-group at 8 f + 4 a + r
  Everything else in the buffers (rows past the logical data, the third block, V^T columns of no key) is seeded FINITE junk.

Reference (`ref_attention`): float64 on the fp16-rounded operands, out[i] = sum_j w_ij v_j with w_i = softmax over keys
j < kv_len of the base-2 scores s_ij = qs_i . k_j, for the queries [q_start, Tq) of every sequence; kv_len = 0 gives zero rows.

Bound (`bound`), per element, derived from the kernels' arithmetic and not from their results:

    |out - ref| <= 2^-9 (w @ |v|) + kv_len 2^-23 max|v| + 2^-24          (+ 2^-11 |ref| for the fp16 output)

  The kernels keep a per-query baseline m with max_j s_ij - 8 <= m <= max_j s_ij (it starts at the first tile's maximum and
  moves up to a tile's maximum only when that overshoots it by more than 8), form P_j = rtz16(2^(s_j - m)) -- fp32 exp2 packed
  to fp16 ROUND TOWARD ZERO -- and return (sum_j P_j v_j) / (sum_j P_j), both sums over the SAME rounded P_j, accumulated in fp32
  by the MFMA.  The key of the largest score has P >= 1, so l = sum_j P_j >= 1.
  * Normal P_j (>= 2^-14) = p_j (1 - d_j) with 0 <= d_j < 2^-10.  With l = sum p_j (1 - d), d the p-weighted mean of the d_j,
    out - ref = sum_j w_j (d - d_j) v_j / (1 - d), and |d - d_j| < 2^-10: at most 2^-10 (w @ |v|) (1 + 2^-10).
  * The scores are fp32 sums of 64 exact fp16 products: an error of at most 64 x 2^-24 sum_d |qs_d k_d| each, a relative 0.7 x that
    in p_j (and the exp2 unit's own 2^-21).  For sum_d |qs_d k_d| < 2^7 that is below 2^-11 per weight, twice over for the
    difference of two weights: the second 2^-10 (w @ |v|).  Together 2^-9 (w @ |v|).
  * A subnormal P_j loses up to 2^-24 absolutely: the numerator loses at most kv_len 2^-24 max|v| (l >= 1 divides it), the row sum
    at most kv_len 2^-24, which moves out by that fraction of |ref| <= max|v|.  Together kv_len 2^-23 max|v|.
  * 2^-24 for the final fp32 product with 1 / l at results near zero; the fp16 store rounds to nearest, 2^-11 |ref|.
  The fp32 accumulation itself (one rounding per MFMA, 2^-24 relative to partial sums that never exceed the final ones by more
  than the rescale undoes) disappears in the slack between the first item's worst case and its typical 1/3 of that.

Emulation (`emulate`): the same arithmetic on the CPU, reading the launch's own buffers through vt_pos: fp32 scores, the
baseline rule above (its start anywhere up to 8 below the first tile's maximum: `slack`), round-toward-zero fp16 P, row sums of
the same P, one fp32 rounding per 64-key tile (the tile's own sum is exact in float64).  `sab` swaps in one of SABOTAGES.

Four kinds of case.  The bound is loose where it must be (with a few hundred keys a weight is ~ 1/T, so two keys' V columns
swapped inside a 32-group move an output by less than 2^-9 |v| only by luck of the data, and a last-tile V^T order error by less
still), so three kinds are EXACT and the numeric kind is for what they cannot see:
  numeric   randn operands, with late dominant keys (k_j = 4 q_i, j in a tile after the first): query i's baseline moves there
            (deferred rescale) and its neighbours' in the same 16-query tile do not.  Held to the bound.
  routing   k_j = seeded +-1 sign vectors, q_i = 6 k_pi(i), pi walking over all keys < kv_len; v[key][d] = 1024 + ((67 key + 13 d
            + 5 h) mod 1021), exact in fp16.  The target's score is 64 x 1.082 = 69.2, every other one at least 26 lower (asserted
            per case; 28 or more in fact), so every off-target P is below the smallest fp16 subnormal whatever the baseline and rounds
            to 0: the fp16 output row i IS v[pi(i)], bit for bit, and the fp32 one within 2^-20 relative.  Catches any wrong
            key <-> V column correspondence exactly.  The K rows past kv_len repeat the valid keys, so a key that escapes the
            mask ties with some query's target.
  uniform   q = 0, v small integers: every P is exactly 1, l = kv_len, out = fp16(fp32(sum v) x fp32(1 / kv_len)) exactly (fp32
            output: to one ulp).  A dropped, doubled or unmasked key changes the sum.
  unit      numeric q and k, v[key][d] = 2^((d mod 5) - 2) for every key < kv_len: the V^T rows then equal the ones-row of the
            row-sum MFMA up to a power of two, so the numerator IS 2^e l bit for bit through every rescale, and out = fp16(2^e l
            x (1 / l)) = 2^e exactly (fp32: within 2^-22).  This is the only kind that sees the row sum taken from anything
            but the rounded P: the bound's first item is the allowance for that rounding, so no numeric case can.
"""
import random

import torch

LOG2E_8 = 1.4426950408889634 / 8.0
KT = 64                             # keys per tile
CANARY16 = 0x6A5A                   # a finite fp16 (3252.0) no output takes
CANARY32 = -777.25
KINDS = ("numeric", "routing", "uniform", "unit")
KEY_LENS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 321)
N_QUERIES = (1, 16, 63, 64, 65, 127, 128, 129, 200)
Q_STARTS = (0, 8, 64, 72, 136)
# (vt_perm, qt_form, out32) -> the instantiation attention_launch picks: vt_perm 0 | 1 = attn_kernel<QT = qt_form, VPERM = vt_perm,
# OUT32>, vt_perm 2 = attn32_kernel<NW = 2 qt_form, 3, true, true, OUT32>
INSTANTIATIONS = tuple((vp, qf, o32) for vp in (0, 1, 2) for qf in (1, 2) for o32 in (0, 1))


def round_up(a, b):
    return -(-a // b) * b


def vt_pos(p, mode):
    """the V^T column of key p"""
    if mode == 1:
        g, i = p // 32, p % 32
        h, f, r = i // 16, (i % 16) // 4, i % 4
        return 32 * g + 8 * f + 4 * h + r
    if mode == 2:
        g, i = p // 16, p % 16
        a, f, r = i // 8, (i % 8) // 4, i % 4
        return 16 * g + 8 * f + 4 * a + r
    assert mode == 0
    return p


for _mode in (0, 1, 2):
    for _base in range(0, 128, 32):
        assert sorted(vt_pos(_p, _mode) for _p in range(_base, _base + 32)) == list(range(_base, _base + 32))


def vt_cols(keys, mode):
    return torch.tensor([vt_pos(int(p), mode) for p in keys], dtype=torch.long)


def rtz16(x):
    """fp32 x >= 0 -> fp16 rounded toward zero (v_cvt_pkrtz), as fp32"""
    h = x.half()
    over = h.float() > x
    return (h.view(torch.int16) - over.to(torch.int16)).view(torch.float16).float()


# ------------------------------------------------------------------------------------------------ layout
def layout(q, k, v, seq_rows, ld_qk, vt_ld, mode, seed):
    """logical q (unscaled), k, v [n_seq][T][H][64] -> (qk [n_seq * seq_rows][ld_qk], vt [n_seq][D][vt_ld]) fp16, T <= seq_rows"""
    n_seq, T, H, hd = q.shape
    D = 64 * H
    assert hd == 64 and T <= seq_rows and ld_qk >= 2 * D and vt_ld % KT == 0 and vt_ld >= round_up(T, 32)
    g = torch.Generator().manual_seed(seed)
    qk = torch.randn(n_seq, seq_rows, ld_qk, generator=g).half()
    qk[:, :T, :D] = (q.double() * LOG2E_8).half().reshape(n_seq, T, D)
    qk[:, :T, D:2 * D] = k.half().reshape(n_seq, T, D)
    vt = (3.0 * torch.randn(n_seq, D, vt_ld, generator=g)).half()
    vt[:, :, vt_cols(range(T), mode)] = v.half().reshape(n_seq, T, D).transpose(1, 2)
    return qk.reshape(n_seq * seq_rows, ld_qk), vt


def logical(a):
    """(qs, k, v) [n_seq][seq_rows][H][64] fp16 read back from a launch's buffers: qs as stored (pre-scaled), v in natural order"""
    n_seq, R, H = a["n_seq"], a["seq_rows"], a["H"]
    D = 64 * H
    qk = a["qk"].reshape(n_seq, R, -1)
    qs = qk[:, :, a["q_col"]:a["q_col"] + D].reshape(n_seq, R, H, 64)
    k = qk[:, :, a["k_col"]:a["k_col"] + D].reshape(n_seq, R, H, 64)
    v = a["vt"][:, :D, vt_cols(range(R), a["vt_perm"])].transpose(1, 2).reshape(n_seq, R, H, 64)
    return qs, k, v


def lens_of(a):
    return list(a["kv_len"]) if a["kv_len"] is not None else [a["kv_len_const"]] * a["n_seq"]


def window(a):
    """bool [n_seq * seq_rows]: the rows the launch writes"""
    m = torch.zeros(a["n_seq"], a["seq_rows"], dtype=torch.bool)
    m[:, a["q_start"]:a["Tq"]] = True
    return m.reshape(-1)


# ------------------------------------------------------------------------------------------------ reference and bound
def ref_attention(qs, k, v, lens, q_start, Tq):
    """float64 on the operands as stored.  Returns (ref, wabs = w @ |v|, vmax) [n_seq][seq_rows][H][64] (vmax: max |v| over the
    keys and columns of that sequence and head), zero outside the queries [q_start, Tq) and for kv_len = 0."""
    n_seq, R, H, _ = qs.shape
    ref = torch.zeros(n_seq, R, H, 64, dtype=torch.float64)
    wabs, vmax = torch.zeros_like(ref), torch.zeros_like(ref)
    for s in range(n_seq):
        L = lens[s]
        if L == 0:
            continue
        qq = qs[s, q_start:Tq].double().transpose(0, 1)            # [H][nq][64]
        kk = k[s, :L].double().transpose(0, 1)
        vv = v[s, :L].double().transpose(0, 1)
        sc = qq @ kk.transpose(1, 2)
        w = torch.exp2(sc - sc.max(dim=-1, keepdim=True).values)
        w = w / w.sum(dim=-1, keepdim=True)
        ref[s, q_start:Tq] = (w @ vv).transpose(0, 1)
        wabs[s, q_start:Tq] = (w @ vv.abs()).transpose(0, 1)
        vmax[s, q_start:Tq] = vv.abs().amax(dim=(1, 2))[None, :, None]
    return ref, wabs, vmax


def bound(ref, wabs, vmax, lens, out32):
    n = torch.tensor(lens, dtype=torch.float64)[:, None, None, None]
    b = 2.0 ** -9 * wabs + n * 2.0 ** -23 * vmax + 2.0 ** -24
    return b if out32 else b + 2.0 ** -11 * ref.abs()


def min_gap(qs, k, lens, q_start, Tq, target):
    """routing: the smallest (target score - any other score) over all queries, in log2 units"""
    gap = float("inf")
    for s in range(qs.shape[0]):
        L = lens[s]
        if L < 2:
            continue
        sc = qs[s, q_start:Tq].double().transpose(0, 1) @ k[s, :L].double().transpose(0, 1).transpose(1, 2)      # [H][nq][L]
        t = target[s][None, :, None].expand(sc.shape[0], -1, 1)
        top = sc.gather(2, t)
        gap = min(gap, (top - sc.scatter(2, t, float("-inf"))).min().item())
    return gap


# ------------------------------------------------------------------------------------------------ emulation
SABOTAGES = {
    "swap16": "keys 4 f + r and 16 + 4 f + r of every 32-group swapped on the V side only",
    "mode1as2": "V^T stored in mode 1 read as mode 2",
    "nomask": "the last tile left unmasked",
    "mask+1": "the mask off by one key",
    "norescale": "the rescale skipped (alpha = 1) when the baseline moves",
    "sum_unrounded": "the row sum taken from the unrounded P",
    "neighbour_len": "kv_len taken from the neighbouring sequence",
}


def empty_out(a):
    n, ld = a["n_seq"] * a["seq_rows"], a["ld_out"]
    if a["out32"]:
        return torch.full((n, ld), CANARY32, dtype=torch.float32)
    return torch.full((n, ld), CANARY16, dtype=torch.int16).view(torch.float16)


def emulate(a, sab=None, slack=0.0):
    """The whole output buffer of the launch `a`, as the kernels compute it (module docstring)."""
    assert sab is None or sab in SABOTAGES
    n_seq, R, H, Tq, q0 = a["n_seq"], a["seq_rows"], a["H"], a["Tq"], a["q_start"]
    D = 64 * H
    lens = lens_of(a)
    qk = a["qk"].reshape(n_seq, R, -1)
    out = empty_out(a)
    mode = 2 if (sab == "mode1as2" and a["vt_perm"] == 1) else a["vt_perm"]
    for s in range(n_seq):
        L = lens[(s + 1) % n_seq] if sab == "neighbour_len" else lens[s]
        nq = Tq - q0
        qq = qk[s, q0:Tq, a["q_col"]:a["q_col"] + D].float().reshape(nq, H, 64).transpose(0, 1)             # [H][nq][64]
        o = torch.zeros(H, nq, 64)
        l = torch.zeros(H, nq)
        m = torch.zeros(H, nq)
        for kt in range(-(-L // KT)):
            keys = torch.arange(kt * KT, kt * KT + KT)
            kk = qk[s, keys.clamp(max=R - 1), a["k_col"]:a["k_col"] + D].float().reshape(KT, H, 64).transpose(0, 1)
            vkeys = keys ^ 16 if sab == "swap16" else keys
            vv = a["vt"][s, :D, vt_cols(vkeys, mode)].float().reshape(H, 64, KT).transpose(1, 2)            # [H][key][d]
            sc = qq @ kk.transpose(1, 2) - m[:, :, None]
            if sab != "nomask":
                sc[:, :, keys >= L + (1 if sab == "mask+1" else 0)] = -1e30
            top = sc.max(dim=-1).values
            delta = top - slack if kt == 0 else torch.where(top > 8.0, top, torch.zeros_like(top))
            alpha = torch.exp2(-delta)
            if sab == "norescale" and kt > 0:
                alpha = torch.ones_like(alpha)
            m = m + delta
            o, l = o * alpha[:, :, None], l * alpha
            e = torch.exp2(sc - delta[:, :, None])
            p = rtz16(e)
            l = (l.double() + (e if sab == "sum_unrounded" else p).double().sum(dim=-1)).float()
            o = (o.double() + p.double() @ vv.double()).float()
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        res = (o * inv[:, :, None]).transpose(0, 1).reshape(nq, D)
        out[s * R + q0:s * R + Tq, :D] = res.to(out.dtype)
    return out


# ------------------------------------------------------------------------------------------------ cases
def case(kind, H, lens, nq, q_start, seq_extra, ld3, vt_extra, vt_perm, qt_form, out32, seed, const=False, ld_out_extra=0):
    """lens: the key length of every sequence (const: one length for all, passed as kv_len_const with a null array)"""
    assert kind in KINDS and (not const or len(set(lens)) == 1)
    return dict(kind=kind, H=H, lens=list(lens), nq=nq, q_start=q_start, seq_extra=seq_extra, ld3=ld3, vt_extra=vt_extra,
                vt_perm=vt_perm, qt_form=qt_form, out32=out32, seed=seed, const=const, ld_out_extra=ld_out_extra)


def case_id(c):
    lens = "x".join(str(v) for v in c["lens"])
    return (f"{c['kind']}-vp{c['vt_perm']}qt{c['qt_form']}o{32 if c['out32'] else 16}-H{c['H']}-L{lens}{'c' if c['const'] else ''}"
            f"-q{c['q_start']}+{c['nq']}-r{c['seq_extra']}-ld{3 if c['ld3'] else 2}-vt{c['vt_extra']}-s{c['seed']}")


def instantiation(c):
    return c["vt_perm"], c["qt_form"], int(bool(c["out32"]))


def shape_of(c):
    Tq = c["q_start"] + c["nq"]
    seq_rows = max(round_up(Tq, 8), round_up(max(c["lens"]), 8)) + c["seq_extra"]
    return Tq, seq_rows, round_up(seq_rows, KT) + c["vt_extra"]


def build(c):
    """The launch of a case: the arguments of ops.attention_ex, plus `case`, `lens`, and what `check` needs (`want` of the exact
    kinds; routing: `gap`)."""
    g = torch.Generator().manual_seed(c["seed"])
    H, lens, q0 = c["H"], c["lens"], c["q_start"]
    n_seq, D = len(lens), 64 * c["H"]
    Tq, R, vt_ld = shape_of(c)
    kind = c["kind"]
    rn = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    q, k, v = rn(n_seq, R, H, 64), rn(n_seq, R, H, 64), rn(n_seq, R, H, 64)
    key = torch.arange(R)[:, None, None]
    hh = torch.arange(H)[None, :, None]
    d = torch.arange(64)[None, None, :]
    valid = torch.zeros(n_seq, R, 1, 1, dtype=torch.bool)
    for s, L in enumerate(lens):
        valid[s, :L] = True
    want = None
    target = []
    if kind in ("numeric", "unit"):
        # late dominant keys: a key of a tile after the first (and, for long sequences, the last valid key) made 4 x one query
        for s, L in enumerate(lens):
            if L > KT + 1:
                j = KT + (7 * s + 3) % (L - KT)
                i = q0 + (11 * s + 5) % c["nq"]
                k[s, j] = 4.0 * q[s, i]
            if L > 2 * KT + 2:
                k[s, L - 1] = 4.0 * q[s, Tq - 1]
    if kind == "unit":
        v = torch.where(valid, torch.exp2(((d % 5) - 2).double()).float().expand(n_seq, R, H, 64), v)
    if kind == "uniform":
        q = torch.zeros_like(q)
        v = torch.where(valid, ((7 * key + 3 * d + hh) % 17 - 8).float().expand(n_seq, R, H, 64), 100.0 + v)
    if kind == "routing":
        k = (torch.randint(0, 2, (n_seq, R, H, 64), generator=g) * 2 - 1).float()
        v = (1024 + (67 * key + 13 * d + 5 * hh) % 1021).float().expand(n_seq, R, H, 64).clone()
        for s, L in enumerate(lens):
            if 0 < L < R:           # the masked rows repeat the valid keys: an unmasked one ties with some query's target
                k[s, L:] = k[s, torch.arange(R - L) % L]
            step = 37 if L % 37 else 41
            t = (step * torch.arange(q0, Tq) + 11) % max(L, 1)
            target.append(t)
            q[s, q0:Tq] = 6.0 * k[s, t]
    ld_qk = (3 if c["ld3"] else 2) * D
    qk, vt = layout(q, k, v, R, ld_qk, vt_ld, c["vt_perm"], c["seed"] + 1)
    a = dict(case=c, kind=kind, lens=list(lens), qk=qk, q_col=0, k_col=D, vt=vt, n_seq=n_seq, H=H, seq_rows=R, Tq=Tq, q_start=q0,
             kv_len=None if c["const"] else list(lens), kv_len_const=lens[0] if c["const"] else 0, vt_perm=c["vt_perm"],
             qt_form=c["qt_form"], out32=int(bool(c["out32"])), ld_out=D + c["ld_out_extra"])
    v16 = v.half().double()
    nz = torch.tensor([L > 0 for L in lens])[:, None, None, None]
    if kind == "routing":
        want = torch.zeros(n_seq, R, H, 64, dtype=torch.float64)
        for s in range(n_seq):
            if lens[s] > 0:
                want[s, q0:Tq] = v16[s, target[s]]
        # what the kind rests on, for every case emitted: off-target P < 2^-25 whatever the baseline, and the reference agrees
        qs16, k16, v16r = logical(a)
        a["gap"] = min_gap(qs16, k16, lens, q0, Tq, target)
        assert a["gap"] > 26.0, (case_id(c), a["gap"])
        assert ((ref_attention(qs16, k16, v16r, lens, q0, Tq)[0] - want).abs() < 2.0 ** -4).all(), case_id(c)
    elif kind == "uniform":
        want = torch.zeros(n_seq, R, H, 64, dtype=torch.float64)
        for s, L in enumerate(lens):
            if L > 0:
                tot = v16[s, :L].sum(dim=0).float()                              # small integers: exact
                want[s, q0:Tq] = (tot * (torch.tensor(1.0) / torch.tensor(float(L)))).double()      # fp32 product with fp32 1 / L
    elif kind == "unit":
        want = (torch.exp2(((d % 5) - 2).double()) * nz).expand(n_seq, R, H, 64).clone()
    if want is not None:
        keep = torch.zeros(n_seq, R, 1, 1, dtype=torch.bool)
        keep[:, q0:Tq] = True
        a["want"] = (want * keep).reshape(n_seq * R, D)
    return a


WANT_REL32 = {"routing": 2.0 ** -20, "uniform": 2.0 ** -23, "unit": 2.0 ** -22}


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else t.view(torch.int32)


def canaries_intact(a, out):
    """every element outside the rows [q_start, Tq) of each sequence and the columns [0, D) still holds the fill pattern"""
    D = 64 * a["H"]
    keep = ~window(a)[:, None].expand(-1, out.shape[1]).clone()
    keep[:, D:] = True
    return torch.equal(bits(out)[keep], bits(empty_out(a))[keep])


def check(a, out, ref=None):
    """Holds the written part of one launch's output buffer to its case: (ok, ratio, text).  numeric: ratio = the largest
    |out - ref| / bound, ok = ratio <= 1 (ref: the (ref, wabs, vmax) of ref_attention, computed here when not given).  Exact
    kinds: ratio = the number of wrong elements.  The canaries are `canaries_intact`'s."""
    D = 64 * a["H"]
    rows = window(a)
    got = out[:, :D].double()[rows]
    if not torch.isfinite(got).all():
        return False, float("inf"), "non-finite output"
    if a["kind"] == "numeric":
        if ref is None:
            ref = ref_attention(*logical(a), a["lens"], a["q_start"], a["Tq"])
        b = bound(*ref, a["lens"], a["out32"]).reshape(-1, D)[rows]
        ratio = ((got - ref[0].reshape(-1, D)[rows]).abs() / b).max().item()
        return ratio <= 1.0, ratio, f"max |out - ref| / bound = {ratio:.3f}"
    want = a["want"][rows]
    if a["out32"]:
        bad = (got - want).abs() > WANT_REL32[a["kind"]] * want.abs()
    else:
        bad = bits(out[:, :D][rows]) != bits(want.half())
    n = int(bad.sum())
    return n == 0, float(n), f"{n} of {bad.numel()} elements differ from the exact value"


def parity_cases():
    """Every kind on every instantiation, with the shapes rotating through KEY_LENS, N_QUERIES, Q_STARTS, 1 .. 5 sequences, 1 .. 3
    heads, both ld_qk, both vt_ld, seq_rows = round_up(Tq, 8) and larger, a length array and a constant; then qt_form = 0 on small
    grids.  Every second case caps its lengths at round_up(Tq, 8), which with seq_extra = 0 gives seq_rows = round_up(Tq, 8)."""
    out = []
    i = 0
    for kind in KINDS:
        for vp, qf, o32 in INSTANTIATIONS:
            nq, q0 = N_QUERIES[i % 9], Q_STARTS[(i // 2) % 5]
            n_seq = 1 + (i * 3) % 5
            const = i % 6 == 5
            lens = [KEY_LENS[(3 * i + 7 * t) % 20] for t in range(n_seq)]
            if i % 2 == 0:
                cap = round_up(q0 + nq, 8)
                lens = [L if L <= cap else max(v for v in KEY_LENS if v <= cap) for L in lens]
            if const:
                lens = [max(lens)] * n_seq
            out.append(case(kind, 1 + i % 3, lens, nq, q0, (0, 8, 24)[(i // 2) % 3], i % 2, KT * ((i // 3) % 2), vp, qf, o32,
                            seed=3000 + i, const=const, ld_out_extra=8 * ((i // 4) % 2)))
            i += 1
    # the launcher's own choice of the form (small grids take the 64-query workgroups), on every family; and kv_len = 0 alone
    for j, kind in enumerate(KINDS):
        out.append(case(kind, 2, [129, 64, 33], 65, 8, 8, j % 2, 0, j % 3, 0, j % 2, seed=3100 + j))
    for vp in (0, 1, 2):
        out.append(case("numeric", 1, [0], 16, 0, 0, 0, 0, vp, 1 + vp % 2, 0, seed=3110 + vp, const=True))
    # every key length in one family each at least once more, as single sequences of the production instantiation, exact kinds
    rng = random.Random(20250519)
    for L in KEY_LENS:
        kind = ("routing", "uniform", "unit")[L % 3]
        out.append(case(kind, 1, [L], rng.choice((16, 65)), 0, 0, 0, 0, rng.choice((1, 2)), rng.choice((1, 2)), 0, seed=3200 + L))
    return out
