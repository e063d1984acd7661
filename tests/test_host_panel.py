"""CPU side of the DiT row-panel kernel's op-level suite (test_gpu_panel.py): the seam is declared, exported and bound, its
refusals come before anything touches a device, and the restatement of panel_cases.py checks itself.  The GPU tests hold
the kernel to `ref_panel` within e = 4 x noise32 per output; these tests establish that such a bound separates a right kernel
from a subtly wrong one (every sabotage of the restatement exceeds it at least tenfold on every case that can show it), that
the helpers agree with themselves (the float32 evaluation passes), and that the restatement is the reference model's layer and
not merely a reading of the kernel (it agrees with the oracle's blocks to within the fp16 rounding of the operands)."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import panel_cases as P
import seedvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

CASES = P.parity_cases()
_memo = {}


def prepared(i):
    """(args, bounds) of case i, computed once for all the tests of this module"""
    if i not in _memo:
        a = P.make_args(CASES[i])
        _memo[i] = (a, P.bounds(a))
    return _memo[i]


def test_every_instantiation_has_a_case():
    got = {P.instantiation(c) for c in CASES}
    want = {(D, g, tm, s) for D in (384, 512) for g in (0, 1) for tm in (1, 2) for s in (P.SEAM_NONE, P.SEAM_HEAD)} | \
           {(D, 0, tm, P.SEAM_MERGE) for D in (384, 512) for tm in (1, 2)}
    assert len(want) == 20 and want <= got
    assert len({P.case_id(c) for c in CASES}) == len(CASES)


def test_seam_is_declared_exported_and_bound():
    from seedvc_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    name = "svc_op_dit_panel"
    assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/seedvc_hip.h"
    assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(ops, "dit_panel")
    body = re.search(r"typedef struct \{([^}]*)\} svc_dit_panel_t;", header).group(1)
    fields = re.findall(r"\**\s*([A-Za-z_0-9]+)\s*[,;]", body)
    assert fields == [f[0] for f in _lib.DitPanel._fields_]


def refusal_args(**kw):
    """A launch the entry point takes (post + qkv, D = 384, 8 rows) with every pointer a dummy, then kw on top."""
    from seedvc_amd import _lib
    e = _lib.DitPanel()
    for name, kind in _lib.DitPanel._fields_:
        if kind is ctypes.c_void_p:
            setattr(e, name, 16)                 # never dereferenced: the checks come first
    e.D, e.I, e.gated, e.tm, e.M, e.Lout, e.seq_rows, e.row_off, e.n_seq = 384, 32, 0, 0, 8, 8, 8, 0, 1
    e.eps, e.do_post, e.do_qkv = 1e-5, 1, 1
    e.c16 = None
    e.vt_ld, e.vt_seq_stride, e.vt_mode = 32, 384 * 32, 1
    e.ldw, e.C, e.T, e.npre, e.head_C, e.ldv = 128, 80, 4, 1, 80, 80
    for k, v in kw.items():
        setattr(e, k, v)
    return e


MERGE = dict(seam=P.SEAM_MERGE, do_post=0)
HEAD = dict(seam=P.SEAM_HEAD, do_qkv=0, do_final=1)
REFUSALS = [
    (dict(D=768), b"D must be"), (dict(I=48), b"multiple of 32"),
    (dict(Lout=6, M=6, seq_rows=6), b"4-row"), (dict(Lout=2, M=8, n_seq=4), b"4-row"), (dict(row_off=2, seq_rows=10), b"4-row"),
    (dict(HEAD, head_C=8), b"head seam"), (dict(HEAD, head_C=24, ldv=24), b"head seam"), (dict(HEAD, head_C=144, ldv=144), b"head seam"),
    (dict(HEAD, ldv=64), b"head seam"),
    (dict(MERGE, row_off=4, seq_rows=12), b"merge seam"), (dict(MERGE, do_post=1), b"merge seam"), (dict(MERGE, T=8), b"merge seam"),
    (dict(HEAD, c16=16), b"head seam"), (dict(HEAD, do_qkv=1), b"head seam"),
    (dict(do_post=0, do_qkv=0, do_final=1), b"no streamed phase"), (dict(do_post=0, do_qkv=0), b"no streamed phase"),
    (dict(tm=3), b"tm is"),
    (dict(wo=None), b"do_post needs"), (dict(vt_ld=8), b"vt_ld"), (dict(M=12), b"n_seq * Lout"), (dict(seam=3), b"unknown seam"),
]


@pytest.mark.parametrize("kw,word", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_refusals_need_no_gpu(kw, word):
    """The argument checks, the launcher's own included, come before anything is allocated, packed or launched."""
    from seedvc_amd import _lib
    fn, err = _lib.lib().svc_op_dit_panel, _lib.lib().svc_last_error
    assert fn(ctypes.byref(refusal_args(**kw)), None) != 0, kw
    assert word in err(), (kw, err())


def test_ulp16_at_the_edges():
    h = lambda v: torch.tensor([v], dtype=torch.float64)     # noqa: E731
    for v, want in [(1.0, 2.0 ** -10), (0.99999, 2.0 ** -11), (2.0, 2.0 ** -9), (1.9999, 2.0 ** -10), (-1.5, 2.0 ** -10),
                    (2.0 ** -14, 2.0 ** -24), (2.0 ** -14 * 0.999, 2.0 ** -24), (2.0 ** -20, 2.0 ** -24), (0.0, 2.0 ** -24),
                    (2.0 ** -13, 2.0 ** -23), (65504.0, 32.0)]:
        assert P.ulp16(h(v)).item() == want, v
    # against torch's own fp16 neighbours, over every finite positive fp16 value
    bits = torch.arange(0, 0x7BFF, dtype=torch.int16)
    v = bits.view(torch.float16).double()
    up = (bits + 1).view(torch.float16).double()
    assert torch.equal(P.ulp16(v), up - v)
    # rounding an fp32 value to fp16, as the kernel does, moves it by at most half that spacing
    x = torch.randn(200000, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * torch.logspace(-8, 4, 200000, dtype=torch.float64)
    x = x.float().double()
    assert ((P.half(x) - x).abs() <= P.ulp16(x) / 2).all()


def test_vt_pos_tables():
    """common.h's vt_perm_pos / vt_perm_pos16 written out for positions 0..63"""
    t1 = [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27, 4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    t2 = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert [P.vt_pos(p, 1) for p in range(64)] == t1 + [32 + v for v in t1]
    assert [P.vt_pos(p, 2) for p in range(64)] == [16 * g + v for g in range(4) for v in t2]
    assert [P.vt_pos(p, 0) for p in range(64)] == list(range(64))
    for base in range(0, 64, 32):
        assert sorted(P.vt_pos(p, 1) for p in range(base, base + 32)) == list(range(base, base + 32))
    for base in range(0, 64, 16):
        assert sorted(P.vt_pos(p, 2) for p in range(base, base + 16)) == list(range(base, base + 16))
    # both keep runs of 4 positions together: the kernel stores 4 rows with one 8-byte store at vt_pos(first)
    for mode in (1, 2):
        assert all(P.vt_pos(p + r, mode) == P.vt_pos(p, mode) + r for p in range(0, 64, 4) for r in range(4))


@pytest.mark.parametrize("i", range(len(CASES)), ids=[P.case_id(c) for c in CASES])
def test_float32_evaluation_meets_the_bound(i):
    a, b = prepared(i)
    r32 = P.ref_panel(a, torch.float32)
    assert set(r32) == set(b)
    for name, (r, mask, e) in b.items():
        assert mask.any() and e > 0.0, name
        assert P.excess(name, P.as_stored(name, r32[name][0]), r, mask, e) <= 1.0, name


@pytest.mark.parametrize("sab", list(P.SABOTAGES))
def test_sabotage_exceeds_the_bound_tenfold(sab):
    """on every case that can show it, at least one element of some output is off by >= 10 e beyond the rounding allowance"""
    n, lowest = 0, {}
    for i, c in enumerate(CASES):
        a, b = prepared(i)
        if not P.SABOTAGES[sab](a):
            continue
        bad = P.ref_panel(a, sab=sab)
        worst, where = 0.0, None
        for name, (r, mask, e) in b.items():
            if name not in bad or not torch.equal(bad[name][1], mask):
                ratio = float("inf")        # not written, or written elsewhere: the canaries show it
            else:
                ratio = P.excess(name, P.as_stored(name, bad[name][0]), r, mask, e)
            if ratio > worst:
                worst, where = ratio, name
        assert worst >= 10.0, (sab, P.case_id(c), worst)
        lowest[where] = min(lowest.get(where, float("inf")), worst)
        n += 1
    assert n >= 4, (sab, n)
    # per output kind: the lowest ratio among the cases whose most visible damage is on that output
    print(f"sabotage '{sab}': {n} cases, lowest worst-element ratio x e by output:", ", ".join(f"{k} {v:.1f}" for k, v in sorted(lowest.items())))


def _abs_lin(w, v):
    return v.abs() @ w.double().abs().T


@pytest.mark.parametrize("gated", [0, 1])
def test_restatement_is_the_oracles_layer(gated):
    """One layer's row-local part from the oracle's own blocks, in float64 on UNROUNDED operands: x + [g] wo(ao), + [g] feed_forward(
    ffn_norm), the next layer's skip_in_linear, attention norm, wqkv and RoPE.  The restatement differs from it by the fp16
    rounding of the operands only: each of the roundings listed in panel_cases (weights, ao, n, h, half(x)) moves a product by
    at most 2^-11 of its size, at most 8 of them stack up in front of any output, so |restatement - oracle| <= 8 * 2^-11 * (sum of
    the |terms| of that output).  The sum of |terms| is the same chain run on absolute values."""
    c = P.case(384, gated, 0, 96, "window", "post+skip+qkv", seed=77, add_one=gated)
    a = P.make_args(c)
    a["x"] = torch.randn(a["x"].shape, generator=torch.Generator().manual_seed(78))     # unit rows: the bound is about the linears
    a["ao"] = torch.randn(a["ao"].shape, generator=torch.Generator().manual_seed(79)).half()
    D = a["D"]
    rows, seq, pos = P.rows_of(a)
    d = lambda t: t.double()     # noqa: E731
    sd = {"ff.w1.weight": d(a["w1"]), "ff.w3.weight": d(a["w3"]), "ff.w2.weight": d(a["w2"])}

    class AsIs(dict):          # the oracle's blocks call .float() on the weights: keep float64
        def __getitem__(self, k):
            t = dict.__getitem__(self, k)
            t.float = lambda: t
            return t
    sd = AsIs(sd)
    one = float(a["add_one"])

    def norm(x, g, w, b):
        return O.rmsnorm(x, d(g), a["eps"]) * (one + d(w)) + d(b)
    x = d(a["x"])[rows]
    ao = d(a["ao"])[rows]
    ga, gf = (d(a["gate_a"]), d(a["gate_f"])) if gated else (1.0, 1.0)
    p1 = F.linear(ao, d(a["wo"]))
    x1 = x + ga * p1
    n = norm(x1, a["g_ffn"], a["w_f"], a["b_f"])
    ff = O.feed_forward(n, sd, "ff")
    x2 = x1 + gf * ff
    skip = d(a["skip_in"])[rows]
    x3 = F.linear(torch.cat([x2, skip], dim=-1), d(a["wskip"]), d(a["bskip"]))
    na = norm(x3, a["g_attn"], a["w_a"], a["b_a"])
    qkv = F.linear(na, d(a["wqkv"]))
    tab = d(a["rope"])[a["row_off"]:a["row_off"] + a["Lout"]]
    M = a["M"]

    def rope(v):
        return O.apply_rope(v.reshape(a["n_seq"], a["Lout"], D // 64, 64), tab).reshape(M, D)
    q, k, v = rope(qkv[:, :D]) * a["q_scale"], rope(qkv[:, D:2 * D]), qkv[:, 2 * D:]

    ref = P.ref_panel(a)
    rel = 8.0 * 2.0 ** -11
    # sums of |terms|
    h_abs = (O.silu(F.linear(n, sd["ff.w1.weight"])) * F.linear(n, sd["ff.w3.weight"])).abs()
    s_x2 = x.abs() + abs(ga) * _abs_lin(a["wo"], ao) + abs(gf) * _abs_lin(a["w2"], h_abs)
    s_x3 = d(a["bskip"]).abs() + _abs_lin(a["wskip"][:, :D], s_x2) + _abs_lin(a["wskip"][:, D:], skip)
    got_x = ref["x"][0][rows]
    assert ((got_x - x3).abs() <= rel * s_x3).all(), ((got_x - x3).abs() / s_x3).max().item() / 2.0 ** -11
    # behind the norm the row is rescaled: the error of x3 reaches n as (its share of the row) x |n|; bound it by the sums again
    rs = torch.rsqrt((x3 * x3).mean(dim=-1, keepdim=True) + a["eps"])
    A = (d(a["g_attn"]) * (one + d(a["w_a"]))).abs()
    s_n = rel * s_x3 * rs * A * 2.0 + 2.0 ** -11 * na.abs()          # x3's error (row sum and element), then n's own rounding
    s_qkv = _abs_lin(a["wqkv"], s_n) + 2.0 ** -11 * _abs_lin(a["wqkv"], na)
    pair = lambda t: (t.reshape(M, -1, 2).abs().sum(-1, keepdim=True).expand(M, -1, 2)).reshape(M, -1)     # noqa: E731
    got_qk = ref["qk"][0][rows]
    assert ((got_qk[:, :D] - q).abs() <= pair(s_qkv[:, :D]) * a["q_scale"] + 1e-12).all()
    assert ((got_qk[:, D:] - k).abs() <= pair(s_qkv[:, D:2 * D]) + 1e-12).all()
    col = torch.tensor([P.vt_pos(int(p_), a["vt_mode"]) for p_ in pos])
    got_v = ref["vt"][0][seq, :, col]
    assert ((got_v - v).abs() <= s_qkv[:, 2 * D:] + 1e-12).all()
    # and the rounding is not vacuous: the restatement does differ from the unrounded layer
    assert (got_x - x3).abs().max() > 1e-5
