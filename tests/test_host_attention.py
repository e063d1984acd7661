"""CPU side of the attention kernels' op-level suite (test_gpu_attention.py): the raw seam is declared, exported and bound, its
refusals come before anything touches a device, and the checks of attention_cases.py check themselves: the emulation of the
kernels' numerics passes them on every case, and every sabotage of the emulation is caught by every case able to show it."""
import ctypes
import os
import re

import pytest
import torch

import attention_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

CASES = A.parity_cases()
IDS = [A.case_id(c) for c in CASES]
_memo = {}


def prepared(i):
    """(launch, reference, unsabotaged emulation) of case i, computed once for all the tests of this module"""
    if i not in _memo:
        a = A.build(CASES[i])
        ref = A.ref_attention(*A.logical(a), a["lens"], a["q_start"], a["Tq"])
        _memo[i] = (a, ref, A.emulate(a))
    return _memo[i]


def test_every_instantiation_has_a_case():
    assert len(A.INSTANTIATIONS) == 12 and len(set(IDS)) == len(CASES)
    for kind in A.KINDS:
        assert set(A.INSTANTIATIONS) <= {A.instantiation(c) for c in CASES if c["kind"] == kind}, kind
    small = [c for c in CASES if c["qt_form"] == 0]
    assert {c["vt_perm"] for c in small} == {0, 1, 2}
    for c in small:         # the launcher's rule: at most 256 workgroups of 128 queries take the 64-query form
        assert -(-c["nq"] // 128) * c["H"] * len(c["lens"]) <= 256


def test_shapes_cover_the_edges():
    assert {L for c in CASES for L in c["lens"]} == set(A.KEY_LENS)
    assert {c["nq"] for c in CASES} == set(A.N_QUERIES) and {c["q_start"] for c in CASES} == set(A.Q_STARTS)
    assert {c["H"] for c in CASES} == {1, 2, 3} and {len(c["lens"]) for c in CASES} == {1, 2, 3, 4, 5}
    assert {bool(c["ld3"]) for c in CASES} == {False, True} and {c["vt_extra"] for c in CASES} == {0, 64}
    assert {c["const"] for c in CASES} == {False, True}
    tight = [A.shape_of(c)[1] == A.round_up(c["q_start"] + c["nq"], 8) for c in CASES]
    assert any(tight) and not all(tight)
    assert any(len(set(c["lens"])) > 2 for c in CASES)          # lengths mixed inside one launch
    for c in CASES:
        Tq, R, vt_ld = A.shape_of(c)
        assert max(c["lens"]) <= R and Tq <= R and A.round_up(max(c["lens"]), 64) <= vt_ld


def test_seam_is_declared_exported_and_bound():
    from seedvc_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    name = "svc_op_attention_ex"
    assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/seedvc_hip.h"
    assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(ops, "attention_ex")
    body = re.search(r"typedef struct \{([^}]*)\} svc_attention_t;", header).group(1)
    fields = re.findall(r"\**\s*([A-Za-z_0-9]+)\s*[,;]", body)
    assert fields == [f[0] for f in _lib.Attention._fields_]
    assert fields == ["q", "k", "vt", "out", "out32", "ld_qk", "vt_seq_stride", "vt_ld", "ld_out", "n_seq", "H", "seq_rows", "Tq",
                      "q_start", "kv_len", "kv_len_const", "vt_perm", "qt_form"]


def refusal_args(**kw):
    """A launch the entry point takes (2 sequences of 72 rows, 2 heads, queries [8, 70)) with every pointer a dummy, then kw on top."""
    from seedvc_amd import _lib
    e = _lib.Attention()
    e.q, e.k, e.vt, e.out = 4096, 4096 + 256, 8192, 16384                  # never dereferenced: the checks come first
    e.ld_qk, e.vt_ld, e.vt_seq_stride, e.ld_out = 256, 128, 128 * 128, 128
    e.n_seq, e.H, e.seq_rows, e.Tq, e.q_start = 2, 2, 72, 70, 8
    e.kv_len_const, e.vt_perm, e.qt_form = 70, 1, 0
    keep = None
    for k, v in kw.items():
        if k == "kv_len":
            keep = (ctypes.c_int64 * len(v))(*v)
            e.kv_len = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int64))
        else:
            setattr(e, k, v)
    return e, keep


REFUSALS = [
    (dict(q=None), b"q, k and vt"), (dict(k=None), b"q, k and vt"), (dict(vt=None), b"q, k and vt"),
    (dict(out32=32768), b"exactly one of out and out32"), (dict(out=None), b"exactly one of out and out32"),
    (dict(vt_perm=3), b"vt_perm"), (dict(vt_perm=-1), b"vt_perm"), (dict(qt_form=3), b"qt_form"), (dict(qt_form=-1), b"qt_form"),
    (dict(Tq=73), b"Tq <= seq_rows"), (dict(Tq=0, q_start=0), b"Tq"),
    (dict(q_start=-1), b"q_start"), (dict(q_start=70), b"q_start"), (dict(q_start=72), b"q_start"),
    (dict(kv_len_const=-1), b"kv_len"), (dict(kv_len_const=73), b"kv_len"), (dict(kv_len_const=72, seq_rows=136, vt_ld=64, vt_seq_stride=128 * 64), b"kv_len"),
    (dict(kv_len=[70, -1]), b"kv_len"), (dict(kv_len=[73, 1]), b"kv_len"), (dict(kv_len=[1, 65], vt_ld=64), b"kv_len"),
    (dict(vt_seq_stride=128 * 128 - 8), b"vt_seq_stride"),
    (dict(vt_ld=96, vt_seq_stride=128 * 96), b"alignment"), (dict(ld_qk=260), b"alignment"), (dict(ld_out=130), b"alignment"),
    (dict(q=4096 + 8), b"alignment"), (dict(vt=8192 + 8), b"alignment"), (dict(out=16384 + 4), b"alignment"),
    (dict(out=None, out32=32768 + 8), b"alignment"),
    (dict(ld_qk=64), b"ld_qk"), (dict(ld_out=64), b"ld_out"), (dict(n_seq=0), b"n_seq"), (dict(H=0), b"H"),
]


@pytest.mark.parametrize("kw,word", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_refusals_need_no_gpu(kw, word):
    """The argument checks come before anything is allocated, copied or launched: dummy pointers, no device."""
    from seedvc_amd import _lib
    fn, err = _lib.lib().svc_op_attention_ex, _lib.lib().svc_last_error
    e, keep = refusal_args(**kw)
    assert fn(ctypes.byref(e), None) != 0, kw
    assert word in err(), (kw, err())


def test_vt_pos_modes():
    """the three column orders: permutations of every 32-group (mode 2 of every 16-group), mode 0 the identity; mode 1 and 2 written
    out once from common.h's prose"""
    t1 = [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27, 4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    t2 = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15]
    assert [A.vt_pos(p, 0) for p in range(384)] == list(range(384))
    assert [A.vt_pos(p, 1) for p in range(64)] == t1 + [32 + v for v in t1]
    assert [A.vt_pos(p, 2) for p in range(64)] == [16 * g + v for g in range(4) for v in t2]
    for mode in (0, 1, 2):
        for base in range(0, 384, 32):
            assert sorted(A.vt_pos(p, mode) for p in range(base, base + 32)) == list(range(base, base + 32))
    for base in range(0, 384, 16):
        assert sorted(A.vt_pos(p, 2) for p in range(base, base + 16)) == list(range(base, base + 16))
    # the layout reads back what it stored, in every mode
    for mode in (0, 1, 2):
        c = A.case("numeric", 2, [70, 33], 65, 0, 8, 1, 64, mode, 1, 0, seed=5)
        a = A.build(c)
        qs, k, v = A.logical(a)
        b = A.build(dict(c, vt_perm=0))
        assert torch.equal(v, A.logical(b)[2]) and torch.equal(qs, A.logical(b)[0]) and torch.equal(k, A.logical(b)[1])
        assert (mode == 0) == torch.equal(a["vt"], b["vt"])


def test_rtz16():
    x = torch.tensor([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10 - 2.0 ** -20, 2.0 ** -24, 2.0 ** -24 * 1.9, 2.0 ** -25, 255.9, 2.0 ** -14 * 1.0001])
    want = torch.tensor([0.0, 1.0, 1.0, 1.0, 2.0 ** -24, 2.0 ** -24, 0.0, 255.875, 2.0 ** -14])
    assert torch.equal(A.rtz16(x), want)
    x = torch.rand(100000, generator=torch.Generator().manual_seed(3)) * 256.0
    r = A.rtz16(x)
    assert (r <= x).all() and ((x - r) < x * 2.0 ** -10 + 2.0 ** -24).all() and torch.equal(r, r.half().float())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_preconditions_and_emulation(i):
    """What each kind rests on holds for the case, and the emulation passes the case's check: with the baseline at the first
    tile's maximum (every kind), and 3 and 7.9 below it (numeric: the bound holds for any baseline within 8 of the maximum)."""
    a, ref, emu = prepared(i)
    c = CASES[i]
    if c["kind"] == "routing":
        assert a["gap"] > 26.0, a["gap"]
        D = 64 * a["H"]
        rows = A.window(a)
        assert ((ref[0].reshape(-1, D) - a["want"])[rows].abs() < 2.0 ** -4).all()
    if c["kind"] == "uniform":
        qs, _, v = A.logical(a)
        assert not qs[:, a["q_start"]:a["Tq"]].any()
        for s, L in enumerate(a["lens"]):
            assert torch.equal(v[s, :L].double(), v[s, :L].double().round()) and v[s, :L].abs().max().item() <= 8 if L else True
    assert A.canaries_intact(a, emu)
    ok, ratio, text = A.check(a, emu, ref)
    assert ok, text
    if c["kind"] == "numeric":
        worst = ratio
        for slack in (3.0, 7.9):
            ok, ratio, text = A.check(a, A.emulate(a, slack=slack), ref)
            assert ok, (slack, text)
            worst = max(worst, ratio)
        print(f"attention emulation {IDS[i]}: worst |emu - ref| / bound = {worst:.3f}")
        # the bound is not vacuous for the reference itself: an exact evaluation in the output's format passes by a wide margin
        exact = A.empty_out(a)
        exact[A.window(a), :64 * a["H"]] = ref[0].reshape(-1, 64 * a["H"])[A.window(a)].to(exact.dtype)
        assert A.check(a, exact, ref)[1] <= 0.5


def test_routing_margin_at_three_lengths():
    """The routing kind at T = 70, 131, 200 with kv_len = T, T - 3, T / 2 + 1: `build` asserts gap > 26 (the need is 25: off-target
    P below half the smallest fp16 subnormal) and |ref - v| < 2^-4; here the margins themselves, which are far wider."""
    worst_gap, worst_ref = float("inf"), 0.0
    for T in (70, 131, 200):
        for L in (T, T - 3, T // 2 + 1):
            for H in (1, 3):
                a = A.build(A.case("routing", H, [L], T, 0, 0, 0, 0, 1, 1, 0, seed=7000 + T + L))
                ref = A.ref_attention(*A.logical(a), a["lens"], 0, T)[0].reshape(-1, 64 * H)
                rows = A.window(a)
                worst_gap = min(worst_gap, a["gap"])
                worst_ref = max(worst_ref, (ref - a["want"])[rows].abs().max().item())
    print(f"routing: smallest target-to-other gap {worst_gap:.1f} (log2 units), largest |ref - v| {worst_ref:.1e}")
    # each of at most 200 off-target keys weighs at most 2^-gap and differs from the target's v by at most 1020
    assert worst_gap > 26.0 and worst_ref <= 200 * 2.0 ** -worst_gap * 1020


# sabotage -> the kinds of which at least one case must be able to show it.  A kind is missing where its construction hides the
# sabotage from EVERY case of it: the unit kind's output is 2^e x l / l whatever the V order, the rescale or the baseline
# (only the mask edge and the row sum show there); uniform P is exactly 1 with no baseline move and no rounding; routing's
# off-target P are 0 rounded or not.
MUST_SHOW = {
    "swap16": ("numeric", "routing", "uniform", "unit"),
    "mode1as2": ("numeric", "routing", "uniform", "unit"),
    "nomask": ("numeric", "routing", "uniform", "unit"),
    "mask+1": ("numeric", "routing", "uniform", "unit"),
    "norescale": ("numeric", "routing"),
    "sum_unrounded": ("numeric", "unit"),
    "neighbour_len": ("numeric", "routing", "uniform", "unit"),
}


@pytest.mark.parametrize("sab", list(A.SABOTAGES))
def test_sabotage_is_caught(sab):
    """A case is able to show a sabotage when the sabotaged emulation differs from the unsabotaged one in any bit (a unit case
    with the fp32 output: in any bit once rounded to fp16, the precision of that kind's claim).  Every able case must catch it: exact kinds by an exact mismatch, numeric ones by exceeding the bound (the excess is printed).

    One exception, by proof and not by measurement: `sum_unrounded` on NUMERIC cases.  The bound's first item, 2^-10 (w @ |v|), is
    the allowance for P's round-toward-zero entering numerator and row sum; a row sum of the unrounded P shifts the output by
    sum_j w_j d_j v_j with 0 <= d_j < 2^-10, which is inside that allowance for any data.  No bound that admits the kernels'
    rounding can reject it.  The unit kind exists for this sabotage: there the row sum must cancel the numerator exactly.  The
    numeric cases' ratios are printed; every able unit case must catch it."""
    able = {k: 0 for k in A.KINDS}
    low, high = float("inf"), 0.0
    for i, c in enumerate(CASES):
        a, ref, emu = prepared(i)
        bad = A.emulate(a, sab=sab)
        if torch.equal(A.bits(bad), A.bits(emu)):
            continue
        if c["kind"] == "unit" and torch.equal(A.bits(bad.half()), A.bits(emu.half())):
            continue        # fp32 output of 2^e x l x (1 / l): its last bits depend on l and are not part of the kind's claim
        able[c["kind"]] += 1
        ok, ratio, text = A.check(a, bad, ref)
        if c["kind"] == "numeric":
            low, high = min(low, ratio), max(high, ratio)
            if sab == "sum_unrounded":
                assert ratio < 1.0, "the proof in the docstring is wrong"
                continue
        assert not ok, (sab, IDS[i], text)
    for kind in MUST_SHOW[sab]:
        assert able[kind] >= 1, (sab, kind, able)
    print(f"sabotage '{sab}': able cases by kind {able}; numeric |bad - ref| / bound from {low:.2f} to {high:.2f}")


def test_every_kind_shows_some_sabotage():
    assert all(any(kind in kinds for kinds in MUST_SHOW.values()) for kind in A.KINDS)
