"""CPU side of the length regulator's op-level suite (test_gpu_lr_ops.py): the test aid svc_op_lr is declared, exported, bound and
documented and refuses bad arguments before anything touches a device; the float64 references of lr_cases.py are pinned to torch
and the oracle; a CPU fp32 emulation of each stage stays under HALF the derived bound; outside delta the fp32 chain gives the
float64 bin in both its forms; and every named sabotage of the reference is caught by a case."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import cases
import lr_cases as L
import seedvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ the seam
def _fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", header).group(1)
    return re.findall(r"\**\s*([A-Za-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", body)


def test_seam_is_declared_exported_bound_and_documented():
    from seedvc_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    fn = "svc_op_lr"
    assert re.search(r"\b" + fn + r"\s*\(", header), fn + " is not declared in include/seedvc_hip.h"
    assert header.index("op-level entry points") < header.index(fn)
    assert fn in _lib.EXPORTS and hasattr(lib, fn) and hasattr(ops, "lr_stage")
    assert _fields(header, "svc_lr_op_t") == [f[0] for f in _lib.LrOp._fields_]
    assert fn in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = open(os.path.join(ROOT, "seed-vc_amd", "csrc", "lr.hip")).read()
    assert f"LR_GN_PARTS = {L.PARTS};" in src and ops.LR_GN_PARTS == L.PARTS
    assert "atomicAdd" not in src and "hipMemsetAsync" not in src          # the fold depends on neither


P = 4096          # dummy device pointers (never dereferenced: the checks come first)


def _args(**kw):
    """a VALID argument set of stage `stage` (3 utterances), then `kw` over it"""
    from seedvc_amd import _lib
    stage = kw.pop("stage", 0)
    v = dict(stage=stage, B=3, tout_max=9, C=80, ld=96, ylens=[9, 0, 4], x=P)
    if stage == 0:
        v.update(feat=P, ld_feat=96, tin_max=7, in_lens=[7, 1, 5], interpolate=1, f0=P, tf0_max=11, f0_lens=[11, 1, 6], f0_emb=P, f0_mask=P,
                 n_bins=256)
    elif stage in (1, 2):
        v.update(stats=P)
        if stage == 2:
            v.update(gamma=P, beta=P, eps=1e-5)
    else:
        v.update(out=P, N=80, ld_out=80)
    v.update(kw)
    e = _lib.LrOp()
    keep = []
    for k, x in v.items():
        if k in ("ylens", "in_lens", "f0_lens") and x is not None:
            keep.append((ctypes.c_int32 * len(x))(*x))
            setattr(e, k, ctypes.cast(keep[-1], ctypes.POINTER(ctypes.c_int32)))
        elif x is not None:
            setattr(e, k, x)
    return e, keep


REFUSALS = [
    (dict(stage=4), b"stage is 0 .. 3"), (dict(stage=-1), b"stage is 0 .. 3"), (dict(B=0), b"B is 1"), (dict(B=65536), b"B is 1"),
    (dict(tout_max=0), b"tout_max is positive"), (dict(ylens=None), b"ylens is required"), (dict(ylens=[9, 10, 4]), b"ylens out of range"),
    (dict(ylens=[9, -1, 4]), b"ylens out of range"), (dict(x=None), b"x is required"), (dict(C=0), b"1 <= C <= ld"), (dict(ld=79), b"1 <= C <= ld"),
    (dict(stage=1, ld=64), b"1 <= C <= ld"), (dict(stage=2, C=-1), b"1 <= C <= ld"),
    # gather
    (dict(tokens=P, emb=P), b"feat or tokens, not both"), (dict(feat=None), b"feat or tokens, not both"), (dict(ld_feat=79), b"ld_feat covers C"),
    (dict(feat=None, tokens=P), b"tokens need emb"), (dict(tin_max=0), b"tin_max is positive"), (dict(in_lens=None), b"in_lens is required"),
    (dict(in_lens=[7, 0, 5]), b"in_lens out of range"), (dict(in_lens=[8, 1, 5]), b"in_lens out of range"),
    (dict(interpolate=0), b"without interpolate"), (dict(f0_emb=None), b"f0 needs f0_emb"), (dict(n_bins=1), b"n_bins is at least 2"),
    (dict(f0=None, f0_mask=None), b"needs f0_mask"), (dict(tf0_max=0), b"tf0_max is positive"), (dict(f0_lens=None), b"f0_lens is required"),
    (dict(f0_lens=[11, 0, 6]), b"f0_lens out of range"), (dict(f0_lens=[12, 1, 6]), b"f0_lens out of range"),
    # the GroupNorm pair
    (dict(stage=1, stats=None), b"stats is required"), (dict(stage=2, stats=None), b"stats is required"), (dict(stage=2, gamma=None), b"gn_mish needs"),
    (dict(stage=2, beta=None), b"gn_mish needs"), (dict(stage=2, eps=0.0), b"gn_mish needs"),
    # mask_copy
    (dict(stage=3, out=None), b"mask_copy needs out"), (dict(stage=3, N=0), b"mask_copy: 1 <= N"), (dict(stage=3, N=97), b"mask_copy: 1 <= N"),
    (dict(stage=3, ld_out=79), b"mask_copy: 1 <= N"),
]


def test_valid_argument_sets_pass_every_check():
    """the bases of the refusal table are themselves accepted.  check_only returns before the first allocation: nothing is
    allocated or launched and no (dummy) pointer is dereferenced, with or without a device"""
    from seedvc_amd import _lib
    for kw in (dict(stage=0), dict(stage=0, f0=None), dict(stage=0, f0=None, f0_emb=None, f0_mask=None), dict(stage=0, feat=None, tokens=P, emb=P),
               dict(stage=0, interpolate=0, in_lens=[9, 1, 5], tin_max=9), dict(stage=1), dict(stage=2), dict(stage=3), dict(stage=3, ld_out=96)):
        e, keep = _args(check_only=1, **kw)
        assert _lib.lib().svc_op_lr(ctypes.byref(e), None) == 0, (kw, _lib.lib().svc_last_error())


@pytest.mark.parametrize("kw,word", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in REFUSALS])
def test_refusals_need_no_gpu(kw, word):
    from seedvc_amd import _lib
    e, keep = _args(check_only=1, **kw)      # (a row of the table that were NOT refused would still launch nothing)
    assert _lib.lib().svc_op_lr(ctypes.byref(e), None) != 0, kw
    err = _lib.lib().svc_last_error()
    assert b"requirement failed" in err and b"svc_op_lr" in err and word in err, (kw, err)


def test_null_argument_is_refused():
    from seedvc_amd import _lib
    assert _lib.lib().svc_op_lr(None, None) != 0 and b"null" in _lib.lib().svc_last_error()


# ------------------------------------------------------------------------------------------------ the index map
def test_sensitive_pairs_are_the_83_and_both_wrong_forms_differ_on_each():
    sp = L.sensitive_pairs()
    assert len(sp) == 83 and {(26, 22), (14, 46), (21, 69), (2, 82), (3, 123), (28, 92)} <= set(sp) and set(L.MODEL_PAIRS) <= set(sp)
    for tin, ylen in sp:
        assert (L.index_formula(ylen, tin, "divide") != L.index_formula(ylen, tin)).any(), (tin, ylen)
    for _, _, tin, ylen, _, _ in cases.LR_CASES.values():
        if tin <= 64 and ylen < 130:
            assert (tin, ylen) not in sp          # what the committed small cases never exercised
    bp = L.benign_pairs()
    assert len(bp) == 83 and not set(bp) & set(sp)
    assert any(t == 1 for t, _ in bp) and any(y == 1 for _, y in bp) and any(t == y for t, y in bp) and any(y < t for t, y in bp)


def test_index_map_is_the_fp32_formula_and_the_oracles():
    for tin, ylen in L.sensitive_pairs() + L.benign_pairs() + ((250, 430), (500, 430)):
        m = L.index_map(ylen, tin)
        assert torch.equal(m, torch.from_numpy(L.index_formula(ylen, tin))) and torch.equal(m, O._nearest_index(ylen, tin)), (tin, ylen)
        assert int(m.min()) >= 0 and int(m.max()) <= tin - 1


# ------------------------------------------------------------------------------------------------ the f0 bin
@pytest.mark.parametrize("n_bins", [256, 20])
def test_f0_sets_and_the_fp32_chain(n_bins):
    f = L.f0_set(n_bins)
    assert L.f0_grid().numel() <= 16384 and tuple(L.f0_boundaries(n_bins).shape) == (n_bins - 1, 17)
    assert bool(torch.isfinite(f).all()) and bool((f >= 0).all())
    b64, inside, lo, hi = L.f0_judgement(f, n_bins)
    # the boundaries are boundaries: each row of set (b) holds both of its bins, and its middle value lies inside delta
    bb = L.f0_bin64(L.f0_boundaries(n_bins), n_bins)
    k = torch.arange(1, n_bins)
    assert torch.equal(bb[:, 0], k) and torch.equal(bb[:, -1], torch.where(k + 1 < n_bins, k + 1, torch.zeros_like(k)))
    assert bool(L.f0_judgement(L.f0_boundaries(n_bins)[:, 8], n_bins)[1].all())
    # the quirks
    q = lambda v: int(L.f0_bin64(torch.tensor([v], dtype=torch.float32), n_bins))
    assert q(0.0) == 1 and q(49.9) == 1 and q(50.0) == 1 and q(1100.0) == n_bins - 1 and q(1500.0) == 0 and q(3e38) == 0
    # the fp32 restatement is the oracle's, bit for bit; outside delta both fp32 forms give the float64 bin; inside, a neighbour
    assert torch.equal(L.f0_bin32(f, n_bins, "two"), O.lr_f0_to_coarse(f, n_bins))
    worst = 0.0
    for form in ("two", "fma"):
        b32 = L.f0_bin32(f, n_bins, form)
        assert torch.equal(b32[~inside], b64[~inside]), form
        assert bool(((b32 == lo) | (b32 == hi))[inside].all()), form
        live = (L.f0_pre64(f, n_bins) > 0) & (f < 2000)
        r = ((L.f0_pre32(f, n_bins, form).double() - L.f0_pre64(f, n_bins)).abs() / L.f0_delta(f, n_bins))[live]
        worst = max(worst, float(r.max()))
    # a condition, not a measurement: the share of the uniform grid that delta leaves out
    share = float(L.f0_judgement(L.f0_grid(), n_bins)[1].double().mean())
    dmax = float(L.f0_delta(torch.tensor([1600.0]), n_bins))
    print(f"n_bins {n_bins}: delta at 1600 Hz {dmax:.3e}, grid share inside delta {100 * share:.4f} %, {int(inside.sum())} of {f.numel()} values inside, "
          f"worst |pre32 - pre64| / delta {worst:.3f}")
    assert share <= 1e-3 and worst <= 0.5


# ------------------------------------------------------------------------------------------------ references against torch and the oracle
@pytest.mark.parametrize("name", list(cases.LR_CASES))
def test_float64_model_agrees_with_the_oracle(name):
    c, sd, x, ylen, f0, meta = cases.lr_case(name)
    ref = O.lr_forward(sd, c, x, ylen, f0)
    got = L.model64(sd, c, x, ylen, f0)
    assert got.shape == ref.shape
    assert (got - ref.double()).abs().max().item() < 5e-5


def test_stage_references_are_torchs():
    x, ylens, C = L.stats_cases()["C80"]
    ref, _ = L.stats_ref(x, ylens, C)
    for b, n in enumerate(ylens):
        v = x[b, :n, :C].double()
        assert torch.allclose(ref[b].sum(0), torch.stack([v.sum(), (v * v).sum()]), rtol=1e-12, atol=0)
    x, stats, gamma, beta, ylens, C = L.mish_cases()["C80"]
    ref, _ = L.mish_ref(x, stats, gamma, beta, ylens, C)
    for b, n in enumerate(ylens):
        if n:
            v = x[b, :n, :C].double().t()[None]          # (1, C, n): GroupNorm(1, C) then Mish, as the module has them
            y = F.mish(F.group_norm(v, 1, gamma.double(), beta.double(), L.EPS))[0].t()
            assert torch.allclose(ref[b, :n, :C], y, rtol=0, atol=1e-9 * (1 + float(v.abs().max())) ** 2), b
        assert bool((ref[b, n:] == 0).all()) and bool((ref[b, :, C:] == 0).all())
    v = torch.tensor([-800.0, -90.0, -1.0, 0.0, 19.999999, 20.0, 20.000001, 21.0, 30.0, 700.0, 800.0], dtype=torch.float64)
    assert torch.equal(L.softplus64(v), F.softplus(v))


# ------------------------------------------------------------------------------------------------ emulation, sabotages
def test_emulation_is_within_half_the_bound():
    for name, (x, ylens, C) in L.stats_cases().items():
        ref, E = L.stats_ref(x, ylens, C)
        bad, worst = L.judge(ref, E, L.stats_emulate(x, ylens, C), scale=0.5)
        print(f"gn_stats {name}: emulation worst error / bound {worst:.3f}")
        assert not bad, name
    for name, (x, stats, gamma, beta, ylens, C) in L.mish_cases().items():
        ref, E = L.mish_ref(x, stats, gamma, beta, ylens, C)
        bad, worst = L.judge(ref, E, L.mish_emulate(x, stats, gamma, beta, ylens, C), scale=0.5)
        print(f"gn_mish {name}: emulation worst error / bound {worst:.3f}, largest bound {float(E.max()):.2e}")
        assert not bad, name


def _caught(sab):
    """the first case on which the sabotaged reference leaves what the true one is held to, or None"""
    if sab in ("index_exact", "index_divide"):
        for tin, ylen in L.sensitive_pairs() + L.benign_pairs():
            if not torch.equal(L.source_index(ylen, tin, 1, sab), L.index_map(ylen, tin)):
                return f"pair {tin} -> {ylen}"
    elif sab in ("round_half_away", "overflow_to_last"):
        # the float64 bin where it changes it (outside delta the device must give the true one); rounding ties exist only in the
        # fp32 chain (no fp32 input of the sets has a float64 pre-round value of k + 0.5 exactly), so the rounding mode is held
        # where the reference is pinned to the oracle: its fp32 restatement, bit for bit
        for n_bins in (256, 20):
            f = L.f0_set(n_bins)
            b64, inside, _, _ = L.f0_judgement(f, n_bins)
            d = (L.f0_bin64(f, n_bins, sab) != b64) & ~inside
            if bool(d.any()):
                return f"n_bins {n_bins}: f0 {float(f[d][0])!r} (float64 bin)"
            d = L.f0_bin32(f, n_bins, "two", sab) != O.lr_f0_to_coarse(f, n_bins)
            if bool(d.any()):
                return f"n_bins {n_bins}: f0 {float(f[d][0])!r} (fp32 restatement against the oracle)"
    elif sab.startswith("stats_"):
        for name, (x, ylens, C) in L.stats_cases().items():
            ref, E = L.stats_ref(x, ylens, C)
            if L.judge(ref, E, L.stats_ref(x, ylens, C, sab)[0])[0]:
                return "gn_stats " + name
    else:
        for name, (x, stats, gamma, beta, ylens, C) in L.mish_cases().items():
            ref, E = L.mish_ref(x, stats, gamma, beta, ylens, C)
            if L.judge(ref, E, L.mish_ref(x, stats, gamma, beta, ylens, C, sab=sab)[0])[0]:
                return "gn_mish " + name
        if sab == "softplus_no_threshold":      # invisible in o (lr_cases.py says why): held at softplus itself
            v = torch.tensor([20.000001, 21.0, 30.0], dtype=torch.float64)
            if not torch.equal(L.softplus64(v, sab), F.softplus(v)):
                return "softplus64 against F.softplus at 21"
    return None


@pytest.mark.parametrize("sab", L.SABOTAGES)
def test_every_sabotage_is_caught_by_a_case(sab):
    hit = _caught(sab)
    print(f"{sab}: {hit}")
    assert hit, sab + " is caught by no case"
