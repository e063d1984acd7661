"""CPU side of the tap-GEMM's op-level suite (test_gpu_kgemm.py): the test aid is declared, exported and bound and refuses bad
arguments before anything touches a device (its own range checks and the new refusals of kgemm_launch); the float64 reference of
kgemm_cases.py is pinned to torch and the oracle; the fp32 emulation stays under HALF the bound on every element of every case;
every named sabotage of the reference leaves the bound on at least one case; the cases cover every enumerator of common.h; and the
aid's host-side range computation, restated in Python, agrees with the rows the reference addresses."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import kgemm_cases as K
import seedvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ the seam
def _fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", header).group(1)
    return re.findall(r"\**\s*([A-Za-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", body)


def test_seam_is_declared_exported_and_bound():
    from seedvc_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fn = "svc_op_kgemm"
    assert re.search(r"\b" + fn + r"\s*\(", header), fn + " is not declared in include/seedvc_hip.h"
    assert header.index("op-level entry points") < header.index(fn)
    assert fn in _lib.EXPORTS and hasattr(lib, fn) and hasattr(ops, "kgemm")
    assert _fields(header, "svc_kgemm_t") == [f[0] for f in _lib.KGemm._fields_]
    assert fn in doc
    fn = "svc_op_permute_vt"
    assert re.search(r"\b" + fn + r"\s*\(", header) and header.index("op-level entry points") < header.index(fn)
    assert fn in _lib.EXPORTS and hasattr(lib, fn) and hasattr(ops, "permute_vt") and fn in doc


P = 4096          # dummy device pointers (16-byte aligned, never dereferenced: the checks come first)


def _args(**kw):
    """a VALID argument set (3 sequences of 5 positions, 3 centred taps on one source), then `kw` over it"""
    from seedvc_amd import _lib
    v = dict(dtype=0, epi=0, form=0, n_src=1, n_taps=3, w=P, w_rows=256, M=15, N=24, Lout=5, a_seq_rows=5, a_off=0, a_stride=1, a_len=5,
             pad_mode=0, reflect_min=0, c_seq_rows=5, c_off=0, c_rows=15, ldc=24, c32=P, vec_ok=1, bias=P)
    src = dict(a_src=[P], a_rows=[15], a_K=[64], tap_src=[0, 0, 0], tap_shift=[-1, 0, 1], tap_K=[64, 64, 64])
    for k in list(kw):
        if k in src:
            src[k] = kw.pop(k)
    v.update(kw)
    e = _lib.KGemm()
    keep = []
    for k, x in src.items():
        for i, y in enumerate(x):
            getattr(e, k)[i] = y
    for k, x in v.items():
        if k in ("seq_len", "a_seq_map") and x is not None:
            keep.append((ctypes.c_int32 * len(x))(*x))
            setattr(e, k, ctypes.cast(keep[-1], ctypes.POINTER(ctypes.c_int32)))
        elif x is not None:
            setattr(e, k, x)
    return e, keep


_QKV = dict(epi=3, N=384, w_rows=512, rope_D=128, ldc=256, c32=None, c16=P, bias=None, rope=P, rope_rows=5, vt=P, vt_ld=64)
_GLU = dict(epi=1, N=64, ldc=32, c32=None, c16=P)
REFUSALS = [
    # the aid's own checks
    (dict(dtype=2), b"dtype is 0"), (dict(epi=4), b"epi is 0 .. 3"), (dict(form=0x41), b"form holds"), (dict(n_src=0), b"n_src is 1 .. 4"),
    (dict(n_src=5), b"n_src is 1 .. 4"), (dict(n_taps=0), b"n_taps is 1 .. 48"), (dict(n_taps=49), b"n_taps is 1 .. 48"), (dict(M=0), b"are positive"),
    (dict(a_stride=0), b"are positive"), (dict(pad_mode=3), b"pad_mode is 0 .. 2"), (dict(w=None), b"w is required"), (dict(a_src=[None]), b"every source"),
    (dict(tap_src=[0, 1, 0]), b"source lies in"), (dict(tap_K=[64, 32, 64]), b"its source's K"), (dict(w_rows=128), b"rounded up to 256"),
    (dict(seq_len=[5, -1, 5]), b"length is negative"), (dict(pad_mode=2, seq_len=[5, 0, 5]), b"KG_PAD_CLAMP has no row"),
    (dict(a_seq_map=[0, -1, 1]), b"a_seq_map entry is negative"),
    # a source row outside its buffer: too few rows, a length beyond the rows, a gather beyond them, a stride, an offset, a clamp
    (dict(a_rows=[14]), b"outside its buffer"), (dict(a_len=6), b"outside its buffer"), (dict(a_seq_map=[0, 3, 1]), b"outside its buffer"),
    (dict(a_stride=2, a_len=10), b"outside its buffer"), (dict(a_off=1), b"outside its buffer"), (dict(seq_len=[5, 5, 6], pad_mode=2), b"outside its buffer"),
    (dict(seq_len=[5, 5, 7], pad_mode=1), b"outside its buffer"),
    # output rows and columns
    (dict(c_off=1), b"output rows"), (dict(c_off=-1, c_seq_rows=9, c_rows=27), b"output rows"), (dict(c_rows=14), b"output rows"), (dict(ldc=16), b"ldc covers"),
    (dict(c32=None), b"an output"), (dict(c16_lo=P), b"c16_lo is an output of the Snake"), (dict(post_a=P), b"come together"),
    # 16-byte access
    (dict(N=20, ldc=24), b"multiples of 8"), (dict(ldc=28), b"multiples of 8"), (dict(c32=P + 4), b"16-byte aligned"), (dict(res=P + 8), b"16-byte aligned"),
    (dict(bias=P + 4), b"16-byte aligned"),
    # QKV buffers
    (dict(_QKV, rope_rows=4), b"rope has a row"), (dict(_QKV, vt_ld=16), b"vt_ld a multiple"), (dict(_QKV, vt_ld=66), b"vt_ld a multiple"), (dict(_QKV, vt_mode=3), b"vt_mode is 0 .. 2"),
    (dict(_QKV, rope=None), b"needs rope"), (dict(_QKV, dtype=1), b"fp32 operands"), (dict(_GLU, dtype=1), b"fp32 operands"),
    # the refusals of kgemm_launch itself
    (dict(_GLU, act=1), b"leave them unset"), (dict(_GLU, gate=P), b"leave them unset"), (dict(_GLU, res=P), b"leave them unset"), (dict(_GLU, res2=P), b"leave them unset"),
    (dict(_GLU, out_scale=0.5), b"leave them unset"), (dict(_GLU, post_relu=1), b"leave them unset"), (dict(_GLU, post_a=P, post_ib=P), b"leave them unset"),
    (dict(_GLU, epi=2, act=4), b"leave them unset"), (dict(_QKV, out_scale=2.0), b"leave them unset"),
    (dict(_GLU, c16=None, c32=P), b"write c16"), (dict(_GLU, N=40, ldc=24), b"multiple of 16"), (dict(_GLU, epi=2, N=72, ldc=40), b"multiple of 16"),
    (dict(_QKV, bias=P), b"no bias and no rowvec"), (dict(_QKV, rowvec=P), b"no bias and no rowvec"), (dict(_QKV, c32=P), b"no c32 output"),
    (dict(_QKV, N=400, w_rows=512), b"N = 3 rope_D"), (dict(_QKV, rope_D=96, N=288, ldc=192), b"N = 3 rope_D"),
]


def test_a_valid_argument_set_passes_every_check():
    """the bases of the refusal table are themselves accepted.  check_only returns before the first allocation: with or without a
    device nothing is allocated, packed or launched, and no (dummy) pointer is dereferenced"""
    from seedvc_amd import _lib
    for kw in ({}, _QKV, _GLU):
        e, keep = _args(check_only=1, **kw)
        assert e.check_only == 1
        assert _lib.lib().svc_op_kgemm(ctypes.byref(e), None) == 0, (kw, _lib.lib().svc_last_error())


@pytest.mark.parametrize("kw,word", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in kw.items() if k not in _QKV or kw.get("epi", 0) == 0 or _QKV.get(k, _GLU.get(k)) != v)
                                                    + ("|qkv" if kw.get("epi") == 3 else "|glu" if kw.get("epi") in (1, 2) else "") for kw, _ in REFUSALS])
def test_refusals_need_no_gpu(kw, word):
    from seedvc_amd import _lib
    e, keep = _args(check_only=1, **kw)      # (a row of the table that were NOT refused would still launch nothing)
    assert _lib.lib().svc_op_kgemm(ctypes.byref(e), None) != 0, kw
    err = _lib.lib().svc_last_error()
    assert b"requirement failed" in err and word in err, (kw, err)


def test_null_argument_is_refused():
    from seedvc_amd import _lib
    assert _lib.lib().svc_op_kgemm(None, None) != 0 and b"null" in _lib.lib().svc_last_error()


@pytest.mark.parametrize("vt,rows,vt_ld,mode", [(None, 4, 64, 1), (P, 0, 64, 1), (P, 4, 0, 1), (P, 4, 48, 1), (P, 4, 64, 3), (P, 4, 64, -1)])
def test_permute_vt_refusals_need_no_gpu(vt, rows, vt_ld, mode):
    from seedvc_amd import _lib
    assert _lib.lib().svc_op_permute_vt(vt, rows, vt_ld, mode, None) != 0
    assert b"svc_op_permute_vt" in _lib.lib().svc_last_error()


# ------------------------------------------------------------------------------------------------ the reference against torch and the oracle
def _conv_case(pad_mode, k, d, L, lens=None, reflect_min=0, B=2, Cin=40, Cout=24):
    left = (k - 1) * d - ((k - 1) * d) // 2
    taps = [(0, t * d - left) for t in range(k)]
    c = K.build("pin", "pin", seed=7 + k + d + L, nseq=B, Lout=L, N=Cout, K=(Cin,), taps=taps, pad_mode=pad_mode, reflect_min=reflect_min,
                seq_len=lens, a_seq_rows=L, terms=("bias",))
    w = c["W"].half().double().reshape(Cout, k, Cin).permute(0, 2, 1).contiguous()       # W[n][t Cin + ci] = w[n][ci][t]
    x = c["src_clean"][0].half().double().reshape(B, L, Cin).permute(0, 2, 1)             # (B, Cin, L)
    return c, x, w, left, (k - 1) * d - left


@pytest.mark.parametrize("mode,torch_mode", [(K.PAD_ZERO, "constant"), (K.PAD_REFLECT, "reflect"), (K.PAD_CLAMP, "replicate")])
@pytest.mark.parametrize("k,d", [(3, 1), (5, 2), (7, 1)])
def test_row_map_is_conv1d_over_pad(mode, torch_mode, k, d):
    c, x, w, left, right = _conv_case(mode, k, d, L=11)
    ref = K.reference(c)["c32"]["ref"][:, :c["N"]].reshape(2, 11, -1)
    y = F.conv1d(F.pad(x, (left, right), mode=torch_mode), w, c["bias"].double(), dilation=d).permute(0, 2, 1)
    assert torch.allclose(ref, y, rtol=0, atol=1e-12)


@pytest.mark.parametrize("ln", [1, 2, 3, 4, 5, 9])
def test_reflect_min_is_the_oracles_small_input_rule(ln):
    """dit.hip's WaveNet form: reflect_min = max(left, right) + 1 on a sequence of `ln` valid rows (k = 5, dilation 2: 4 | 4)"""
    c, x, w, left, right = _conv_case(K.PAD_REFLECT, 5, 2, L=9, lens=[ln, 9], reflect_min=5)
    ref = K.reference(c)["c32"]["ref"][:, :c["N"]].reshape(2, 9, -1)
    y = O.sconv1d_reflect(x[0:1, :, :ln], w, c["bias"].double(), dilation=2).permute(0, 2, 1)[0]
    assert torch.allclose(ref[0, :ln], y, rtol=0, atol=1e-12)


def test_paired_epilogues_are_silu_and_tanh_sigmoid():
    for nm, fn in (("swiglu-N64-M65", lambda a, b: F.silu(a) * b), ("tanhsig-N64-M65", lambda a, b: torch.tanh(a) * torch.sigmoid(b))):
        c = K.case(nm)
        v = K.accumulate(c, c["src"])[0] + c["bias"].double()[None]
        assert torch.allclose(K.reference(c)["c16"]["ref"][:, :32], fn(v[:, 0::2], v[:, 1::2]), rtol=0, atol=1e-12)


def test_rope_is_the_oracles_interleaved_rotation():
    c = K.case("qkv-D128-L7x3-vt1")
    D = 128
    v = K.accumulate(c, c["src"])[0]
    ref = K.reference(c)["c16"]["ref"][:, :2 * D].reshape(3, 7, 2 * D)
    for part, scale in ((0, float(torch.tensor(c["q_scale"], dtype=torch.float32))), (1, 1.0)):
        x = v[:, part * D:(part + 1) * D].reshape(3, 7, 2, 64)
        y = O.apply_rope(x, c["rope"].double()).reshape(3, 7, D) * scale
        assert torch.allclose(ref[..., part * D:(part + 1) * D], y, rtol=0, atol=1e-12)
    vt = K.reference(c)["vt"]["ref"].reshape(3, D, -1)
    for p in range(7):
        assert torch.equal(vt[:, :, K.vt_pos(p, 1)], v[:, 2 * D:].reshape(3, 7, D)[:, p])


def test_vt_pos_is_the_two_permutations_of_common_h():
    m1 = [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27, 4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]
    m2 = [0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19, 24, 25, 26, 27, 20, 21, 22, 23, 28, 29, 30, 31]
    for base in (0, 32, 96):
        assert [K.vt_pos(base + p, 1) for p in range(32)] == [base + v for v in m1]
        assert [K.vt_pos(base + p, 2) for p in range(32)] == [base + v for v in m2]
        assert [K.vt_pos(base + p, 0) for p in range(32)] == [base + p for p in range(32)]
    src = open(os.path.join(ROOT, "seed-vc_amd", "csrc", "common.h")).read()
    assert "(pos & ~31) | (((pos >> 2) & 3) << 3) | (((pos >> 4) & 1) << 2) | (pos & 3)" in src
    assert "(pos & ~12) | ((pos & 4) << 1) | ((pos & 8) >> 1)" in src


# ------------------------------------------------------------------------------------------------ cases, emulation, sabotages
def test_reference_is_finite_where_written_and_cases_are_named_once():
    for c in K.all_cases():
        for name, e in K.reference(c).items():
            assert bool(torch.isfinite(e["ref"][e["mask"]]).all()) and bool((e["E"][e["mask"]] >= 0).all()), (c["name"], name)
            assert bool(e["mask"].any()), (c["name"], name)


def test_cases_cover_every_enumerator_of_common_h():
    src = open(os.path.join(ROOT, "seed-vc_amd", "csrc", "common.h")).read()
    enums = {}
    for body in re.findall(r"enum \{([^}]*KG_[^}]*)\}", src):
        body = re.sub(r"/\*.*?\*/|//[^\n]*", "", body, flags=re.S)
        for name, val in re.findall(r"(KG_[A-Z_0-9]+)\s*=\s*(\d+)", body):
            enums[name] = int(val)
    cs = K.all_cases()
    acts = {n: v for n, v in enums.items() if n.startswith("KG_ACT_")}
    epis = {n: v for n, v in enums.items() if n.startswith("KG_EPI_")}
    pads = {n: v for n, v in enums.items() if n.startswith("KG_PAD_")}
    assert len(acts) >= 9 and len(epis) >= 5 and len(pads) == 3
    assert sorted(acts.values()) == sorted(K.ACT.values()) and sorted(pads.values()) == [K.PAD_ZERO, K.PAD_REFLECT, K.PAD_CLAMP]
    for n, v in acts.items():
        assert any(c["epi"] == 0 and c["act"] == v for c in cs), n + " has no case"
    for n, v in pads.items():
        assert any(c["pad_mode"] == v for c in cs), n + " has no case"
    for n, v in epis.items():
        if n == "KG_EPI_STORE_GELU":       # selected by the launch for STORE with KG_ACT_GELU
            assert any(c["epi"] == 0 and c["act"] == K.ACT["gelu"] for c in cs)
        else:
            assert any(c["epi"] == v for c in cs), n + " has no case"
    assert {c["vt_mode"] for c in cs if c["epi"] == 3} == {0, 1, 2}
    assert max(enums["KG_EPI_QKV_ROPE"], *K.EPI.values()) == 3


@pytest.mark.parametrize("group", K.GROUPS)
def test_emulation_is_within_half_the_bound(group):
    worst = 0.0
    for c in [c for c in K.all_cases() if c["group"] == group]:
        bad, r = K.judge(K.reference(c), K.emulate(c), scale=0.5)
        assert not bad, (c["name"], bad, r)
        worst = max(worst, r)
    print(f"{group}: emulation worst error / bound {worst:.3f}")


def test_every_sabotage_is_caught_by_a_named_case():
    cs = K.all_cases()
    for sab in K.SABOTAGES:
        caught = None
        for c in cs:
            hits = K.differs(c, sab)
            if hits:
                caught = (c["name"], hits)
                break
        print(f"{sab}: {caught}")
        assert caught, sab + " is caught by no case"


def test_host_range_computation_agrees_with_the_reference():
    for c in K.all_cases():
        rows = K.source_rows(c)
        rng = K.host_ranges(c)
        for t, idx in enumerate(rows):
            for s in range(K.nseq_of(c)):
                r = idx[s * c["Lout"]:(s + 1) * c["Lout"]]
                r = r[r >= 0]
                if r.numel():
                    assert rng[(s, t)] == (int(r.min()), int(r.max())), (c["name"], s, t)
                    assert 0 <= int(r.min()) and int(r.max()) < c["src"][c["taps"][t][0]].shape[0], c["name"]
                else:
                    assert (s, t) not in rng, (c["name"], s, t)
        assert c["c_off"] + c["Lout"] <= c["c_seq_rows"] and K.nseq_of(c) * c["c_seq_rows"] <= K.c_rows_of(c)
