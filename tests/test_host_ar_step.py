"""CPU side of the AR step kernels' op-level suite (test_gpu_ar_step.py): the two test aids are declared, exported and bound and
refuse bad arguments before anything touches a device; the float64 references of ar_step_cases.py, composed into whole layers,
reproduce the oracle's forward_generate (prefill + 3 steps, one through each path); the cases cover the seams the kernels are built
around; the reference is finite on every case; the fp32 emulation stays under HALF the bound on every element of every case;
and every named sabotage of the reference is caught by every case named for it."""
import ctypes
import os
import re

import pytest
import torch

import ar_step_cases as A
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
    for fn, st, cls, wrap in (("svc_op_ar_attn", "svc_ar_attn_t", _lib.ArAttn, "ar_attn"), ("svc_op_ar_linear", "svc_ar_linear_t", _lib.ArLinear, "ar_linear")):
        assert re.search(r"\b" + fn + r"\s*\(", header), fn + " is not declared in include/seedvc_hip.h"
        assert header.index("op-level entry points") < header.index(fn)
        assert fn in _lib.EXPORTS and hasattr(lib, fn) and hasattr(ops, wrap)
        assert _fields(header, st) == [f[0] for f in cls._fields_]
        assert fn in doc


P = 4096          # dummy device pointers (never dereferenced: the checks come first)
_HOST = ("slots", "seq_S", "pos")


def _fill(e, v):
    keep = []
    for k, x in v.items():
        if x is None:
            continue
        if k in _HOST:
            keep.append((ctypes.c_int32 * len(x))(*x))
            setattr(e, k, ctypes.cast(keep[-1], ctypes.POINTER(ctypes.c_int32)))
        else:
            setattr(e, k, x)
    return e, keep


def _attn_args(base, **kw):
    """a VALID argument set of `kind`, then `kw` over it"""
    from seedvc_amd import _lib
    kind = base
    v = dict(kind=kind, H=4, Hkv=2, Lmax=16, n_slots=3, n=2, x=P, ldq=512, kc=P, vc=P, rope=P, slots=[2, 0], seq_S=[3, 2],
             pos=[1, 2, 3, 4, 5] * 2 if kind in (3, 5) else [1, 2, 3, 4], y16=P, q_out=P, hres=P, eps=1e-5, wo=P, part=P)
    v.update(kw)
    return _fill(_lib.ArAttn(), v)


ATTN_REFUSALS = [
    (0, dict(kind=6), b"kind is 0 .. 5"), (0, dict(kind=-1), b"kind is 0 .. 5"), (2, dict(Hkv=3), b"H % Hkv"), (1, dict(H=0), b"H is 1 .. 64"),
    (0, dict(Lmax=7), b"Lmax is 8 .. 8192"), (3, dict(Lmax=8193), b"Lmax is 8 .. 8192"), (2, dict(n_slots=0), b"n_slots"), (2, dict(n_slots=65), b"n_slots"),
    (0, dict(x=None), b"are required"), (1, dict(kc=None), b"are required"), (2, dict(vc=None), b"are required"), (3, dict(slots=None), b"are required"),
    (4, dict(pos=None), b"are required"), (0, dict(n=0), b"n is 1"), (2, dict(n=65, slots=list(range(3)) * 21 + [0, 1]), b"n is 1"),
    (0, dict(slots=[3]), b"slot lies in"), (2, dict(slots=[2, -1]), b"slot lies in"), (2, dict(slots=[1, 1]), b"named twice"),
    (3, dict(slots=[2, 2]), b"named twice"), (5, dict(slots=[0, 0]), b"named twice"), (3, dict(seq_S=None), b"seq_S"), (3, dict(seq_S=[3, 0]), b"S[i]"),
    (5, dict(seq_S=[-1, 2]), b"S[i]"), (0, dict(pos=[1, 16, 3, 4]), b"positions"), (1, dict(pos=[1, -1]), b"positions"), (2, dict(pos=[1, 2, 3, 16]), b"positions"),
    (3, dict(pos=[1, 2, 3, 4, 5, 1, 2, 3, 4, 16]), b"positions"), (4, dict(pos=[-1, 2, 3, 4]), b"positions"), (0, dict(y16=None), b"y16"),
    (3, dict(y16=None), b"y16"), (1, dict(rope=None), b"rope"), (5, dict(rope=None), b"rope"), (4, dict(q_out=None), b"q_out"), (4, dict(ldq=511), b"q_out"),
    (1, dict(hres=None), b"hres, wo and part"), (1, dict(part=None), b"hres, wo and part"), (1, dict(H=17, Hkv=1), b"D <= 1024"),
]


def _ids(rows):
    return [f"{a}," + ",".join(f"{k}={'list' if isinstance(v, list) and len(v) > 6 else v}" for k, v in kw.items()) for a, kw, _ in rows]


@pytest.mark.parametrize("kind,kw,word", ATTN_REFUSALS, ids=_ids(ATTN_REFUSALS))
def test_attn_refusals_need_no_gpu(kind, kw, word):
    from seedvc_amd import _lib
    e, keep = _attn_args(kind, **kw)
    assert _lib.lib().svc_op_ar_attn(ctypes.byref(e), None) != 0, kw
    assert word in _lib.lib().svc_last_error(), (kw, _lib.lib().svc_last_error())


def _linear_args(base_path, base_role, **kw):
    from seedvc_amd import _lib
    v = dict(path=base_path, role=A.NAMES.index(base_role), D=128, I=256, H=2, Hkv=1, V=65, Lmax=16, rows=3, n_slots=4, x=P, gamma=P, eps=1e-5, W=P, W2=P, res=P,
             part=P, out32=P, out16=P, out2=P, q_out=P, kc=P, vc=P, rope=P, slots=[3, 1, 0], pos=[1, 2, 3, 4, 5, 6])
    v.update(kw)
    return _fill(_lib.ArLinear(), v)


LINEAR_REFUSALS = [
    (0, "qkv", dict(path=3), b"path is 0 .. 2"), (0, "qkv", dict(role=5), b"role is 0 .. 4"), (1, "wo", dict(role=-1), b"role is 0 .. 4"),
    (1, "qkv", dict(H=3, D=192, Hkv=2), b"H % Hkv"), (0, "w13", dict(D=96), b"multiples of 64"), (1, "w2", dict(I=100), b"multiples of 64"),
    (2, "w13", dict(I=0), b"multiples of 64"), (0, "head", dict(H=3), b"D == 64 H"), (0, "head", dict(V=0), b"V is 1 .. 4096"),
    (1, "head", dict(V=4097), b"V is 1 .. 4096"), (0, "wo", dict(rows=0), b"S = 1 .. 8"), (0, "qkv", dict(rows=9, pos=[1] * 18), b"S = 1 .. 8"),
    (1, "w13", dict(rows=0), b"B = 1 .. 64"), (1, "head", dict(rows=65), b"B = 1 .. 64"),
    # the shapes for which svc_ar_create clears the decode step
    (2, "w13", dict(I=2624), b"path 2 holds"), (2, "w2", dict(I=2624), b"path 2 holds"), (2, "qkv", dict(D=1088, H=17), b"path 2 holds"),
    (0, "w2", dict(x=None), b"x and W"), (2, "head", dict(W=None), b"x and W"), (0, "w13", dict(gamma=None), b"gamma"), (1, "head", dict(gamma=None), b"gamma"),
    (0, "wo", dict(res=None), b"need res"), (2, "w2", dict(res=None), b"need res"), (1, "w13", dict(out16=None), b"out16"), (0, "head", dict(out32=None), b"out32"),
    (2, "wo", dict(W2=None), b"W2 and out2"), (2, "wo", dict(out2=None), b"W2 and out2"), (2, "w13", dict(part=None), b"part and out2"),
    (0, "qkv", dict(q_out=None), b"the qkv role needs"), (1, "qkv", dict(rope=None), b"the qkv role needs"), (1, "qkv", dict(slots=None), b"the qkv role needs"),
    (0, "qkv", dict(Lmax=7), b"Lmax is 8 .. 8192"), (1, "qkv", dict(Lmax=8193), b"Lmax is 8 .. 8192"), (1, "qkv", dict(n_slots=65), b"n_slots"),
    (0, "qkv", dict(slots=[4]), b"slot lies in"), (1, "qkv", dict(slots=[3, 1, 1]), b"named twice"), (1, "qkv", dict(slots=[3, -1, 0]), b"slot lies in"),
    (0, "qkv", dict(pos=[1, 2, 16, 4, 5, 6]), b"positions"), (1, "qkv", dict(pos=[1, 2, 3, 4, 5, -1]), b"positions"),
]


@pytest.mark.parametrize("path,role,kw,word", LINEAR_REFUSALS, ids=[f"p{p}-{r}," + ",".join(f"{k}={v}" for k, v in kw.items()) for p, r, kw, _ in LINEAR_REFUSALS])
def test_linear_refusals_need_no_gpu(path, role, kw, word):
    from seedvc_amd import _lib
    e, keep = _linear_args(path, role, **kw)
    assert _lib.lib().svc_op_ar_linear(ctypes.byref(e), None) != 0, kw
    assert word in _lib.lib().svc_last_error(), (kw, _lib.lib().svc_last_error())


def test_null_arguments_are_refused():
    from seedvc_amd import _lib
    assert _lib.lib().svc_op_ar_attn(None, None) != 0 and b"null" in _lib.lib().svc_last_error()
    assert _lib.lib().svc_op_ar_linear(None, None) != 0 and b"null" in _lib.lib().svc_last_error()


# ------------------------------------------------------------------------------------------------ the reference against the oracle
def _model():
    from seedvc_amd import specs, weights
    cfg = specs.ar_config(dim=192, n_head=3, n_local_heads=1, n_layer=2, intermediate_size=320, vocab_size=65, max_seq_len=32)
    sd = {k: v.half().float() if v.dim() == 2 else v for k, v in weights.make_state_dict(specs.ar_state_spec(cfg), seed=5, prefix="ar.").items()}
    return cfg, sd          # matrices exactly representable in fp16: the references and the oracle see the same weights


def _layers(cfg, sd):
    I = cfg["intermediate_size"]
    out = []
    for i in range(cfg["n_layer"]):
        p = f"model.layers.{i}."
        w13 = torch.stack([sd[p + "feed_forward.w1.weight"], sd[p + "feed_forward.w3.weight"]], 1).reshape(2 * I, -1)       # (w1_j, w3_j) interleaved
        out.append(dict(wqkv=sd[p + "attention.wqkv.weight"], wo=sd[p + "attention.wo.weight"], w13=w13, w2=sd[p + "feed_forward.w2.weight"],
                        g_attn=sd[p + "attention_norm.weight"], g_ffn=sd[p + "ffn_norm.weight"]))
    return out


def _forward_rows(cfg, sd, path, attn_kind, x, ip, kp, kc, vc, rope):
    """rows through every layer on the references of `path` (0 gemv_pair | 1 bgemm) and attention `attn_kind`; caches (L, 1, Hkv, Lmax, 64)"""
    D, I, H, Hkv = cfg["dim"], cfg["intermediate_size"], cfg["n_head"], cfg["n_local_heads"]
    base = dict(path=path, D=D, I=I, H=H, Hkv=Hkv, V=cfg["vocab_size"], eps=cfg["norm_eps"], rope=rope, pos=[ip, kp])
    h = x.double()
    for i, ly in enumerate(_layers(cfg, sd)):
        rows = A.ref_linear(dict(base, role="qkv", x=h, W=ly["wqkv"], gamma=ly["g_attn"]))["rows"]
        for r in rows:
            kc[i][0, :, r["row"]], vc[i][0, :, r["row"]] = r["k"].reshape(Hkv, 64), r["v"].reshape(Hkv, 64)
        y = torch.stack([torch.cat([hd["y"] for hd in A.ref_attn_row(r["q"], kc[i][0], vc[i][0], kp[s], H, Hkv)]) for s, r in enumerate(rows)])
        h = A.ref_linear(dict(base, role="wo", x=y, W=ly["wo"], res=h))["out"]
        ff = A.ref_linear(dict(base, role="w13", x=h, W=ly["w13"], gamma=ly["g_ffn"]))["out"]
        h = A.ref_linear(dict(base, role="w2", x=ff, W=ly["w2"], res=h))["out"]
    return A.ref_linear(dict(base, role="head", x=h[-1:], W=sd["model.output.weight"], gamma=sd["model.norm.weight"]))["out"][0]


def _forward_dec(cfg, sd, x, ip, kp, kc, vc, rope):
    """one row through the references of the B = 1 decode step, on weights composed in float64 as svc_ar_create composes them"""
    D, I, H, Hkv = cfg["dim"], cfg["intermediate_size"], cfg["n_head"], cfg["n_local_heads"]
    base = dict(path=2, D=D, I=I, H=H, Hkv=Hkv, V=cfg["vocab_size"], eps=cfg["norm_eps"])
    L = _layers(cfg, sd)
    h, h_mid, ff = x.double()[None], None, None
    for i, ly in enumerate(L):
        wq = ly["wqkv"].double() * ly["g_attn"].double()[None]                       # Wq' = wqkv diag(gamma)
        if i == 0:
            qkv_raw = A.ref_linear(dict(base, role="qkv", x=h, W=wq))["out"]
        else:
            r = A.ref_linear(dict(base, role="wo", x=ff, res=h_mid, W2=L[i - 1]["w2"], W=torch.cat([wq @ L[i - 1]["w2"].double(), wq], 1)))
            h, qkv_raw = r["out"], r["out2"]
        a = A.ref_dec_attn2(dict(H=H, Hkv=Hkv, pos=[[ip], [kp]], x=qkv_raw, hres=h[0], eps=cfg["norm_eps"], rope=rope, kc=kc[i], vc=vc[i], slots=[0],
                                 wo=ly["wo"]), sab="y_not_rounded")          # the fp16 rounding of y is the kernel's own deviation: pinned without it
        kc[i][0, :, a["row"]], vc[i][0, :, a["row"]] = a["k"].reshape(Hkv, 64), a["v"].reshape(Hkv, 64)
        r = A.ref_linear(dict(base, role="w13", x=h, part=a["part"], W=ly["w13"], gamma=ly["g_ffn"]))
        ff, h_mid = r["out"], r["out2"]
    h = A.ref_linear(dict(base, role="w2", x=ff, res=h_mid, W=L[-1]["w2"]))["out"]
    return A.ref_linear(dict(base, role="head", x=h, W=sd["model.output.weight"], gamma=sd["model.norm.weight"]))["out"][0]


def test_references_composed_into_layers_reproduce_the_oracle():
    """prefill of 5 rows (gemv_pair references, ar_attn), then three steps: the decode step's references, the batched ones, and the
    gemv_pair ones again -- against oracle.ar_forward_generate, 5e-5 max abs on the logits"""
    cfg, sd = _model()
    g = A.gen(11)
    S, Lmax = 5, cfg["max_seq_len"]
    rope = O.rope_table(Lmax, 64, cfg["rope_base"], bf16_round=True)
    caches = O.ar_new_cache(cfg)
    kc = [torch.zeros(1, cfg["n_local_heads"], Lmax, 64, dtype=torch.float64) for _ in range(cfg["n_layer"])]
    vc = [torch.zeros_like(k) for k in kc]
    xs = [A.randn(g, S, cfg["dim"])] + [A.randn(g, 1, cfg["dim"]) for _ in range(3)]
    pos = [list(range(S))] + [[S + t] for t in range(3)]
    worst = 0.0
    for t, (x, p) in enumerate(zip(xs, pos)):
        want = O.ar_forward_generate(sd, cfg, x[None], torch.tensor(p), torch.tensor(p), caches)[0, 0].double()
        if t == 1:
            got = _forward_dec(cfg, sd, x[0], p[0], p[0], kc, vc, rope)
        else:
            got = _forward_rows(cfg, sd, 1 if t == 2 else 0, 2 if t == 2 else 0, x, p, p, kc, vc, rope)
        d = float((got - want).abs().max())
        print(f"call {t} ({'prefill' if t == 0 else 'step'}): max |reference - oracle| on the logits {d:.2e}")
        worst = max(worst, d)
    assert worst <= 5e-5, worst


# ------------------------------------------------------------------------------------------------ the cases
def test_cases_cover_the_seams():
    cs = A.all_cases()
    kind = lambda k: [c for c in cs if c.get("kind") == k]          # noqa: E731
    heads = lambda k: {(c["H"], c["Hkv"]) for c in kind(k)}          # noqa: E731
    for k in (0, 1, 2):
        assert heads(k) >= set(A.HEADS), k
    assert heads(3) >= set(A.HEADS_PREFILL)
    assert {c["pos"][1][0] for c in kind(1)} >= {0, 1, 7, 63, 255, 256, 257, 511, 512, 513, 767, 768, 1023, 1024, 1029, 4095, 8191}
    assert {c["Lmax"] for c in kind(1)} >= {8, 1030, 4096, 8192} and all(c["pos"][0][0] != c["pos"][1][0] for c in kind(1))
    assert {len(c["slots"]) for c in kind(2)} >= {1, 16, 17, 33, 64} and {c["Lmax"] for c in kind(2)} >= {8, 1030, 8192}
    assert {k for c in kind(2) for k in c["pos"][1]} >= {0, 31, 32, 510, 511, 512, 513, 1023, 1024, 1025, 1029, 8191, 7}
    assert {len(c["pos"][1]) for c in kind(0)} >= {1, 3, 8, 17} and {c["Lmax"] for c in kind(0)} >= {8, 2050, 8192}
    assert {k for c in kind(0) for k in c["pos"][1]} >= {0, 15, 16, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 7}
    assert {S for c in kind(3) for S in c["seq_S"]} >= {1, 15, 16, 17, 33, 64}
    tile_max = {k0 + min(S, s0 + 16) - 1 for c in kind(3) for k0, S in zip([c["pos"][1][sum(c["seq_S"][:i])] for i in range(len(c["seq_S"]))], c["seq_S"])
                for s0 in range(0, S, 16)}
    assert tile_max >= {0, 30, 31, 32, 33, 63, 64}, sorted(tile_max)
    assert all(c["slots"] == sorted(c["slots"], reverse=True) and len(set(c["slots"])) == len(c["slots"]) for c in kind(3) + kind(5))
    lin = [c for c in cs if "path" in c]
    for p in (0, 1, 2):
        assert {(c["D"], c["I"]) for c in lin if c["path"] == p} >= set(A.SIZES), p
        assert {c["role"] for c in lin if c["path"] == p} == set(A.NAMES)
    assert {c["V"] for c in lin if c["role"] == "head"} >= {17, 33, 65, 1024, 4093}
    assert {c["rows"] for c in lin if c["path"] == 0} >= {1, 5, 8} and {c["rows"] for c in lin if c["path"] == 1} >= {1, 16, 17, 48, 49, 64}
    assert any(c["I"] == 2624 and c["path"] == 0 for c in lin) and any(c.get("inplace") for c in lin)
    # every cache row holds finite non-zero values, so a read of a wrong row shows
    for c in cs:
        if "kc" in c:
            assert bool(torch.isfinite(c["kc"]).all()) and bool((c["kc"] != 0).all()) and bool((c["vc"] != 0).all()), c["name"]
    # writers: first, last and mid-cache rows, and two rows of one call into adjacent cache rows
    for c in kind(4):
        kp = c["pos"][1]
        assert any(b - a == 1 for a, b in zip(kp, kp[1:])), c["name"]
    assert {k for c in kind(4) for k in c["pos"][1]} >= {0, 7, 1029, 500, 8191}


KERNELS = sorted({A.kernel_of(c) for c in A.all_cases()})


@pytest.mark.parametrize("kernel", KERNELS)
def test_reference_is_finite_and_the_emulation_stays_under_half_the_bound(kernel):
    worst = 0.0
    cases = [c for c in A.all_cases() if A.kernel_of(c) == kernel]
    for c in cases:
        for name, ref, E, half in A.expected(c):
            assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(E).all()) and bool((E >= 0).all()), (c["name"], name)
        bad, r = A.compare(c, A.emulated(c))
        assert not bad, (c["name"], bad)
        worst = max(worst, r)
    print(f"{kernel}: {len(cases)} cases, emulation worst error / bound {worst:.3f}")
    assert worst <= 0.5, worst


@pytest.mark.parametrize("name", sorted(A.SABOTAGES))
def test_every_sabotage_is_caught_by_its_cases(name):
    """the emulation stands in for the kernel: it passes against the true reference (test above) and fails against the sabotaged one
    in EVERY case named for the sabotage"""
    cases = [c for c in A.all_cases() if A.SABOTAGES[name](c)]
    assert len(cases) >= 3, name
    missed = [c["name"] for c in cases if not A.compare(c, A.emulated(c), sab=name)[0]]
    print(f"{name}: caught in {len(cases) - len(missed)} of {len(cases)} cases")
    assert not missed, missed
