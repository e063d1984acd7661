"""CPU side of the AR sampler's op-level suite (test_gpu_ar_sampler.py): the test aid is declared, exported and bound and
refuses bad arguments before anything touches a device; the float64 reference of ar_sampler_cases.py agrees with the oracle
(probabilities, winner, and the generate loop's rules); the case conditions hold; the fp32 emulation of both kernels passes
every check; and every named sabotage of it fails at least one check in a case named for it."""
import ctypes
import os
import re

import pytest
import torch

import ar_sampler_cases as A
import seedvc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
NAN = float("nan")


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
    assert re.search(r"\bsvc_op_ar_sampler\s*\(", header), "svc_op_ar_sampler is not declared in include/seedvc_hip.h"
    assert header.index("op-level entry points") < header.index("svc_op_ar_sampler")
    assert "svc_op_ar_sampler" in _lib.EXPORTS and hasattr(lib, "svc_op_ar_sampler") and hasattr(ops, "ar_sampler")
    assert _fields(header, "svc_ar_sampler_t") == [f[0] for f in _lib.ArSampler._fields_]
    assert "svc_op_ar_sampler" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the contract of svc_ar_sample is written down where its callers read it
    doc = header[header.index("Replaces `sample(logits"):header.index("int svc_ar_sample(")]
    assert "top_p >= 1 removes nothing" in doc and "suppress_token >= vocab is refused" in doc


_I32 = ("s_cnt", "s_done", "s_max_new", "s_min_before_eos", "s_eos", "s_has_noise", "pos")
_F32 = ("s_temperature", "s_top_p", "s_rep_pen")


def _args(base, **kw):
    """a VALID argument set of form `base` with dummy device pointers (never dereferenced: the checks come first), then `kw` over it"""
    from seedvc_amd import _lib
    form, B = base, 3 if base == 2 else 1
    v = dict(form=form, V=17, logits=4096, idx_out=8192, suppress=-1, rep_pen=1.5, temperature=0.7, top_p=0.7, exp_noise=12288)
    if form:
        v.update(D=8, B=B, max_new=8, Lmax=10, toks=16384, noise=20480, emb=24576, next_x=28672, idx_out=None, exp_noise=None,
                 s_cnt=[3] * B, s_done=[0] * B, s_max_new=[8] * B, s_min_before_eos=[2] * B, s_eos=[16] * B, s_has_noise=[1] * B,
                 s_temperature=[0.7] * B, s_top_p=[0.7] * B, s_rep_pen=[1.5] * B, s_seed=[1] * B, pos=[1] * B + [2] * B)
    v.update(kw)
    e, keep = _lib.ArSampler(), []
    for k, x in v.items():
        if x is None:
            continue
        if k in _I32 or k in _F32 or k == "s_seed":
            ct = ctypes.c_int32 if k in _I32 else ctypes.c_float if k in _F32 else ctypes.c_uint64
            keep.append((ct * len(x))(*x))
            setattr(e, k, ctypes.cast(keep[-1], ctypes.POINTER(ct)))
        else:
            setattr(e, k, x)
    return e, keep


REFUSALS = [
    (0, dict(form=3), b"form is 0 .. 2"), (0, dict(form=-1), b"form is 0 .. 2"), (0, dict(V=0), b"V is 1 .. 4096"), (2, dict(V=4097), b"V is 1 .. 4096"),
    (0, dict(logits=None), b"logits"), (1, dict(logits=None), b"logits"), (0, dict(idx_out=None), b"idx_out"),
    (0, dict(n_prev=-1), b"n_prev"), (0, dict(n_prev=3), b"n_prev"), (0, dict(suppress=17), b"suppress"), (0, dict(suppress=4096), b"suppress"),
    (0, dict(rep_pen=NAN), b"rep_pen"), (0, dict(rep_pen=-1.0), b"rep_pen"), (0, dict(step=-1), b"step"),
    (1, dict(s_cnt=[0]), b"cnt >= 1"), (2, dict(s_cnt=[3, 0, 3]), b"cnt >= 1"), (1, dict(s_cnt=[8]), b"cnt < max_new"),
    (2, dict(s_cnt=[3, 9, 3]), b"cnt < max_new"), (2, dict(s_cnt=[3, 8, 3]), b"cnt < max_new"),
    (2, dict(s_cnt=[3, 5, 3], s_max_new=[8, 4, 8], s_done=[0, 1, 0]), b"cnt < max_new"),
    (2, dict(B=0), b"B is 1 .. 64"), (2, dict(B=65), b"B is 1 .. 64"), (1, dict(max_new=0), b"max_new and D"), (2, dict(D=0), b"max_new and D"),
    (2, dict(s_max_new=[8, 0, 8]), b"a slot's max_new"), (2, dict(s_max_new=[8, 9, 8]), b"a slot's max_new"),
    (1, dict(emb=None), b"emb, next_x, toks and pos"), (2, dict(next_x=None), b"emb, next_x, toks and pos"),
    (1, dict(toks=None), b"emb, next_x, toks and pos"), (2, dict(pos=None), b"emb, next_x, toks and pos"),
    (1, dict(s_eos=None), b"per-slot arrays"), (2, dict(s_done=None), b"done, max_new and has_noise"),
    (1, dict(s_eos=[17]), b"eos"), (2, dict(s_eos=[16, -1, 16]), b"eos"), (1, dict(s_rep_pen=[NAN]), b"rep_pen"), (2, dict(s_rep_pen=[1.0, 1.0, -0.5]), b"rep_pen"),
    (2, dict(Lmax=0), b"Lmax"), (2, dict(pos=[1, 10, 1, 2, 2, 2]), b"positions"), (2, dict(pos=[1, 1, 1, 2, 2, -1]), b"positions"),
    (2, dict(noise=None), b"noise buffer"),
]


@pytest.mark.parametrize("form,kw,word", REFUSALS, ids=[f"f{f}," + ",".join(f"{k}={v}" for k, v in kw.items()) for f, kw, _ in REFUSALS])
def test_refusals_need_no_gpu(form, kw, word):
    from seedvc_amd import _lib
    e, keep = _args(form, **kw)
    assert _lib.lib().svc_op_ar_sampler(ctypes.byref(e), None) != 0, kw
    assert word in _lib.lib().svc_last_error(), (kw, _lib.lib().svc_last_error())


# ------------------------------------------------------------------------------------------------ the reference
ORACLE_IDS = ("cut-V17-plain-k5", "cut-V257-plain-k64", "cut-V4093-plain-k1024", "cut-V4096-plain-k4095", "cut-V65-plain-below",
              "pen-V257-rp1.5-n7", "pen-V17-rp1.5-n300", "pen-V4093-rp1.5-n4093", "temp-V1025-T0.05", "temp-V65-T2.0", "ninf-V257-k100")


@pytest.mark.parametrize("cid", ORACLE_IDS)
def test_float64_restatement_agrees_with_the_oracle(cid):
    """top_p < 1 and no ties: the oracle's fp32 evaluation, to fp32 noise, and the same winner"""
    c = A.sample_case_by_id(cid)
    assert A.f32(c["top_p"]) < 1 and c["logits"][torch.isfinite(c["logits"])].unique().numel() == int(torch.isfinite(c["logits"]).sum())
    r = A.ref_sample(c)
    theirs = O.ar_logits_to_probs(c["logits"], torch.tensor(c["prev"]) if c["prev"] else None, None if c["suppress"] is None else [c["suppress"]],
                                  c["T"], c["top_p"], c["rep_pen"])
    assert (theirs.double() - r["p"]).abs().max().item() < 1e-6
    assert torch.equal(theirs > 0, r["p"] > 0)
    assert int(O.ar_sample(theirs, c["q"])) == r["win"]


def _generate_by_the_slot_rules(sd, cfg, prompt_text, prompt_target, exp_noise, T, top_p, rp):
    """seedvc_oracle.ar_generate's loop with the oracle's forward, but sampling by ref_sample and looping by ref_slot_step"""
    V, eos, Lmax = cfg["vocab_size"], cfg["vocab_size"] - 1, cfg["max_seq_len"]
    sep, emb = sd["sep_token_emb"].reshape(1, 1, -1), sd["model.embeddings.weight"]
    tgt = emb[prompt_target[0]][None]
    seq = torch.cat([sep, prompt_text, sep, tgt], dim=1)
    input_pos = torch.cat([torch.arange(prompt_text.size(1) + 1), torch.tensor([0]), torch.arange(tgt.size(1)) + 1])
    kv_pos = torch.arange(seq.size(1))
    caches = O.ar_new_cache(cfg)
    lg = O.ar_forward_generate(sd, cfg, seq, input_pos, kv_pos, caches)[0, -1]
    case = lambda lg, t, prev: A.sample_case("", V, lg, exp_noise[t], prev=prev, suppress=eos if t < 10 else None, rep_pen=rp, T=T, top_p=top_p)   # noqa: E731
    toks = [A.ref_sample(case(lg, 0, []))["win"]] + [0] * 4000
    cnt, ip, kp = 1, int(input_pos[-1]), int(kv_pos[-1])
    done = kp + 1 >= Lmax                     # the host's first step: the same rule as the kernel's tail
    ip, kp = (ip, kp) if done else (ip + 1, kp + 1)
    while not done:
        lg = O.ar_forward_generate(sd, cfg, emb[toks[cnt - 1]].reshape(1, 1, -1), torch.tensor([ip]), torch.tensor([kp]), caches)[0, -1]
        win = A.ref_sample(case(lg, cnt, [toks[0]]))["win"]
        _, toks, cnt, done, ip, kp = A.ref_slot_step(win, toks, cnt, 0, len(toks), eos, ip, kp, Lmax)
    return toks[:cnt]


@pytest.mark.parametrize("how", ["eos", "cache_full"])
def test_slot_rules_agree_with_the_oracles_generate_loop(how):
    """the penalty sees toks[0] only, EOS is suppressed while cnt < 10, EOS ends the loop uncounted, a full cache ends it"""
    from seedvc_amd import specs, weights
    cfg = specs.ar_config(dim=64, n_head=1, n_local_heads=1, n_layer=1, intermediate_size=128, vocab_size=17, max_seq_len=64 if how == "eos" else 24)
    sd = weights.make_state_dict(specs.ar_state_spec(cfg), seed=5, prefix="ar.")
    g = torch.Generator().manual_seed(17)
    text, target = torch.randn(1, 3, 64, generator=g), torch.randint(0, 16, (1, 2), generator=g)
    q = -torch.log(torch.rand(64, 17, generator=g).clamp_min(2.0 ** -24))
    if how == "eos":
        q[:, 16] = 1e-6                       # EOS wins as soon as it is allowed and inside the nucleus
    theirs = O.ar_generate(sd, cfg, text, target, q, 0.7, 0.9, 1.5)[0].tolist()
    mine = _generate_by_the_slot_rules(sd, cfg, text, target, q, 0.7, 0.9, 1.5)
    room = cfg["max_seq_len"] - (3 + 2 + 2) + 1
    assert (10 <= len(theirs) < room) if how == "eos" else len(theirs) == room, (len(theirs), room)
    assert mine == theirs


def test_case_conditions_hold():
    smallest = A.assert_conditions()
    print(f"smallest p_sorted[k] of a planted cut: {smallest:.3e} (condition: >= {A.P_AT_CUT})")
    assert set(c["V"] for c in A.sample_cases()) == set(A.VS)
    ks = set(c.get("planted_k") for c in A.sample_cases() if c["id"].startswith("cut-V4096-"))
    assert set(A.KS) | {4095} <= ks


# ------------------------------------------------------------------------------------------------ emulation and sabotages
def test_emulation_passes_every_check():
    worst = 0.0
    for c in A.sample_cases():
        idx, p = A.emu_sample(c)
        fails, ratio = A.check_sample(c, A.ref_sample(c), idx, p)
        assert not fails, (c["id"], fails)
        worst = max(worst, ratio)
    for c in A.loop1_cases():
        fails, ratio = A.check_loop1(c, A.ref_loop1(c), A.emu_loop1(c))
        assert not fails, (c["id"], fails)
        worst = max(worst, ratio)
    for c in A.slots_cases():
        fails = A.check_slots(c, A.ref_slots(c), A.emu_slots(c))
        assert not fails, (c["id"], fails)
    print(f"fp32 emulation: worst error / bound of the kept probabilities {worst:.3f}")
    assert worst <= 0.5


SABOTAGES = sorted(A.SAMPLE_SABOTAGES) + sorted(A.LOOP_SABOTAGES)


@pytest.mark.parametrize("name", SABOTAGES)
def test_every_sabotage_fails_in_the_cases_named_for_it(name):
    if name in A.SAMPLE_SABOTAGES:
        for cid in A.SAMPLE_SABOTAGES[name]:
            c = A.sample_case_by_id(cid)
            idx, p = A.emu_sample(c, name)
            assert A.check_sample(c, A.ref_sample(c), idx, p)[0], (name, cid)
        return
    loop1_ids, slot_targets = A.LOOP_SABOTAGES[name]
    for cid in loop1_ids:
        c = next(c for c in A.loop1_cases() if c["id"] == cid)
        assert A.check_loop1(c, A.ref_loop1(c), A.emu_loop1(c, name))[0], (name, cid)
    for cid, kind in slot_targets:
        c = next(c for c in A.slots_cases() if c["id"] == cid)
        fails = A.check_slots(c, A.ref_slots(c), A.emu_slots(c, name))
        hit = [b for b in fails if (b is None if kind is None else b is not None and c["kind"][b] == kind)]
        assert hit, (name, cid, kind, fails)


def test_the_sabotages_tested_are_the_sabotages_defined():
    import inspect
    src = inspect.getsource(A.emu_sample) + inspect.getsource(A.emu_slots) + inspect.getsource(A.loop1_sample) + inspect.getsource(A.slot_sample)
    used = set(re.findall(r'sab [!=]= "([a-z_0-9]+)"', src))
    assert used == set(SABOTAGES) and len(SABOTAGES) == 17
    assert not set(A.SAMPLE_SABOTAGES) & set(A.LOOP_SABOTAGES)
