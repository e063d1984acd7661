"""The tap-GEMM (csrc/kgemm_tile.h, launched from kgemm.hip and kgemm_big.hip) at op level, through ops.kgemm: ONE kgemm_launch per
call on caller-supplied operands, nothing else between packing and readback.

kgemm_cases.py states the reference, derives the bound and builds the cases; test_host_kgemm.py pins the reference to torch and
the oracle, holds the fp32 emulation to half the bound and shows that every named sabotage leaves the bound.  Held here:
  numeric    EVERY element of every output within the derived bound (fp16 outputs: bound + the format's half step), by mechanism
             group; each case prints its error / bound, each group its worst
  exact      every canary row and canary column holds its fill; so do rows at and above M, rows outside [c_off, c_off + Lout) of
             each sequence and V^T columns at and above Lout; an output that was not requested does not exist for the launch
  relations  bit for bit: a sequence alone, among companions and in another slot; NaN in every source row the row map must not
             read (rows above seq_len, the sequences a_seq_map skips, rows below a_off: the DEFAULT content of the cases' sources)
             against finite values there; NaN in the padded W rows and behind the bias; every tile form against the default;
             c32-only, c16-only and both
  cross      a 3-tap launch against ops.conv1d_cl_ex(force_gemm=True) on the same operands; the V^T of vt_mode 1 and 2 against
             attention_permute_vt (ops.permute_vt) of the mode-0 result, whole buffers
  refusals   every SVC_REQUIRE of kgemm_check and the aid's range checks raise and leave a context whose next launch is right

A device error other than a refusal ends the whole pytest session (pytest.exit, return code 3) from run(): nothing more is launched
on a device that has faulted, so a run that stops there is a FAILED run, not a short pass.
"""
import time

import pytest
import torch

import kgemm_cases as K

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def run(c, **over):
    """one launch -> {output: the WHOLE buffer on the CPU, guards included}"""
    from seedvc_amd import ops
    kw = {k: over.pop(k) for k in ("w_pad",) if k in over}
    try:
        o = ops.kgemm(dict(c, **over), guard=K.GUARD, fill32=K.F32_FILL, fill16=K.F16_FILL, **kw)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "requirement failed" in str(e):
            raise
        pytest.exit(f"{c['name']}: the device reported an error, nothing more is launched: {e}", returncode=3)
    return {k: v.cpu() for k, v in o.items() if k != "guard"}


def untouched(t):
    """bool mask of the elements that still hold their fill"""
    return (t == K.F32_FILL) if t.dtype == torch.float32 else (bits(t) == K.F16_FILL)


def values(c, o, exp):
    """the buffers between the guards as float64, after the exact checks: canary rows, and every element the reference does not
    mark as written (canary columns, rows at and above M, rows outside the window, V^T columns at and above Lout)"""
    G = K.GUARD
    assert set(o) == set(exp), (sorted(o), sorted(exp))
    out = {}
    for name, e in exp.items():
        t = o[name]
        assert bool(untouched(t[:G]).all()) and bool(untouched(t[-G:]).all()), f"{c['name']}: {name}: a canary row was written"
        t = t[G:-G]
        assert t.shape == e["mask"].shape, (name, t.shape, e["mask"].shape)
        if name == "c32" and c.get("c_init") is not None:      # run in place: what the launch does not write keeps its initial value
            kept = bits(t) == bits(c["c_init"])
        else:
            kept = untouched(t)
        assert bool(kept[~e["mask"]].all()), f"{c['name']}: {name}: an element outside the written set was written"
        v = t.double()
        if e["kind"] == "lo":
            v = v + o["c16"][G:-G].double()          # judged on hi + lo
        out[name] = v
    return out


def check(c, **over):
    exp = K.reference(c)
    return K.judge(exp, values(c, run(c, **over), exp))


@pytest.mark.parametrize("group", K.GROUPS)
def test_every_element_within_the_bound(group):
    cases = [c for c in K.all_cases() if c["group"] == group]
    fails, worst, t0 = [], 0.0, time.time()
    for c in cases:
        bad, r = check(c)
        print(f"{c['name']}: error / bound {r:.3f}" + (f"   OUT OF BOUND in {bad}" if bad else ""))
        if bad:
            fails.append((c["name"], bad, round(r, 3)))
        worst = max(worst, r)
    print(f"{group}: {len(cases)} cases, worst error / bound {worst:.3f}, {time.time() - t0:.1f} s")
    assert not fails, fails


def test_activation_function_constants():
    """erff, expm1f and tanhf on an exact pre-activation (W selects one column of A): the function's own error, in the units the
    bound uses.  Printed for DESIGN.md; the constants of kgemm_cases.py are twice the figures first measured."""
    G = K.GUARD
    for name, const in (("gelu", K.K_GELU), ("elu", K.K_EXPM1), ("tanh", K.K_TANH)):
        c = K.case("actonly-" + name)
        got = run(c)["c32"][G:-G, :c["N"]].double()
        v = K.accumulate(c, c["src"])[0]
        ref = K.act_apply(v, torch.zeros_like(v), K.ACT[name], 0.0)[0]
        unit = v.abs() if name == "gelu" else ref.abs()
        live = unit > 0
        k = float(((got - ref).abs()[live] / (K.U * unit[live])).max())
        assert bool((got[~live] == ref[~live]).all())
        print(f"{name}: worst own error {k:.3f} u (constant {const})")
        assert k <= const, (name, k)


# ---------------------------------------------------------------------------------------------------------------- relations
def test_source_rows_outside_the_row_map_are_never_read():
    """the cases' sources hold NaN in every row the map must not read; finite values there change no bit of any buffer"""
    for name in ("ragged-zero", "ragged-reflect", "seqmap-gather", "window", "map-L5-stride2", "map-L13-stride5", "reflect-min-len4", "clamp-len1",
                 "tanhsig-reflect", "map-L64-stride5"):
        c = K.case(name)
        assert any(bool(torch.isnan(t).any()) for t in c["src"]), name
        a, b = run(c), run(c, src=c["src_clean"])
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), (name, k)


def test_padded_weight_rows_and_the_bias_tail_reach_no_output():
    for name in ("tile-M65-N72", "tile-M129-N136", "scalar-N33", "tile-M64-N24", "swiglu-N160-M65", "qkv-D128-L7x3-vt1"):
        c = K.case(name)
        over = dict(w_pad=float("nan"))
        if c.get("bias") is not None:
            over["bias"] = torch.cat([c["bias"], torch.full((16,), float("nan"))])
        a, b = run(c), run(c, **over)
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), (name, k)


def _one_sequence(c, s, slot, nslots):
    """sequence s of case c alone, as sequence `slot` of an nslots-sequence launch whose other sequences read other rows"""
    assert c.get("a_seq_map") is None
    rows = c["a_seq_rows"]
    g = K.gen(99)
    src = []
    for t in c["src_clean"]:
        buf = K.randn(g, nslots * rows, t.shape[1])
        buf[slot * rows:(slot + 1) * rows] = t[s * rows:(s + 1) * rows]
        src.append(buf)
    d = dict(c, src=src, M=nslots * c["Lout"])
    if c.get("seq_len") is not None:
        d["seq_len"] = [c["seq_len"][s] if i == slot else min(3, c["Lout"]) for i in range(nslots)]
    for k in ("rowvec", "gate"):
        if c.get(k) is not None and c[k].dim() == 2:
            buf = K.randn(g, nslots, c["N"])
            buf[slot] = c[k][s]
            d[k] = buf
    assert all(c.get(k) is None for k in ("res", "res2"))
    d.pop("c_rows", None)
    return d


@pytest.mark.parametrize("name", ["ragged-reflect", "map-L13-stride2", "tanhsig-rowvecN", "qkv-D128-L7x3-vt2", "c_off3"])
def test_a_sequence_is_the_same_alone_among_companions_and_in_another_slot(name):
    c = K.case(name)
    G, cs = K.GUARD, c["c_seq_rows"]
    full = run(c, src=c["src_clean"])
    for s, slot, nslots in ((0, 0, 1), (1, 0, 1), (2, 0, 1), (1, 3, 5), (2, 0, 2)):
        one = run(_one_sequence(c, s, slot, nslots))
        for k in full:
            per = c["rope_D"] if k == "vt" else cs
            assert torch.equal(bits(one[k][G + slot * per:G + (slot + 1) * per]), bits(full[k][G + s * per:G + (s + 1) * per])), (name, k, s, slot, nslots)


@pytest.mark.parametrize("group", [g for g in K.GROUPS if g != "actonly"])
def test_every_tile_form_equals_the_default_bit_for_bit(group):
    n = 0
    for c in [c for c in K.all_cases() if c["group"] == group]:
        forms = [f for f in K.forms_of(c) if f != c["form"]]
        if not forms:
            continue
        base = run(c, form=0)
        for f in forms:
            o = run(c, form=f)
            n += 1
            for k in base:
                assert torch.equal(bits(o[k]), bits(base[k])), (c["name"], hex(f), k)
    print(f"{group}: {n} launches under a form override")
    assert n > 0, group + ": no case of the group reaches launch_wide"


@pytest.mark.parametrize("name", ["gelu-c32+c16", "store-" + "+".join(K.ALL_TERMS), "scalar-N33", "act-tanh", "swiglu-sat30"])
def test_one_output_alone_agrees_with_both(name):
    c = K.case(name)
    both = run(c)
    paired = c["epi"] != 0
    for want in ((("want_c16",) if paired else ("want_c32",)), ("want_c16",)):
        o = run(c, want_c32=int("want_c32" in want), want_c16=int("want_c16" in want), want_c16_lo=0)
        assert set(o) == {w[5:] for w in want}
        for k in o:
            assert torch.equal(bits(o[k]), bits(both[k])), (name, k)
    for w in ("gelu-c32", "gelu-c16"):          # the launch picks the GELU instantiation for each output set
        if name == "gelu-c32+c16":
            o = run(K.case(w))
            for k in o:
                assert torch.equal(bits(o[k]), bits(both[k])), (w, k)


# ---------------------------------------------------------------------------------------------------------------- cross
@pytest.mark.parametrize("k,d,Cin,Cout", [(3, 1, 40, 72), (3, 2, 64, 24)])
def test_three_taps_equal_the_conv_entry_point_on_the_tap_gemm(k, d, Cin, Cout):
    from seedvc_amd import ops
    B, L = 2, 37
    left = (k - 1) * d // 2
    c = K.build(f"cross-k{k}-d{d}", "cross", seed=400 + d, nseq=B, Lout=L, N=Cout, K=(Cin,), taps=[(0, t * d - left) for t in range(k)], terms=("bias",))
    exp = K.reference(c)
    got = values(c, run(c), exp)
    bad, r = K.judge(exp, got)
    assert not bad, r
    w = c["W"].reshape(Cout, k, Cin).permute(0, 2, 1).contiguous()
    x = c["src_clean"][0].reshape(B, L, Cin)
    y, _, _, took = ops.conv1d_cl_ex(x.cuda(), w.cuda(), c["bias"].cuda(), dilation=d, pad_left=left, dtype="f16", force_gemm=True)
    assert not took["kconv"]
    y = y.cpu().reshape(B * L, Cout)
    mine = got["c32"][:, :Cout]
    e = exp["c32"]
    assert bool(((y.double() - mine).abs() <= 2 * e["E"][:, :Cout]).all())
    assert torch.equal(bits(y), bits(mine.float())), "same operands, same k order: the two entry points give the same bits"


@pytest.mark.parametrize("name", ["qkv-D128-L70x3", "qkv-D128-L7x3", "qkv-D256-L64x1"])
def test_vt_modes_equal_attention_permute_vt_of_the_natural_order(name):
    """whole buffers, fill columns included: attention_permute_vt (ops.permute_vt) moves the fill inside its groups of 32 as well"""
    from seedvc_amd import ops
    G = K.GUARD
    c0 = K.case(name + "-vt0")
    nat = run(c0)["vt"][G:-G]
    assert bool(untouched(nat[:, c0["Lout"]:]).all())
    for mode in (1, 2):
        o = run(K.case(f"{name}-vt{mode}"), src=c0["src"], W=c0["W"], rope=c0["rope"])["vt"][G:-G]
        perm = ops.permute_vt(nat.cuda(), mode).cpu()
        assert torch.equal(bits(o), bits(perm)), (name, mode)
        cols = torch.tensor([K.vt_pos(p, mode) for p in range(c0["Lout"])])          # and the Python restatement agrees
        assert torch.equal(bits(o[:, cols]), bits(nat[:, :c0["Lout"]])), (name, mode)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusals():
    """every SVC_REQUIRE of kgemm_check (the kgemm_launch section of test_host_kgemm.py's table, as launches), then the aid's range checks"""
    c = K.case("swiglu-N64-M65")
    t = K.case("tanhsig-N64-M65")
    q = K.case("qkv-D128-L5x3-vt1")
    m = K.case("map-L5-stride2")
    g = K.gen(3)
    full = K.randn(g, K.c_rows_of(c), c["ldc"])
    W = lambda n, k=64: K.randn(g, n, k)           # noqa: E731
    unset = "leave them unset"
    return [
        (c, dict(act=1), unset), (t, dict(act=4), unset), (c, dict(gate=K.randn(g, 64)), unset), (c, dict(res=full), unset), (c, dict(res2=full), unset),
        (c, dict(out_scale=0.5), unset), (q, dict(out_scale=2.0), unset), (c, dict(post_relu=1), unset),
        (c, dict(post_a=K.randn(g, 8), post_ib=K.randn(g, 8), post_n=8), unset),
        (c, dict(want_c16=0, want_c32=1), "write c16"), (c, dict(N=40, W=W(40), bias=None), "multiple of 16"), (t, dict(N=72, W=W(72), bias=None, ldc=48), "multiple of 16"),
        (q, dict(bias=torch.zeros(384)), "no bias and no rowvec"), (q, dict(rowvec=torch.zeros(384)), "no bias and no rowvec"), (q, dict(want_c32=1), "no c32 output"),
        (q, dict(N=400, W=W(400)), "N = 3 rope_D"), (q, dict(rope_D=96, N=288, W=W(288)), "N = 3 rope_D"),
        (q, dict(rope=q["rope"][:4]), "rope has a row"), (q, dict(vt_ld=16), "vt_ld a multiple"), (q, dict(vt_mode=3), "vt_mode is 0 .. 2"),
        (m, dict(a_seq_rows=13), "outside its buffer"), (m, dict(a_off=4), "outside its buffer"), (m, dict(src=[m["src"][0][:-2]]), "outside its buffer"),
        (m, dict(a_seq_map=[0, 3, 1]), "outside its buffer"), (m, dict(c_off=1), "output rows"), (m, dict(c_rows=14), "output rows"),
        (m, dict(pad_mode=2, seq_len=[5, 0, 5]), "KG_PAD_CLAMP"), (m, dict(seq_len=[5, -1, 5]), "length is negative"), (m, dict(ldc=28), "multiples of 8"),
        (m, dict(ldc=16), "ldc covers"), (m, dict(form=0x41), "form holds"), (m, dict(dtype=2), "dtype is 0"), (c, dict(dtype=1), "fp32 operands"),
    ]


def test_refusals_raise_and_launch_nothing():
    rows = _refusals()
    for base, over, word in rows:
        with pytest.raises(RuntimeError, match=word):
            run(base, **over)
    c = rows[0][0]
    bad, r = check(c)          # the context is intact and the next launch is right
    assert not bad, r
