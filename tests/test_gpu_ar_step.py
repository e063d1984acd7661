"""The AR step kernels at op level: ar_attn, dec_attn2, battn, ar_prefill_attn, the two RoPE / cache writers (ops.ar_attn, kinds
0 .. 5) and the skinny linears gemv_pair, bgemm and dec_* in their five roles (ops.ar_linear, paths 0 .. 2) -- ONE call of the
model's launch function per call, in the template instance the model selects.

ar_step_cases.py states the reference, derives the bound and builds the cases; test_host_ar_step.py pins the reference to the
oracle, holds the fp32 emulation to half the bound and shows that each check catches the sabotage it is for.  Held here:
  exact      every canary row; every cache element other than the written rows (whole buffers, bit for bit); the written rows at
             (slot, kv head, kv_pos); the rows of q_out and y16 at and beyond nb still hold their fill; part is written for all
             H x D entries and nowhere else
  numeric    EVERY element of every output and every written cache element within the derived bound (fp16 outputs: bound + the
             format's half step); each test prints its worst error / bound
  relations  bit for bit, as the code comments promise: a slot alone, at another row of B = 17 and B = 64 among other neighbours,
             and with NaN in the padding rows (battn, bgemm in all roles); NaN in every cache row above the prefix (ar_attn, battn,
             ar_prefill_attn); a prefill row alone in its tile or followed by 15 later rows; dec_attn2 whatever the cache row
             kv_pos held and with 1e30 in the rows above; heads that share a KV head and are given the same q
  cross      the four attention kernels on the same q, cache and position within the sum of their bounds; the qkv role of path
             0, of path 1 and ar_rope_cache on the same input
"""
import pytest
import torch

import ar_step_cases as A

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

WORST = {}          # kernel -> largest error / bound seen so far in this run


def note(kernel, ratio):
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def body(o, name, rows=None):
    """the rows between the guards of a returned buffer, on the CPU, after the canary check"""
    t, G = o[name].cpu(), o["guard"]
    fill = A.F16_FILL if t.dtype == torch.float16 else A.F32_FILL
    assert bool((t[:G] == fill).all()) and bool((t[-G:] == fill).all()), f"{name}: a canary row was written"
    t = t[G:-G]
    if rows is not None:            # the rows at and beyond the live ones still hold their fill
        assert bool((t[rows:] == fill).all()), f"{name}: a padding row was written"
        t = t[:rows]
    return t


def call(c, **over):
    """one launch for the case -> the buffers in the order of A.expected(c), plus the untouched-cache check where the kernel only
    reads the caches"""
    from seedvc_amd import ops
    a = dict(c, **over)
    if "path" in c:
        o = ops.ar_linear(a, guard=A.GUARD, fill32=A.F32_FILL, fill16=A.F16_FILL)
        live = c["rows"] if c["path"] != 2 else 1
        if c["role"] == "qkv" and c["path"] != 2:
            return [body(o, "q_out", live), body(o, "kc").reshape(c["kc"].shape), body(o, "vc").reshape(c["vc"].shape)]
        # the batched PLAIN and GLU epilogues write the padding rows of their output too (finite or not): only the live rows count
        name = "out16" if c["role"] == "w13" else "out32"
        out = [body(o, name)[:live]]
        if "out2" in o:
            out.append(body(o, "out2"))
        return out
    o = ops.ar_attn(a, guard=A.GUARD, fill32=A.F32_FILL, fill16=A.F16_FILL)
    kc, vc = body(o, "kc").reshape(c["kc"].shape), body(o, "vc").reshape(c["vc"].shape)
    kind = c["kind"]
    if kind in (0, 2, 3):
        assert torch.equal(bits(kc), bits(a["kc"])) and torch.equal(bits(vc), bits(a["vc"])), "an attention kernel wrote the cache"
        return [body(o, "y16", len(c["pos"][1]))]
    return [body(o, "part" if kind == 1 else "q_out"), kc, vc]


KERNELS = sorted({A.kernel_of(c) for c in A.all_cases()})


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_element_within_the_bound(kernel):
    cases = [c for c in A.all_cases() if A.kernel_of(c) == kernel]
    fails, worst = [], 0.0
    for c in cases:
        bad, r = A.compare(c, call(c))
        print(f"{c['name']}: error / bound {r:.3f}" + (f"   OUT OF BOUND in {bad}" if bad else ""))
        if bad:
            fails.append((c["name"], bad, round(r, 3)))
        worst = max(worst, r)
    note(kernel, worst)
    print(f"{kernel}: {len(cases)} cases, worst error / bound {worst:.3f}")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------- relations
def battn_single(c, b):
    """slot b of a battn case as a B = 1 call on the same caches"""
    return dict(c, x=c["x"][b:b + 1], slots=[c["slots"][b]], pos=[[c["pos"][0][b]], [c["pos"][1][b]]])


def test_battn_slot_is_the_same_alone_in_a_batch_and_beside_nan():
    c = A.case("k2-H12x2-L1030-kp512_513_1023+14")          # B = 17
    B = len(c["slots"])
    full = call(c)[0]
    assert torch.equal(bits(full), bits(call(c, pad=0.0)[0]))          # padding rows of q: NaN (default) or zeros
    for b in (0, 7, 16):
        assert torch.equal(bits(call(battn_single(c, b))[0][0]), bits(full[b])), b
    # the same slots at other rows of a B = 64 batch among different neighbours (the other rows reuse the caches of the 17)
    g = A.gen(77)
    perm = [int(v) for v in torch.randperm(B, generator=g)]
    kc = torch.cat([c["kc"], A.caches(g, 64 - B, c["Hkv"], c["Lmax"])[0]])
    vc = torch.cat([c["vc"], A.caches(g, 64 - B, c["Hkv"], c["Lmax"])[1]])
    rows = [63 - 3 * i for i in range(B)]
    x = A.randn(g, 64, 64 * c["H"], scale=0.35)
    slots, ip, kp = [None] * 64, [3] * 64, [int(v) for v in torch.randint(0, c["Lmax"], (64,), generator=g)]
    free = list(range(B, 64))
    for i, r in enumerate(rows):
        slots[r], ip[r], kp[r] = c["slots"][perm[i]], c["pos"][0][perm[i]], c["pos"][1][perm[i]]
        x[r] = c["x"][perm[i]]
    for r in range(64):
        if slots[r] is None:
            slots[r] = free.pop()
    big = call(dict(c, x=x, kc=kc, vc=vc, slots=slots, pos=[ip, kp]))[0]
    for i, r in enumerate(rows):
        assert torch.equal(bits(big[r]), bits(full[perm[i]])), (r, perm[i])


@pytest.mark.parametrize("role", A.NAMES)
def test_bgemm_slot_is_the_same_alone_in_a_batch_and_beside_nan(role):
    c = A.linear_case(1, role, 192, 320, 65, 17, 900 + A.NAMES.index(role), inplace=role in ("wo", "w2"))
    full = call(c)
    zero = call(c, pad=0.0)
    for a, b in zip(full, zero):
        assert torch.equal(bits(a), bits(b)), "a padding row of the input reached a live row"
    for b in (0, 9, 16):
        one = dict(c, x=c["x"][b:b + 1], rows=1)
        if "res" in c:
            one["res"] = c["res"][b:b + 1]
        if role == "qkv":
            one.update(slots=[c["slots"][b]], pos=[[c["pos"][0][b]], [c["pos"][1][b]]])
        got = call(one)
        assert torch.equal(bits(got[0][0]), bits(full[0][b])), (role, b)
        if role == "qkv":      # its cache row, bit for bit
            sl, kp = c["slots"][b], c["pos"][1][b]
            assert torch.equal(bits(got[1][sl, :, kp]), bits(full[1][sl, :, kp])) and torch.equal(bits(got[2][sl, :, kp]), bits(full[2][sl, :, kp]))
    # the same rows at other row indices of B = 64 among different neighbours
    big = A.linear_case(1, role, 192, 320, 65, 64, 950 + A.NAMES.index(role), inplace=role in ("wo", "w2"))
    big["W"] = c["W"]
    if "gamma" in c:
        big["gamma"] = c["gamma"]
    rows = [63 - 3 * i for i in range(17)]
    for i, r in enumerate(rows):
        big["x"][r] = c["x"][i]
        if "res" in c:
            big["res"][r] = c["res"][i]
        if role == "qkv":
            big["pos"][0][r], big["pos"][1][r] = c["pos"][0][i], c["pos"][1][i]
    if role == "qkv":
        big["rope"] = c["rope"]
    got = call(big)
    for i, r in enumerate(rows):
        assert torch.equal(bits(got[0][r]), bits(full[0][i])), (role, r)
        if role == "qkv":
            kp = c["pos"][1][i]
            assert torch.equal(bits(got[1][big["slots"][r], :, kp]), bits(full[1][c["slots"][i], :, kp]))
            assert torch.equal(bits(got[2][big["slots"][r], :, kp]), bits(full[2][c["slots"][i], :, kp]))


def nan_above(c, top_of_slot):
    kc, vc = c["kc"].clone(), c["vc"].clone()
    for sl, top in top_of_slot.items():
        kc[sl, :, top + 1:] = float("nan")
        vc[sl, :, top + 1:] = float("nan")
    return kc, vc


@pytest.mark.parametrize("name", ["k0-H4x1-L2050-kp1022_1023_1024+5", "k0-H2x1-L8-kp0_3_7", "k2-H5x1-L1030-kp510_511_512+30", "k2-H6x2-L8192-kp8191_1023_1024",
                                  "k2-H1x1-L8-kp0", "k3-H12x2-L128-kp32_31_63", "k3-H3x1-L128-kp0_40", "k3-H14x2-L128-kp16_1"])
def test_nan_above_the_prefix_changes_no_bit(name):
    """ar_attn, battn: no row above a slot's largest kv_pos is addressed; ar_prefill_attn: none above the sequence's last row"""
    c = A.case(name)
    top = {}
    for r, kp in enumerate(c["pos"][1]):
        sl = A.row_slot(c, r)
        top[sl] = max(top.get(sl, -1), kp)
    clean = call(c)[0]
    kc, vc = nan_above(c, top)
    # slots that no row names are NaN altogether
    for sl in range(c["kc"].shape[0]):
        if sl not in top:
            kc[sl], vc[sl] = float("nan"), float("nan")
    dirty = call(c, kc=kc, vc=vc)[0]
    assert bool(torch.isfinite(dirty.float()).all())
    assert torch.equal(bits(clean), bits(dirty))


def test_prefill_row_is_the_same_alone_in_its_tile_or_followed_by_15_rows():
    c = A.attn_case(3, 12, 2, 128, [31], 960, seq_S=[16])
    full = call(c)[0]
    for n in (1, 2, 15):
        part = call(dict(c, x=c["x"][:n], seq_S=[n], pos=[c["pos"][0][:n], c["pos"][1][:n]]))[0]
        assert torch.equal(bits(part), bits(full[:n])), n


@pytest.mark.parametrize("name", ["k1-H12x2-L1030-kp700-late", "k1-H9x3-L1030-kp257", "k1-H2x1-L8-kp0", "k1-H2x1-L1030-kp1029", "k1-H16x4-L1030-kp512"])
def test_dec_attn2_ignores_the_cache_row_kv_pos_and_finite_rows_above(name):
    c = A.case(name)
    kp, sl = c["pos"][1][0], c["slots"][0]
    clean = call(c)
    kc, vc = c["kc"].clone(), c["vc"].clone()
    kc[sl, :, kp], vc[sl, :, kp] = 123.5, -77.0          # whatever finite values the row held
    kc[sl, :, kp + 1:], vc[sl, :, kp + 1:] = 1e30, -1e30      # large finite values above (NaN there is outside the contract)
    dirty = call(c, kc=kc, vc=vc)
    assert torch.equal(bits(clean[0]), bits(dirty[0])), "part changed"
    assert torch.equal(bits(clean[1][sl, :, kp]), bits(dirty[1][sl, :, kp])) and torch.equal(bits(clean[2][sl, :, kp]), bits(dirty[2][sl, :, kp]))
    assert torch.equal(bits(dirty[1][sl, :, kp + 1:]), bits(kc[sl, :, kp + 1:])), "a row above kv_pos was written"


@pytest.mark.parametrize("kind, H, Hkv", [(0, 12, 2), (2, 12, 2), (3, 12, 2), (0, 4, 1), (2, 5, 1), (3, 14, 2), (3, 8, 1), (2, 9, 3)])
def test_heads_of_one_kv_head_with_the_same_q_agree(kind, H, Hkv):
    c = A.attn_case(kind, H, Hkv, 1030 if kind != 3 else 128, [513, 40] if kind != 3 else [31], 970, seq_S=[17] if kind == 3 else None)
    G = H // Hkv
    x = c["x"].reshape(-1, Hkv, G, 64).clone()
    x[:] = x[:, :, :1]
    y = call(dict(c, x=x.reshape(c["x"].shape)))[0].reshape(-1, Hkv, G, 64)
    assert torch.equal(bits(y), bits(y[:, :, :1].expand_as(y).contiguous()))


@pytest.mark.parametrize("H, Hkv, kp", [(12, 2, 700), (4, 1, 255), (16, 4, 512), (3, 1, 0)])
def test_the_four_attention_kernels_agree(H, Hkv, kp):
    """the same q, cache and position through ar_attn, battn, ar_prefill_attn and dec_attn2 (identity rotation, rstd = 1, wo = I, the
    new key and value equal to cache row kv_pos): each within its bound of the reference, so pairwise within the sum"""
    g = A.gen(980 + H)
    Lmax, D = 1030, 64 * H
    kc, vc = A.caches(g, 1, Hkv, Lmax)
    q = A.randn(g, 1, D, scale=0.35)
    ys, Es = {}, {}
    for kind in (0, 2, 3):
        c = dict(kind=kind, H=H, Hkv=Hkv, Lmax=Lmax, kc=kc, vc=vc, slots=[0], pos=[[5], [kp]], seq_S=[1] if kind == 3 else None, x=q, name=f"cross-{kind}")
        (_, ref, E, half), = A.expected(c)
        ys[kind], Es[kind] = call(c)[0].double(), E + half
        assert bool(((ys[kind] - ref).abs() <= Es[kind]).all()), kind
    rope = A.rope_unit(g, Lmax)
    rope[5, :, 0], rope[5, :, 1] = 1.0, 0.0
    hres = torch.ones(D)
    hres[::2] = -1.0                                            # mean square exactly 1, eps = 0: rstd = 1
    x = torch.cat([q[0], kc[0, :, kp].reshape(-1), vc[0, :, kp].reshape(-1)])[None]
    c1 = dict(kind=1, H=H, Hkv=Hkv, Lmax=Lmax, kc=kc, vc=vc, slots=[0], pos=[[5], [kp]], x=x, hres=hres, eps=0.0, wo=torch.eye(D).half(), rope=rope,
              name="cross-1")
    part = call(c1)[0].double()
    ys[1] = torch.stack([part[h, 64 * h:64 * h + 64] for h in range(H)]).reshape(1, D)
    off = part.clone()
    for h in range(H):
        off[h, 64 * h:64 * h + 64] = 0
    assert bool((off == 0).all()), "wo = I: part[h] is zero outside the head's own 64 rows"
    (_, ref1, E1, _), = A.expected(c1)[:1]
    Es[1] = torch.stack([E1[h, 64 * h:64 * h + 64] for h in range(H)]).reshape(1, D) + half      # part holds fp16(y): + the half step
    for a in (0, 1, 2, 3):
        for b in range(a + 1, 4):
            d = (ys[a] - ys[b]).abs()
            assert bool((d <= Es[a] + Es[b]).all()), (a, b, float((d / (Es[a] + Es[b])).max()))


@pytest.mark.parametrize("D, I", [(192, 320), (768, 2304)])
def test_the_three_cache_writers_agree(D, I):
    """the qkv role of path 0 (S = 5), of path 1 (five slots, the same rows) and ar_rope_cache fed with the reference projection"""
    c0 = A.linear_case(0, "qkv", D, I, 17, 5, 990)
    H, Hkv = c0["H"], c0["Hkv"]
    r0 = A.expected(c0)
    g0 = call(c0)
    g = A.gen(991)
    kc5, vc5 = A.caches(g, 5, Hkv, c0["Lmax"])
    c1 = dict(c0, path=1, kc=kc5, vc=vc5, slots=[4, 3, 2, 1, 0], name="writers-p1")
    r1 = A.expected(c1)
    g1 = call(c1)
    x = c0["x"].double()
    proj = ((x / torch.sqrt((x * x).mean(-1, keepdim=True) + c0["eps"]) * c0["gamma"].double()) @ c0["W"].double().T).float()
    c4 = dict(kind=4, H=H, Hkv=Hkv, Lmax=c0["Lmax"], kc=c0["kc"], vc=c0["vc"], slots=c0["slots"], pos=c0["pos"], x=proj, rope=c0["rope"], name="writers-k4")
    r4 = A.expected(c4)
    g4 = call(c4)
    for (name, ref, E, half), got in list(zip(r0, g0)) + list(zip(r1, g1)) + list(zip(r4, g4)):
        assert A.within(got, ref, E, half)[0], name
    # q_out row by row, and the written cache rows, pairwise within the sum of the bounds (+ the fp32 rounding of kind 4's input)
    slack = 3e-7 * r0[0][1].abs().max()
    assert bool(((g0[0].double() - g1[0].double()).abs() <= r0[0][2] + r1[0][2]).all())
    assert bool(((g0[0].double() - g4[0].double()).abs() <= r0[0][2] + r4[0][2] + slack).all())
    for s in range(5):
        kp, s0, s1 = c0["pos"][1][s], c0["slots"][0], c1["slots"][s]
        for i in (1, 2):
            d = (g0[i][s0, :, kp].double() - g1[i][s1, :, kp].double()).abs()
            assert bool((d <= r0[i][2][s0, :, kp] + r1[i][2][s1, :, kp]).all()), (s, i)


def test_decode_step_replays_are_checked_against_the_cache():
    """svc_ar_decode_step advances its device positions on every replay: the replay that would write cache row max_seq_len (and read
    the RoPE row behind the table) is refused before the graph is launched, and so is a replay without positions to advance"""
    from seedvc_amd import specs, weights
    from seedvc_amd.ar import ARModel
    cfg = specs.ar_config(dim=64, n_head=1, n_local_heads=1, n_layer=1, intermediate_size=128, vocab_size=17, max_seq_len=8)
    sd = weights.make_state_dict(specs.ar_state_spec(cfg), seed=3, prefix="ar.")
    m = ARModel(cfg, sd, "cuda:0")
    x = A.randn(A.gen(1), 64).cuda()
    with pytest.raises(RuntimeError, match="set_pos"):
        m.decode_step(x)                                   # nothing to advance yet
    a = m.decode_step(x, 6, 6)
    b = m.decode_step(x)                                   # positions 7: the last row of the cache
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())
    with pytest.raises(RuntimeError, match="position out of range"):
        m.decode_step(x)                                   # positions 8 = max_seq_len
    m.forward_generate(x.reshape(1, 1, 64), torch.tensor([2]), torch.tensor([2]))
    with pytest.raises(RuntimeError, match="set_pos"):
        m.decode_step(x)                                   # the prefill rewrote the device positions
    assert bool(torch.isfinite(m.decode_step(x, 3, 3)).all())


def test_worst_ratios_of_this_run():
    """prints what the tests above measured (run after them); the bound itself is asserted element by element"""
    for k, r in sorted(WORST.items()):
        print(f"worst error / bound, {k}: {r:.3f}" + ("   (above 0.5)" if r > 0.5 else ""))
    assert all(r <= 1.0 for r in WORST.values())
