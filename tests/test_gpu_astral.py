"""GPU parity of the ASTRAL tokenizer (csrc/astral.hip) against the float64 restatement of astral_cases.py: the ConvNeXt block
seam on ragged clips whose padding is NaN, the whole head at the small and the released sizes in both precisions, independence
of companions bit for bit, the index and duration-reduction ops exactly, tokens against the float64 logits under the margin rule, the
one call over the windows of long clips against the literal driver loop and against the device's own one-window calls,
`pipeline.v2_content_tokens`, and the SSL seam against the w2v handle.  Each float64 reference is computed once (astral_cases caches
it).  Every figure is printed before it is asserted."""
import pytest
import torch
import torch.nn.functional as F

import astral_cases as AC
import w2v_cases as VC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
OV_S = AC.OV * 320 / 16000


def _tok(name, precision, **head_over):
    from seedvc_amd.astral import AstralTokenizer
    k = AC.case(name)
    c = k["cfg"]
    if head_over:
        c = dict(c, heads=[dict(h, **head_over) for h in c["heads"]])
    return AstralTokenizer(k["ssl_sd"], k["heads"], cfg=c, device=DEV, precision=precision)


@pytest.fixture(scope="module")
def small():
    return {p: _tok("S", p) for p in (0, 1)}


@pytest.fixture(scope="module")
def full():
    return {p: _tok("F", p) for p in (0, 1)}


def _ragged(rows_list, width, fill=float("nan")):
    buf = torch.full((len(rows_list), max(t.shape[0] for t in rows_list), width), fill)
    for b, t in enumerate(rows_list):
        buf[b, :t.shape[0]] = t.float()
    return buf


# ------------------------------------------------------------------------------------------------ 1. block seam
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", ["S", "F"])
def test_block_seam(name, precision):
    """one block (dwconv + LayerNorm, pwconv1, GRN, pwconv2) on nine ragged clips in ONE call; rows at and above a clip's count are NaN
    on input and keep a sentinel on output.  The bound is the block's own: min(cap of one block, 4 x the one-block figure measured)."""
    k, sc = AC.case(name), AC.seam_case(name)
    m = _tok(name, precision, n_blocks=1)
    Ts = AC.SEAM_T
    Din, D = k["cfg"]["ssl"]["d_model"], k["cfg"]["heads"][0]["dim"]
    out = torch.full((len(Ts), max(Ts), D), 7.0, device=DEV)
    got = m.convnext(0, _ragged(sc["h"], Din).to(DEV), Ts, out=out).cpu()
    worst = 0.0
    for b, t in enumerate(Ts):
        assert torch.isfinite(got[b, :t]).all() and (got[b, t:] == 7.0).all(), f"T = {t}: NaN inside or rows above the count written"
        worst = max(worst, AC.rel_rms(got[b, :t], sc["x"][b]))
    bound = AC.block_bound(name, precision)
    print(f"block seam {name} precision {precision}: worst rel RMS(device - float64) over T = {Ts}: {worst:.3e} (bound {bound:.1e})")
    m.close()
    assert worst <= bound


# ------------------------------------------------------------------------------------------------ 2. whole head
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", ["S", "F"])
def test_whole_head(small, full, name, precision):
    k = AC.case(name)
    m = (small if name == "S" else full)[precision]
    Ts = list(k["T"])
    h = _ragged(k["h"], k["cfg"]["ssl"]["d_model"]).to(DEV)
    ex = ez = zmax = 0.0
    for hk in range(2):
        x = m.convnext(hk, h, Ts)
        z = m.logits(hk, x, Ts).cpu()
        x = x.cpu()
        for b, t in enumerate(Ts):
            assert torch.isfinite(x[b, :t]).all() and torch.isfinite(z[b, :t]).all()
            ex, ez = max(ex, AC.rel_rms(x[b, :t], k["x"][hk][b])), max(ez, AC.rel_rms(z[b, :t], k["z"][hk][b]))
            zmax = max(zmax, (z[b, :t].double() - k["z"][hk][b]).abs().max().item())
    bx, bz = AC.rms_bound(name, precision, "x"), AC.rms_bound(name, precision, "z")
    srms = max(t.pow(2).mean().sqrt().item() for t in k["x"][0])
    print(f"whole head {name} precision {precision}: rel RMS x {ex:.3e} (bound {bx:.1e}), z {ez:.3e} (bound {bz:.1e}), max |z - z64| {zmax:.3e}; "
          f"stream RMS {srms:.2f} (errors are relative to max(1, RMS))")
    assert ex <= bx and ez <= bz


# ------------------------------------------------------------------------------------------------ 3. independence
def test_independence_of_companions(small):
    m, k = small[1], AC.case("S")
    Ts = list(AC.SEAM_T)
    B = len(Ts)
    h = _ragged(k["h"], 128)
    x = m.convnext(0, h.to(DEV), Ts)
    z = m.logits(0, x, Ts)
    rev_x = m.convnext(0, h.flip(0).to(DEV), Ts[::-1])
    rev_z = m.logits(0, rev_x, Ts[::-1])
    m.set_window_group(1)
    one_x = m.convnext(0, h.to(DEV), Ts)
    m.set_window_group(0)
    for b, t in enumerate(Ts):
        alone_x = m.convnext(0, h[b:b + 1, :t].to(DEV), [t])
        alone_z = m.logits(0, alone_x, [t])
        assert torch.equal(alone_x[0], x[b, :t]) and torch.equal(alone_z[0], z[b, :t]), f"T = {t} differs from its one-clip call"
        assert torch.equal(rev_x[B - 1 - b, :t], x[b, :t]) and torch.equal(rev_z[B - 1 - b, :t], z[b, :t]), "the order of the clips changes a clip's bits"
        assert torch.equal(one_x[b, :t], x[b, :t]), "the group size changes a clip's bits"
    # a clip among zero-padded companions is NOT the clip over the zero-padded rectangle: the latter moves the logits by O(1)
    padded = torch.zeros(1, 85, 128)
    padded[0, :65] = k["h"][6].float()
    zp = m.logits(0, m.convnext(0, padded.to(DEV), [85]), [85])
    assert (zp[0, :65] - z[6, :65]).abs().max().item() > 0.1


def test_one_call_independence(small):
    m, cc = small[1], AC.clip_case()
    buf = cc["buf"].to(DEV)
    tok, rows = m.tokens_batch(buf, AC.CLIP_LENS, overlap_s=OV_S)
    assert rows == [62, 99, 100, 178] and tok.shape == (2, 4, 178) and tok.dtype == torch.int32
    for b, n in enumerate(AC.CLIP_LENS):
        alone, r1 = m.tokens_batch(buf[b:b + 1, :n], [n], overlap_s=OV_S)
        assert r1 == [rows[b]] and torch.equal(alone[:, 0], tok[:, b, :rows[b]])
        assert (tok[:, b, rows[b]:] == -1).all()
    for group in (2, 1):
        m.set_window_group(group)
        t2, _ = m.tokens_batch(buf, AC.CLIP_LENS, overlap_s=OV_S)
        m.set_window_group(0)
        assert torch.equal(t2, tok)
    tr, _ = m.tokens_batch(buf.flip(0), AC.CLIP_LENS[::-1], overlap_s=OV_S)
    assert torch.equal(tr.flip(1), tok)


@pytest.mark.parametrize("precision", [0, 1])
def test_ssl_seam_independence(small, precision):
    """the SSL seam's rows of a clip, bit for bit: alone, among companions, in reversed order, and in window groups of 1 and 2 (more
    clips than the group: the later groups write behind the earlier ones and reuse the group's tables and workspace)"""
    m, tc = small[precision], AC.token_case()
    lens = list(AC.TOKEN_LENS)
    B = len(lens)
    buf = torch.full((B, max(lens)), float("nan"))
    for b, w in enumerate(tc["waves"]):
        buf[b, :w.numel()] = w
    s, rows = m.ssl(buf.to(DEV), lens)
    assert rows == [AC.window_rows(AC.CFG_S, n) for n in lens]
    rev, rrows = m.ssl(buf.flip(0).to(DEV), lens[::-1])
    assert rrows == rows[::-1]
    grouped = {}
    for group in (1, 2):
        m.set_window_group(group)
        grouped[group] = (m.ssl(buf.to(DEV), lens)[0], m.ssl(buf.flip(0).to(DEV), lens[::-1])[0])
        m.set_window_group(0)
    for b, (n, r) in enumerate(zip(lens, rows)):
        assert torch.isfinite(s[b, :r]).all()
        alone, r1 = m.ssl(buf[b:b + 1, :n].to(DEV), [n])
        assert r1 == [r] and torch.equal(alone[0, :r], s[b, :r]), f"{n} samples differ from their one-clip call"
        assert torch.equal(rev[B - 1 - b, :r], s[b, :r]), "the order of the clips changes a clip's bits"
        for group, (fwd, bwd) in grouped.items():
            assert torch.equal(fwd[b, :r], s[b, :r]), f"window group {group} changes a clip's bits"
            assert torch.equal(bwd[B - 1 - b, :r], s[b, :r]), f"window group {group}, reversed order, changes a clip's bits"


# ------------------------------------------------------------------------------------------------ 4. index op
@pytest.mark.parametrize("bits", [1, 5, 11, 16])
def test_bsq_index_op(bits):
    from seedvc_amd import astral
    g = torch.Generator().manual_seed(bits)
    for rows in (1, 63, 4097):
        z = torch.randn(rows, bits, generator=g)
        special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, float("inf"), float("-inf")])
        pos = torch.randint(0, rows * bits, (min(rows * bits, 64),), generator=g)
        z.view(-1)[pos] = special[torch.arange(pos.numel()) % special.numel()]
        got = astral.bsq_index_device(z.to(DEV)).cpu()
        assert got.dtype == torch.int32 and torch.equal(got.long(), AC.bsq_index(z)), (bits, rows)


# ------------------------------------------------------------------------------------------------ 5. reduction op
@pytest.mark.parametrize("alphabet", [2, 32])
def test_tokens_reduce_op(alphabet):
    from seedvc_amd import astral
    rows = [1, 2, 64, 65, 1000]
    g = torch.Generator().manual_seed(alphabet)
    tok = torch.full((5, 1000), -7, dtype=torch.int32)
    for b, n in enumerate(rows):
        tok[b, :n] = torch.randint(0, alphabet, (n,), generator=g).int()
    tok[2, :64] = 3                                          # one run
    red, cnt = astral.reduce_tokens(tok.to(DEV), rows)
    counts = cnt.tolist()                                    # the one read-back
    red = red.cpu()
    for b, n in enumerate(rows):
        want = torch.unique_consecutive(tok[b, :n])
        assert counts[b] == want.numel() and torch.equal(red[b, :counts[b]], want), b
        assert (red[b, counts[b]:] == -1).all()
    assert counts[2] == 1


# ------------------------------------------------------------------------------------------------ 6. tokens against float64
@pytest.mark.parametrize("precision", [0, 1])
def test_tokens_against_float64(small, precision):
    m, tc = small[precision], AC.token_case()
    lens = list(AC.TOKEN_LENS)
    buf = torch.full((len(lens), max(lens)), float("nan"))
    for b, w in enumerate(tc["waves"]):
        buf[b, :w.numel()] = w
    tok, rows = m.tokens_batch(buf.to(DEV), lens, overlap_s=0.0)
    assert rows == [1, 1, 9, 49] == [AC.window_rows(AC.CFG_S, n) for n in lens]
    mg = AC.MARGIN["S"][precision]
    # the logit error behind the margin, measured through the seams on the device's own SSL rows
    s, _ = m.ssl(buf.to(DEV), lens)
    zerr = 0.0
    for hk in range(2):
        z = m.logits(hk, m.convnext(hk, s, rows), rows).cpu()
        for b, r in enumerate(rows):
            zerr = max(zerr, (z[b, :r].double() - tc["z"][hk][b]).abs().max().item())
            assert torch.equal(AC.bsq_index(z[b, :r]).int(), tok[hk, b, :r].cpu()), "the one call's tokens are not the signs of the seams' logits"
    print(f"tokens S precision {precision}: max |device - float64| logit error through the SSL front {zerr:.3e} (margin {mg})")
    assert mg is not None, "record 4 x the measured logit error in astral_cases.MARGIN"
    for hk in range(2):
        for b, r in enumerate(rows):
            outside, inside, frac = AC.check_tokens(tok[hk, b, :r], tc["z"][hk][b], mg)
            print(f"  head {hk} clip {b} ({r} rows): {outside} bits differ outside the margin, {inside} inside")
            assert outside == 0
        assert AC.excluded_fraction(torch.cat(tc["z"][hk]), mg) <= AC.MAX_EXCLUDED
    assert zerr <= mg


# ------------------------------------------------------------------------------------------------ 7. one call over long clips
@pytest.mark.parametrize("precision", [0, 1])
def test_one_call_over_long_clips(small, precision):
    m, cc = small[precision], AC.clip_case()
    buf = cc["buf"].to(DEV)
    tok, rows, red, cnt = m.tokens_batch(buf, AC.CLIP_LENS, overlap_s=OV_S, reduce_head=1)
    counts = cnt.tolist()
    tok_c, red_c = tok.cpu(), red.cpu()
    mg = AC.MARGIN["S"][precision]
    assert mg is not None, "record 4 x the measured logit error in astral_cases.MARGIN"
    for b, n in enumerate(AC.CLIP_LENS):
        loop = [[], []]                                     # the literal loop through the device's own one-window calls
        for start, ns, drop in VC.driver_plan(n, 32000, AC.OV * 320):
            t1, r1 = m.tokens_batch(buf[b:b + 1, start:start + ns], [ns], overlap_s=0.0)
            for hk in range(2):
                loop[hk].append(t1[hk, 0, drop:r1[0]])
        for hk in range(2):
            assert torch.equal(torch.cat(loop[hk]), tok[hk, b, :rows[b]]), f"clip {b} head {hk}: the one call differs from the loop of one-window calls"
            z64 = cc["z"][b][hk]
            assert z64.shape[0] == rows[b]
            outside, inside, frac = AC.check_tokens(tok_c[hk, b, :rows[b]], z64, mg)
            print(f"one call precision {precision} clip {b} head {hk}: {outside} bits differ outside the margin {mg:.1e}, {inside} inside, {100 * frac:.2f} % of bits inside")
            assert outside == 0 and frac <= AC.MAX_EXCLUDED
        want = torch.unique_consecutive(tok_c[1, b, :rows[b]])
        assert counts[b] == want.numel() and torch.equal(red_c[b, :counts[b]], want) and (red_c[b, counts[b]:] == -1).all()
        assert (tok_c[:, b, rows[b]:] == -1).all()


def test_reduced_may_not_overlap_tokens(small):
    """the one call refuses a `reduced` buffer inside the token plane before it launches anything (the reduction reads its neighbours)"""
    from seedvc_amd import _lib
    m = small[1]
    wave = torch.zeros(1, 4000, device=DEV)
    tok = torch.full((2, 1, 12), 5, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = m._fn("tokens")(m._h, _lib.ptr(wave), _lib.i32_host([4000]), 1, 4000, 0, _lib.ptr(tok), 12, 1, _lib.ptr(tok[1]), _lib.ptr(cnt), _lib.stream_ptr())
    assert rc != 0 and b"must not overlap" in _lib.lib().svc_last_error()
    assert (tok == 5).all()


# ------------------------------------------------------------------------------------------------ 8. pipeline
def test_v2_content_tokens(small):
    from seedvc_amd import pipeline
    m, cc = small[1], AC.clip_case()
    lens = [20000, 3000, 32400, 16000, 57700]                # 3 sources and 2 targets
    buf = torch.zeros(5, 57700)
    for b, n in enumerate(lens):
        buf[b, :n] = AC.make_wave(n, 30 + b)
    recs = pipeline.v2_content_tokens(m, buf.to(DEV), lens, overlap_s=OV_S)
    tok, rows = m.tokens_batch(buf.to(DEV), lens, overlap_s=OV_S)
    red, counts = m.reduce(tok[1], rows)
    assert len(recs) == 5
    for b, r in enumerate(recs):
        assert set(r) == {"wide", "narrow", "narrow_reduced"}
        for v in r.values():
            assert v.dtype == torch.int64 and v.device.type == "cuda" and v.dim() == 2 and v.size(0) == 1
        assert r["wide"].shape == (1, rows[b]) and torch.equal(r["wide"][0], tok[0, b, :rows[b]].long())
        assert torch.equal(r["narrow"][0], tok[1, b, :rows[b]].long())
        assert r["narrow_reduced"].shape == (1, counts[b]) and torch.equal(r["narrow_reduced"][0], red[b])
        assert r["wide"].min() >= 0 and r["wide"].max() < 2048 and r["narrow"].max() < 32
    assert pipeline.v2_ar_prompt(recs[3]["narrow_reduced"], recs[0]["narrow_reduced"]).shape == (1, counts[3] + counts[0])
    _, idx, fl = m.tokenize(buf[1:2, :3000], [3000], head=1)
    assert idx.dtype == torch.int64 and fl.tolist() == [rows[1]] and torch.equal(idx[0], recs[1]["narrow"][0])


# ------------------------------------------------------------------------------------------------ 9. SSL seam
@pytest.mark.parametrize("precision", [0, 1])
def test_ssl_seam(small, precision):
    """The residual stream after the last layer against the float64 front without encoder.layer_norm, under 8i's bounds read as the
    project's cap is read on a stream (relative to its RMS, 2.0 here; measured 6.40e-5 / 7.73e-4 relative in precision 0 / 1, i.e. 1.28e-4 /
    1.55e-3 absolute, the same fp16-attention rounding that gives 6.3e-5 behind the w2v handle's final LayerNorm); and LayerNorm of these rows
    is the w2v handle's output."""
    from seedvc_amd.wav2vec2 import Wav2Vec2Content
    m, k, tc = small[precision], AC.case("S"), AC.token_case()
    lens = list(AC.TOKEN_LENS)
    buf = torch.full((len(lens), max(lens)), float("nan"))
    for b, w in enumerate(tc["waves"]):
        buf[b, :w.numel()] = w
    out = torch.full((len(lens), 50, 128), 7.0, device=DEV)
    s, rows = m.ssl(buf.to(DEV), lens, out=out)
    s = s.cpu()
    got, want64 = torch.cat([s[b, :r] for b, r in enumerate(rows)]), torch.cat(tc["ssl"])
    e, scale = AC.rel_rms(got, want64), want64.pow(2).mean().sqrt().item()
    bound = VC.RMS_BOUND["S"][precision]                     # 8i's bounds; the stream's RMS exceeds 1, so they are relative to it
    print(f"SSL seam precision {precision}: RMS(device - float64, no final LayerNorm) = {e:.3e} of the stream's RMS {scale:.2f} "
          f"(absolute {e * scale:.3e}; bound {bound:.1e}, relative)")
    assert all((s[b, r:] == 7.0).all() for b, r in enumerate(rows)) and e <= bound
    sd1 = dict(k["ssl_sd"])
    sd1["encoder.layer_norm.weight"], sd1["encoder.layer_norm.bias"] = torch.ones(128), torch.zeros(128)
    w2v = Wav2Vec2Content(sd1, cfg=k["cfg"]["ssl"], device=DEV, precision=precision)
    want, r2 = w2v.content_batch(buf.to(DEV), lens, overlap_s=0.0)
    assert r2 == rows
    d = max((F.layer_norm(s[b, :r], (128,), eps=1e-5) - want[b, :r].cpu()).abs().max().item() for b, r in enumerate(rows))
    print(f"SSL seam precision {precision}: max |LayerNorm(ssl rows) - w2v handle| = {d:.3e} (bound 1e-5)")
    w2v.close()
    assert d <= 1e-5
