"""GPU parity of the wav2vec 2.0 base family (HuBERT-base / wav2vec2-base: group-norm extractor, positional-conv groups of 48
channels, post-LN encoder; csrc/wav2vec2.hip through svc_w2v_create_ex) against the float64 restatement of
w2v_base_cases.py: the extractor and positional-conv seams on clips whose padding is NaN, the whole model at the small and the
HuBERT-base widths in both precisions, the one call over the windows of long clips against the literal driver loop, the bits of a
window whatever shares its call, the old family through the new creator, and `pipeline.content_conditions`.  Each float64 reference
is computed once (w2v_base_cases caches it)."""

import pytest
import torch

import w2v_base_cases as BC
import w2v_cases as VC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
OV = 20                                                      # overlap rows of the one-call tests (windows of 32 000 samples)
CLIP_LENS = (20000, 32000, 32400, 57700)                     # 1 + 1 + 2 + 3 windows; the last window of clip 2 keeps one row, of clip 3 none
POS_T = (1, 63, 64, 65, 100)                                 # shorter than k / 2, one below / at / past a tile, two tiles


def _make(name, precision, **over):
    from seedvc_amd.wav2vec2 import Wav2Vec2Content
    k = BC.case(name)
    return Wav2Vec2Content(k["sd"], cfg=dict(k["cfg"], **over), device=DEV, precision=precision)


@pytest.fixture(scope="module")
def models():
    """the handles of both configurations and precisions, made on first use and closed at the end of the module"""
    made = {}

    def get(name, precision, **over):
        key = (name, precision, tuple(sorted(over.items())))
        if key not in made:
            made[key] = _make(name, precision, **over)
        return made[key]

    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def clips():
    """the four clips of the one-call tests in a [4][60 000] buffer, NaN above each end"""
    buf = torch.full((len(CLIP_LENS), 60000), float("nan"))
    for b, n in enumerate(CLIP_LENS):
        buf[b, :n] = VC.make_wave(n, 20 + b)
    return buf


@pytest.fixture(scope="module")
def one_call(models, clips):
    return {p: models("BS", p).content_batch(clips.to(DEV), CLIP_LENS, overlap_s=OV * 320 / 16000) for p in (0, 1)}


# ------------------------------------------------------------------------------------------------ 1. extractor seam
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("dc", [False, True], ids=["normalised", "dc_offset"])
@pytest.mark.parametrize("name", ["BS", "BF"])
def test_extractor_seam(models, name, dc, precision):
    """One call with clips of 400 (79 conv0 frames: most of the 64 partial blocks are empty), 4 001, 16 000 and 32 000 samples, NaN
    above each clip's end; the projected rows against float64.  `dc_offset`: raw samples + 0.5 into a handle with do_normalize = 0, the
    input on which uncentred channel statistics would cancel (the float32 restatement itself stays at 1.9e-6 on it, so 0.5 stands)."""
    m = models(name, precision, do_normalize=False) if dc else models(name, precision)
    c = BC.case(name)["cfg"]
    D = c["d_model"]
    x, want = BC.extractor_case(name, dc)
    lens = BC.EXT_LENS
    buf = torch.full((len(lens), max(lens)), float("nan"))
    for b, t in enumerate(x):
        buf[b, :t.numel()] = t
    out = torch.full((len(lens), 100, D), 7.0, device=DEV)
    got, rows = m.features(buf.to(DEV), lens, out=out)
    got = got.cpu()
    assert rows == [1, 12, 49, 99] == [BC.frames(c, n) for n in lens]
    worst = 0.0
    for b, n in enumerate(lens):
        assert want[b].shape == (rows[b], D) and torch.isfinite(got[b, :rows[b]]).all()
        assert (got[b, rows[b]:] == 7.0).all(), "rows at and above the clip's count were written"
        e = BC.rms(got[b, :rows[b]], want[b])
        print(f"extractor {name} {'dc' if dc else 'norm'} precision {precision}, {n} samples: RMS(device - float64) = {e:.3e}")
        worst = max(worst, e)
    print(f"extractor seam {name} precision {precision}: worst RMS = {worst:.3e} (bound {BC.SEAM_BOUND['extractor'][precision]:.1e})")
    alone, r1 = m.features(buf[1:2, :lens[1]].to(DEV), lens[1:2])
    rev, _ = m.features(buf.flip(0).to(DEV), lens[::-1])
    assert r1 == [rows[1]] and torch.equal(alone[0, :rows[1]].cpu(), got[1, :rows[1]]), "a clip differs from its one-clip call"
    for b in range(len(lens)):
        assert torch.equal(rev[len(lens) - 1 - b, :rows[b]].cpu(), got[b, :rows[b]]), "the order of the clips changes a clip's bits"
    if dc:                                                   # do_normalize = 0: the normalisation seam is the identity below the length
        nz = m.normalize(buf.to(DEV), lens, out=torch.full(buf.shape, 7.0, device=DEV)).cpu()
        for b, n in enumerate(lens):
            assert torch.equal(nz[b, :n], buf[b, :n]) and (nz[b, n:] == 7.0).all()
    assert worst <= BC.SEAM_BOUND["extractor"][precision]


# ------------------------------------------------------------------------------------------------ 2. positional conv seam
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name", ["BS", "BF"], ids=["k16g4_d192", "k128g16_d768"])
def test_posconv_seam(models, name, precision):
    """Groups of 48 channels, T in {1, 63, 64, 65, 100} in one ragged call, against float64; rows at and above rows[b] untouched; a
    group reads no other group's channels (the padded K step must see written zeros, not its neighbours)."""
    m, k = models(name, precision), BC.case(name)
    c, sd = k["cfg"], k["sd"]
    D, T, B = c["d_model"], max(POS_T), len(POS_T)
    g = torch.Generator().manual_seed(77)
    h = torch.full((B, T, D), float("nan"))
    for b, t in enumerate(POS_T):
        h[b, :t] = torch.randn(t, D, generator=g)
    out = torch.full((B, T, D), 7.0, device=DEV)
    got = m.posconv(h.to(DEV), POS_T, out=out).cpu()
    worst = 0.0
    for b, t in enumerate(POS_T):
        want = BC.posconv(sd, c, h[b, :t])
        wrong = BC.posconv(sd, c, h[b, :t], drop="first")
        e, e_wrong = BC.rms(got[b, :t], want), BC.rms(got[b, :t], wrong)
        print(f"positional conv {name} precision {precision}, T = {t}: RMS(device - float64) = {e:.3e} (first output dropped: {e_wrong:.2e})")
        worst = max(worst, e)
        assert torch.isfinite(got[b, :t]).all() and (got[b, t:] == 7.0).all()
        assert e_wrong > 0.05
        alone = m.posconv(h[b:b + 1, :t].to(DEV), [t]).cpu()
        assert torch.equal(alone[0], got[b, :t]), f"T = {t} differs from its one-clip call"
    print(f"positional conv {name} precision {precision}: worst RMS = {worst:.3e} (bound {BC.SEAM_BOUND['posconv'][precision]:.1e})")
    rev = m.posconv(h.flip(0).to(DEV), POS_T[::-1]).cpu()
    for b, t in enumerate(POS_T):
        assert torch.equal(rev[B - 1 - b, :t], got[b, :t]), "the order of the clips changes a clip's bits"
    poisoned = h.clone()
    poisoned[:, :, 48:] = float("nan")                       # every group but the first
    gp = m.posconv(poisoned.to(DEV), POS_T).cpu()
    for b, t in enumerate(POS_T):
        assert torch.equal(gp[b, :t, :48], got[b, :t, :48]), "a group read another group's channels"
    assert worst <= BC.SEAM_BOUND["posconv"][precision]


# ------------------------------------------------------------------------------------------------ 3. whole model
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name,B", [("BS", 1), ("BS", 3), ("BF", 1)])
def test_whole_model(models, name, B, precision):
    """audio in, last_hidden_state out, against the float64 restatement (n_heads = 3 in BS: no power-of-two head count is assumed)"""
    m, k = models(name, precision), BC.case(name)
    lens = list(k["lens"][:B])
    buf = torch.full((B, max(lens)), float("nan"))
    for b in range(B):
        buf[b, :lens[b]] = k["waves"][b]
    S, rows = m.content_batch(buf.to(DEV), lens, overlap_s=0.0)
    S = S.cpu()
    assert rows == [t.shape[0] for t in k["ref"][:B]] and all(torch.isfinite(S[b, :rows[b]]).all() for b in range(B))
    e = BC.rms(torch.cat([S[b, :rows[b]] for b in range(B)]), torch.cat(k["ref"][:B]))
    print(f"model {name} B={B} precision {precision}: RMS(device - float64) = {e:.3e} (bound {BC.RMS_BOUND[name][precision]:.1e})")
    assert e <= BC.RMS_BOUND[name][precision]
    if name == "BS" and B == 1:                              # do_normalize = 0: the raw samples go in
        m0 = models(name, precision, do_normalize=False)
        S0, _ = m0.content_batch(buf.to(DEV), lens, overlap_s=0.0)
        e0 = BC.rms(S0[0, :rows[0]].cpu(), BC.model(k["sd"], k["cfg"], k["waves"][0], do_normalize=False))
        print(f"model {name} do_normalize=0 precision {precision}: RMS(device - float64) = {e0:.3e}")
        assert e0 <= BC.RMS_BOUND[name][precision]


# ------------------------------------------------------------------------------------------------ 4. one call
@pytest.mark.parametrize("precision", [0, 1])
def test_one_call_matches_the_driver_loop(models, clips, one_call, precision):
    k = BC.case("BS")
    m = models("BS", precision)
    S, rows = one_call[precision]
    S = S.cpu()
    assert rows == [m.rows(n, OV) for n in CLIP_LENS] == [62, 99, 100, 178] and S.shape == (4, 178, 192)
    for b, n in enumerate(CLIP_LENS):
        want = BC.driver_content(k["sd"], k["cfg"], clips[b, :n], OV)
        assert want.shape == (rows[b], 192)
        e = BC.rms(S[b, :rows[b]], want)
        print(f"one call, clip {b} ({n} samples, {rows[b]} rows), precision {precision}: RMS = {e:.3e} (bound {BC.RMS_BOUND['BS'][precision]:.1e})")
        assert torch.isfinite(S[b]).all() and e <= BC.RMS_BOUND["BS"][precision]
        assert (S[b, rows[b]:] == 0).all()


@pytest.mark.parametrize("precision", [0, 1])
def test_window_bits_do_not_depend_on_companions(models, clips, one_call, precision):
    """every window's rows: alone, among companions, under the reversed order, in groups of one"""
    m = models("BS", precision)
    S, rows = one_call[precision]
    ov_s = OV * 320 / 16000
    for b, n in enumerate(CLIP_LENS):
        alone, r1 = m.content_batch(clips[b:b + 1, :n].to(DEV), [n], overlap_s=ov_s)
        assert r1 == [rows[b]] and torch.equal(alone[0], S[b, :rows[b]])
    Sr, _ = m.content_batch(clips.flip(0).to(DEV), CLIP_LENS[::-1], overlap_s=ov_s)
    assert torch.equal(Sr.flip(0), S)
    m.set_window_group(1)
    S1, _ = m.content_batch(clips.to(DEV), CLIP_LENS, overlap_s=ov_s)
    m.set_window_group(0)
    assert torch.equal(S1, S)


# ------------------------------------------------------------------------------------------------ 5. the old family
def test_old_family_through_the_new_creator_keeps_its_bits(clips):
    """a layer-norm / stable-layer-norm handle made by svc_w2v_create_ex with ext = {1, 1} computes what svc_w2v_create's does"""
    from seedvc_amd.wav2vec2 import Wav2Vec2Content, c_ext
    k = VC.case("S")
    named = dict(k["cfg"], do_normalize=True)
    assert c_ext(k["cfg"]) is None and (c_ext(named).do_normalize, c_ext(named).feat_proj_layer_norm) == (1, 1)
    for precision in (0, 1):
        old = Wav2Vec2Content(k["sd"], cfg=k["cfg"], device=DEV, precision=precision)
        new = Wav2Vec2Content(k["sd"], cfg=named, device=DEV, precision=precision)
        a, ra = old.content_batch(clips.to(DEV), CLIP_LENS, overlap_s=OV * 320 / 16000)
        b, rb = new.content_batch(clips.to(DEV), CLIP_LENS, overlap_s=OV * 320 / 16000)
        assert ra == rb and torch.isfinite(a).all() and torch.equal(a, b)
        old.close()
        new.close()


# ------------------------------------------------------------------------------------------------ 6. content_conditions
def test_content_conditions_runs_with_a_base_model(models, clips):
    import cases
    from seedvc_amd import pipeline
    from seedvc_amd.length_regulator import InterpolateRegulator
    m = models("BS", 1)
    lc = cases.specs.lr_config("tiny", channels=64, in_channels=192)
    lsd = cases.weights.make_state_dict(cases.specs.lr_state_spec(lc), seed=17, prefix="lr.")
    lr = InterpolateRegulator(lc, lsd, DEV)
    src, ref = clips[3:4, :CLIP_LENS[3]].to(DEV), clips[0:1, :CLIP_LENS[0]].to(DEV)
    ov = OV * 320 / 16000
    cond, prompt = pipeline.content_conditions(m, lr, src, [CLIP_LENS[3]], [211], ref, [CLIP_LENS[0]], [77], overlap_s=ov)
    waves = torch.zeros(2, CLIP_LENS[3], device=DEV)
    waves[0], waves[1, :CLIP_LENS[0]] = src[0], ref[0]
    S, rows = m.content_batch(waves, [CLIP_LENS[3], CLIP_LENS[0]], overlap_s=ov)
    want_c = lr(S[:1], ylens=torch.LongTensor([211]), in_lens=rows[:1])[0]
    want_p = lr(S[1:], ylens=torch.LongTensor([77]), in_lens=rows[1:])[0]
    assert cond.shape == (1, 211, lc["out_channels"]) and prompt.shape == (1, 77, lc["out_channels"])    # the shapes it returns for XLS-R
    assert torch.equal(cond, want_c) and torch.equal(prompt, want_p) and torch.isfinite(cond).all()
