"""GPU parity of the wav2vec 2.0 content encoder (csrc/wav2vec2.hip) against the float64 restatement of w2v_cases.py: the
LayerNorm+GELU row kernel, the normalisation, extractor and positional-conv seams on clips whose padding is NaN, the encoder on the
small and the XLS-R-sized configuration in both precisions, the one call over the windows of long clips against the literal driver
loop, and `pipeline.content_conditions`.  Each float64 reference is computed once (w2v_cases caches it)."""

import pytest
import torch
import torch.nn.functional as F

import w2v_cases as VC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
OV = 20                                                      # overlap rows of the one-call tests (config S: windows of 32 000 samples)
CLIP_LENS = (20000, 32000, 32400, 57700)                     # 1 + 1 + 2 + 3 windows; the last window of clip 2 keeps one row, of clip 3 none
POS_T = (1, 7, 63, 64, 65, 129, 300)                         # both paddings overlap, shorter than k / 2, one past a tile, several tiles


def _model(name, precision, **over):
    from seedvc_amd.wav2vec2 import Wav2Vec2Content
    k = VC.case(name)
    if over:
        c = dict(k["cfg"], **over)
        return Wav2Vec2Content(VC.make_state_dict(c, seed=31), cfg=c, device=DEV, precision=precision), c
    return Wav2Vec2Content(k["sd"], cfg=k["cfg"], device=DEV, precision=precision)


@pytest.fixture(scope="module")
def small():
    return {p: _model("S", p) for p in (0, 1)}


@pytest.fixture(scope="module")
def clips():
    """the four clips of the one-call tests in a [4][60 000] buffer, NaN above each end"""
    buf = torch.full((len(CLIP_LENS), 60000), float("nan"))
    for b, n in enumerate(CLIP_LENS):
        buf[b, :n] = VC.make_wave(n, 20 + b)
    return buf


@pytest.fixture(scope="module")
def one_call(small, clips):
    return {p: small[p].content_batch(clips.to(DEV), CLIP_LENS, overlap_s=OV * 320 / 16000) for p in (0, 1)}


def _ln_gelu(x, gamma, beta):
    from seedvc_amd import _lib
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y = torch.empty_like(xd)
    _lib.check(_lib.lib().svc_op_layernorm_gelu(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(y), x.shape[0], x.shape[1], 1e-5, _lib.stream_ptr()))
    return y.cpu()


# ------------------------------------------------------------------------------------------------ 1. op seam
def test_layernorm_gelu_is_the_erf_form():
    """gamma = 0 makes the LayerNorm output exactly beta, so the kernel's GELU sees pre-activations under the test's control: 2048
    values over +-6, within 1e-6 of float64 erf-GELU; the tanh form is 1e-4 and more away"""
    g = torch.Generator().manual_seed(4)
    D = 2048
    beta = torch.linspace(-6.0, 6.0, D)
    got = _ln_gelu(torch.randn(5, D, generator=g), torch.zeros(D), beta)
    want = F.gelu(beta.double())
    e = (got.double() - want).abs().max().item()
    tanh_gap = (F.gelu(beta.double(), approximate="tanh") - want).abs().max().item()
    print(f"LayerNorm+GELU row kernel: max |device - float64 erf-GELU| = {e:.3e} (bound 1e-6; the tanh form is {tanh_gap:.1e} away)")
    assert e <= 1e-6 and tanh_gap > 1e-4


@pytest.mark.parametrize("D", [64, 512])
def test_layernorm_gelu_is_two_pass(D):
    """rows with mean 100 and std 1: a one-pass E[x^2] - E[x]^2 variance lands near 3e-4, a two-pass form near 1e-5"""
    g = torch.Generator().manual_seed(D)
    rows = 37                                                # not a multiple of the 4 rows of a workgroup
    x = 100.0 + torch.randn(rows, D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    want = F.gelu(F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5))
    e = (_ln_gelu(x, gamma, beta).double() - want).abs().max().item()
    print(f"LayerNorm+GELU D={D}: max |device - float64| = {e:.3e} (bound 1e-4)")
    assert e <= 1e-4


# ------------------------------------------------------------------------------------------------ 2. normalisation seam
def test_normalize_seam(small):
    m = small[1]
    lens = (400, 5000, 16001, 3000, 777)
    g = torch.Generator().manual_seed(8)
    buf = torch.full((5, 16001), float("nan"))
    buf[0, :400], buf[1, :5000], buf[2, :16001] = 3 * VC.make_wave(400, 1), 3 * VC.make_wave(5000, 2), 3 * VC.make_wave(16001, 3)
    buf[3, :3000] = 100.0 + torch.randn(3000, generator=g)  # DC offset 100, std 1: a one-pass variance loses it
    buf[4, :777] = 0.0
    out = torch.full((5, 16001), 7.0, device=DEV)
    got = m.normalize(buf.to(DEV), lens, out=out).cpu()
    for b, n in enumerate(lens):
        assert (got[b, n:] == 7.0).all(), "samples at and above the length were written"
        y = got[b, :n].double()
        if b == 4:
            assert (y == 0).all()
            continue
        want = VC.normalize(buf[b, :n])
        e, big = (y - want).abs().max().item(), buf[b, :n].abs().max().item()
        mean, var = y.mean().item(), y.var(unbiased=False).item()
        print(f"normalise clip {b} ({n} samples): max err {e:.3e} (bound {1e-5 * big:.1e}), mean {mean:.2e}, var - 1 {var - 1:.2e} (bounds 1e-5)")
        assert e <= 1e-5 * big and abs(mean) <= 1e-5 and abs(var - 1) <= 1e-5
        alone = m.normalize(buf[b:b + 1, :n].to(DEV), [n]).cpu()
        assert torch.equal(alone[0], got[b, :n]), f"clip {b} differs from its one-clip call"


# ------------------------------------------------------------------------------------------------ 3. extractor seam
@pytest.mark.parametrize("precision", [0, 1])
def test_extractor_seam(small, precision):
    m = small[precision]
    k = VC.case("S")
    lens = (400, 719, 720, 1039, 1040, 5123, 16000)
    norm = [VC.normalize(VC.make_wave(n, 60 + i)) for i, n in enumerate(lens)]
    buf = torch.full((len(lens), 16000), float("nan"))
    for b, x in enumerate(norm):
        buf[b, :x.numel()] = x.float()
    out = torch.full((len(lens), 50, 128), 7.0, device=DEV)
    got, rows = m.features(buf.to(DEV), lens, out=out)
    got = got.cpu()
    assert rows == [1, 1, 2, 2, 3, 15, 49] == [VC.frames(k["cfg"], n) for n in lens]
    worst = 0.0
    for b, n in enumerate(lens):
        want = VC.extractor(k["sd"], k["cfg"], buf[b, :n])
        assert want.shape == (rows[b], 128) and torch.isfinite(got[b, :rows[b]]).all()
        assert (got[b, rows[b]:] == 7.0).all(), "rows at and above the clip's count were written"
        worst = max(worst, VC.rms(got[b, :rows[b]], want))
        alone, r1 = m.features(buf[b:b + 1, :n].to(DEV), [n])
        assert r1 == [rows[b]] and torch.equal(alone[0, :rows[b]].cpu(), got[b, :rows[b]]), f"clip {b} differs from its one-clip call"
    print(f"extractor seam precision {precision}: worst RMS(device - float64) = {worst:.3e} (bound {VC.RMS_BOUND['S'][precision]:.1e})")
    assert worst <= VC.RMS_BOUND["S"][precision]


# ------------------------------------------------------------------------------------------------ 4. positional conv seam
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("size", ["k16g2", "k128g16"])
def test_posconv_seam(small, size, precision):
    """Against F.conv1d(padding = k // 2)[..., :-1] in float64 on the operands the device multiplies (rounded to fp16 in precision 1), so
    that what is left is fp32 accumulation over k * 64 products of an O(1) sum: RMS bound 1e-5.  The same conv with the FIRST output
    dropped is far outside."""
    if size == "k16g2":
        m, c, sd = small[precision], VC.case("S")["cfg"], VC.case("S")["sd"]
    else:
        m, c = _model("F", precision, n_layers=1, ffn_dim=64, conv_dim=64)
        sd = VC.make_state_dict(c, seed=31)
    D, T, B = c["d_model"], max(POS_T), len(POS_T)
    g = torch.Generator().manual_seed(77)
    h = torch.full((B, T, D), float("nan"))
    for b, t in enumerate(POS_T):
        h[b, :t] = torch.randn(t, D, generator=g)
    out = torch.full((B, T, D), 7.0, device=DEV)
    got = m.posconv(h.to(DEV), POS_T, out=out).cpu()
    worst = 0.0
    for b, t in enumerate(POS_T):
        want = VC.posconv(sd, c, h[b, :t], gemm16=precision == 1)
        wrong = VC.posconv(sd, c, h[b, :t], gemm16=precision == 1, drop="first")
        e, e_wrong = VC.rms(got[b, :t], want), VC.rms(got[b, :t], wrong)
        worst = max(worst, e)
        assert torch.isfinite(got[b, :t]).all() and (got[b, t:] == 7.0).all()
        assert e <= 1e-5 and e_wrong > 0.05, (b, t, e, e_wrong)
        alone = m.posconv(h[b:b + 1, :t].to(DEV), [t]).cpu()
        assert torch.equal(alone[0], got[b, :t]), f"T = {t} differs from its one-clip call"
    print(f"positional conv {size} precision {precision}: worst RMS = {worst:.3e} (bound 1e-5)")
    rev = m.posconv(h.flip(0).to(DEV), POS_T[::-1]).cpu()
    for b, t in enumerate(POS_T):
        assert torch.equal(rev[B - 1 - b, :t], got[b, :t]), "the order of the clips changes a clip's bits"
    poisoned = h.clone()
    poisoned[:, :, 64:] = float("nan")                       # every group but the first
    gp = m.posconv(poisoned.to(DEV), POS_T).cpu()
    for b, t in enumerate(POS_T):
        assert torch.equal(gp[b, :t, :64], got[b, :t, :64]), "a group read another group's channels"
    if size != "k16g2":
        m.close()


# ------------------------------------------------------------------------------------------------ 5. encoder
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_encoder_small(small, B, precision):
    m, k = small[precision], VC.case("S")
    rows = [t.shape[0] for t in k["h"][:B]]
    T = max(rows)
    h = torch.full((B, T, 128), float("nan"))
    for b in range(B):
        h[b, :rows[b]] = k["h"][b].float()
    got = m.encode(h.to(DEV), rows).cpu()
    e = VC.rms(torch.cat([got[b, :rows[b]] for b in range(B)]), torch.cat(k["ref"][:B]))
    print(f"encoder S B={B} precision {precision}: RMS(device - float64) = {e:.3e} (bound {VC.RMS_BOUND['S'][precision]:.1e})")
    assert all(torch.isfinite(got[b, :rows[b]]).all() for b in range(B)) and e <= VC.RMS_BOUND["S"][precision]
    if B == 3:                                               # a clip's rows: alone, among companions, reversed, in groups of one
        alone = m.encode(h[1:2, :rows[1]].to(DEV), rows[1:2]).cpu()
        rev = m.encode(h.flip(0).to(DEV), rows[::-1]).cpu()
        m.set_window_group(1)
        one = m.encode(h.to(DEV), rows).cpu()
        m.set_window_group(0)
        assert torch.equal(alone[0], got[1, :rows[1]])
        for b in range(B):
            assert torch.equal(rev[B - 1 - b, :rows[b]], got[b, :rows[b]]) and torch.equal(one[b, :rows[b]], got[b, :rows[b]])


@pytest.mark.parametrize("precision", [0, 1])
def test_model_xlsr_sizes(precision):
    """XLS-R widths (4 layers), one clip of 1.9 s, audio in: the whole chain against the float64 restatement"""
    m, k = _model("F", precision), VC.case("F")
    n = k["lens"][0]
    got = m.semantic_fn(k["waves"][0][None])[0].cpu()
    assert got.shape == k["ref"][0].shape == (VC.frames(k["cfg"], n), 1024) and torch.isfinite(got).all()
    e = VC.rms(got, k["ref"][0])
    print(f"model F precision {precision}: RMS(device - float64) = {e:.3e} (bound {VC.RMS_BOUND['F'][precision]:.1e})")
    assert e <= VC.RMS_BOUND["F"][precision]
    m.close()


# ------------------------------------------------------------------------------------------------ 6. one call
@pytest.mark.parametrize("precision", [0, 1])
def test_one_call_matches_the_driver_loop(small, clips, one_call, precision):
    k = VC.case("S")
    m = small[precision]
    S, rows = one_call[precision]
    S = S.cpu()
    assert rows == [m.rows(n, OV) for n in CLIP_LENS] == [62, 99, 100, 178] and S.shape == (4, 178, 128)
    for b, n in enumerate(CLIP_LENS):
        want = VC.driver_content(k["sd"], k["cfg"], clips[b, :n], OV)
        assert want.shape == (rows[b], 128)
        e = VC.rms(S[b, :rows[b]], want)
        print(f"one call, clip {b} ({n} samples, {rows[b]} rows), precision {precision}: RMS = {e:.3e} (bound {VC.RMS_BOUND['S'][precision]:.1e})")
        assert torch.isfinite(S[b]).all() and e <= VC.RMS_BOUND["S"][precision]
        assert (S[b, rows[b]:] == 0).all()


def test_one_call_rows_do_not_depend_on_companions(small, clips, one_call):
    m = small[1]
    S, rows = one_call[1]
    ov_s = OV * 320 / 16000
    for b, n in enumerate(CLIP_LENS):
        alone, r1 = m.content_batch(clips[b:b + 1, :n].to(DEV), [n], overlap_s=ov_s)
        assert r1 == [rows[b]] and torch.equal(alone[0], S[b, :rows[b]])
    for group in (2, 1):                                     # 6 computed windows in groups of 2 and of 1
        m.set_window_group(group)
        S2, _ = m.content_batch(clips.to(DEV), CLIP_LENS, overlap_s=ov_s)
        m.set_window_group(0)
        assert torch.equal(S2, S)
    Sr, _ = m.content_batch(clips.flip(0).to(DEV), CLIP_LENS[::-1], overlap_s=ov_s)
    assert torch.equal(Sr.flip(0), S)
    sem = m.semantic_fn(clips[0:1, :CLIP_LENS[0]])
    assert sem.shape == (1, rows[0], 128) and torch.equal(sem[0], S[0, :rows[0]])


def test_one_call_argument_errors(small, clips):
    m = small[1]
    with pytest.raises(RuntimeError, match="receptive field"):
        m.content_batch(clips[:1, :399].to(DEV), [399], overlap_s=OV * 320 / 16000)
    with pytest.raises(RuntimeError, match="overlap_rows"):
        m.content_batch(clips[:1, :20000].to(DEV), [20000], overlap_s=2.0)


# ------------------------------------------------------------------------------------------------ 7. content_conditions
def test_content_conditions_runs_unchanged(small, clips):
    import cases
    from seedvc_amd import pipeline
    from seedvc_amd.length_regulator import InterpolateRegulator
    m = small[1]
    lc = cases.specs.lr_config("tiny", channels=64, in_channels=128)
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
    assert cond.shape == (1, 211, lc["out_channels"]) and prompt.shape == (1, 77, lc["out_channels"])
    assert torch.equal(cond, want_c) and torch.equal(prompt, want_p) and torch.isfinite(cond).all()
