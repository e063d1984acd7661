"""GPU parity of the Whisper content encoder (csrc/whisper.hip) against the float64 restatement of whisper_cases.py: the two op
seams (erf-GELU in the tap-GEMM epilogue, the two-pass LayerNorm), the log-mel seam on clips whose padding is NaN, the encoder
on the small and the whisper-small configuration in both precisions, the one call over the windows of long clips against the
literal driver loop, and `pipeline.content_conditions`.  Each float64 reference is computed once (whisper_cases caches it)."""

import pytest
import torch

import whisper_cases as WC

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
KG_ACT_GELU = 8
OV = 20                                                      # overlap rows of the one-call tests (config S: 100 rows per window)
CLIP_LENS = (20000, 32000, 32001, 57605)                     # 1 + 1 + 2 + 3 windows; the last window of clips 2 and 3 keeps one row


def _model(name, precision):
    from seedvc_amd.whisper import WhisperContent
    k = WC.case(name)
    return WhisperContent(k["sd"], cfg=k["cfg"], mel_basis=k["basis"], device=DEV, precision=precision)


@pytest.fixture(scope="module")
def small():
    return {p: _model("S", p) for p in (0, 1)}


@pytest.fixture(scope="module")
def clips():
    """the four clips of the one-call tests in a [4][60 000] buffer, NaN above each end"""
    buf = torch.full((len(CLIP_LENS), 60000), float("nan"))
    for b, n in enumerate(CLIP_LENS):
        buf[b, :n] = WC.make_wave(n, 20 + b)
    return buf


@pytest.fixture(scope="module")
def one_call(small, clips):
    return {p: small[p].content_batch(clips.to(DEV), CLIP_LENS, overlap_s=OV * 320 / 16000) for p in (0, 1)}


# ------------------------------------------------------------------------------------------------ 1. op seams
def test_gelu_epilogue_is_the_erf_form():
    """GELU through svc_op_linear on the fp32 path, pre-activations in +-6: within 1e-6 of float64 erf-GELU of the SAME
    pre-activations (the plain linear's own error is taken out by feeding its device output to the reference)."""
    from seedvc_amd import ops
    g = torch.Generator().manual_seed(3)
    M, N, K = 200, 72, 32                                    # more than one tile of rows, N no multiple of the tile
    a = torch.rand(M, K, generator=g) * 2 - 1
    w = (torch.rand(N, K, generator=g) * 2 - 1) * (6.0 / K)
    b = (torch.rand(N, generator=g) * 2 - 1) * 5.0
    plain = ops.linear(a.to(DEV), w.to(DEV), b.to(DEV), dtype="f32", act=0).cpu()
    got = ops.linear(a.to(DEV), w.to(DEV), b.to(DEV), dtype="f32", act=KG_ACT_GELU).cpu()
    lin64 = a.double() @ w.double().T + b.double()
    assert 4.0 < plain.abs().max() <= 6.5
    want = torch.nn.functional.gelu(plain.double())
    e, e_lin = (got.double() - want).abs().max().item(), (plain.double() - lin64).abs().max().item()
    tanh_gap = (torch.nn.functional.gelu(plain.double(), approximate="tanh") - want).abs().max().item()
    print(f"erf-GELU epilogue: max |device - float64| = {e:.3e} (bound 1e-6; the linear's own error {e_lin:.1e}; tanh form is {tanh_gap:.1e} away)")
    assert e <= 1e-6 and tanh_gap > 1e-4


@pytest.mark.parametrize("D", [128, 768])
def test_layernorm_is_two_pass(D):
    """rows with mean 100 and std 1: a one-pass E[x^2] - E[x]^2 variance lands near 3e-4, a two-pass form near 1e-5"""
    from seedvc_amd import _lib
    g = torch.Generator().manual_seed(D)
    rows = 37                                                # not a multiple of the 4 rows of a workgroup
    x = 100.0 + torch.randn(rows, D, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y = torch.empty_like(xd)
    _lib.check(_lib.lib().svc_op_layernorm(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(y), rows, D, 1e-5, _lib.stream_ptr()))
    want = torch.nn.functional.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    e = (y.cpu().double() - want).abs().max().item()
    print(f"layernorm D={D}: max |device - float64| = {e:.3e} (bound 1e-4)")
    assert e <= 1e-4


# ------------------------------------------------------------------------------------------------ 2. mel seam
def test_mel_seam(small):
    k = WC.case("S")
    P, lens = k["cfg"]["max_source_positions"], k["lens"]                 # (20 000, 32 000, 513)
    buf = torch.full((3, 32000), float("nan"))
    for b, n in enumerate(lens):
        buf[b, :n] = k["waves"][b]
    m = small[0]
    got = m.mel(buf.to(DEV), lens).cpu()
    assert got.shape == (3, 80, 2 * P) and torch.isfinite(got).all()
    for b, n in enumerate(lens):
        want = k["feats"][b]
        mean_log = (got[b].double() - want).abs().mean().item()
        # back to the linear scale where the clamp to max - 8 is not active: relative to the frame's largest value
        pw = WC.mel_power(k["waves"][b], P, k["basis"])
        lin_got = 10.0 ** (got[b].double() * 4.0 - 4.0)
        live = (4.0 * want - 4.0) > (4.0 * want.max() - 4.0) - 8.0 + 1e-6
        rel = ((lin_got - pw).abs() * live / pw.max(dim=0, keepdim=True).values.clamp(min=1e-30)).max().item()
        print(f"mel seam clip {b} ({n} samples): mean |log-mel diff| = {mean_log:.3e} (bound 1e-4), linear rel = {rel:.3e} (bound 1e-4)")
        assert mean_log <= 1e-4 and rel <= 1e-4
        alone = m.mel(buf[b:b + 1, :max(n, 1)].to(DEV), [n]).cpu()
        assert torch.equal(alone[0], got[b]), f"clip {b} differs from its one-clip call"
    zero = m.mel(torch.zeros(1, 4000, device=DEV), [4000]).cpu()
    assert (zero == -1.5).all()


# ------------------------------------------------------------------------------------------------ 3. encoder
def _encode_checks(m, name, B, precision):
    k = WC.case(name)
    c = k["cfg"]
    feats = k["feats"][:B].float()
    got = m.encode(feats.to(DEV)).cpu()
    assert got.shape == (B, c["max_source_positions"], c["d_model"]) and torch.isfinite(got).all()
    e = WC.rms(got, k["ref"][:B])                            # every window is computed alone: the first B rows of the cached reference
    print(f"encoder {name} B={B} precision {precision}: RMS(device - float64) = {e:.3e} (bound {WC.RMS_BOUND[precision]:.1e})")
    assert e <= WC.RMS_BOUND[precision]
    return feats, got


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_encoder_small(small, B, precision):
    m = small[precision]
    feats, got = _encode_checks(m, "S", B, precision)
    if B == 3:                                               # a window's rows: alone, among companions, reversed, in groups of one
        alone = m.encode(feats[1:2].to(DEV)).cpu()
        rev = m.encode(feats.flip(0).to(DEV)).cpu()
        m.set_window_group(1)
        one = m.encode(feats.to(DEV)).cpu()
        m.set_window_group(0)
        assert torch.equal(alone[0], got[1]) and torch.equal(rev.flip(0), got) and torch.equal(one, got)


@pytest.mark.parametrize("precision", [0, 1])
def test_encoder_whisper_small(precision):
    m = _model("F", precision)
    _encode_checks(m, "F", 1, precision)
    m.close()


def test_attention_form_does_not_change_with_the_group():
    """whisper-small geometry crosses the grid-size threshold of the attention launch between one and two windows: the handle
    pins the form, so a window's bits stay the same (checked on a 1500-row, 12-head, 1-layer model)"""
    from seedvc_amd.whisper import WhisperContent
    c = dict(WC.CFG_F, n_layers=1, ffn_dim=768)
    sd = WC.make_state_dict(c, seed=5)
    m = WhisperContent(sd, cfg=c, device=DEV, precision=1)
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(3, 80, 3000, generator=g) * 0.5
    got = m.encode(feats.to(DEV)).cpu()
    alone = m.encode(feats[2:3].to(DEV)).cpu()
    assert torch.isfinite(got).all() and torch.equal(alone[0], got[2])
    m.close()


# ------------------------------------------------------------------------------------------------ 4. one call
@pytest.mark.parametrize("precision", [0, 1])
def test_one_call_matches_the_driver_loop(small, clips, one_call, precision):
    k = WC.case("S")
    m = small[precision]
    S, rows = one_call[precision]
    S = S.cpu()
    lib_rows = [m.rows(n, OV) for n in CLIP_LENS]
    assert rows == lib_rows == [63, 100, 101, 181] and S.shape == (4, 181, 128)
    for b, n in enumerate(CLIP_LENS):
        want = WC.driver_content(k["sd"], k["cfg"], clips[b, :n], OV, k["basis"])
        assert want.shape == (rows[b], 128)
        e = WC.rms(S[b, :rows[b]], want)
        print(f"one call, clip {b} ({n} samples, {rows[b]} rows), precision {precision}: RMS = {e:.3e} (bound {WC.RMS_BOUND[precision]:.1e})")
        assert torch.isfinite(S[b]).all() and e <= WC.RMS_BOUND[precision]
        assert (S[b, rows[b]:] == 0).all()


def test_one_call_rows_do_not_depend_on_companions(small, clips, one_call):
    m = small[1]
    S, rows = one_call[1]
    for b, n in enumerate(CLIP_LENS):
        alone, r1 = m.content_batch(clips[b:b + 1, :n].to(DEV), [n], overlap_s=OV * 320 / 16000)
        assert r1 == [rows[b]] and torch.equal(alone[0], S[b, :rows[b]])
    m.set_window_group(2)                                    # 7 windows in groups of 2: a clip's windows fall into different groups
    S2, _ = m.content_batch(clips.to(DEV), CLIP_LENS, overlap_s=OV * 320 / 16000)
    m.set_window_group(0)
    assert torch.equal(S2, S)
    sem = m.semantic_fn(clips[0:1, :CLIP_LENS[0]])
    assert sem.shape == (1, CLIP_LENS[0] // 320 + 1, 128) and torch.equal(sem[0], S[0, :rows[0]])


def test_one_call_argument_errors(small, clips):
    from seedvc_amd import _lib
    m = small[1]
    out = torch.empty(4, 100, 128, device=DEV)
    w = clips.to(DEV)
    rc = _lib.lib().svc_whisper_content(m._h, _lib.ptr(w), _lib.i32_host(list(CLIP_LENS)), 4, 60000, OV, _lib.ptr(out), 100, _lib.stream_ptr())
    assert rc != 0 and b"Rmax" in _lib.lib().svc_last_error()
    rc = _lib.lib().svc_whisper_content(m._h, _lib.ptr(w), _lib.i32_host(list(CLIP_LENS)), 4, 60000, 100, _lib.ptr(out), 100, _lib.stream_ptr())
    assert rc != 0 and b"overlap_rows" in _lib.lib().svc_last_error()


# ------------------------------------------------------------------------------------------------ 5. content_conditions
def test_content_conditions_is_the_three_calls(small, clips):
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
