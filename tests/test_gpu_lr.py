"""GPU parity of the length regulator through the C ABI: `svc_lr_forward` vs the oracle and the
committed outputs of the reference's `InterpolateRegulator` (v1 continuous +- f0, v2 discrete, v2 embedding-only)."""
import pytest
import torch

import cases
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _model(c, sd):
    from seedvc_amd.length_regulator import InterpolateRegulator
    return InterpolateRegulator(c, sd, "cuda:0")


@pytest.mark.parametrize("name", list(cases.LR_CASES))
def test_lr_matches_reference_outputs(name, golden):
    c, sd, x, ylen, f0, meta = cases.lr_case(name)
    m = _model(c, sd)
    res = m(x.cuda(), ylens=torch.LongTensor([ylen]), n_quantizers=3, f0=None if f0 is None else f0.cuda())
    assert len(res) == (5 if c["version"] == 1 else 2)
    y = res[0].cpu()
    assert res[1].tolist() == [ylen if c["n_convs"] else min(ylen, meta["tin"])]
    ref_o = O.lr_forward(sd, c, x, ylen, f0)
    assert y.shape == ref_o.shape
    err_o = (y - ref_o).abs().max().item()
    g = torch.from_numpy(golden[name + ".out"])
    err_g = ((y[:, ::4] if name.endswith("_full") else y) - g).abs().max().item()
    print(f"{name}: max|hip - oracle| {err_o:.2e}  max|hip - reference| {err_g:.2e}")
    assert err_o < 5e-5 and err_g < 5e-5          # fp32 MFMA contractions, fp32 elementwise; |out| ~ 0.5


def test_lr_batch_is_independent_utterances():
    """Ragged batch: own input length, output length and f0 length per utterance; one empty utterance."""
    c, sd, _, _, _, _ = cases.lr_case("lr_base_r")
    m = _model(c, sd)
    tins, ylens, tf0s = [31, 12, 20, 9], [37, 40, 11, 0], [45, 30, 45, 8]
    B, Tin, Tf = len(tins), max(tins), max(tf0s)
    x = cases.randn("lrb.x", 5, B, Tin, c["in_channels"])
    f0 = 80.0 + 700.0 * cases.rand("lrb.f0", 5, B, Tf)
    out, olens, *_ = m(x.cuda(), ylens=torch.LongTensor(ylens), f0=f0.cuda(), in_lens=tins, f0_lens=tf0s)
    out = out.cpu()
    assert out.shape == (B, max(ylens), c["out_channels"]) and olens.tolist() == ylens
    for b in range(B):
        if ylens[b] == 0:
            assert out[b].abs().max().item() == 0.0
            continue
        ref = O.lr_forward(sd, c, x[b:b + 1, :tins[b]], ylens[b], f0[b:b + 1, :tf0s[b]])
        assert (out[b, :ylens[b]] - ref[0]).abs().max().item() < 5e-5
        assert out[b, ylens[b]:].abs().max().item() == 0.0 if ylens[b] < max(ylens) else True


@pytest.mark.parametrize("tin,ylen", [(26, 22), (14, 46), (21, 69), (3, 123)])
@pytest.mark.parametrize("name", ["lr_base_r", "lr_v2_r"])
def test_lr_on_pairs_where_float_and_integer_index_differ(name, tin, ylen):
    """The nearest index is the fp32 formula, not t * tin // ylen: pairs on which the two differ (lr_cases.sensitive_pairs), for
    the content (features and tokens) and, with an f0 track of tin frames, for tf0 -> ylen.  A wrong index swaps a whole row."""
    import lr_cases
    assert (tin, ylen) in lr_cases.sensitive_pairs()
    c, sd, _, _, _, _ = cases.lr_case(name)
    tag = f"lrp.{name}.{tin}.{ylen}"
    if c["is_discrete"]:
        x = (cases.rand(tag + ".tok", 3, 1, tin) * c["codebook_size"]).long().clamp(max=c["codebook_size"] - 1)
    else:
        x = cases.randn(tag + ".x", 3, 1, tin, c["in_channels"])
    f0 = None
    if c["f0_condition"]:
        f0 = 60.0 + 900.0 * cases.rand(tag + ".f0", 3, 1, tin)
        assert not bool(lr_cases.f0_judgement(f0[0], c["n_f0_bins"])[1].any())          # no bin of this track is a rounding decision
    out = _model(c, sd)(x.cuda(), ylens=torch.LongTensor([ylen]), f0=None if f0 is None else f0.cuda())[0].cpu()
    ref = O.lr_forward(sd, c, x, ylen, f0)
    assert out.shape == ref.shape and (out - ref).abs().max().item() < 5e-5


def _ragged_batch(pad):
    c, sd, _, _, _, _ = cases.lr_case("lr_base_r")
    tins, ylens, tf0s = [31, 12, 20, 9, 26], [37, 40, 11, 0, 22], [45, 30, 45, 8, 26]
    B, Tin, Tf = len(tins), max(tins), max(tf0s)
    x = cases.randn("lrb.x", 5, B, Tin, c["in_channels"])
    f0 = 80.0 + 700.0 * cases.rand("lrb.f0", 5, B, Tf)
    for b in range(B):
        x[b, tins[b]:] = pad
        f0[b, tf0s[b]:] = pad
    return c, sd, x, f0, tins, ylens, tf0s


def test_lr_batch_ignores_nan_padding_and_repeats_bit_for_bit():
    """NaN in x beyond in_lens and in f0 beyond f0_lens; two calls of the same batch are the same bits; each utterance alone is
    its batch row, bit for bit (the GroupNorm sums are folded in a fixed order)."""
    c, sd, x, f0, tins, ylens, tf0s = _ragged_batch(float("nan"))
    m = _model(c, sd)
    kw = dict(ylens=torch.LongTensor(ylens), in_lens=tins, f0_lens=tf0s)
    out = m(x.cuda(), f0=f0.cuda(), **kw)[0].cpu()
    again = m(x.cuda(), f0=f0.cuda(), **kw)[0].cpu()
    assert torch.equal(out, again) and bool(torch.isfinite(out).all())
    for b in range(len(tins)):
        assert out[b, ylens[b]:].abs().max().item() == 0.0 if ylens[b] < max(ylens) else True
        if ylens[b] == 0:
            continue
        ref = O.lr_forward(sd, c, x[b:b + 1, :tins[b]], ylens[b], f0[b:b + 1, :tf0s[b]])
        assert (out[b, :ylens[b]] - ref[0]).abs().max().item() < 5e-5
        alone = m(x[b:b + 1, :tins[b]].cuda(), ylens=torch.LongTensor([ylens[b]]), f0=f0[b:b + 1, :tf0s[b]].cuda())[0].cpu()
        assert torch.equal(alone[0], out[b, :ylens[b]]), b


def test_lr_feeds_the_sampler():
    """content -> length regulator -> `mu` -> CFM sampler, all on the device, against the oracle chain."""
    from seedvc_amd.cfm import CFM
    cfg, dsd, inp, meta = cases.dit_case("tiny_r")
    lc = cases.specs.lr_config("tiny", channels=cfg["Dc"], in_channels=64)
    lsd = cases.weights.make_state_dict(cases.specs.lr_state_spec(lc), seed=91, prefix="lr.")
    T = inp["mu"].shape[1]
    P = inp["prompt"].shape[-1]
    content = cases.randn("lrs.c", 9, 1, 15, 64)
    mu = _model(lc, lsd)(content.cuda(), ylens=torch.LongTensor([T]))[0]
    mel = CFM(cfg, dsd, "cuda:0").inference(mu, torch.LongTensor([T]), inp["prompt"].cuda(), inp["style"].cuda(), None, 3,
                                            inference_cfg_rate=0.7, z=inp["z"].cuda()).cpu()
    mu_o = O.lr_forward(lsd, lc, content, T)
    ref = O.cfm_sample(dsd, cfg, inp["z"], T, inp["prompt"], mu_o, inp["style"], 3, 0.7)
    assert (mel - ref)[:, :, P:].abs().mean().item() < 1e-3
