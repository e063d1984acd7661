"""GPU parity of the ragged reference front-end: a batch of reference clips of different lengths through the log-mel, the
Kaldi fbank and CAMPPlus in one call each (`svc_mel_forward_ragged`, `svc_kaldi_fbank_ragged`, `svc_campplus_forward_ragged`),
every row against the oracle run alone on the clip and against the existing one-clip calls.  The padding of every batch is
NaN (frontend_ragged_cases.py): nothing at or above a clip's end may be read as a value."""
import pytest
import torch

import cases
import frontend_ragged_cases as R
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------- CAMPPlus
@pytest.fixture(scope="module")
def cp_r():
    from seedvc_amd.campplus import CAMPPlus
    c, sd, _ = cases.campplus_case(R.CP_MODEL)
    m = CAMPPlus(c, sd, DEV)
    feat = R.cp_batch(c)
    return c, sd, m, feat, m(feat.to(DEV), lens=R.CP_LENS).cpu()


def test_campplus_ragged_rows_equal_oracle_alone(cp_r):
    c, sd, m, feat, out = cp_r
    assert out.shape == (len(R.CP_LENS), c["embedding_size"]) and torch.isfinite(out).all()
    for b, n in enumerate(R.CP_LENS):
        want = O.campplus_forward(sd, c, feat[b:b + 1, :n])
        e = (out[b:b + 1] - want).abs().max().item()
        one = m(feat[b:b + 1, :n].to(DEV)).cpu()
        e1 = (out[b:b + 1] - one).abs().max().item()
        print(f"clip {b} ({n} frames): vs oracle alone {e:.2e}, vs the one-clip call {e1:.2e} (equal {torch.equal(out[b:b + 1], one)})")
        assert e < 2e-5                                   # fp32 MFMA throughout: the project's CAMPPlus bound
        assert e1 < 1e-5                                  # the existing batch-independence figure


def test_campplus_ragged_rows_do_not_depend_on_neighbours(cp_r):
    c, sd, m, feat, out = cp_r
    B = len(R.CP_LENS)
    again = m(feat.to(DEV), lens=R.CP_LENS).cpu()
    assert torch.equal(out, again)                        # a second call: identical bits
    rev = m(feat.flip(0).to(DEV), lens=R.CP_LENS[::-1]).cpu().flip(0)
    e = (rev - out).abs().max().item()
    other = R.cp_batch(c, ids=[9] + list(range(1, B)))    # row 0 replaced by another 260-frame clip
    swapped = m(other.to(DEV), lens=R.CP_LENS).cpu()
    e2 = (swapped[1:] - out[1:]).abs().max().item()
    print(f"reversed order: max |diff| {e:.2e}; row 0 replaced: rows 1.. move by {e2:.2e}, row 0 by {(swapped[0] - out[0]).abs().max():.2e}")
    assert e < 1e-5 and e2 < 1e-5
    assert (swapped[0] - out[0]).abs().max().item() > 1e-3      # and row 0 is another voice
    assert torch.isfinite(rev).all() and torch.isfinite(swapped).all()


def test_campplus_ragged_equal_lengths_is_the_plain_call(cp_r):
    c, sd, m, _, _ = cp_r
    _, _, feat = cases.campplus_case(R.CP_MODEL)          # (2, 57, 80), no padding
    plain = m(feat.to(DEV))
    assert torch.equal(m(feat.to(DEV), lens=[feat.shape[1]] * feat.shape[0]), plain)
    with pytest.raises(NotImplementedError):
        m(feat.to(DEV), x_lens=[57, 57])                  # the reference's keyword still raises
    with pytest.raises(RuntimeError, match="lens"):
        m(feat.to(DEV), lens=[57, 58])


def test_campplus_ragged_full_model(golden):
    from seedvc_amd.campplus import CAMPPlus
    c, sd, feat = R.cp_full_batch()
    m = CAMPPlus(c, sd, DEV)
    out = m(feat.to(DEV), lens=R.CP_FULL_LENS).cpu()
    assert torch.isfinite(out).all()
    e0 = (out[0:1] - torch.from_numpy(golden["campplus_full.emb"])).abs().max().item()
    n = R.CP_FULL_LENS[1]
    e1 = (out[1:2] - O.campplus_forward(sd, c, feat[1:2, :n])).abs().max().item()
    print(f"campplus_full: row 0 (500 frames) vs the reference's output {e0:.2e}; row 1 ({n} frames) vs oracle alone {e1:.2e}")
    assert e0 < 2e-5 and e1 < 2e-5


# -------------------------------------------------------------------------------------------------------------- log-mel
def _mel_fn(c, basis):
    from seedvc_amd.audio import MelSpectrogram
    return MelSpectrogram(c["n_fft"], c["n_mels"], c["sr"], c["hop"], c["n_fft"], c["fmin"], c["fmax"], center=False, mel_basis=basis)


@pytest.mark.parametrize("name", ["mel_r", "mel_22k"])
def test_mel_ragged_rows_equal_oracle_alone(name, golden):
    c, y, basis, lens = R.mel_batch(name)
    fe = _mel_fn(c, basis)
    pad_value = -3.25
    m = fe(y.to(DEV), lens=lens, pad_value=pad_value).cpu()
    assert m.shape == (len(lens), c["n_mels"], max(lens) // c["hop"])
    for b, n in enumerate(lens):
        fr = n // c["hop"]
        o = O.mel_spectrogram(y[b:b + 1, :n], basis, c["n_fft"], c["hop"], c["n_fft"])
        assert o.shape[-1] == fr
        l1 = (m[b:b + 1, :, :fr] - o).abs().mean().item()
        one = fe(y[b:b + 1, :n].to(DEV)).cpu()
        print(f"{name}: clip {b} ({n} samples, {fr} frames): mean |diff| vs oracle alone {l1:.2e}; equal to the one-clip call: "
              f"{torch.equal(m[b:b + 1, :, :fr], one)}")
        assert l1 < 1e-4                                  # the existing criterion (test_mel_matches_reference_outputs)
        assert torch.equal(m[b:b + 1, :, :fr], one)       # a frame's GEMM rows do not depend on its neighbours
        assert (m[b, :, fr:] == pad_value).all()
    if name == "mel_22k":                                 # row 0 is the golden clip: the reference's own output
        ref = torch.from_numpy(golden[name + ".mel"])
        g = m[0:1]
        assert g.shape == ref.shape
        lin_err = ((g.exp() - ref.exp()).abs() / ref.exp().amax(dim=1, keepdim=True).clamp_min(1e-3)).max().item()
        log_err, l1 = (g - ref).abs().max().item(), (g - ref).abs().mean().item()
        print(f"{name}: row 0 vs the reference's output: log-mel max err {log_err:.2e}, mean {l1:.2e}, relative linear err {lin_err:.2e}")
        assert lin_err < 1e-4 and l1 < 1e-4 and log_err < 2e-2
    z = fe(y.to(DEV), lens=lens).cpu()                    # the default pad value is zero
    assert all((z[b, :, n // c["hop"]:] == 0).all() for b, n in enumerate(lens))


def test_mel_ragged_equal_lengths_is_the_plain_call():
    c, y, basis = cases.mel_case("mel_r")
    fe = _mel_fn(c, basis)
    plain = fe(y.to(DEV))
    assert torch.equal(fe(y.to(DEV), lens=[y.shape[1]] * y.shape[0]), plain)
    with pytest.raises(RuntimeError, match="lens"):
        fe(y.to(DEV), lens=[400, 24])                     # a clip no longer than the reflect padding


# ---------------------------------------------------------------------------------------------------------- Kaldi fbank
@pytest.fixture(scope="module")
def fb():
    from seedvc_amd.campplus import CAMPPlus
    c, sd, _ = cases.campplus_case(R.CP_MODEL)
    m = CAMPPlus(c, sd, DEV)
    y = R.fbank_batch()
    return c, sd, m, y, m.fbank_batch(y.to(DEV), R.FB_LENS).cpu()


def test_fbank_ragged_rows_equal_restatement_alone(fb):
    c, sd, m, y, got = fb
    assert got.shape == (len(R.FB_LENS), R.fbank_frames(max(R.FB_LENS)), c["feat_dim"])
    for b, n in enumerate(R.FB_LENS):
        nb = R.fbank_frames(n)
        ref = O.kaldi_fbank(y[b:b + 1, :n])
        assert ref.shape == (nb, c["feat_dim"])
        d = got[b, :nb] - ref
        live = ref > -14.0                                # bins well above the log floor
        err = d[live].abs().max().item()
        floor = d[~live].abs().max().item() if (~live).any() else 0.0
        one = m.fbank(y[b, :n].to(DEV)).cpu()
        print(f"fbank clip {b} ({n} samples, {nb} frames): max |diff| over live bins {err:.3e}, floor bins {floor:.3e}; equal to the "
              f"one-clip call: {torch.equal(got[b, :nb], one)}")
        assert err < 2e-3 and floor < 0.5                 # the existing criteria (test_kaldi_fbank_vs_restatement)
        assert torch.equal(got[b, :nb], one)
        assert (got[b, nb:] == 0).all()


def test_fbank_ragged_subtract_mean(fb):
    c, sd, m, y, raw = fb
    got = m.fbank_batch(y.to(DEV), R.FB_LENS, subtract_mean=True).cpu()
    assert torch.equal(got, m.fbank_batch(y.to(DEV), R.FB_LENS, subtract_mean=True).cpu())
    for b, n in enumerate(R.FB_LENS):
        nb = R.fbank_frames(n)
        x = raw[b, :nb].double()
        want = (x - x.mean(dim=0, keepdim=True)).float()
        # fp32 sum of nb terms of magnitude <= max|x|, then one subtraction: nb roundings of 2^-24 relative to max|x|
        bound = nb * 2.0 ** -24 * raw[b, :nb].abs().max().item()
        e = (got[b, :nb] - want).abs().max().item()
        print(f"fbank clip {b} ({nb} frames): mean-normalised vs torch {e:.3e} (bound {bound:.3e})")
        assert e <= bound
        assert (got[b, nb:] == 0).all()


# --------------------------------------------------------------------------------------- style_batch, enrol_references
def test_style_batch_and_enrol_references(fb):
    from seedvc_amd.cfm import CFM
    from seedvc_amd.pipeline import HotPath, enrol_references
    from seedvc_amd.vocoder import HiFT
    c, sd, m, y16, _ = fb
    lens16 = list(R.FB_LENS[:2])                          # the two clips with at least 8 frames
    w16 = y16[:2].to(DEV)
    style = m.style_batch(w16, lens16)
    assert style.shape == (2, c["embedding_size"])
    for b, n in enumerate(lens16):
        ref = O.kaldi_fbank(y16[b:b + 1, :n])
        want = O.campplus_forward(sd, c, (ref - ref.mean(dim=0, keepdim=True))[None])
        e = (style[b:b + 1].cpu() - want).abs().max().item()
        e1 = (style[b:b + 1] - m.style(w16[b, :n])).abs().max().item()
        print(f"style clip {b} ({n} samples): vs the oracle chain {e:.2e}, vs CAMPPlus.style alone {e1:.2e}")
        assert e < 5e-3                                   # the existing figure (fbank parity through the network)
        assert e1 < 1e-4
    cm, y, basis, lens = R.mel_batch("mel_22k")
    fe = _mel_fn(cm, basis)
    w = y.to(DEV)
    rec = enrol_references(fe, m, w, lens, w16, lens16)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")               # a warm call enqueues from host integers only
    try:
        again = enrol_references(fe, m, w, lens, w16, lens16)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert sorted(rec) == ["prompt", "prompt_lens", "style"]
    assert rec["prompt_lens"] == [n // cm["hop"] for n in lens] == [86, 35]
    assert rec["prompt"].shape == (2, cm["n_mels"], 86) and torch.equal(rec["style"], style)
    assert torch.equal(rec["prompt"], again["prompt"]) and torch.equal(rec["style"], again["style"])
    assert torch.equal(rec["prompt"], fe(w, lens=lens))
    for b, n in enumerate(lens):
        P = rec["prompt_lens"][b]
        o = O.mel_spectrogram(y[b:b + 1, :n], basis, cm["n_fft"], cm["hop"], cm["n_fft"])
        assert (rec["prompt"][b:b + 1, :, :P].cpu() - o).abs().mean().item() < 1e-4
        assert (rec["prompt"][b, :, P:] == 0).all()
    # the record is what HotPath.convert_batch_ragged takes
    cfg, dsd, _, _ = cases.dit_case("tiny_r")
    hc, vsd, _, _, _, _ = cases.hift_case("hift_r")
    assert cfg["C"] == cm["n_mels"] and cfg["style_dim"] == c["embedding_size"]
    hp = HotPath(CFM(cfg, dsd, DEV), HiFT(hc, vsd, DEV))
    S = [40, 24]
    x_lens = [p + s for p, s in zip(rec["prompt_lens"], S)]
    mu = cases.randn("fr.mu", 7, 2, max(x_lens), cfg["Dc"]).to(DEV)
    out = hp.convert_batch_ragged(mu, rec["prompt"], rec["style"], x_lens, rec["prompt_lens"], 2, 0.7)
    assert len(out) == 2
    for b, (mel, wave) in enumerate(out):
        assert mel.shape == (1, cfg["C"], S[b]) and torch.isfinite(mel).all() and torch.isfinite(wave).all()
