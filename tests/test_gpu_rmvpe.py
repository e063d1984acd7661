"""GPU parity of the RMVPE pitch extractor (csrc/rmvpe.hip): every stage against the float64 restatement of rmvpe_cases.py
-- the network alone on a shallow and on the full-size model, a ragged batch whose padding is NaN, the mel and decode seams,
audio to F0 end to end -- and the drivers' pitch step (`svc_f0_adjust`, `pipeline.f0_conditions`) against their torch lines.
Each float64 reference is computed once per clip (rmvpe_cases caches it) and shared by the tests that need it."""
import numpy as np
import pytest
import torch

import rmvpe_cases as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
FR = R.CLIP_FRAMES                                           # (70, 32, 160, 33)


def _device_model(kind):
    from seedvc_amd.rmvpe import RMVPE
    c, sd, _ = R.model(kind)
    return RMVPE(sd, mel_basis=R.basis(), device=DEV, cfg=c)


@pytest.fixture(scope="module")
def full():
    return _device_model("full")


@pytest.fixture(scope="module")
def ragged(full):
    """the ragged salience call on the four clips (NaN above each end), shared by the tests below"""
    mel = R.mel_batch()
    return mel, full.salience(mel.to(DEV), FR).cpu()


def _sal_err(got, kind, cid):
    want = R.clip_salience(kind, cid, R.CLIP_LENS[cid])
    return (got.double() - want).abs().max().item()


def test_shallow_net_salience():
    """one level, one block, one intermediate layer, T = 32: pool, transposed conv, concatenation and GRU without the depth"""
    m = _device_model("shallow")
    mel = R.mel_batch((R.CLIP_LENS[1],), ids=[1])
    got = m.salience(mel.to(DEV)).cpu()[0]
    e = _sal_err(got, "shallow", 1)
    print(f"shallow net, 32 frames: max |salience - float64| = {e:.3e} (bound {R.SALIENCE_TOL:.1e})")
    assert got.shape == (32, 360) and torch.isfinite(got).all()
    assert e <= R.SALIENCE_TOL


@pytest.mark.parametrize("cid", [1, 3, 0])                    # 32 frames (no padding), 33 (pads to 64), 70 (pads to 96)
def test_full_net_single_clip(full, cid):
    mel = R.mel_batch((R.CLIP_LENS[cid],), ids=[cid])
    got = full.salience(mel.to(DEV)).cpu()[0]
    e = _sal_err(got, "full", cid)
    print(f"full-size net, {FR[cid]} frames: max |salience - float64| = {e:.3e} (bound {R.SALIENCE_TOL:.1e})")
    assert got.shape == (FR[cid], 360) and torch.isfinite(got).all()
    assert e <= R.SALIENCE_TOL


def test_ragged_rows_equal_the_one_clip_call_and_float64(full, ragged):
    mel, out = ragged
    assert out.shape == (4, max(FR), 360) and torch.isfinite(out).all()
    for b, n in enumerate(FR):
        one = full.salience(mel[b:b + 1, :, :n].to(DEV)).cpu()[0]
        e = _sal_err(out[b, :n], "full", b)
        print(f"ragged row {b} ({n} frames): max |salience - float64 alone| = {e:.3e}; equal to the one-clip call: {torch.equal(out[b, :n], one)}")
        assert torch.equal(out[b, :n], one)                  # bit for bit
        assert e <= R.SALIENCE_TOL
        assert (out[b, n:] == 0).all()


def test_ragged_rows_do_not_depend_on_neighbours_order_or_grouping(full, ragged):
    mel, out = ragged
    rev = full.salience(mel.flip(0).to(DEV), FR[::-1]).cpu().flip(0)
    assert torch.equal(rev, out)                             # reversed batch order: identical bits
    other = R.mel_batch(ids=[9, 1, 2, 3])                    # row 0 replaced by another clip of the same length
    swapped = full.salience(other.to(DEV), FR).cpu()
    assert torch.equal(swapped[1:], out[1:]) and torch.isfinite(swapped).all()
    assert (swapped[0] - out[0]).abs().max().item() > 1e-3   # and row 0 is another clip
    full.set_plane_budget(1)                                 # forces groups of one clip
    try:
        grouped = full.salience(mel.to(DEV), FR).cpu()
    finally:
        full.set_plane_budget(0)
    assert torch.equal(grouped, out)


def test_mel_seam(full):
    waves = R.wave_batch()
    got = full.mel(waves.to(DEV), R.CLIP_LENS).cpu()
    assert got.shape == (4, R.N_MELS, max(FR)) and torch.isfinite(got).all()
    for b, n in enumerate(R.CLIP_LENS):
        want = R.clip_mel(b, n)
        g = got[b, :, :FR[b]].double()
        l1 = (g - want).abs().mean().item()
        lin = ((g.exp() - want.exp()).abs() / want.exp().amax(dim=0, keepdim=True)).max().item()
        print(f"mel row {b} ({n} samples, {FR[b]} frames): mean |log-mel diff| {l1:.2e}, linear error / frame max {lin:.2e}, "
              f"max |log-mel diff| {(g - want).abs().max().item():.2e}")
        assert l1 < R.MEL_TOL and lin < R.MEL_TOL
        assert (got[b, :, FR[b]:] == 0).all()
        one = full.mel(waves[b:b + 1, :n].to(DEV), [n]).cpu()
        assert torch.equal(one[0], got[b, :, :FR[b]])


def _synthetic_salience():
    """(2, 12, 360): smooth bumps whose maxima sit below, at and above 0.03, at bin 0, at bin 359, and an exact tie"""
    g = np.random.default_rng(5)
    s = (g.random((2, 12, 360)) * 0.01).astype(np.float32)
    k = np.arange(360)
    for i, (centre, peak) in enumerate([(100, 0.9), (0, 0.8), (359, 0.7), (2, 0.5), (357, 0.6), (180, 0.02), (40, 0.2), (300, 0.031)]):
        s[0, i] += (peak * np.exp(-0.5 * ((k - centre) / 2.0) ** 2)).astype(np.float32)
    s[0, 8] = 0.0
    s[0, 8, 77] = 0.03                                       # the maximum is exactly the threshold: unvoiced
    s[0, 9] = 0.001
    s[0, 9, 50] = s[0, 9, 200] = 0.7                         # an exact tie: the first maximum wins
    s[0, 10] = 0.0
    s[0, 10, 5] = np.float32(0.03) + np.float32(1e-6)        # just above
    s[0, 11] = 0.0
    s[0, 11, 0] = 0.4                                        # a lone peak at the first bin
    s[1, :5] = s[0, :5][::-1]
    s[1, 5:] = np.nan                                        # above row 1's five frames: never read
    return torch.from_numpy(s)


def test_decode_seam(full):
    sal = _synthetic_salience()
    lens = [12, 5]
    got = full.decode(sal.to(DEV), lens, thred=0.03).cpu().numpy()
    for b, n in enumerate(lens):
        want = R.np_decode(sal[b, :n].numpy(), 0.03)
        voiced = want > 0
        rel = np.abs(got[b, :n][voiced] - want[voiced]) / want[voiced]
        print(f"decode row {b}: {voiced.sum()} voiced of {n}, max relative F0 error {rel.max():.2e}")
        assert (got[b, :n][~voiced] == 0).all()              # unvoiced frames are exactly 0
        assert rel.max() < 1e-5
        assert (got[b, n:] == 0).all()
    w0 = R.np_decode(sal[0].numpy(), 0.03)
    assert w0[5] == 0 and w0[8] == 0 and w0[7] > 0 and w0[10] > 0          # below, at and above the threshold are all present
    assert abs(w0[9] - 10 * 2 ** ((20 * 50 + R.CENTS0) / 1200)) / w0[9] < 1e-3   # the tie went to bin 50


@pytest.mark.parametrize("rows", [(0, 2)])                    # the 70- and the 160-frame clip in one ragged call
def test_end_to_end_f0(full, rows):
    lens = [R.CLIP_LENS[b] for b in rows]
    waves = R.wave_batch(lens, ids=list(rows))
    f0 = full.f0_batch(waves.to(DEV), lens, thred=0.03).cpu().numpy()
    assert f0.shape == (2, max(FR[b] for b in rows)) and np.isfinite(f0).all()
    dev_arg = full.salience(full.mel(waves.to(DEV), lens), [FR[b] for b in rows]).argmax(dim=-1).cpu().numpy()
    for i, b in enumerate(rows):
        n = FR[b]
        sal = R.clip_salience("full", b, R.CLIP_LENS[b], False)          # the all-float64 chain: audio -> mel -> network
        want = R.np_decode(sal.numpy(), 0.03)
        keep = R.top2_margin(sal) >= 10 * R.SALIENCE_TOL
        left_out = int((~keep).sum())
        got = f0[i, :n]
        bins_equal = dev_arg[i, :n] == np.argmax(sal.numpy(), axis=1)
        rel = np.abs(got - want)[keep] / want[keep]
        print(f"clip {b} ({n} frames): {left_out} frames left out (top-two margin < {10 * R.SALIENCE_TOL:.1e}); on the rest "
              f"max relative F0 error {rel.max():.2e}, arg-max bin equal on {int(bins_equal[keep].sum())} of {int(keep.sum())}")
        assert left_out <= 0.2 * n
        assert (want[keep] > 0).all() and (got[keep] > 0).all()
        assert bins_equal[keep].all()
        assert rel.max() < 1e-4
        assert (f0[i, n:] == 0).all()
    one = full.infer_from_audio(waves[0, :lens[0]].numpy(), thred=0.03)  # the reference's signature: numpy in, numpy out
    assert isinstance(one, np.ndarray) and one.shape == (FR[rows[0]],) and np.array_equal(one, f0[0, :FR[rows[0]]])


@pytest.mark.parametrize("auto", [True, False])
def test_f0_adjust_against_the_drivers_lines(auto):
    from seedvc_amd.rmvpe import f0_adjust
    alt, alt_lens, ori, ori_lens, semis = R.f0_tracks()
    out, med = f0_adjust(alt.to(DEV), alt_lens, ori.to(DEV), ori_lens, auto, semis, return_medians=True)
    out, med = out.cpu(), med.cpu()
    assert torch.isfinite(out).all()
    for b in range(alt.shape[0]):
        a, o = alt[b, :alt_lens[b]], ori[b, :ori_lens[b]]
        want, m_alt, m_ori = R.ref_f0_adjust(a, o, auto, semis[b])
        got = out[b, :alt_lens[b]]
        rel = ((got - want).abs() / want).max().item()
        mrel = max(abs(med[b, 0].item() - m_alt.item()) / max(abs(m_alt.item()), 1e-30) if m_alt.item() else abs(med[b, 0].item()),
                   abs(med[b, 1].item() - m_ori.item()) / max(abs(m_ori.item()), 1e-30) if m_ori.item() else abs(med[b, 1].item()))
        print(f"row {b} ({int((a > 1).sum())} / {int((o > 1).sum())} voiced, {semis[b]:+} semitones, auto {auto}): "
              f"median rel err {mrel:.2e}, output rel err {rel:.2e}")
        assert mrel < 1e-6 and rel < 1e-5
        assert ((got[a <= 1] - 1e-5).abs() < 1e-9).all()     # unvoiced frames become 1e-5, not 0
        assert (out[b, alt_lens[b]:] == 0).all()


def test_f0_conditions(full):
    from seedvc_amd import pipeline
    src_ids, ref_ids = (0, 3), (1, 2)
    src_lens, ref_lens = [R.CLIP_LENS[i] for i in src_ids], [R.CLIP_LENS[i] for i in ref_ids]
    src, ref = R.wave_batch(src_lens, ids=list(src_ids)).to(DEV), R.wave_batch(ref_lens, ids=list(ref_ids)).to(DEV)
    f0_ori, ori_frames, shifted, alt_frames = pipeline.f0_conditions(full, src, src_lens, ref, ref_lens, True, [2.0, -1.0])
    assert ori_frames == [FR[i] for i in ref_ids] and alt_frames == [FR[i] for i in src_ids]
    assert f0_ori.shape == (2, max(ori_frames)) and shifted.shape == (2, max(alt_frames))
    f0_alt = full.f0_batch(src, src_lens).cpu()
    assert torch.equal(f0_ori.cpu(), full.f0_batch(ref, ref_lens).cpu())
    for b in range(2):
        want, _, _ = R.ref_f0_adjust(f0_alt[b, :alt_frames[b]], f0_ori[b, :ori_frames[b]].cpu(), True, [2.0, -1.0][b])
        rel = ((shifted[b, :alt_frames[b]].cpu() - want).abs() / want).max().item()
        print(f"pair {b}: shifted F0 against the drivers' lines on the device tracks: max rel err {rel:.2e}")
        assert rel < 1e-5
