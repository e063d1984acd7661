"""GPU tests of the ragged HiFT call: one vocoder call for utterances of different lengths, each result being that of the
utterance run alone, and of `HotPath.convert_batch_ragged` / `convert_long_batch(ragged_vocoder=True)` on top of it.

Bounds.  Against the CPU oracle alone on each utterance's own frames, f0 and draws: waveform RMS < 1e-4 per utterance
(WAVE_RMS of test_gpu_vocoder.py), every precision; f0 is pinned to the oracle's f0 of the utterance alone because the decoder
is chaotic in f0 (test_gpu_vocoder.py), and the predictor is checked on its own within that file's 2e-5 relative bound.
Against the HIP vocoder's plain call on the utterance alone: bit for bit.  The only length-dependent kernel choice is
`Lout >= 192` (KCONV_MIN_ROWS in csrc/conv_util.h: the resident-tile / fp8-correction convs), and a ragged micro-batch never
mixes utterances for which any stage length falls on different sides of it (svc_hift::kernel_class), so every utterance runs
the kernels it runs alone: the threshold the code implies is one frame, in every precision, which is what BIT_EXACT_FROM
states.  Every comparison prints its RMS before it asserts."""
import functools

import numpy as np
import pytest
import torch

import cases
import hift_ragged_cases as R
import long_batch_cases as LB
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

DEV = "cuda:0"
WAVE_RMS = 1e-4
MEL_L1 = 1e-3
F0_REL = 2e-5
BIT_EXACT_FROM = 1           # frames; the ragged BigVGAN call holds 192 in the split modes (see the module docstring)
PRECISIONS = ["fp32", "fp16x3", "fp16p8"]


@functools.lru_cache(maxsize=None)
def _case(name=R.MODEL, lens=tuple(R.LENS)):
    c, sd, _, _, _, _ = cases.hift_case(name)
    bt = R.batch(c, sd, list(lens))                      # NaN in every padding frame, f0 slot and noise sample
    return c, sd, bt, R.ragged_reference(sd, c, bt, list(lens))


def _voc(name=R.MODEL, precision="fp16p8"):
    from seedvc_amd.vocoder import HiFT
    c, sd, _, _, _, _ = cases.hift_case(name)
    return HiFT(c, sd, DEV, precision=precision)


def _run(voc, bt, lens, f0=True, **kw):
    return voc(bt["mel"].to(DEV), f0=bt["f0"].to(DEV) if f0 else None, phase0=bt["phase0"].to(DEV), noise=bt["noise"].to(DEV),
               lens=lens, **kw)


def _alone(voc, bt, b, n, up, f0=True, **kw):
    return voc(bt["mel"][b:b + 1, :, :n].contiguous().to(DEV), f0=bt["f0"][b:b + 1, :n].contiguous().to(DEV) if f0 else None,
               phase0=bt["phase0"][b:b + 1].to(DEV), noise=bt["noise"][b:b + 1, :, :n * up].contiguous().to(DEV), **kw)


def _check_vs_alone(voc, y, bt, lens, up, what, f0=True, rows=None):
    for b in (range(len(lens)) if rows is None else rows):
        n = lens[b]
        if n == 0:
            assert (y[b] == 0).all(), f"{what}: empty utterance {b} is not an all-zero row"
            continue
        alone = _alone(voc, bt, b, n, up, f0=f0).cpu().reshape(-1)
        got = y[b, :n * up]
        e = R.rms(got, alone)
        print(f"{what}: utterance {b} ({n} frames) vs the HIP vocoder alone: RMS {e:.3e}, equal {torch.equal(got, alone)}")
        if n >= BIT_EXACT_FROM:
            assert torch.equal(got, alone), f"{what}: utterance {b} ({n} frames) differs from its run alone"


def _check_vs_oracle(y, ref, lens, up, what):
    assert y.shape == ref.shape
    assert torch.isfinite(y).all()
    for b, n in enumerate(lens):
        assert (y[b, n * up:] == 0).all(), f"{what}: utterance {b} ({n} frames): tail not zero"
        if n:
            e = R.rms(y[b, :n * up], ref[b, :n * up])
            print(f"{what}: utterance {b} ({n} frames): waveform RMS vs the oracle alone {e:.3e}")
            assert e < WAVE_RMS


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_vs_oracle_alone(precision):
    c, sd, bt, ref = _case()
    y = _run(_voc(precision=precision), bt, R.LENS).cpu()
    _check_vs_oracle(y, ref, R.LENS, R.total_up(c), f"{R.MODEL} [{precision}]")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_f0_predictor(precision):
    """f0=None: the predictor sees each utterance alone; rows of the returned f0 are zero at and above lens[b]."""
    c, sd, bt, _ = _case()
    voc = _voc(precision=precision)
    up = R.total_up(c)
    y, f0 = _run(voc, bt, R.LENS, f0=False, return_f0=True)
    y, f0 = y.cpu(), f0.cpu()
    assert f0.shape == (len(R.LENS), max(R.LENS)) and torch.isfinite(f0).all() and torch.isfinite(y).all()
    for b, n in enumerate(R.LENS):
        assert (f0[b, n:] == 0).all() and (y[b, n * up:] == 0).all()
        if n:
            want = O.hift_f0_predictor(sd, bt["mel"][b:b + 1, :, :n])[0]
            rel = ((f0[b, :n] - want).abs() / want.abs().clamp_min(1.0)).max().item()
            ya, fa = _alone(voc, bt, b, n, up, f0=False, return_f0=True)
            print(f"[{precision}] utterance {b} ({n} frames): f0 max rel err vs the oracle alone {rel:.3e}; equal to the HIP run alone: "
                  f"f0 {torch.equal(f0[b, :n], fa.cpu()[0])}, wave {torch.equal(y[b, :n * up], ya.cpu()[0])}")
            assert rel < F0_REL
            assert torch.equal(f0[b, :n], fa.cpu()[0])               # the predictor is fp32 in every precision
            if n >= BIT_EXACT_FROM:
                assert torch.equal(y[b, :n * up], ya.cpu()[0])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_vs_hip_alone(precision):
    c, sd, bt, _ = _case()
    voc = _voc(precision=precision)
    y = _run(voc, bt, R.LENS).cpu()
    _check_vs_alone(voc, y, bt, R.LENS, R.total_up(c), f"{R.MODEL} [{precision}]")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_invariance(precision):
    """Order, neighbours, micro-batch size and a warm handle leave every utterance bit-identical."""
    c, sd, bt, _ = _case()
    lens, up = R.LENS, R.total_up(c)
    voc = _voc(precision=precision)
    base = _run(voc, bt, lens).cpu()

    def same(y, rows, what, row_of=lambda b: b):
        for b in rows:
            n = lens[b]
            assert torch.equal(y[row_of(b), :n * up], base[b, :n * up]), f"{what}: utterance {b} ({n} frames)"
            assert (y[row_of(b), n * up:] == 0).all()

    rows = list(range(len(lens)))
    same(_run(voc, bt, lens).cpu(), rows, "second call on the warm handle")
    perm = [4, 8, 0, 10, 7, 2, 5, 9, 1, 6, 3]
    btp = {k: v[perm] for k, v in bt.items()}
    same(_run(voc, btp, [lens[b] for b in perm]).cpu(), rows, "permuted", row_of=perm.index)
    for mb in (5, 16, 32):
        voc.set_microbatch(mb)
        same(_run(voc, bt, lens).cpu(), rows, f"micro-batch {mb}")
    voc.set_microbatch(0)
    for keep in (rows[0::2], rows[1::2]):                 # every other utterance replaced by another one of its length
        ids = [b if b in keep else 50 + b for b in rows]
        other = R.batch(c, sd, lens, ids=ids)
        assert all(torch.equal(other["mel"][b, :, :lens[b]], bt["mel"][b, :, :lens[b]]) == (b in keep) for b in rows if lens[b])
        same(_run(voc, other, lens).cpu(), keep, "other neighbours")


def test_ragged_more_than_64_utterances():
    """B = 70 at the default micro-batch of 32."""
    c, sd, _, _, _, _ = cases.hift_case(R.MODEL)
    lens = [[300, 201, 192, 191, 47, 5, 1, 0, 250, 24][(3 * b) % 10] for b in range(70)]
    bt = R.batch(c, sd, lens, ids=[b % 10 for b in range(70)])
    up = R.total_up(c)
    voc = _voc()
    y = _run(voc, bt, lens).cpu()
    assert y.shape == (70, 300 * up) and torch.isfinite(y).all()
    for b, n in enumerate(lens):
        assert (y[b, n * up:] == 0).all()
    _check_vs_alone(voc, y, bt, lens, up, f"{R.MODEL} B = 70", rows=range(0, 70, 3))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_equal_lengths_equal_the_uniform_call(precision):
    c, sd, _, _, _, _ = cases.hift_case(R.MODEL)
    voc = _voc(precision=precision)
    voc.set_microbatch(2)
    for S in (24, 200):
        bt = {k: v.to(DEV) for k, v in R.batch(c, sd, [S] * 5).items()}
        plain = voc(bt["mel"], f0=bt["f0"], phase0=bt["phase0"], noise=bt["noise"])
        assert torch.equal(voc(bt["mel"], f0=bt["f0"], phase0=bt["phase0"], noise=bt["noise"], lens=[S] * 5), plain)
        assert torch.equal(voc(bt["mel"], f0=bt["f0"], phase0=bt["phase0"], noise=bt["noise"], lens=torch.LongTensor([S] * 5)), plain)
        y0, f0 = voc(bt["mel"], phase0=bt["phase0"], noise=bt["noise"], return_f0=True)
        y1, f1 = voc(bt["mel"], phase0=bt["phase0"], noise=bt["noise"], return_f0=True, lens=[S] * 5)
        assert torch.equal(y0, y1) and torch.equal(f0, f1)
        seeds = [11 + b for b in range(5)]                 # the draws made on the device: seeded plain against seeded ragged
        assert torch.equal(voc(bt["mel"], f0=bt["f0"], seeds=seeds), voc(bt["mel"], f0=bt["f0"], seeds=seeds, lens=[S] * 5))


def test_ragged_errors_leave_the_handle_usable():
    c, sd, bt, ref = _case()
    voc = _voc()
    m = {k: v[:3].nan_to_num(0.0) for k, v in bt.items()}
    with pytest.raises(RuntimeError, match="lens"):
        _run(voc, m, [300, 301, 3])
    with pytest.raises(RuntimeError, match="lens"):
        _run(voc, m, [50, -1, 3])
    with pytest.raises(ValueError):
        _run(voc, m, [50, 3])
    _check_vs_oracle(_run(voc, bt, R.LENS).cpu(), ref, R.LENS, R.total_up(c), "after the errors")


def test_ragged_full_size():
    c, sd, bt, ref = _case("hift_full", tuple(R.FULL_LENS))
    lens, up = R.FULL_LENS, R.total_up(c)
    voc = _voc("hift_full", "fp16p8")
    y = _run(voc, bt, lens).cpu()
    _check_vs_oracle(y, ref, lens, up, "hift_full [fp16p8]")
    _check_vs_alone(voc, y, bt, lens, up, "hift_full [fp16p8]")


# ------------------------------------------------------------------------------------------------- HotPath.convert_batch_ragged
def _pair(which):
    from seedvc_amd.cfm import CFM
    from seedvc_amd.vocoder import BigVGAN, HiFT
    if which == "hift":
        cfg, sd, _, _ = cases.dit_case("tiny_r")
        c, vsd, _, _, _, _ = cases.hift_case("hift_r")
        return cfg, CFM(cfg, sd, DEV), HiFT(c, vsd, DEV), R.total_up(c), c
    cfg, sd, _, _ = cases.dit_case("small_r")
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")       # the 80-mel reduced BigVGAN (bigvgan_r takes 20 mels, the sampler emits 80)
    return cfg, CFM(cfg, sd, DEV), BigVGAN(h, vsd, DEV), 8, None


@pytest.mark.parametrize("which", ["hift", "bigvgan"])
def test_convert_batch_ragged_equals_convert_batch_alone(which):
    from seedvc_amd.pipeline import HotPath
    cfg, cfm, voc, hop, c = _pair(which)
    hp = HotPath(cfm, voc)
    x_lens, P = [230, 61, 216], [16, 9, 3]                 # output frames 214, 52, 213
    S = [t - p for t, p in zip(x_lens, P)]
    B, T, Pmax, Smax = 3, max(x_lens), max(P), max(S)
    mu = torch.cat([cases.randn(f"cbr.mu{b}", 6, 1, T, cfg["Dc"]) for b in range(B)]).to(DEV)
    z = torch.cat([cases.randn(f"cbr.z{b}", 6, 1, cfg["C"], T) for b in range(B)]).to(DEV)
    prompt = torch.cat([cases.logmel(f"cbr.p{b}", 6, 1, cfg["C"], Pmax) for b in range(B)]).to(DEV)
    style = torch.cat([cases.randn(f"cbr.s{b}", 6, 1, cfg["style_dim"]) for b in range(B)]).to(DEV)
    kw = None
    if which == "hift":
        nh = c["nb_harmonics"] + 1
        kw = dict(f0=(120.0 + 80.0 * cases.rand("cbr.f0", 6, B, Smax)).to(DEV),
                  phase0=((cases.rand("cbr.ph", 6, B, nh, 1) * 2 - 1) * float(np.pi)).to(DEV),
                  noise=cases.randn("cbr.n", 6, B, nh, Smax * hop).to(DEV))
    out = hp.convert_batch_ragged(mu, prompt, style, x_lens, P, 3, 0.7, z=z, vocoder_kwargs=kw)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")               # a warm step enqueues from host integers only
    try:
        again = hp.convert_batch_ragged(mu, prompt, style, x_lens, P, 3, 0.7, z=z, vocoder_kwargs=kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(out) == B
    for b in range(B):
        mel, wave = out[b]
        assert mel.shape == (1, cfg["C"], S[b]) and wave.shape == (1, S[b] * hop)
        assert torch.equal(mel, again[b][0]) and torch.equal(wave, again[b][1])
        kb = None
        if kw:
            kb = dict(f0=kw["f0"][b:b + 1, :S[b]].contiguous(), phase0=kw["phase0"][b:b + 1],
                      noise=kw["noise"][b:b + 1, :, :S[b] * hop].contiguous())
        m1, w1 = hp.convert_batch(mu[b:b + 1, :x_lens[b]].contiguous(), prompt[b:b + 1, :, :P[b]].contiguous(), style[b:b + 1], 3, 0.7,
                                  z=z[b:b + 1, :, :x_lens[b]].contiguous(), vocoder_kwargs=kb)
        l1, e = (mel - m1).abs().mean().item(), R.rms(wave, w1)
        print(f"{which}: utterance {b} ({S[b]} frames) vs convert_batch alone: mel L1 {l1:.3e} (equal {torch.equal(mel, m1)}), "
              f"wave RMS {e:.3e} (equal {torch.equal(wave, w1)})")
        if S[b] >= 192:
            assert torch.equal(mel, m1) and torch.equal(wave, w1)
        else:
            assert l1 < MEL_L1 and e < WAVE_RMS
    # one output length: one plain vocoder call
    calls = []
    hp.vocoder = lambda m, **k: calls.append(k) or voc(m, **k)
    hp.convert_batch_ragged(mu[:2], prompt[:2], style[:2], [100, 95], [10, 5], 3, 0.7)
    assert len(calls) == 1 and "lens" not in calls[0]


# ------------------------------------------------------------------------------------- convert_long_batch(ragged_vocoder=True)
class _PinnedHiFT:
    """HiFT with the draws of chunk k pinned in row k's leading part: what a caller who wants pinned draws in ragged mode wraps
    the vocoder with.  `draws(S)` is the per-chunk function of the grouped path, called in plan order."""

    def __init__(self, voc, draws):
        self.voc, self.draws, self.ragged_calls = voc, draws, 0

    def __call__(self, mel, lens=None):
        S = [mel.size(2)] * mel.size(0) if lens is None else list(lens)
        d = [self.draws(s) for s in S]
        noise = torch.zeros(len(S), d[0]["noise"].size(1), mel.size(2) * (d[0]["noise"].size(2) // S[0]), device=mel.device)
        for k, dk in enumerate(d):
            noise[k, :, :dk["noise"].size(2)] = dk["noise"][0]
        self.ragged_calls += lens is not None
        return self.voc(mel, phase0=torch.cat([dk["phase0"] for dk in d]), noise=noise, lens=lens)


def test_long_batch_with_the_ragged_hift_call():
    """`convert_long_batch(ragged_vocoder=True)` with a HiFT: the chunks of a micro-batch take one `lens=` call.  Same set-up
    and bound as the grouped-path test of test_gpu_long_batch.py: within 1e-4 of `convert_long_device`."""
    from seedvc_amd import specs
    from seedvc_amd.pipeline import HotPath
    from seedvc_amd.vocoder import HiFT
    STEPS, WINDOW, OVERLAP = 3, 40, 4
    c, sd, _, _, _, _ = cases.hift_case("hift_r")
    hop, nh, Dc, P = specs.hift_total_upsample(c), c["nb_harmonics"] + 1, 8, 16
    voc = HiFT(c, sd, DEV)
    counter = [0]

    def draws(S):
        k = counter[0]
        counter[0] += 1
        return dict(phase0=((cases.rand(f"lb.hift.phase{k}", 9, 1, nh, 1) * 2 - 1) * float(np.pi)).to(DEV),
                    noise=cases.randn(f"lb.hift.noise{k}", 9, 1, nh, S * hop).to(DEV))
    utts = [(cases.randn(f"lb.hift.cond{S}", 9, 1, S, Dc).to(DEV), cases.randn("lb.hift.pc", 9, 1, P, Dc).to(DEV),
             cases.logmel("lb.hift.mel2", 9, 1, 80, P).to(DEV), cases.randn("lb.hift.style", 9, 1, 4).to(DEV)) for S in (70, 45)]
    pinned = _PinnedHiFT(voc, draws)
    outs = HotPath(LB.MelMixCFM(80, DEV), pinned).convert_long_batch(utts, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP,
                                                                      ragged_vocoder=True)
    assert counter[0] == 7 and pinned.ragged_calls == 1      # 70 frames: 24 24 24 10, 45 frames: 24 24 5 -- one ragged call
    counter[0] = 0
    hp = HotPath(LB.MelMixCFM(80, DEV), voc)
    for u, out in zip(utts, outs):
        seq = hp.convert_long_device(*u, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP, vocoder_kwargs_fn=draws)
        assert out.shape == seq.shape and out.shape[1] == u[0].size(1) * hop
        rms = R.rms(out.cpu(), seq.cpu())
        print(f"HiFT, {u[0].size(1)} frames: ragged batch vs device loop RMS {rms:.3e} (signal RMS {seq.pow(2).mean().sqrt().item():.3e})")
        assert rms < 1e-4
