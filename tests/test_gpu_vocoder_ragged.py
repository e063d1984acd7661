"""GPU tests of the ragged BigVGAN call: one vocoder call for utterances of different lengths, each result being that of
the utterance run alone.

Bounds.  Against the CPU oracle alone on each utterance's own frames: waveform RMS < 1e-4 per utterance (WAVE_RMS of
test_gpu_vocoder.py), every precision.  Against the HIP vocoder run alone: bit for bit for every utterance of at least
192 frames -- which kernel a conv takes depends on the layer and on `Lout >= 192`, never on the batch -- and the oracle's
bound below that, where a layer may take the resident-tile / fp8-correction form in the padded call and the tap-GEMM
alone.  In fp32 no layer's choice depends on the length, so there the comparison is bit for bit at every length >= 1."""
import functools

import pytest
import torch

import ar_batch_cases as A
import cases
import seedvc_oracle as O
import v2_chain_cases as V
import vocoder_ragged_cases as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

WAVE_RMS = 1e-4
BIT_EXACT_FROM = 192
PRECISIONS = ["fp32", "fp16x3", "fp16p8"]


@functools.lru_cache(maxsize=None)
def _case(name):
    h, sd, _, _ = cases.bigvgan_case(name)
    mel = R.batch_mel(h, R.LENS)                         # padding frames are NaN
    return h, sd, mel, R.ragged_reference(sd, h, mel, R.LENS)


def _voc(name, precision="fp16p8"):
    from seedvc_amd.vocoder import BigVGAN
    h, sd, _, _ = cases.bigvgan_case(name)
    return BigVGAN(h, sd, "cuda:0", precision=precision)


def _alone(voc, mel, b, n):
    return voc(mel[b:b + 1, :, :n].contiguous().cuda()).cpu().reshape(-1)


def _check_vs_alone(voc, y, mel, lens, up, what, exact_from=BIT_EXACT_FROM, rows=None):
    for b in (range(len(lens)) if rows is None else rows):
        n = lens[b]
        if n == 0:
            assert (y[b] == 0).all(), f"{what}: empty utterance {b} is not an all-zero row"
            continue
        alone = _alone(voc, mel, b, n)
        got = y[b, 0, :n * up]
        e = R.rms(got, alone)
        print(f"{what}: utterance {b} ({n} frames) vs the HIP vocoder alone: RMS {e:.3e}, equal {torch.equal(got, alone)}")
        if n >= exact_from:
            assert torch.equal(got, alone), f"{what}: utterance {b} ({n} frames) differs from its run alone"
        else:
            assert e < WAVE_RMS


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", R.MODELS)
def test_ragged_vs_oracle_alone(name, precision):
    h, sd, mel, ref = _case(name)
    up = R.total_up(h)
    y = _voc(name, precision)(mel.cuda(), lens=R.LENS).cpu()
    assert y.shape == ref.shape
    assert torch.isfinite(y).all()
    for b, n in enumerate(R.LENS):
        assert (y[b, 0, n * up:] == 0).all(), f"utterance {b} ({n} frames): tail not zero"
        if n:
            e = R.rms(y[b, 0, :n * up], ref[b, 0, :n * up])
            print(f"{name} [{precision}]: utterance {b} ({n} frames): waveform RMS vs the oracle alone {e:.3e}")
            assert e < WAVE_RMS


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", R.MODELS)
def test_ragged_vs_hip_alone(name, precision):
    h, sd, mel, _ = _case(name)
    voc = _voc(name, precision)
    y = voc(mel.cuda(), lens=R.LENS).cpu()
    _check_vs_alone(voc, y, mel, R.LENS, R.total_up(h), f"{name} [{precision}]", exact_from=1 if precision == "fp32" else BIT_EXACT_FROM)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", R.MODELS)
def test_ragged_invariance(name, precision):
    """Order, micro-batch size and neighbours leave every utterance of >= 192 frames bit-identical."""
    h, sd, mel, _ = _case(name)
    lens, up = R.LENS, R.total_up(h)
    voc = _voc(name, precision)
    base = voc(mel.cuda(), lens=lens).cpu()
    long_rows = [b for b, n in enumerate(lens) if n >= BIT_EXACT_FROM]
    assert len(long_rows) == 4

    def same(y, rows, what, row_of=lambda b: b):
        for b in rows:
            n = lens[b]
            assert torch.equal(y[row_of(b), 0, :n * up], base[b, 0, :n * up]), f"{what}: utterance {b} ({n} frames)"
            assert (y[row_of(b), 0, n * up:] == 0).all()

    perm = [4, 8, 0, 7, 2, 5, 1, 6, 3]
    yp = voc(mel[perm].cuda(), lens=[lens[b] for b in perm]).cpu()
    same(yp, long_rows, "permuted", row_of=perm.index)
    for mb in (1, 3, 32):
        voc.set_microbatch(mb)
        y = voc(mel.cuda(), lens=lens).cpu()
        same(y, long_rows, f"micro-batch {mb}")
        assert (y[lens.index(0)] == 0).all() and torch.isfinite(y).all()      # at 1: a micro-batch of one empty utterance
    voc.set_microbatch(0)
    for keep in (long_rows[0::2], long_rows[1::2]):       # every other utterance replaced by another mel of its length
        ids = [b if b in keep else 50 + b for b in range(len(lens))]
        other = R.batch_mel(h, lens, ids=ids)
        assert all(torch.equal(other[b, :, :lens[b]], mel[b, :, :lens[b]]) == (b in keep) for b in range(len(lens)) if lens[b])
        same(voc(other.cuda(), lens=lens).cpu(), keep, "other neighbours")


@pytest.mark.parametrize("name", R.MODELS)
def test_ragged_more_than_64_utterances(name):
    """B = 70 at the default micro-batch of 32: two micro-batches and a remainder."""
    h, sd, _, _ = cases.bigvgan_case(name)
    lens = [[430, 301, 192, 191, 47, 5, 1, 0, 250, 200][(3 * b) % 10] for b in range(70)]
    mel = R.batch_mel(h, lens)
    up = R.total_up(h)
    voc = _voc(name)
    y = voc(mel.cuda(), lens=lens).cpu()
    assert y.shape == (70, 1, 430 * up) and torch.isfinite(y).all()
    for b, n in enumerate(lens):
        assert (y[b, 0, n * up:] == 0).all()
    _check_vs_alone(voc, y, mel, lens, up, f"{name} B = 70")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_repeatable_after_nan_in_the_allocator(precision):
    h, sd, mel, _ = _case("bigvgan_r2")
    voc = _voc("bigvgan_r2", precision)
    first = voc(mel.cuda(), lens=R.LENS).cpu()
    junk = torch.full((64 << 20,), float("nan"), device="cuda")     # 256 MB of NaN handed back to the caching allocator
    torch.cuda.synchronize()
    del junk
    second = voc(mel.cuda(), lens=R.LENS).cpu()
    assert torch.isfinite(second).all()
    assert torch.equal(first, second)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", R.MODELS)
def test_equal_lengths_equal_the_uniform_call(name, precision):
    h, sd, _, _ = cases.bigvgan_case(name)
    voc = _voc(name, precision)
    voc.set_microbatch(2)
    for S in (24, 200):
        mel = R.batch_mel(h, [S] * 5).cuda()
        assert torch.equal(voc(mel, lens=[S] * 5), voc(mel))
        assert torch.equal(voc(mel, lens=torch.LongTensor([S] * 5)), voc(mel))


def test_ragged_errors_leave_the_handle_usable():
    h, sd, mel, ref = _case("bigvgan_r2")
    voc = _voc("bigvgan_r2")
    m = mel[:3, :, :50].contiguous().nan_to_num(0.0).cuda()
    with pytest.raises(RuntimeError, match="lens"):
        voc(m, lens=[50, 51, 3])
    with pytest.raises(RuntimeError, match="lens"):
        voc(m, lens=[50, -1, 3])
    with pytest.raises(ValueError):
        voc(m, lens=[50, 3])
    y = voc(mel.cuda(), lens=R.LENS).cpu()
    up = R.total_up(h)
    for b, n in enumerate(R.LENS):
        if n:
            assert R.rms(y[b, 0, :n * up], ref[b, 0, :n * up]) < WAVE_RMS


# ------------------------------------------------------------------------------------------------------------- V2HotPath
class _Counting:
    def __init__(self, voc):
        self.voc, self.calls = voc, 0

    def __call__(self, mel, **kw):
        self.calls += 1
        return self.voc(mel, **kw)


def _hotpath(ragged_vocoder):
    from seedvc_amd.ar import ARModel
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath
    from seedvc_amd.vocoder import BigVGAN
    M = V.models()
    ar = ARModel(*M["ar"], "cuda:0")
    ar.setup_caches(max_batch_size=4)
    hp = V2HotPath(ar, InterpolateRegulator(*M["ar_lr"], "cuda:0"), InterpolateRegulator(*M["cfm_lr"], "cuda:0"),
                   CFM(*M["dit"], "cuda:0"), BigVGAN(*M["voc"], "cuda:0"), ragged_vocoder=ragged_vocoder)
    hp.vocoder = _Counting(hp.vocoder)
    return hp


def _convert(hp, ks):
    us = [V.utterance(k) for k in ks]
    targets = [hp.prepare_target(u["target_narrow"], u["target_tokens"], u["target_mel"], u["style"]) for u in us]
    out = hp.convert_batch([u["src_narrow"].cuda() for u in us], targets, [u["frames_per_token"] for u in us], V.N_STEPS,
                           cfg_rates=V.CFG_RATES, exp_noise=[u["noise"].cuda() for u in us], z=[u["z"].cuda() for u in us],
                           max_new=A.MAX_NEW)
    torch.cuda.synchronize()
    return out


def test_v2_hotpath_one_vocoder_call():
    ks = V.qualified()[:3]
    assert len({V.utterance(k)["ylen"] for k in ks}) == 3
    on, off = _hotpath(True), _hotpath(False)
    a, b = _convert(on, ks), _convert(off, ks)
    assert on.vocoder.calls == 1 and off.vocoder.calls == 3
    h, vsd = V.models()["voc"]
    for k, x, y in zip(ks, a, b):
        assert torch.equal(x["tokens"], y["tokens"]) and torch.equal(x["mel"], y["mel"])
        assert x["mel"].shape == y["mel"].shape and x["wave"].shape == y["wave"].shape
        e = R.rms(x["wave"], y["wave"])
        e_or = R.rms(x["wave"].cpu(), O.bigvgan_forward(vsd, h, x["mel"].cpu()).reshape(1, -1))
        print(f"utterance {k} ({x['mel'].shape[2]} frames): ragged vs grouped wave RMS {e:.3e}, ragged vs oracle {e_or:.3e}")
        assert e < WAVE_RMS and e_or < WAVE_RMS
    # one distinct length: the grouped path, whatever the switch
    on.vocoder.calls = 0
    _convert(on, [ks[0], ks[0]])
    assert on.vocoder.calls == 1


# ------------------------------------------------------------------------------------------------------------- full size
def test_ragged_full_size():
    h, sd, _, _ = cases.bigvgan_case("bigvgan_full")
    lens = R.FULL_LENS
    up = R.total_up(h)
    mel = R.batch_mel(h, lens)
    voc = _voc("bigvgan_full", "fp16p8")
    y = voc(mel.cuda(), lens=lens).cpu()
    assert torch.isfinite(y).all()
    _check_vs_alone(voc, y, mel, lens, up, "bigvgan_full [fp16p8]", rows=[0, 1, 2])
    ref = R.ragged_reference(sd, h, mel, lens)
    for b, n in enumerate(lens):
        assert (y[b, 0, n * up:] == 0).all()
        e = R.rms(y[b, 0, :n * up], ref[b, 0, :n * up])
        print(f"bigvgan_full [fp16p8]: utterance {b} ({n} frames): waveform RMS vs the oracle alone {e:.3e}")
        assert e < WAVE_RMS
