"""The vocoders' pointwise kernels at op level: act_cl_kernel / act_cl2_kernel (csrc/aa_act.hip) through ops.act_cl -- ONE
act_cl_launch per call -- and the HiFT signal stages (phase prefix + source, STFT, frames, overlap-add, mel_to_cl, ew_cl of
csrc/vocoder.hip) through ops.hift_signal, which calls the launchers svc_hift::run calls.

vocoder_pointwise_cases.py states the layouts and the float64 references, derives every bound and builds the cases;
test_host_vocoder_pointwise.py shows that each check catches the sabotage it is for.  What is held here:
  numeric    every stage meets its per-element bound against the float64 reference (each test prints its largest error / bound)
  exact      pad channels, rows at and above lens[b], samples past a row's end and frame rows at and above nf[b] are zero words;
             guard rows and unmapped output rows keep their canaries; no NaN comes out although x, f0, the noise, the samples,
             the frames and the mel hold NaN wherever the kernels must not read; byte 0 of the fp8 word is q8(hi); |lo| is at
             most half an fp16 step of hi; leaky ReLU, mel_to_cl and ew_cl are predicted bit for bit
  relations  each sequence of a batch of 3 equals itself run alone; each ragged row equals the uniform launch of its utterance
             with L = lens[b]
"""
import pytest
import torch

import vocoder_pointwise_cases as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

ACT = V.act_cases()
_refs = {}
FORM_ARGS = {"f32": ("f32", None), "f16": ("f16", None), "f16+lo": ("f16", "f16"), "f16+p8": ("f16", "p8")}


def act_ref(c):
    key = V.act_id(c)
    if key not in _refs:
        _refs[key] = V.ref_act(c)
    return _refs[key]


def run_act(c, form):
    from seedvc_amd import ops
    out, lo = FORM_ARGS[form]
    hi, p_lo, g = ops.act_cl(V.act_x(c, form), c["C"], V.act_ld(c, form), taps=c["taps"], a=c["a"], inv_b=c["ib"], out=out, lo=lo,
                             mode=c["mode"], slope=c["slope"], lens=c["lens"], guard=V.GUARD, fill16=V.CANARY16, fill32=V.CANARY32)
    return hi.cpu(), (None if p_lo is None else p_lo.cpu()), g


def hift(a):
    from seedvc_amd import ops
    out, lo = ops.hift_signal(a, fill16=V.CANARY16, fill32=V.CANARY32)
    return out.cpu(), (None if lo is None else lo.cpu())


def same_words(a, b, what):
    n = int((V.bits(a) != V.bits(b)).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} words differ"


def act_relations(c, form, hi, lo, g):
    """batch == alone, and ragged row == the uniform launch of that utterance with L = lens[b], in every plane, bit for bit"""
    L = c["L"]
    for b, n in enumerate(V.act_lens(c)):
        rows = slice(g + b * L, g + b * L + L)
        alone = dict(c, B=1, data=c["data"][b:b + 1], lens=None if c["lens"] is None else [n])
        hb, lb, _ = run_act(alone, form)
        same_words(hi[rows], hb[g:g + L], f"{V.act_id(c)} {form}: sequence {b} in the batch against itself alone (hi)")
        if lo is not None:
            same_words(lo[rows], lb[g:g + L], f"{V.act_id(c)} {form}: sequence {b} in the batch against itself alone (lo)")
        if c["lens"] is not None and n > 0:
            uni = dict(c, B=1, L=n, lens=None, data=c["data"][b:b + 1, :n])
            hu, lu, _ = run_act(uni, form)
            same_words(hi[g + b * L:g + b * L + n], hu[g:g + n], f"{V.act_id(c)} {form}: ragged row {b} against the uniform launch (hi)")
            if lo is not None:
                same_words(lo[g + b * L:g + b * L + n], lu[g:g + n], f"{V.act_id(c)} {form}: ragged row {b} against the uniform launch (lo)")


@pytest.mark.parametrize("ch", range(len(V.ACT_CHANNELS)), ids=[f"C{c[0]}" for c in V.ACT_CHANNELS])
@pytest.mark.parametrize("form", V.FORMS)
def test_act_anti_aliased(form, ch):
    """mode 0: every length, the ragged sets and the large-argument case of this channel count, in this output form"""
    worst, worst_norm, where = 0.0, 0.0, ""
    for c in ACT:
        if c["ch"] != ch:
            continue
        ref, u = act_ref(c)
        hi, lo, g = run_act(c, form)
        fails, ratio, norm = V.check_act(c, form, hi, lo, g, ref, u)
        if ratio > worst:
            worst, where = ratio, V.act_id(c)
        if form == "f32" and not c["big"]:
            worst_norm = max(worst_norm, norm)
        assert not fails, (V.act_id(c), form, fails, f"normalised error {norm:.3e}")
        act_relations(c, form, hi, lo, g)
    print(f"act_cl mode 0 {form} C={V.ACT_CHANNELS[ch][0]}: worst error / bound {worst:.3f} ({where}); "
          f"largest |y - ref| / (|ref| + 1) {worst_norm:.3e}")


def test_act_tau32():
    """the figure TAU32 is 4 x of: the largest |y - ref| / (|ref| + 1) of the fp32 form over all numeric mode-0 cases (printed for
    vocoder_pointwise_cases.py and DESIGN.md), held to the committed constant"""
    norm = {}
    for c in ACT:
        if not c["big"]:
            ref, u = act_ref(c)
            norm[c["C"]] = max(norm.get(c["C"], 0.0), V.check_act(c, "f32", *run_act(c, "f32"), ref, u)[2])
    print(f"act_cl mode 0: largest |y - ref| / (|ref| + 1) {max(norm.values()):.3e}; by channel count "
          + ", ".join(f"{k}: {v:.3e}" for k, v in norm.items()) + f"; TAU32 = {V.TAU32:.3e}")
    assert max(norm.values()) <= V.TAU32


@pytest.mark.parametrize("form", V.FORMS)
def test_act_pointwise_modes(form):
    """modes 1 and 2: fp32 out runs act_cl_kernel, fp16 out the pair kernel; mode 1's sweep to |a x| = 1e3"""
    worst, where = 0.0, ""
    for c in V.act_pointwise_cases():
        ref, u = V.ref_act(c)
        hi, lo, g = run_act(c, form)
        fails, ratio, _ = V.check_act(c, form, hi, lo, g, ref, u)
        if ratio > worst:
            worst, where = ratio, V.act_id(c)
        assert not fails, (V.act_id(c), form, fails)
        act_relations(c, form, hi, lo, g)
    print(f"act_cl modes 1, 2 {form}: worst error / bound {worst:.3f} ({where})")


SOURCE = V.source_cases()


@pytest.mark.parametrize("c", SOURCE, ids=[V.source_id(c) for c in SOURCE])
def test_hift_source(c):
    ref, bound = V.ref_source(c)
    out, _ = hift(V.source_args(c))
    fails, ratio = V.check_rows(out, ref, bound, "source")
    print(f"hift source {V.source_id(c)}: worst error / bound {ratio:.3f}")
    assert not fails, fails


STFT = V.stft_cases()


@pytest.mark.parametrize("c", STFT, ids=[V.stft_id(c) for c in STFT])
def test_hift_stft(c):
    ref, bound = V.ref_stft(c)
    out, _ = hift(V.stft_args(c))
    fails, ratio = V.check_rows(out, ref, bound, "stft")
    print(f"hift stft {V.stft_id(c)}: worst error / bound {ratio:.3f}")
    assert not fails, fails


ISTFT = V.istft_cases()


@pytest.mark.parametrize("c", ISTFT, ids=[V.istft_id(c) for c in ISTFT])
def test_hift_frames_and_overlap_add(c):
    """the frames stage against the irfft half of istft16; the overlap-add stage alone on those frames; and the two chained
    against istft16 of the pre-activations"""
    fr_ref, fr_bound = V.ref_frames(c)
    fr, _ = hift(V.frames_args(c))
    fails, r_frames = V.check_rows(fr.reshape(fr_ref.shape), fr_ref, fr_bound, "frames")
    assert not fails, fails
    a = V.ola_args(c, fr)
    out, _ = hift(a)
    ref, bound = V.ref_ola(c, fr)
    fails, r_ola = V.check_ola(c, out, ref, bound)
    assert not fails, fails
    ref, bound = V.ref_ola(c, fr_ref, fr_bound)
    fails, r_chain = V.check_ola(c, out, ref, bound)
    print(f"hift {V.istft_id(c)}: worst error / bound: frames {r_frames:.3f}, overlap-add {r_ola:.3f}, chained {r_chain:.3f}")
    assert not fails, fails


@pytest.mark.parametrize("form", list(V.VD))
def test_mel_to_cl_and_ew_cl(form):
    """pure casts: every plane bit for bit, the (C, S_in) -> [S][ld] mapping with S < S_in, zeros by selection under a NaN tail"""
    for ragged in (False, True):
        c = V.mel_case(ragged)
        hi, lo = hift(V.mel_args(c, form))
        want_hi, want_lo = V.mel_want(c, form)
        same_words(hi, want_hi, f"mel_to_cl {form} ragged={ragged} hi")
        assert (lo is None) == (want_lo is None)
        if lo is not None:
            same_words(lo, want_lo, f"mel_to_cl {form} ragged={ragged} lo")
    for mode in (2, 3):
        c = V.ew_case(mode)
        hi, lo = hift(V.ew_args(c, form))
        want_hi, want_lo = V.ew_want(c, form)
        same_words(hi, want_hi, f"ew_cl mode {mode} {form} hi")
        if lo is not None:
            same_words(lo, want_lo, f"ew_cl mode {mode} {form} lo")
