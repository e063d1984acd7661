"""CPU side of the vocoder pointwise kernels' op-level suite (test_gpu_vocoder_pointwise.py): the two test aids are declared,
exported and bound and refuse bad arguments before anything touches a device; the float64 restatements of
vocoder_pointwise_cases.py agree with the oracle's originals; the fp32 emulation of every stage stays within its bound and passes
its exact checks; and every named sabotage of an emulation fails at least one check in a case that targets it."""
import ctypes
import os
import re

import pytest
import torch

import kconv_cases as K
import seedvc_oracle as O
import vocoder_pointwise_cases as V
import vocoder_ragged_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

ACT = V.act_cases()
_refs = {}


def act_ref(c):
    key = V.act_id(c)
    if key not in _refs:
        _refs[key] = V.ref_act(c)
    return _refs[key]


# ------------------------------------------------------------------------------------------------ the seams
def _fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", header).group(1)
    return re.findall(r"\**\s*([A-Za-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", body)


def test_seams_are_declared_exported_and_bound():
    from seedvc_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    for name, wrapper, struct, cls in (("svc_op_act_cl", "act_cl", "svc_act_cl_t", _lib.ActCl),
                                       ("svc_op_hift_signal", "hift_signal", "svc_hift_signal_t", _lib.HiftSignal)):
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS and hasattr(lib, name) and hasattr(ops, wrapper)
        assert _fields(header, struct) == [f[0] for f in cls._fields_]
    assert "svc_op_act_cl" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "svc_op_hift_signal" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _act_args(**kw):
    from seedvc_amd import _lib
    e = _lib.ActCl()
    e.x, e.y_hi, e.y_lo, e.a, e.inv_b = 4096, 8192, 16384, 32768, 65536          # never dereferenced: the checks come first
    e.ldx, e.ldy, e.out_f16, e.B, e.C, e.L = 64, 64, 1, 3, 33, 65
    keep = None
    for k, v in kw.items():
        if k == "lens":
            keep = (ctypes.c_int32 * len(v))(*v)
            e.lens = ctypes.cast(keep, ctypes.POINTER(ctypes.c_int32))
        else:
            setattr(e, k, v)
    return e, keep


ACT_REFUSALS = [
    (dict(x=None), b"x and y_hi"), (dict(y_hi=None), b"x and y_hi"), (dict(B=0), b"positive"), (dict(L=0), b"positive"),
    (dict(C=65), b"cover C"), (dict(mode=3), b"mode"), (dict(mode=-1), b"mode"), (dict(a=None), b"a and inv_b"),
    (dict(lo_fmt=2), b"lo_fmt"), (dict(lo_fmt=1, y_lo=None), b"lo_fmt 1 needs y_lo"), (dict(out_f16=0), b"fp16 output"),
    (dict(mode=1, lens=[1, 2, 3]), b"mode 0 only"), (dict(lens=[65, 66, 0]), b"lens out of range"), (dict(lens=[-1, 0, 0]), b"lens out of range"),
    (dict(x=4100), b"alignment"), (dict(y_hi=8194), b"alignment"),
]


@pytest.mark.parametrize("kw,word", ACT_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in ACT_REFUSALS])
def test_act_cl_refusals_need_no_gpu(kw, word):
    from seedvc_amd import _lib
    e, keep = _act_args(**kw)
    assert _lib.lib().svc_op_act_cl(ctypes.byref(e), None) != 0, kw
    assert word in _lib.lib().svc_last_error(), (kw, _lib.lib().svc_last_error())


def _hift_args(stage, **kw):
    from seedvc_amd import _lib
    e = _lib.HiftSignal()
    e.stage = stage
    for name in ("in", "phase0", "noise", "lin_w", "lin_b", "out", "out_lo"):
        setattr(e, name, 4096)
    e.B, e.n_utt, e.NH, e.up, e.S, e.S_in, e.F, e.Lw, e.ld, e.C, e.vd, e.mode = 3, 3, 9, 8, 5, 7, 17, 64, 32, 20, 2, 2
    keep = []
    for k, v in kw.items():
        if k in ("src", "len", "lw", "nf"):
            keep.append((ctypes.c_int32 * len(v))(*v))
            setattr(e, k, ctypes.cast(keep[-1], ctypes.POINTER(ctypes.c_int32)))
        else:
            setattr(e, k, v)
    return e, keep


HIFT_REFUSALS = [
    (0, {}, b"stage"), (7, {}, b"stage"), (1, {"in": None}, b"in and out"), (2, dict(out=None), b"in and out"), (1, dict(B=0), b"positive"),
    (1, dict(B=4), b"n_utt"), (4, dict(src=[0, 3, 1]), b"src out of range"), (1, dict(S=8), b"S_in"), (5, dict(len=[5, 6, 0]), b"len out of range"),
    (2, dict(lw=[64, 32, 12]), b"come together"), (2, dict(lw=[64, 32, 65], nf=[17, 9, 4]), b"out of range"),
    (4, dict(lw=[64, 32, 12], nf=[17, 18, 4]), b"out of range"), (2, dict(ld=16), b"18 columns"),
    (2, dict(lw=[64, 8, 0], nf=[17, 3, 0]), b"lw >= 9"), (2, dict(lw=[64, 32, 0], nf=[17, 10, 0]), b"lw >= 9"), (2, dict(Lw=60), b"lw >= 9"),
    (3, dict(ld=17), b"ld >= 18"), (1, dict(noise=None), b"phase0, noise"), (1, dict(NH=0), b"NH and up"),
    (5, dict(vd=4), b"vd"), (6, dict(ld=16), b"vd"), (5, dict(out_lo=None), b"out_lo"), (6, dict(mode=1), b"mode is 2 or 3"),
]


@pytest.mark.parametrize("stage,kw,word", HIFT_REFUSALS, ids=[f"s{s}," + ",".join(f"{k}={v}" for k, v in kw.items()) for s, kw, _ in HIFT_REFUSALS])
def test_hift_signal_refusals_need_no_gpu(stage, kw, word):
    from seedvc_amd import _lib
    e, keep = _hift_args(stage, **kw)
    assert _lib.lib().svc_op_hift_signal(ctypes.byref(e), None) != 0, kw
    assert word in _lib.lib().svc_last_error(), (kw, _lib.lib().svc_last_error())


# ------------------------------------------------------------------------------------------------ the restatements
def test_float64_restatements_agree_with_the_oracle():
    """each float64 reference against the oracle's own fp32 / mixed evaluation, to fp32 noise"""
    c = V.act_case(145, 2)
    x = c["data"].transpose(1, 2).contiguous()
    mine = V.ref_act(c)[0].transpose(1, 2)
    assert (O.anti_alias_act(x, c["taps"], c["a"], c["ib"]).double() - mine).abs().max().item() < 5e-6
    c = V.act_case(321, 1, lens=[144, 145, 143], poison=False)
    mine = V.ref_act(c)[0].transpose(1, 2)
    theirs = R.act_ragged(c["data"].transpose(1, 2).contiguous(), c["lens"], c["taps"], c["a"], c["ib"])
    assert (theirs.double() - mine).abs().max().item() < 5e-6
    # source: the oracle on each utterance alone
    c = V.source_case(9, 8, False)
    cfg = dict(nb_harmonics=8, sampling_rate=22050, nsf_alpha=0.1, nsf_sigma=0.003, nsf_voiced_threshold=10, istft_hop=4, upsample_rates=[2])
    sd = {"m_source.l_linear.weight": c["lin_w"][None, :], "m_source.l_linear.bias": c["lin_b"]}
    n = c["S"] * c["up"]
    theirs = O.hift_source(sd, cfg, c["f0"], c["phase0"][:, :, None], c["noise"][:, :, :n])[:, 0]
    assert (theirs.double() - V.ref_source(c)[0]).abs().max().item() < 2e-5          # fp32 theta of cum ~ 10: 2 pi ulp32 and fp32 sin
    c = V.stft_case(36)
    re, im = O.stft16(c["s"])
    mine = V.ref_stft(c)[0]
    assert (re.transpose(1, 2).double() - mine[..., 0:9]).abs().max().item() < 1e-5
    assert (im.transpose(1, 2).double() - mine[..., 9:18]).abs().max().item() < 1e-5
    c = V.istft_case(9)
    v = c["post"][:, :, :18]
    theirs = O.istft16(torch.exp(v[..., :9]).transpose(1, 2), torch.sin(v[..., 9:]).transpose(1, 2))
    fr, _ = V.ref_frames(c)
    mine = V.ref_ola(dict(c, limit=1e30), fr)[0]
    assert (theirs.double() - mine).abs().max().item() < 2e-4 * mine.abs().max().item()


def test_cases_cover_the_edges():
    assert {c["L"] for c in ACT} == set(V.ACT_LENGTHS) and {c["ch"] for c in ACT} == {0, 1, 2, 3}
    assert sum(c["lens"] is not None for c in ACT) == 5 and sum(c["big"] for c in ACT) == 1
    big = [c for c in ACT if c["big"]][0]
    assert abs((big["a"].double() * act_ref(big)[1]).abs().max().item() - 1e3) < 1.0
    sweep = V.act_pointwise_cases()[-1]
    assert 999.0 < (sweep["a"] * sweep["data"]).abs().max().item() < 1001.0
    for c in V.source_cases():
        if c["kind"] == "numeric":
            f0 = c["f0"][~torch.isnan(c["f0"])]
            assert bool(((f0 == 0) | ((f0 >= 80) & (f0 <= 400))).all()) and bool((f0 == 0).any()) and bool((f0 > 0).any())
    lim = [c for c in V.istft_cases() if c["kind"] == "limit"][0]
    ref = V.ref_ola(lim, V.ref_frames(lim)[0])[0]
    assert bool((ref.abs() == float(V.f32(lim["limit"]))).any()) and bool((ref.abs() < lim["limit"]).any())
    clip = [c for c in V.istft_cases() if c["kind"] == "clip"][0]
    assert torch.exp(clip["post"][..., :9]).min().item() > 100.0


# ------------------------------------------------------------------------------------------------ act_cl
@pytest.mark.parametrize("form", V.FORMS)
def test_act_emulation_passes(form):
    worst, worst_norm = 0.0, 0.0
    for c in ACT + V.act_pointwise_cases():
        ref, u = act_ref(c)
        fails, ratio, norm = V.check_act(c, form, *V.emu_act(c, form), ref, u)
        assert not fails, (V.act_id(c), form, fails)
        worst = max(worst, ratio)
        if c["mode"] == 0 and not c["big"] and form == "f32":
            worst_norm = max(worst_norm, norm)
    print(f"act_cl emulation, {form}: worst error / bound {worst:.3f}; mode 0 largest |y - ref| / (|ref| + 1) {worst_norm:.2e}")


def test_act_emulation_relations():
    """the relations the GPU file asserts hold for the emulation: a sequence of a batch equals itself alone, a ragged row equals
    the uniform launch of its utterance with L = lens[b]"""
    c = V.act_case(321, 1, lens=[144, 145, 143])
    hi, _, g = V.emu_act(c, "f32")
    for b, n in enumerate(c["lens"]):
        alone = dict(c, L=n, B=1, lens=None, data=c["data"][b:b + 1, :n])
        hb, _, _ = V.emu_act(alone, "f32")
        assert torch.equal(hi[g + b * 321:g + b * 321 + n], hb[g:g + n])


# (sabotage, the case that targets it, the form it shows in)
ACT_TARGETS = [
    ("clamp_L-2", V.act_case(13, 1), "f32"), ("clamp_L-2", V.act_case(321, 3), "f32"),
    ("clamp_batch_L", V.act_case(321, 1, lens=[144, 145, 143], poison=False), "f32"),
    ("swap_taps01", V.act_case(65, 2), "f32"), ("odd_even", V.act_case(7, 0), "f32"), ("no_x2_tail", V.act_case(145, 3), "f32"),
    ("lo_unrounded", V.act_case(80, 1), "f16+lo"), ("lo_unrounded", V.act_case(80, 1), "f16+p8"),
]


@pytest.mark.parametrize("sab,c,form", ACT_TARGETS, ids=[f"{s}-{V.act_id(c)}-{f}" for s, c, f in ACT_TARGETS])
def test_act_sabotage_exceeds_tau32_tenfold(sab, c, form):
    """the hard condition: the sabotaged emulation's normalised error is at least 10 x TAU32, and the check fails"""
    ref, u = V.ref_act(c)
    hi, lo, g = V.emu_act(c, form, sab)
    fails, ratio, norm = V.check_act(c, form, hi, lo, g, ref, u)
    if form != "f32":        # the planes' sum against the reference
        n = c["B"] * c["L"]
        hv = hi[g:g + n, :c["C"]].view(torch.float16).double()
        lv = lo[g:g + n, :c["C"]].view(torch.float16).double() if form == "f16+lo" else \
            V.f8_decode((lo[g:g + n, :c["C"]].to(torch.int32) >> 8) & 0xFF) / 2048.0
        r = ref.reshape(n, -1)
        norm = ((hv + lv - r).abs() / (r.abs() + 1)).max().item()
    print(f"sabotage {sab} on {V.act_id(c)} {form}: normalised error {norm:.2e} = {norm / V.TAU32:.0f} x TAU32; failed: {fails}")
    assert fails and norm >= 10.0 * V.TAU32


def test_act_sabotages_with_exact_checks():
    """the ragged clamp at the batch's L reads the NaN rows; swapped fp8 bytes break byte 0 == q8(hi)"""
    c = V.act_case(65, 2, lens=[65, 64, 1])
    ref, u = V.ref_act(c)
    assert "hi: non-finite output" in V.check_act(c, "f32", *V.emu_act(c, "f32", "clamp_batch_L"), ref, u)[0]
    assert "p8: byte 0 is not q8(hi)" in V.check_act(c, "f16+p8", *V.emu_act(c, "f16+p8", "p8_bytes_swapped"), ref, u)[0]
    # the fp8 plane decodes to kconv_cases.act_planes_p8 of the values it was cut from
    n, C = c["B"] * c["L"], c["C"]
    hi, lo, g = V.emu_act(c, "f16+p8")
    w = lo[g:g + n, :C].to(torch.int32) & 0xFFFF
    a_hi, b0, b1 = K.act_planes_p8(V.emu_values(c).reshape(n, C))
    assert torch.equal(hi[g:g + n, :C].view(torch.float16).double(), a_hi)
    assert torch.equal(V.f8_decode(w & 0xFF), b0) and torch.equal(V.f8_decode(w >> 8), b1)
    # and the buffers' own checks: a lost canary, a non-zero pad channel, a written row past lens[b]
    hi, lo, g = V.emu_act(c, "f16+lo")
    for name, (r, col) in {"canary": (g - 1, 0), "pad": (g + 3, c["C"]), "above": (g + 2 * 65 + 1, 0)}.items():
        bad = hi.clone()
        bad[r, col] = 1
        assert V.check_act(c, "f16+lo", bad, lo, g, ref, u)[0], name
    assert set(s for s, _, _ in ACT_TARGETS) | {"clamp_batch_L", "p8_bytes_swapped"} == set(V.ACT_SABOTAGES)


# ------------------------------------------------------------------------------------------------ HiFT stages
def test_source_emulation_and_sabotages():
    worst = {}
    caught = {s: [] for s in V.SRC_SABOTAGES}
    for c in V.source_cases():
        ref, bound = V.ref_source(c)
        fails, ratio = V.check_rows(V.emu_source(c), ref, bound, "source")
        assert not fails, (V.source_id(c), fails)
        kind = "numeric" if c["kind"] == "numeric" else "unvoiced"
        worst[kind] = max(worst.get(kind, 0.0), ratio)
        for sab in V.SRC_SABOTAGES:
            if V.check_rows(V.emu_source(c, sab), ref, bound, "source")[0]:
                caught[sab].append(V.source_id(c))
    print("source emulation: worst error / bound", worst)
    # each in the cases named for it: the offset in every voiced case, the stride in every case of more than one harmonic row, the
    # phase row in the ragged numeric cases (src is a permutation there)
    for c in V.source_cases():
        if c["kind"] == "numeric":
            assert V.source_id(c) in caught["r_not_r+1"], V.source_id(c)
            assert (V.source_id(c) in caught["phase0_by_row"]) == c["ragged"], V.source_id(c)
        if c["kind"].startswith("onehot_w") and not c["kind"].endswith("w0"):
            assert V.source_id(c) in caught["noise_stride_S"], V.source_id(c)


def test_stft_emulation_and_sabotages():
    worst = 0.0
    caught = {s: [] for s in V.STFT_SABOTAGES}
    for c in V.stft_cases():
        ref, bound = V.ref_stft(c)
        fails, ratio = V.check_rows(V.emu_stft(c), ref, bound, "stft")
        assert not fails, (V.stft_id(c), fails)
        worst = max(worst, ratio)
        for sab in V.STFT_SABOTAGES:
            if V.check_rows(V.emu_stft(c, sab), ref, bound, "stft")[0]:
                caught[sab].append(V.stft_id(c))
    print(f"stft emulation: worst error / bound {worst:.3f}")
    ragged = [V.stft_id(c) for c in V.stft_cases() if c["ragged"]]
    assert set(ragged) <= set(caught["reflect_at_Lw"]) and set(ragged) <= set(caught["nf+1"])
    assert "Lw64-ragged-randn" in caught["nf-1"] and "Lw20-plain-randn" in caught["nf-1"]
    assert {V.stft_id(c) for c in V.stft_cases() if c["kind"] == "randn"} <= set(caught["imag_sign"])


def test_istft_emulation_and_sabotages():
    worst = {"frames": 0.0, "ola": 0.0, "chain": 0.0}
    caught = {s: [] for s in V.ISTFT_SABOTAGES}
    for c in V.istft_cases():
        fr_ref, fr_bound = V.ref_frames(c)
        fr = V.emu_frames(c)
        fails, ratio = V.check_rows(fr, fr_ref, fr_bound, "frames")
        assert not fails, (V.istft_id(c), fails)
        worst["frames"] = max(worst["frames"], ratio)
        if V.check_rows(V.emu_frames(c, "nyquist_sign"), fr_ref, fr_bound, "frames")[0]:
            caught["nyquist_sign"].append(V.istft_id(c))
        # the stage alone on the emulated frames, and the chain against istft16 of the pre-activations
        a = V.ola_args(c, fr)
        ref, bound = V.ref_ola(c, fr)
        fails, ratio = V.check_ola(c, V.emu_ola(c, a["in"]), ref, bound)
        assert not fails, (V.istft_id(c), fails)
        worst["ola"] = max(worst["ola"], ratio)
        ref2, bound2 = V.ref_ola(c, fr_ref, fr_bound)
        fails, ratio = V.check_ola(c, V.emu_ola(c, a["in"]), ref2, bound2)
        assert not fails, (V.istft_id(c), fails)
        worst["chain"] = max(worst["chain"], ratio)
        for sab in ("env_minus_one", "ola_nf-1"):
            if V.check_ola(c, V.emu_ola(c, a["in"], sab), ref, bound)[0]:
                caught[sab].append(V.istft_id(c))
        if c["ragged"]:     # a write into the unmapped row, and a frame read past nf[b] (NaN)
            bad = V.emu_ola(c, a["in"])
            bad[1, 0] = 0.0
            assert V.check_ola(c, bad, ref, bound)[0]
    print("frames / overlap-add emulation: worst error / bound", worst)
    ids = {V.istft_id(c) for c in V.istft_cases()}
    assert set(caught["nyquist_sign"]) == ids and set(caught["env_minus_one"]) == ids and set(caught["ola_nf-1"]) == ids


def test_cast_predictions():
    """mel_to_cl / ew_cl: the predictions have the properties the GPU file relies on (zeros by selection, exact planes)"""
    for ragged in (False, True):
        c = V.mel_case(ragged)
        hi, lo = V.mel_want(c, "f16+lo")
        v = hi.view(torch.float16).float() + lo.view(torch.float16).float()
        assert bool(torch.isfinite(v).all()) and not bool(v[:, :, c["C"]:].any())
        for j, n in enumerate(c["lens"]):
            assert not bool(v[j, n:].any())
            assert (v[j, :n, :c["C"]] - c["mel"][c["src"][j], :, :n].T).abs().max().item() <= 2.0 ** -20 * 16 if n else True
    c = V.ew_case(2)
    hi, _ = V.ew_want(c, "f32")
    x = c["x"][:, :c["C"]]
    assert torch.equal(hi[:, :c["C"]][x < 0], (x * V.f32(0.1))[x < 0]) and torch.equal(hi[:, :c["C"]][x > 0], x[x > 0])
