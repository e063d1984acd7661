"""The fp16p8 precision plan on the device: the range-census kernels against their CPU statement (voc_plan_cases.py), and the
plan's contracts on small BigVGAN / HiFT fixtures -- an in-range model is left alone, the full plan is fp16x3 bit for bit, a
hostile model is caught and repaired, no plan depends on the batch, and a conv pair whose producer cannot write byte pairs runs.

Errors are relative, RMS(err) / RMS(oracle).  Measured values (MI355X) are in DESIGN.md, section 8w, and
profiles/vocoder_plan.json."""
import pytest
import torch

import voc_plan_cases as V

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

WAVE_RMS = 1e-4     # the bound test_hift_vs_reference_golden applies to the f0-pinned decoder


def _bigvgan(variant, precision="fp16p8"):
    from seedvc_amd.vocoder import BigVGAN
    h, sd, mel, ref = V.bigvgan_fixture(variant)
    return BigVGAN(h, sd, "cuda:0", precision=precision), mel.cuda(), ref


def _hift(variant, precision="fp16p8", **ov):
    from seedvc_amd.vocoder import HiFT
    c, sd, mel, f0, phase0, noise, ref = V.hift_fixture(variant, **ov)
    return HiFT(c, sd, "cuda:0", precision=precision), dict(x=mel.cuda(), f0=f0.cuda(), phase0=phase0.cuda(), noise=noise.cuda()), ref


def _full(voc):
    return {k: True for k in voc.plan_names()}


# ---- 1. the census op
def test_range_census_matches_the_cpu_statement():
    from seedvc_amd import ops
    hi, lo = V.census_planes()
    B, L, C, ld = V.CENSUS_SHAPE
    lens = list(V.CENSUS_LENS)
    ref = V.census_ref(hi, lo, C, lens)
    got = ops.range_census(hi, lo, C, lens)
    print("census:", got)
    for k in V.COUNTS:
        assert got[k] == ref[k], k
    assert got["max_hi"] == ref["max_hi"]
    bound = V.sum_bound(sum(lens) * C)
    for k in V.SUMS:
        rel = abs(got[k] - ref[k]) / ref[k]
        print(f"{k}: {got[k]!r} vs {ref[k]!r}: rel {rel:.2e} (bound {bound:.2e})")
        assert rel <= bound, k
    assert ops.range_census(hi, lo, C, lens) == got                      # two runs: identical bits
    # without lens every row is live: the NaN rows must be replaced first
    hi2, lo2 = hi.clone(), lo.clone()
    hi2[:, :, :C], lo2[:, :, :C] = hi2[:, :, :C].nan_to_num(0.0), lo2[:, :, :C].nan_to_num(0.0)
    assert ops.range_census(hi2, lo2, C) == got


def test_weight_census_matches_the_cpu_statement():
    from seedvc_amd import ops
    w = V.census_weight()
    ref, ex_ref = V.weight_census_ref(w)
    got, ex = ops.weight_census(w)
    assert ex == ex_ref
    bound = V.sum_bound(w.shape[1] * w.shape[2])
    zero = ref == 0
    assert (got[zero] == 0).all() and zero[5].all() and zero[40].all()
    rel = ((got - ref).abs() / ref.clamp_min(1e-300))[~zero].max().item()
    print(f"weight census: max rel {rel:.2e} (bound {bound:.2e}); omega_hi max {(ref[:, 1] / ref[:, 0]).nan_to_num().max():.3g}, "
          f"omega_lo max {(ref[:, 3] / ref[:, 2]).nan_to_num().max():.3g}")
    assert rel <= bound
    got2, _ = ops.weight_census(w)
    assert torch.equal(got, got2)


# ---- 2. / 3. the empty and the full plan
@pytest.mark.parametrize("voc_name", ["bigvgan", "hift"])
def test_empty_and_full_plan(voc_name):
    if voc_name == "bigvgan":
        voc, mel, _ = _bigvgan("in_range")
        x3, _, _ = _bigvgan("in_range", "fp16x3")
        run = lambda v: v(mel)                              # noqa: E731
        cal = lambda v: v.calibrate(mel)                    # noqa: E731
    else:
        voc, kw, _ = _hift("in_range")
        x3, _, _ = _hift("in_range", "fp16x3")
        run = lambda v: v(**kw)                             # noqa: E731
        cal = lambda v: v.calibrate(**kw)                   # noqa: E731
    names = voc.plan_names()
    assert len(names) > 0 and len(set(names)) == len(names)
    assert voc.precision_plan == {k: False for k in names}
    with pytest.raises(RuntimeError):
        x3.plan_names()
    y0 = run(voc)
    rows = cal(voc)
    for r in rows:
        print(f"{voc_name} in_range {r['name']}: L {r['L']} rho {r['rho']:.2e} eta {r['eta']:.2e} omega {r['omega_hi']:.2e} "
              f"{r['omega_lo']:.2e} max|hi| {r['max_hi']:.3g} veto {r['veto']}")
    assert [r["name"] for r in rows] == names and all(r["L"] >= 192 and r["n"] > 0 for r in rows)
    # an in-range model: nothing is vetoed, and the output is what it was, bit for bit
    assert not any(r["veto"] for r in rows) and not any(voc.precision_plan.values())
    assert torch.equal(run(voc), y0)
    assert cal(voc) == rows                                 # same material, same rows
    # the full plan: every conv and its producer switch format together, and the result is the fp16x3 handle's
    voc.precision_plan = _full(voc)
    assert all(voc.precision_plan.values())
    y_full, y_x3 = run(voc), run(x3)
    assert torch.equal(y_full, y_x3)
    assert not torch.equal(y_full, y0)
    voc.reset_plan()
    assert torch.equal(run(voc), y0)


# ---- 4. hostile fixtures
_R0 = {}


def _r0(voc_name):
    """E_p8 / E_x3 on the in-range fixture (measured here, shared by the cases below)"""
    if voc_name not in _R0:
        if voc_name == "bigvgan":
            (p8, mel, ref), (x3, _, _) = _bigvgan("in_range"), _bigvgan("in_range", "fp16x3")
            e_p8, e_x3 = V.rel_rms(p8(mel).cpu(), ref), V.rel_rms(x3(mel).cpu(), ref)
        else:
            (p8, kw, ref), (x3, _, _) = _hift("in_range"), _hift("in_range", "fp16x3")
            e_p8, e_x3 = V.rel_rms(p8(**kw).cpu(), ref), V.rel_rms(x3(**kw).cpu(), ref)
        print(f"{voc_name} in_range: E_p8 {e_p8:.3e} E_x3 {e_x3:.3e} r0 {e_p8 / e_x3:.2f}")
        _R0[voc_name] = e_p8 / e_x3
    return _R0[voc_name]


@pytest.mark.parametrize("voc_name,variant", [("bigvgan", "quiet"), ("bigvgan", "gains"), ("hift", "gains")])
def test_hostile_fixture_is_caught_and_repaired(voc_name, variant):
    """calibrate vetoes at least one conv and E_plan <= 2 r0 E_x3, r0 = E_p8 / E_x3 of the in-range fixture measured here (the 2:
    a conv just under tau carries up to ~3x the in-range correction error in the one-conv simulation, diluted by its in-range
    neighbours); on the quiet fixture the empty plan must be worse than the calibrated one.
    Measured on an MI355X (E_p8 / E_plan / E_x3; vetoed): BigVGAN r0 2.24, quiet 1.840e-4 / 1.787e-4 / 1.787e-4 (36 of 36),
    gains 2.28e-5 / 2.94e-5 / 3.30e-5 (29 of 36); HiFT r0 2.87, gains 2.43e-5 / 4.55e-5 / 4.50e-5 (22 of 48).  DESIGN.md 8w says
    why quiet is 1.03x and not the simulation's ~10x (fp16x3 itself sits at 1.8e-4 there) and why the gain rows do not rank."""
    r0 = _r0(voc_name)
    if voc_name == "bigvgan":
        voc, mel, ref = _bigvgan(variant)
        x3, _, _ = _bigvgan(variant, "fp16x3")
        run = lambda v: v(mel).cpu()                        # noqa: E731
        e_p8 = V.rel_rms(run(voc), ref)
        rows = voc.calibrate(mel)
    else:
        voc, kw, ref = _hift(variant)
        x3, _, _ = _hift(variant, "fp16x3")
        run = lambda v: v(**kw).cpu()                       # noqa: E731
        e_p8 = V.rel_rms(run(voc), ref)
        rows = voc.calibrate(**kw)
    n_veto = sum(r["veto"] for r in rows)
    e_plan, e_x3 = V.rel_rms(run(voc), ref), V.rel_rms(run(x3), ref)
    print(f"{voc_name} {variant}: vetoed {n_veto} of {len(rows)}; E_p8 {e_p8:.3e} E_plan {e_plan:.3e} E_x3 {e_x3:.3e} "
          f"r0 {r0:.2f} bound {2 * r0 * e_x3:.3e}")
    assert n_veto >= 1
    assert sum(voc.precision_plan.values()) == n_veto
    assert e_plan <= 2 * r0 * e_x3
    if variant == "quiet":
        assert e_p8 > e_plan


# ---- 5. the batch contract under a mixed plan
@pytest.mark.parametrize("voc_name", ["bigvgan", "hift"])
def test_mixed_plan_keeps_the_batch_contract(voc_name):
    if voc_name == "bigvgan":
        voc, mel, _ = _bigvgan("in_range")
        lens = [V.BIG_S, 48, 57]                            # every stage of every utterance keeps >= 192 rows alone
        mel3 = torch.cat([mel, mel[:1] * 0.9], 0)
        run = lambda b, n: voc(mel3[b:b + 1, :, :n])[0, 0]                  # noqa: E731
        for b, n in enumerate(lens):
            mel3[b, :, n:] = float("nan")
        batch = lambda: voc(mel3, lens=lens)[:, 0]                          # noqa: E731
    else:
        voc, kw, _ = _hift("in_range")
        lens = [V.HIFT_S, 24, 29]
        kw3 = {k: torch.cat([v, v[:1]], 0) for k, v in kw.items()}
        kw3["x"][2] *= 0.9
        for b, n in enumerate(lens):
            kw3["x"][b, :, n:] = float("nan")
        up = voc.total_up
        run = lambda b, n: voc(kw3["x"][b:b + 1, :, :n], f0=kw3["f0"][b:b + 1, :n], phase0=kw3["phase0"][b:b + 1],      # noqa: E731
                               noise=kw3["noise"][b:b + 1, :, :n * up])[0]
        batch = lambda: voc(lens=lens, **kw3)                               # noqa: E731
    names = voc.plan_names()
    voc.precision_plan = {k: i % 2 == 0 for i, k in enumerate(names)}
    assert 0 < sum(voc.precision_plan.values()) < len(names)
    up = voc.total_up
    y = batch()
    for b, n in enumerate(lens):
        assert torch.equal(y[b, :n * up], run(b, n)), f"utterance {b} ({n} frames) differs from the run alone"
        assert (y[b, n * up:] == 0).all()
    voc.set_microbatch(1)
    y1 = batch()
    voc.set_microbatch(2)
    assert torch.equal(y1, y) and torch.equal(batch(), y)


# ---- 6. a producer that cannot write byte pairs
def test_pair_with_a_tap_gemm_producer_runs():
    """HiFT with an 11-tap ResBlock of dilation 7: (k - 1) * dil = 70 > 64, so convs1.2 runs on the tap-GEMM, which cannot
    write the byte pairs convs2.2 (on the resident-tile kernel) would read under fp16p8: that pair runs fp16x3 on fp16 planes."""
    dils = [[1, 3, 5], [1, 3, 5], [1, 3, 7]]
    voc, kw, ref = _hift("in_range", resblock_dilation_sizes=dils)
    y = voc(**kw).cpu()                                     # the parent commit refuses this forward
    rms = (y - ref).pow(2).mean().sqrt().item()
    print(f"hift dil 7: waveform RMS vs oracle {rms:.3e} (signal rms {ref.pow(2).mean().sqrt():.3f})")
    assert rms < WAVE_RMS
    x3, _, _ = _hift("in_range", "fp16x3", resblock_dilation_sizes=dils)
    assert not torch.equal(y, x3(**kw).cpu())               # the other convs still run p8
    voc.precision_plan = _full(voc)
    assert torch.equal(voc(**kw).cpu(), x3(**kw).cpu())
