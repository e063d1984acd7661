"""Sampler seams inside the fused row-panel launches (csrc/fused.hip, SEAM template parameter): the first panel of a step
builds its rows itself (x block of the merge linear + static term, prefix-token rows, zero pad rows) and the last panel
runs the mlp output head.  `set_fused_seams(mask)`: bit 0 merge, bit 1 head; mask 0 issues the separate launches
(prefix rows, merge GEMM, two head GEMMs).  The fused path is forced on with `set_fused_min_rows(0)`.

Bounds are the ones tests/test_gpu_fused.py uses for the same comparisons."""
import functools

import pytest
import torch

import cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


def _cfm(name):
    from seedvc_amd.cfm import CFM
    cfg, sd, inp, meta = cases.dit_case(name)
    cfm = CFM(cfg, sd, "cuda:0")
    assert cfm.estimator.fused_available
    cfm.estimator.set_fused_min_rows(0)
    return cfm, cfg, inp, meta


@pytest.mark.parametrize("name", ["tiny_full", "small_full", "v2_full"])
def test_seams_vs_reference_golden(name, golden):
    """Estimator call and sampler, seams on (mask 3) and off (mask 0): each against the reference golden, and on against
    off.  tiny / v2 take both seams; small (WaveNet head) takes the merge seam only."""
    cfm, cfg, inp, meta = _cfm(name)
    T, P = meta["T"], meta["P"]
    prompt_x = torch.zeros(1, cfg["C"], T)
    prompt_x[..., :P] = inp["prompt"]
    ref_s = torch.from_numpy(golden[name + ".sample"])
    ref_e = torch.from_numpy(golden[name + ".est"])
    est, smp = {}, {}
    for mask in (3, 0):
        cfm.estimator.set_fused_seams(mask)
        est[mask] = cfm.estimator(inp["x"].cuda(), prompt_x.cuda(), torch.LongTensor([T]), inp["t"], inp["style"].cuda(), inp["mu"].cuda()).cpu()
        smp[mask] = cfm.inference(inp["mu"].cuda(), torch.LongTensor([T]), inp["prompt"].cuda(), inp["style"].cuda(), None,
                                  meta["n_steps"], inference_cfg_rate=meta["cfg_rate"], z=inp["z"].cuda()).cpu()
        e = (est[mask] - ref_e).abs().mean().item() / ref_e.abs().mean().item()
        s = (smp[mask] - ref_s).abs().mean().item()
        print(f"{name}, seams {mask}: estimator rel L1 {e:.3e}, sampler L1 {s:.3e}")
    d_e = (est[3] - est[0]).abs().mean().item() / ref_e.abs().mean().item()
    d_s = (smp[3] - smp[0]).abs().mean().item()
    print(f"{name}: seams on vs off: estimator rel L1 {d_e:.3e}, sampler L1 {d_s:.3e}")
    for mask in (3, 0):
        assert (est[mask] - ref_e).abs().mean().item() / ref_e.abs().mean().item() < 5e-3
        assert (smp[mask] - ref_s).abs().mean().item() < 1e-3
    assert d_e < 1e-3 and d_s < 1e-3          # two fp16-operand paths


B, T, P = 5, 200, 90
LENS = [200, 173, 200, 96, 131]
PLENS = [90, 40, 64, 33, 90]


@functools.lru_cache(maxsize=None)
def _ragged():
    """ONE tiny_full handle and the ragged batch of test_fused_ragged_batch_and_window: two streams x 5 x 208 rows = 2080
    rows = 16.25 panels, so panels straddle sequences and the last one is partial."""
    cfm, cfg, inp, meta = _cfm("tiny_full")
    mu = cases.randn("fz.mu", 7, B, T, cfg["Dc"]).cuda()
    prompt = cases.logmel("fz.p", 7, B, cfg["C"], P).cuda()
    style = cases.randn("fz.s", 7, B, cfg["style_dim"]).cuda()
    z = cases.randn("fz.z", 7, B, cfg["C"], T).cuda()
    return cfm, mu, prompt, style, z


def _batch(cfm, mu, prompt, style, z, plens=PLENS, t=T):
    lens = [min(n, t) for n in LENS]
    pl = [min(a, b) for a, b in zip(plens, lens)]
    return cfm.inference(mu[:, :t], torch.LongTensor(lens), prompt, style, None, 3, inference_cfg_rate=0.7, z=z[:, :, :t], prompt_lens=pl)


@functools.lru_cache(maxsize=None)
def _ragged_on():
    """The mask-3 result of the ragged batch on a handle nothing else has run on yet."""
    cfm, mu, prompt, style, z = _ragged()
    cfm.estimator.set_fused_seams(3)
    return _batch(cfm, mu, prompt, style, z).clone()


@pytest.mark.parametrize("plens", [PLENS, [90, 40, 64, 0, 90]], ids=["window", "win0"])
def test_seams_ragged_batch(plens):
    """Every utterance of the ragged batch against its own single run, and seams on against off; once with the last-layer
    window behind the shortest prompt (row_off = win0 > 0) and once with a prompt length of 0 (win0 = 0: all rows)."""
    _ragged_on()
    cfm, mu, prompt, style, z = _ragged()
    cfm.estimator.set_fused_seams(3)
    out = _batch(cfm, mu, prompt, style, z, plens)
    for b in range(B):
        one = cfm.inference(mu[b:b + 1, :LENS[b]], torch.LongTensor([LENS[b]]), prompt[b:b + 1, :, :plens[b]], style[b:b + 1], None, 3,
                            inference_cfg_rate=0.7, z=z[b:b + 1, :, :LENS[b]])
        assert torch.isfinite(one).all()
        d = (one[0] - out[b, :, :LENS[b]]).abs().max().item()
        print(f"utterance {b}: batch vs single run, max |d| {d:.3e}")
        assert d < 2e-4, (b, d)
    cfm.estimator.set_fused_seams(0)
    off = _batch(cfm, mu, prompt, style, z, plens)
    cfm.estimator.set_fused_seams(3)
    for b in range(B):
        d = (out[b, :, :LENS[b]] - off[b, :, :LENS[b]]).abs().mean().item()
        print(f"utterance {b}: seams on vs off, L1 {d:.3e}")
        assert d < 2e-4, (b, d)


def test_seams_bit_exact_invariances():
    """On mask 3: the micro-batch split, graph replay and what an earlier call with another length left in the workspace
    change no bit (no kernel pre-writes the token and pad rows of xin any more: the first panel writes every row)."""
    want = _ragged_on()
    cfm, mu, prompt, style, z = _ragged()
    cfm.estimator.set_fused_seams(3)
    cfm.estimator.set_microbatch(2)
    split = _batch(cfm, mu, prompt, style, z)
    cfm.estimator.set_microbatch(0)
    assert torch.equal(split, want)
    cfm.estimator.set_graphs(True)
    runs = [_batch(cfm, mu, prompt, style, z).clone() for _ in range(3)]      # eager, capture + replay, replay
    cfm.estimator.set_graphs(False)
    assert torch.equal(runs[2], want) and torch.equal(runs[1], want) and torch.equal(runs[0], want)
    short = _batch(cfm, mu, prompt, style, z, t=120)
    assert torch.isfinite(short).all() and short.shape[-1] == 120
    again = _batch(cfm, mu, prompt, style, z)
    fresh_cfm, _, _, _ = _cfm("tiny_full")
    fresh = _batch(fresh_cfm, mu, prompt, style, z)
    assert torch.equal(again, fresh) and torch.equal(again, want)


def test_seams_fallback_and_back():
    """Mask 0 runs the separate launches; mask 3 afterwards on the same handle repeats the first mask-3 result bit for bit.
    Masks 1 and 2 (one seam each) stay within the on / off bound of the ragged test."""
    want = _ragged_on()
    cfm, mu, prompt, style, z = _ragged()
    cfm.estimator.set_fused_seams(0)
    off = _batch(cfm, mu, prompt, style, z).clone()
    for mask in (1, 2):
        cfm.estimator.set_fused_seams(mask)
        one = _batch(cfm, mu, prompt, style, z)
        d = max((one[b, :, :LENS[b]] - off[b, :, :LENS[b]]).abs().mean().item() for b in range(B))
        print(f"seams {mask} vs 0: worst utterance L1 {d:.3e}")
        assert d < 2e-4
        assert not torch.equal(one, off)          # the seam did run: another summation order
    cfm.estimator.set_fused_seams(3)
    back = _batch(cfm, mu, prompt, style, z)
    assert torch.equal(back, want)
    with pytest.raises(RuntimeError):
        cfm.estimator.set_fused_seams(4)
    cfm.estimator.set_fused_seams(3)
