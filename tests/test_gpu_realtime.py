"""GPU side of real-time sessions: `svc_sola_step` against the numpy statement of its formula (realtime_cases.py;
test_host_realtime.py pins that to the reference GUI's own lines), `pipeline.RealtimeEngine` bit for bit against the numpy
session with exactly rounded stand-ins, without a host synchronisation, and within the pipeline's bounds of the oracle with real
models behind HiFT and BigVGAN."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB
import realtime_cases as RT
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
i32 = lambda v: (C.c_int32 * len(v))(*[int(x) for x in v])      # noqa: E731


def _check_row(tag, infer, before, fi, fo, block, Ls, o, out, after):
    """One stream of one step.  The offset: the float64 score at the kernel's offset is within 4 Lb 2^-24 |b|_2 of the
    float64 maximum -- twice the worst-case error 2 gamma_Lb |b| of an fp32 normalised dot product of Lb terms in any
    summation order (no row is skipped; an all-zero buffer makes the bound 0 and every score 0).  Given that offset, the
    output and the new buffer are the model's, bit for bit."""
    Lb = len(before)
    assert 0 <= o <= Ls, (tag, o)
    want_out, want_new, _, scores = RT.sola_model(infer, before, fi, fo, block, Ls, offset=o)
    bound = 4 * Lb * 2.0 ** -24 * float(np.linalg.norm(before.astype(np.float64)))
    assert scores.max() - scores[o] <= bound, (tag, o, int(np.argmax(scores)), scores.max() - scores[o], bound)
    if not before.any():
        assert o == 0, (tag, o)
    assert np.array_equal(out, want_out), tag
    assert np.array_equal(after, want_new), tag


# ------------------------------------------------------------------------------------------------------- svc_sola_step
KERNEL_CASES = [   # name, block, Lb, Ls, start, samples of the row past the window
    ("gui_scalar", 3969, 882, 441, 10907, 441),
    ("x4_aligned", 64, 16, 12, 8, 8),              # 16-byte stores; loads 16-byte where start + o* is a multiple of 4
    ("x4_start_odd", 64, 16, 12, 7, 5),            # 16-byte stores, rows and start off the 16-byte grid
    ("Ls0", 40, 16, 0, 3, 0),
    ("block_lt_Lb_x4", 8, 32, 10, 4, 4),           # the new buffer starts inside the faded samples, written over the old one
    ("block_lt_Lb_scalar", 7, 30, 9, 2, 3),
    ("block_eq_Lb", 32, 32, 7, 0, 0),
    ("Lb_tail_of_3", 50, 19, 300, 1, 2),           # Lb % 4 = 3: the scalar tail of the score loop; two offsets per lane
]


@pytest.mark.parametrize("name,block,Lb,Ls,start,extra", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_sola_step_equals_the_model(name, block, Lb, Ls, start, extra):
    """70 streams (two launches) on permuted slots of an 80-row state; NaN before `start` and past the window; rows 0 .. 4
    have an all-zero buffer, rows 5 .. 14 are loud (x30) up to the middle of the searched samples and quiet (x0.3) after it."""
    from seedvc_amd import _lib
    rng = np.random.default_rng(len(name) * 1000 + block)
    N, max_slots = 70, 80
    n_inf = block + Lb + Ls
    stride = start + n_inf + extra
    slots = rng.permutation(max_slots)[:N]
    x = rng.standard_normal((N, n_inf)).astype(np.float32)
    half = (Lb + Ls) // 2                                # the step lies inside the samples the search reads
    x[5:15, :half] *= np.float32(30.0)
    x[5:15, half:] *= np.float32(0.3)
    state = rng.standard_normal((max_slots, Lb)).astype(np.float32)
    state[slots[:5]] = 0
    state[slots[15:20]] *= np.float32(1e-3)
    wave = np.full((N, stride), np.nan, np.float32)
    wave[:, start:start + n_inf] = x
    fi, fo = RT.gui_windows(Lb)
    d_wave, d_state, d_fi, d_fo = (torch.from_numpy(a).to(DEV) for a in (wave, state, fi, fo))
    out = torch.full((N, block), float("nan"), device=DEV)
    offs = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().svc_sola_step(_lib.ptr(d_wave), stride, start, N, _lib.ptr(d_state), max_slots, i32(slots), _lib.ptr(d_fi),
                                        _lib.ptr(d_fo), block, Lb, Ls, _lib.ptr(out), _lib.ptr(offs), _lib.stream_ptr()))
    torch.cuda.synchronize()
    out, offs, after = out.cpu().numpy(), offs.cpu().numpy(), d_state.cpu().numpy()
    for k in range(N):
        _check_row((name, k), x[k], state[slots[k]], fi, fo, block, Ls, int(offs[k]), out[k], after[slots[k]])
    untouched = np.setdiff1d(np.arange(max_slots), slots)
    assert len(untouched) == 10 and np.array_equal(after[untouched], state[untouched])
    if Ls > 0:
        assert len(set(offs[20:].tolist())) > 1          # the search does move


def test_sola_step_without_offsets_and_in_one_launch():
    """offsets = NULL, three streams: the same out and state as the call that reports them."""
    from seedvc_amd import _lib
    rng = np.random.default_rng(9)
    block, Lb, Ls, start, stride = 64, 16, 12, 4, 100
    wave = torch.from_numpy(rng.standard_normal((3, stride)).astype(np.float32)).to(DEV)
    state0 = torch.from_numpy(rng.standard_normal((4, Lb)).astype(np.float32)).to(DEV)
    fi, fo = (torch.from_numpy(w).to(DEV) for w in RT.gui_windows(Lb))
    res = []
    for with_offsets in (True, False):
        st, out = state0.clone(), torch.empty(3, block, device=DEV)
        offs = torch.empty(3, dtype=torch.int32, device=DEV) if with_offsets else None
        _lib.check(_lib.lib().svc_sola_step(_lib.ptr(wave), stride, start, 3, _lib.ptr(st), 4, i32([3, 0, 1]), _lib.ptr(fi), _lib.ptr(fo),
                                            block, Lb, Ls, _lib.ptr(out), _lib.ptr(offs), _lib.stream_ptr()))
        torch.cuda.synchronize()
        res.append((st.cpu(), out.cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][0][2], state0[2].cpu())


# ------------------------------------------------------------------------------------ the engine with the exact stand-ins
def _fake_refs():
    return [(cases.randn(f"rt.pc{s}", 142, 1, P, cases.CHUNK_DC).to(DEV), cases.logmel(f"rt.mel{s}", 142, 1, cases.CHUNK_C, P).to(DEV),
             cases.randn(f"rt.style{s}", 142, 1, 3).to(DEV)) for s, P in enumerate(RT.FAKE_PROMPTS)]


def _fake_engine(max_streams=4):
    from seedvc_amd.pipeline import RealtimeEngine
    cfm, voc = LB.BatchedFakeCFM(DEV), RT.FakeVocoder()
    return RealtimeEngine(RT.FakeLR(), cfm, voc, max_streams=max_streams, **RT.FAKE_GEOMETRY), cfm, voc


def _sessions():
    fi, fo = RT.gui_windows(RT.FAKE_GEOMETRY["sola_buffer"])
    contents = [RT.planted_session(s) for s in range(3)]
    return contents, [RT.session_model(c, fi, fo) for c in contents]


def _content(contents, streams, k):
    return torch.from_numpy(np.stack([contents[s][k] for s in streams])).to(DEV)


def test_three_streams_in_one_engine_equal_the_numpy_session():
    contents, models = _sessions()
    eng, cfm, voc = _fake_engine()
    slots = [eng.open(*r) for r in _fake_refs()]
    assert slots == [0, 1, 2]
    for k in range(5):
        order = [0, 1, 2] if k < 3 else [2, 0, 1]          # the same streams in another order: the prompts are stacked anew
        out, parts = eng.step([slots[s] for s in order], _content(contents, order, k), 10, 0.7, return_parts=True)
        assert out.shape == (3, RT.FAKE_GEOMETRY["block"]) and out.dtype == torch.float32 and out.is_cuda
        assert parts["mel"].shape == (3, cases.CHUNK_C, 12) and parts["infer"].shape == (3, 72) and parts["offsets"].dtype == torch.int32
        for row, s in enumerate(order):
            want_out, want_new, want_o, scores, before = models[s][k]
            assert int(parts["offsets"][row]) == want_o == RT.FAKE_OFFSETS[s][k], (s, k)
            assert np.array_equal(out[row].cpu().numpy(), want_out), (s, k)
            assert np.array_equal(eng.state[slots[s]].cpu().numpy(), want_new), (s, k)
    assert cfm.batch_sizes == [3] * 5 and voc.calls == [(3, 12)] * 5       # one sampler and one vocoder call per step
    assert not eng.state[3].any()


@pytest.mark.parametrize("stream", [0, 1, 2])
def test_each_stream_alone_equals_the_numpy_session(stream):
    contents, models = _sessions()
    eng, _, _ = _fake_engine(max_streams=1)
    slot = eng.open(*_fake_refs()[stream])
    for k in range(5):
        out = eng.step([slot], _content(contents, [stream], k), 10, 0.7)
        assert np.array_equal(out[0].cpu().numpy(), models[stream][k][0]), k
        assert np.array_equal(eng.state[slot].cpu().numpy(), models[stream][k][1]), k


def test_a_reopened_slot_starts_from_zeros_and_reset_does_too():
    contents, models = _sessions()
    eng, _, _ = _fake_engine()
    refs = _fake_refs()
    slots = [eng.open(*r) for r in refs]
    for k in range(2):
        eng.step(slots, _content(contents, [0, 1, 2], k), 10, 0.7)
    assert eng.state[1].any()
    eng.close(1)
    assert eng.open(*refs[2]) == 1                              # stream 2's reference on the freed slot
    eng.reset(0)
    out = eng.step([0, 1], _content(contents, [0, 2], 0), 10, 0.7)
    assert np.array_equal(out[0].cpu().numpy(), models[0][0][0]) and np.array_equal(out[1].cpu().numpy(), models[2][0][0])
    assert np.array_equal(eng.state[1].cpu().numpy(), models[2][0][1])
    with pytest.raises(ValueError):
        eng.step([0, 0], _content(contents, [0, 0], 0), 10, 0.7)


def test_a_step_does_not_synchronise():
    """With the stand-ins (device-only torch operations), a step under torch's synchronisation debug mode raises nothing:
    no .item(), no copy to the host, no blocking upload.  (A torch without that mode runs the steps unwatched.)"""
    watch = hasattr(torch.cuda, "set_sync_debug_mode")
    contents, models = _sessions()
    eng, _, _ = _fake_engine()
    slots = [eng.open(*r) for r in _fake_refs()]
    xs = [_content(contents, [0, 1, 2], k) for k in range(3)]
    eng.step(slots, xs[0], 10, 0.7)                             # the first step stacks the prompts
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode() if watch else None
    if watch:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)        # "a prototype feature"
            torch.cuda.set_sync_debug_mode("error")
    try:
        out1 = eng.step(slots, xs[1], 10, 0.7)
        out2, parts = eng.step(slots, xs[2], 10, 0.7, return_parts=True)
    finally:
        if watch:
            torch.cuda.set_sync_debug_mode(before)
    for s in range(3):
        assert np.array_equal(out1[s].cpu().numpy(), models[s][1][0]) and np.array_equal(out2[s].cpu().numpy(), models[s][2][0])
        assert int(parts["offsets"][s]) == RT.FAKE_OFFSETS[s][2]


# ------------------------------------------------------------------------------------------------------------ real models
STEPS, CFG_RATE, S_REAL, PROMPTS = 3, 0.7, 40, (16, 11)


def _real_front():
    from seedvc_amd import specs, weights
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    cfg, sd, _, _ = cases.dit_case("tiny_r")
    preset, ov, tin, _, tf0, seed = cases.LR_CASES["lr_tiny_r"]
    assert tf0 == 0
    lcfg = specs.lr_config(preset, **ov, out_channels=cfg["Dc"])        # the case's regulator, its last 1x1 conv as wide as the DiT's content input
    assert lcfg["version"] == 1 and not lcfg["is_discrete"]
    lsd = weights.make_state_dict(specs.lr_state_spec(lcfg), seed=seed, prefix="lr.")
    return dict(cfg=cfg, sd=sd, lcfg=lcfg, lsd=lsd, tin=tin, cfm=CFM(cfg, sd, DEV), lr=InterpolateRegulator(lcfg, lsd, DEV))


def _run_real(tag, vocoder, hop, block, Lb, Ls, tail, oracle_wave, kwargs_fn):
    """Three blocks of two streams (prompts of 16 and 11 frames).  Per block and stream: the mel against
    O.lr_forward -> O.cfm_sample (L1 < 1e-3), `infer` against the oracle vocoder on the engine's own mel (RMS < 1e-4) --
    test_gpu_pipeline.py's bounds for the same stages -- and the SOLA stage against `sola_model` on the engine's own `infer`
    and carried buffer, as in the kernel test."""
    from seedvc_amd.pipeline import RealtimeEngine
    m = _real_front()
    cfg, S = m["cfg"], S_REAL
    eng = RealtimeEngine(m["lr"], m["cfm"], vocoder, S, hop, block, Lb, Ls, tail=tail, max_streams=3)
    refs = [(cases.randn(f"rt.real.pc{i}", 143, 1, P, cfg["Dc"]), cases.logmel(f"rt.real.mel{i}", 143, 1, cfg["C"], P),
             cases.randn(f"rt.real.style{i}", 143, 1, cfg["style_dim"])) for i, P in enumerate(PROMPTS)]
    assert eng.open(*refs[0]) == 0 and eng.open(*refs[1]) == 1 and eng.open(*refs[0]) == 2
    eng.close(1)
    slots = [2, eng.open(*refs[1])]                              # stream 0 on slot 2, stream 1 on slot 1
    assert slots == [2, 1]
    fi, fo = eng.fade_in.cpu().numpy(), eng.fade_out.cpu().numpy()
    Pmax, n_inf, start = max(PROMPTS), block + Lb + Ls, S * hop - tail - (block + Lb + Ls)
    assert (eng.start, eng.n_inf) == (start, n_inf)
    for k in range(3):
        x = cases.randn(f"rt.real.x{k}", 143, 2, m["tin"], m["lcfg"]["in_channels"])
        z = cases.randn(f"rt.real.z{k}", 143, 2, cfg["C"], Pmax + S)
        kw = kwargs_fn(k)
        before = eng.state.cpu().numpy().copy()
        out, parts = eng.step(slots, x.to(DEV), STEPS, CFG_RATE, z=z.to(DEV), vocoder_kwargs={a: b.to(DEV) for a, b in kw.items()},
                              return_parts=True)
        out, mel, infer, offs = out.cpu(), parts["mel"].cpu(), parts["infer"].cpu(), parts["offsets"].cpu()
        after = eng.state.cpu().numpy()
        assert out.shape == (2, block) and mel.shape == (2, cfg["C"], S) and infer.shape == (2, n_inf)
        for b, (pc, mel2, style) in enumerate(refs):
            P = PROMPTS[b]
            cond = O.lr_forward(m["lsd"], m["lcfg"], x[b:b + 1], S)
            want_mel = O.cfm_sample(m["sd"], cfg, z[b:b + 1, :, :P + S], P + S, mel2, torch.cat([pc, cond], 1), style, STEPS,
                                    CFG_RATE)[:, :, P:]
            l1 = (mel[b:b + 1] - want_mel).abs().mean().item()
            want_wave = oracle_wave(mel[b:b + 1], {a: v[b:b + 1] for a, v in kw.items()}).reshape(-1)
            rms = (infer[b] - want_wave[start:start + n_inf]).pow(2).mean().sqrt().item()
            print(f"{tag} block {k} stream {b}: mel L1 vs oracle {l1:.3e}; infer RMS vs oracle vocoder {rms:.3e} "
                  f"(signal RMS {want_wave.pow(2).mean().sqrt().item():.3e}); offset {int(offs[b])}")
            assert l1 < 1e-3
            assert rms < 1e-4
            _check_row((tag, k, b), infer[b].numpy(), before[slots[b]], fi, fo, block, Ls, int(offs[b]), out[b].numpy(),
                       after[slots[b]])
        assert np.array_equal(after[0], before[0]) and not after[0].any()      # slot 0 is open and idle


def test_real_models_with_hift():
    """tiny_r DiT, the lr_tiny_r regulator and hift_r with phase0, noise and f0 pinned per block.  f0 is pinned like the
    draws because HiFT's source integrates f0 over the whole row: the 2e-5 relative difference between the device's and the
    oracle's f0 predictor grows with the row length (test_gpu_vocoder.py pins f0 for its 1e-4 bound for the same reason)."""
    from seedvc_amd import specs
    from seedvc_amd.vocoder import HiFT
    c, sd, _, _, _, _ = cases.hift_case("hift_r")
    hop, nh = specs.hift_total_upsample(c), c["nb_harmonics"] + 1
    assert c["in_channels"] == 80

    def draws(k):
        f0 = 80.0 + 300.0 * cases.rand(f"rt.hift.f0{k}", 144, 2, S_REAL)
        f0 = torch.where(cases.rand(f"rt.hift.uv{k}", 144, 2, S_REAL) < 0.25, torch.zeros_like(f0), f0)
        return dict(f0=f0, phase0=(cases.rand(f"rt.hift.phase{k}", 144, 2, nh, 1) * 2 - 1) * float(np.pi),
                    noise=cases.randn(f"rt.hift.noise{k}", 144, 2, nh, S_REAL * hop))
    q = hop // 4
    _run_real("hift", HiFT(c, sd, DEV), hop, 8 * q, 2 * q, q, q // 2,
              lambda mel, kw: O.hift_forward(sd, c, mel, kw["phase0"], kw["noise"], f0=kw["f0"]), draws)


def test_real_models_with_bigvgan():
    from seedvc_amd.vocoder import BigVGAN
    h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")              # upsample rates [4, 2]: hop 8
    _run_real("bigvgan", BigVGAN(h, vsd, DEV), 8, 96, 32, 16, 8, lambda mel, kw: O.bigvgan_forward(vsd, h, mel), lambda k: {})
