"""GPU side of long-form conversion as a pool of chunks: `svc_chunks_assemble` and `svc_chunks_gather_cond` against the
numpy statements of their formulas (long_batch_cases.py; test_host_long_batch.py pins those to the reference's fixtures),
`HotPath.convert_long_batch` bit for bit against the reference's own loop with the exact stand-ins, within the sequential
loop's bound of the oracle with real models, and with the real HiFT behind the grouped vocoder path."""
import ctypes as C

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
OVW = cases.CHUNK_OVERLAP * cases.CHUNK_HOP
i32 = lambda v: (C.c_int32 * len(v))(*[int(x) for x in v])      # noqa: E731


def _want(golden, key):
    return torch.from_numpy(golden[key].astype(np.float32).reshape(-1))


# ---------------------------------------------------------------------------------------------------- svc_chunks_assemble
def _assemble_gpu(waves, lens, first, last, ov, stride):
    from seedvc_amd import _lib
    fi, fo = (torch.from_numpy(f).to(DEV) for f in LB.fades(ov))
    W = torch.from_numpy(LB.padded_rows(waves, stride)).to(DEV)             # NaN at and above lens[k]
    n_out = sum(n - (0 if l else ov) for n, l in zip(lens, last))
    out = torch.full((n_out,), float("nan"), device=DEV)
    _lib.check(_lib.lib().svc_chunks_assemble(_lib.ptr(W), C.c_longlong(stride), i32(lens), i32(first), i32(last), len(lens),
                                              _lib.ptr(fi), _lib.ptr(fo), ov,
                                              _lib.ptr(out), C.c_longlong(n_out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("name", list(cases.CHUNKSTREAM_CASES))
@pytest.mark.parametrize("extra", [8, 5], ids=["stride_x4", "stride_odd"])      # the 16-byte and the 4-byte path
def test_assemble_equals_the_reference_stream(name, extra, golden):
    waves, lens, first, last = LB.chunkstream_rows(name)
    got = _assemble_gpu(waves, lens, first, last, OVW, max(lens) + extra)
    assert torch.equal(got, _want(golden, f"chunkstream.{name}.out"))


def test_assemble_nine_utterances_in_one_call(golden):
    rows = [LB.chunkstream_rows(n) for n in cases.CHUNKSTREAM_CASES] + [LB.chunkloop_rows(n) for n in cases.CHUNKLOOP_CASES]
    keys = [f"chunkstream.{n}.out" for n in cases.CHUNKSTREAM_CASES] + [f"chunkloop.{n}.out" for n in cases.CHUNKLOOP_CASES]
    waves, lens, first, last = (sum((r[i] for r in rows), []) for i in range(4))
    got = _assemble_gpu(waves, lens, first, last, OVW, max(lens) + 8)
    want = torch.cat([_want(golden, k) for k in keys])
    assert got.shape == want.shape
    assert torch.equal(got, want)
    assert torch.equal(got, torch.from_numpy(LB.assemble_model(LB.padded_rows(waves, max(lens) + 8), lens, first, last, OVW)))


def test_assemble_more_chunks_than_one_launch_takes():
    """70 chunks in 9 utterances (a seam crosses the 64-chunk launch boundary), lengths that are not multiples of 4."""
    rng = np.random.default_rng(5)
    ov, per_utt = 6, [9, 8, 8, 8, 8, 8, 8, 8, 5]
    lens, first, last = [], [], []
    for n in per_utt:
        for k in range(n):
            lens.append(int(rng.integers(ov, 40)) if k < n - 1 else int(rng.integers(0, 40)))
            first.append(k == 0)
            last.append(k == n - 1)
    assert len(lens) == 70 and not first[64]
    waves = [rng.standard_normal(n).astype(np.float32) for n in lens]
    got = _assemble_gpu(waves, lens, first, last, ov, 43)
    assert torch.equal(got, torch.from_numpy(LB.assemble_model(LB.padded_rows(waves, 43), lens, first, last, ov)))


# ------------------------------------------------------------------------------------------------- svc_chunks_gather_cond
@pytest.mark.parametrize("Dc", [6, 512], ids=["Dc6_4byte", "Dc512_16byte"])
def test_gather_cond_equals_the_model(Dc):
    from seedvc_amd import _lib
    rng = np.random.default_rng(Dc)
    U, Pmax, P, R, N = 2, 9, [5, 9], 300, 70                       # 70 chunks: more than one launch
    pc = rng.standard_normal((U, Pmax, Dc)).astype(np.float32)
    cond = rng.standard_normal((R, Dc)).astype(np.float32)
    utt = [int(k >= 40) for k in range(N)]
    rows = [int(rng.integers(0, 31)) for _ in range(N)]
    rows[3], rows[69] = 0, 30
    row0 = [int(rng.integers(0, R - r + 1)) for r in rows]
    row0[69] = R - 30                                                # the last rows of cond
    T = Pmax + 30 + 2                                                # two frames that no chunk fills
    mu = torch.full((N, T, Dc), float("nan"), device=DEV)
    d_pc, d_cond = torch.from_numpy(pc).to(DEV), torch.from_numpy(cond).to(DEV)
    _lib.check(_lib.lib().svc_chunks_gather_cond(_lib.ptr(d_pc), i32(P), U, Pmax, _lib.ptr(d_cond), R, i32(utt), i32(row0), i32(rows), N,
                                                 Dc, T, _lib.ptr(mu), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(mu.cpu(), torch.from_numpy(LB.gather_model(pc, P, cond, utt, row0, rows, T)))


# ------------------------------------------------------------------------------- convert_long_batch with the exact fakes
def _loop_utts(names):
    out = []
    for n in names:
        c = cases.chunkloop_case(n)
        out.append(tuple(c[k].to(DEV) for k in ("cond", "prompt_condition", "mel2", "style2")))
    return out


def _run_fakes(names, ragged, max_chunks=64, **kw):
    from seedvc_amd.pipeline import HotPath
    cfm, voc = LB.BatchedFakeCFM(DEV), LB.FakeVocoder(ragged)
    outs = HotPath(cfm, voc).convert_long_batch(_loop_utts(names), 10, 0.7, cases.CHUNK_HOP, cases.CHUNK_WINDOW,
                                                overlap_frame_len=cases.CHUNK_OVERLAP, max_chunks=max_chunks,
                                                ragged_vocoder=ragged, **kw)
    return [o.cpu() for o in outs], cfm, voc


def test_six_utterances_in_one_call_equal_the_references_own_loop(golden):
    names = list(cases.CHUNKLOOP_CASES)
    outs, cfm, voc = _run_fakes(names, True)
    assert cfm.batch_sizes == [15] and len(voc.calls) == 1 and voc.calls[0][2] is not None       # one sampler, one ragged vocoder call
    for n, o in zip(names, outs):
        want = _want(golden, f"chunkloop.{n}.out")
        assert o.shape == (1, want.numel())
        assert torch.equal(o[0], want), n
    grouped, cfm, voc = _run_fakes(names, False)
    assert [c[:2] for c in voc.calls] == [(11, 40), (3, 17), (1, 28)] and all(c[2] is None for c in voc.calls)
    for a, b in zip(outs, grouped):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", list(cases.CHUNKLOOP_CASES))
def test_each_utterance_alone_equals_the_references_own_loop(name, golden):
    for ragged in (True, False):
        outs, _, _ = _run_fakes([name], ragged)
        assert len(outs) == 1 and torch.equal(outs[0][0], _want(golden, f"chunkloop.{name}.out"))


def test_micro_batches_and_vocoder_paths_agree(golden):
    names = list(cases.CHUNKLOOP_CASES)
    want = [_want(golden, f"chunkloop.{n}.out") for n in names]
    for max_chunks in (64, 2, 1):
        for ragged in (True, False):
            outs, cfm, _ = _run_fakes(names, ragged, max_chunks)
            assert cfm.batch_sizes == [min(max_chunks, 15 - k) for k in range(0, 15, max_chunks)]
            for o, w in zip(outs, want):
                assert torch.equal(o[0], w), (max_chunks, ragged)


def test_noise_calls_and_an_empty_utterance(golden):
    """noise_fn sees the calls of the sequential loops, in plan order; an utterance without source frames gives (1, 0) and
    disturbs nothing around it."""
    from seedvc_amd.pipeline import HotPath
    utts = _loop_utts(["loop2", "loop5"])
    empty = (utts[0][0][:, :0], utts[0][1], utts[0][2], utts[0][3])
    seen = []

    def noise(T):
        seen.append(T)
        return torch.zeros(1, cases.CHUNK_C, T, device=DEV)
    outs = HotPath(LB.BatchedFakeCFM(DEV), LB.FakeVocoder(True)).convert_long_batch(
        [utts[0], empty, utts[1]], 10, 0.7, cases.CHUNK_HOP, cases.CHUNK_WINDOW, overlap_frame_len=cases.CHUNK_OVERLAP, noise_fn=noise)
    assert seen == [60, 37, 60, 60, 60, 60, 37]
    assert outs[1].shape == (1, 0)
    assert torch.equal(outs[0][0].cpu(), _want(golden, "chunkloop.loop2.out"))
    assert torch.equal(outs[2][0].cpu(), _want(golden, "chunkloop.loop5.out"))


# ------------------------------------------------------------------------------------------------------------ real models
HOP, WINDOW, OVERLAP, STEPS = 8, 40, 4, 3        # bigvgan_r2: upsample rates [4, 2]
_models_cache, _oracle_cache = {}, {}


def _models():
    if not _models_cache:
        from seedvc_amd.cfm import CFM
        from seedvc_amd.vocoder import BigVGAN
        cfg, sd, _, _ = cases.dit_case("tiny_r")
        h, vsd, _, _ = cases.bigvgan_case("bigvgan_r2")
        _models_cache.update(cfm=CFM(cfg, sd, DEV), voc=BigVGAN(h, vsd, DEV), cfg=cfg, sd=sd, h=h, vsd=vsd)
    return _models_cache


def _noise(cfg, T):
    return cases.randn(f"dl.z{T}", 3, 1, cfg["C"], T)


def _utt(cfg, S_total, P):
    """The inputs of test_device_chunk_loop_equals_host_chunk_loop, the prompt cut to its first P frames."""
    return (cases.randn(f"dl.cond{S_total}", 3, 1, S_total, cfg["Dc"]), cases.randn("dl.pc", 3, 1, 16, cfg["Dc"])[:, :P].contiguous(),
            cases.logmel("dl.mel2", 3, 1, cfg["C"], 16)[:, :, :P].contiguous(), cases.randn("dl.style", 3, 1, cfg["style_dim"]))


def _oracle(S_total, P):
    if (S_total, P) not in _oracle_cache:
        m = _models()
        cfg, sd = m["cfg"], m["sd"]
        cond, pc, mel2, style = _utt(cfg, S_total, P)
        _oracle_cache[(S_total, P)] = O.chunked_convert(
            lambda cc: O.cfm_sample(sd, cfg, _noise(cfg, cc.size(1)), cc.size(1), mel2, cc, style, STEPS, 0.7),
            lambda mel: O.bigvgan_forward(m["vsd"], m["h"], mel).reshape(1, -1), cond, pc, mel2, style, HOP, WINDOW,
            overlap_frame_len=OVERLAP)
    return _oracle_cache[(S_total, P)]


def _rms(a, b):
    return (a - b).pow(2).mean().sqrt().item()


def _run_real(specs):
    from seedvc_amd.pipeline import HotPath
    m = _models()
    cfg = m["cfg"]
    hp = HotPath(m["cfm"], m["voc"])
    noise = lambda T: _noise(cfg, T).to(DEV)      # noqa: E731
    utts = [tuple(t.to(DEV) for t in _utt(cfg, S, P)) for S, P in specs]
    outs = hp.convert_long_batch(utts, STEPS, 0.7, HOP, WINDOW, overlap_frame_len=OVERLAP, noise_fn=noise)
    seq = [hp.convert_long_device(*u, STEPS, 0.7, HOP, WINDOW, overlap_frame_len=OVERLAP, noise_fn=noise) for u in utts]
    return [o.cpu() for o in outs], [s.cpu() for s in seq]


@pytest.mark.parametrize("S_total", [70, 24, 45])          # several chunks / a single chunk / a short last chunk
def test_real_models_match_the_oracle(S_total):
    """Waveform RMS against `O.chunked_convert` below 5e-3: the bound test_chunked_long_utterance_matches_oracle applies to
    the sequential loop on the same models and sizes.  The difference to `convert_long_device` is printed, not bounded:
    which DiT kernel a launch takes depends on its row count, so a chunk in a batch may differ from its B = 1 run in the
    last bits (measured: RMS 1.9e-7 at 70 frames and 1.3e-7 at 45, against 3.1e-5 of either path to the oracle)."""
    (out,), (seq,) = _run_real([(S_total, 16)])
    ref = _oracle(S_total, 16)
    assert out.shape == ref.shape == seq.shape
    rms, d = _rms(out, ref), _rms(out, seq)
    print(f"S_total {S_total}: batched vs oracle RMS {rms:.3e}; sequential device loop vs oracle {_rms(seq, ref):.3e}; "
          f"batched vs device loop RMS {d:.3e}, bit-identical: {torch.equal(out, seq)}")
    assert rms < 5e-3
    if S_total <= WINDOW - 16:      # one chunk: the batched path makes the loop's own B = 1 calls, so the samples are the same
        assert torch.equal(out, seq)


def test_real_models_three_utterances_one_call():
    """The three as ONE call, one of them with a shorter prompt (P = 11: other windows, two chunks of 29 and 20 frames):
    each within the same bound of its own oracle run."""
    specs = [(70, 16), (24, 16), (45, 11)]
    outs, seqs = _run_real(specs)
    for (S_total, P), out, seq in zip(specs, outs, seqs):
        ref = _oracle(S_total, P)
        assert out.shape == ref.shape == seq.shape
        rms = _rms(out, ref)
        print(f"S_total {S_total}, P {P}: batched (3 utterances, one call) vs oracle RMS {rms:.3e}; sequential vs oracle "
              f"{_rms(seq, ref):.3e}; batched vs device loop RMS {_rms(out, seq):.3e}, bit-identical: {torch.equal(out, seq)}")
        assert rms < 5e-3


# ------------------------------------------------------------------------------------------- a vocoder without a ragged call
def test_hift_takes_the_grouped_path_with_pinned_draws():
    """The real HiFT behind the exact stand-in sampler: `ragged_vocoder=None` picks one plain call per distinct chunk length,
    `vocoder_kwargs_fn` pins phase0 / noise per chunk.  The mels are identical to the sequential loop's (the stand-in's rows
    are independent), only HiFT's batch size differs: RMS below 1e-4, the project's vocoder bound."""
    from seedvc_amd import specs
    from seedvc_amd.pipeline import HotPath
    from seedvc_amd.vocoder import HiFT
    c, sd, _, _, _, _ = cases.hift_case("hift_r")
    assert c["in_channels"] == 80
    hop, nh, Dc, P = specs.hift_total_upsample(c), c["nb_harmonics"] + 1, 8, 16
    hp = HotPath(LB.MelMixCFM(80, DEV), HiFT(c, sd, DEV))
    counter = [0]

    def draws(S):
        k = counter[0]
        counter[0] += 1
        return dict(phase0=((cases.rand(f"lb.hift.phase{k}", 9, 1, nh, 1) * 2 - 1) * float(np.pi)).to(DEV),
                    noise=cases.randn(f"lb.hift.noise{k}", 9, 1, nh, S * hop).to(DEV))
    utts = [(cases.randn(f"lb.hift.cond{S}", 9, 1, S, Dc).to(DEV), cases.randn("lb.hift.pc", 9, 1, P, Dc).to(DEV),
             cases.logmel("lb.hift.mel2", 9, 1, 80, P).to(DEV), cases.randn("lb.hift.style", 9, 1, 4).to(DEV)) for S in (70, 45)]
    outs = hp.convert_long_batch(utts, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP, vocoder_kwargs_fn=draws)
    assert counter[0] == 7                          # 70 frames: 24 24 24 10, 45 frames: 24 24 5 -- one call per chunk
    counter[0] = 0
    for u, out in zip(utts, outs):
        seq = hp.convert_long_device(*u, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP, vocoder_kwargs_fn=draws)
        assert out.shape == seq.shape and out.shape[1] == u[0].size(1) * hop
        rms = _rms(out.cpu(), seq.cpu())
        print(f"HiFT, {u[0].size(1)} frames: grouped batch vs device loop RMS {rms:.3e} (signal RMS {seq.pow(2).mean().sqrt().item():.3e})")
        assert rms < 1e-4
    with pytest.raises(ValueError):
        hp.convert_long_batch(utts, STEPS, 0.7, hop, WINDOW, overlap_frame_len=OVERLAP, vocoder_kwargs_fn=draws, ragged_vocoder=True)
