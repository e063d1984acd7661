"""CPU side of long-form conversion as a pool of chunks (`svc_chunks_gather_cond`, `svc_chunks_assemble`,
`pipeline.long_batch_plan`, `HotPath.convert_long_batch`): the entry points are declared, exported and bound; their
argument checks come before anything touches a device; the planner gives the drivers' chunk boundaries, output lengths and
micro-batches; and the numpy model the GPU tests compare with reproduces the reference-generated fixtures bit for bit."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svc_chunks_gather_cond", "svc_chunks_assemble")
torch.set_grad_enabled(False)
i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
ll = ctypes.c_longlong
ONE = ctypes.c_void_p(16)                           # never dereferenced: the checks come first


def test_chunk_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert callable(pipeline.long_batch_plan)
    p = inspect.signature(pipeline.HotPath.convert_long_batch).parameters
    assert p["overlap_frame_len"].default == 16 and p["max_chunks"].default == 64 and p["ragged_vocoder"].default is None
    assert p["noise_fn"].default is None and p["vocoder_kwargs_fn"].default is None


def _gather(prompt_lens=(3,), U=1, Pmax=4, R=20, utt=(0,), row0=(2,), rows=(5,), Dc=8, T=9):
    from seedvc_amd import _lib
    return _lib.lib().svc_chunks_gather_cond(ONE, i32(*prompt_lens), U, Pmax, ONE, R, i32(*utt), i32(*row0), i32(*rows), len(utt),
                                             Dc, T, ONE, None)


@pytest.mark.parametrize("bad", [dict(utt=(1,)), dict(utt=(-1,)), dict(prompt_lens=(5,)), dict(prompt_lens=(-1,)), dict(rows=(-1,)),
                                 dict(row0=(-1,)), dict(row0=(16,)), dict(rows=(7,)), dict(Dc=0),
                                 dict(prompt_lens=(3, 4), U=2, utt=(0, 1), row0=(2, 7), rows=(5, 6))],
                         ids=["utt_above", "utt_negative", "prompt_above_Pmax", "prompt_negative", "rows_negative", "row0_negative",
                              "rows_past_R", "prompt_plus_rows_above_T", "Dc_zero", "second_chunk_above_T"])
def test_gather_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _gather(**bad) != 0
    assert b"chunks_gather_cond" in _lib.lib().svc_last_error()


def _assemble(lens=(40, 40, 20), first=(1, 0, 0), last=(0, 0, 1), ov=16, out_len=None, stride=64):
    from seedvc_amd import _lib
    if out_len is None:
        out_len = sum(n - (0 if l else ov) for n, l in zip(lens, last))
    return _lib.lib().svc_chunks_assemble(ONE, ll(stride), i32(*lens), i32(*first), i32(*last), len(lens), ONE, ONE, ov, ONE,
                                          ll(out_len), None)


@pytest.mark.parametrize("bad", [dict(lens=(40, -1, 20), out_len=44), dict(lens=(40, 10, 20)), dict(first=(1, 1, 0)),
                                 dict(last=(0, 1, 1), out_len=84), dict(first=(0, 0, 0)), dict(last=(0, 0, 0), out_len=52),
                                 dict(out_len=67), dict(ov=-1, out_len=100)],
                         ids=["negative_length", "middle_chunk_shorter_than_overlap", "first_after_a_chunk_that_is_not_last",
                              "not_first_after_a_last_chunk", "first_chunk_not_flagged_first", "last_chunk_not_flagged_last",
                              "out_len_is_not_the_sum_of_bodies", "negative_overlap"])
def test_assemble_argument_errors_need_no_gpu(bad):
    from seedvc_amd import _lib
    assert _assemble(**bad) != 0
    assert b"chunks_assemble" in _lib.lib().svc_last_error()


def test_empty_calls_touch_nothing():
    """No chunks: nothing to launch, so even null pointers are fine (and no device is needed)."""
    from seedvc_amd import _lib
    lib = _lib.lib()
    assert lib.svc_chunks_gather_cond(None, i32(), 0, 0, None, 0, i32(), i32(), i32(), 0, 8, 9, None, None) == 0
    assert lib.svc_chunks_assemble(None, ll(0), i32(), i32(), i32(), 0, None, None, 16, None, ll(0), None) == 0
    assert lib.svc_chunks_assemble(None, ll(0), i32(), i32(), i32(), 0, None, None, 16, None, ll(8), None) != 0


# ---------------------------------------------------------------------------------------------------------- the planner
LOOP_SAMPLES = {"loop1": 320, "loop1s": 136, "loop2": 328, "loop2b": 512, "loop4": 800, "loop5": 904}


def _loop_plan(names, **kw):
    from seedvc_amd.pipeline import long_batch_plan
    return long_batch_plan([cases.CHUNKLOOP_CASES[n][0] for n in names], [cases.CHUNK_P] * len(names), cases.CHUNK_WINDOW,
                           cases.CHUNK_OVERLAP, cases.CHUNK_HOP, **kw)


def test_plan_equals_chunk_plan_per_utterance(golden):
    from seedvc_amd.pipeline import chunk_plan
    names = list(cases.CHUNKLOOP_CASES)
    plan = _loop_plan(names)
    assert plan["out_lens"] == [LOOP_SAMPLES[n] for n in names]
    assert plan["out_lens"] == [golden[f"chunkloop.{n}.out"].shape[-1] for n in names]
    for u, n in enumerate(names):
        mine = [c for c in plan["chunks"] if c[0] == u]
        ref = chunk_plan(cases.CHUNKLOOP_CASES[n][0], cases.CHUNK_WINDOW - cases.CHUNK_P, cases.CHUNK_OVERLAP)
        assert [(c[1], c[2], c[4]) for c in mine] == ref
        assert [c[3] for c in mine] == [k == 0 for k in range(len(ref))]
        assert _loop_plan([n])["out_lens"] == [LOOP_SAMPLES[n]]
    assert [c[0] for c in plan["chunks"]] == sorted(c[0] for c in plan["chunks"])            # utterance-major
    assert [(c[1], c[2]) for c in _loop_plan(["loop5"])["chunks"]] == [(0, 40), (24, 40), (48, 40), (72, 40), (96, 17)]
    assert _loop_plan(["loop5"])["bodies"] == [192, 192, 192, 192, 136]
    assert sum(plan["bodies"]) == sum(plan["out_lens"])


def test_plan_micro_batches():
    names = list(cases.CHUNKLOOP_CASES)
    n = len(_loop_plan(names)["chunks"])
    assert n == 1 + 1 + 2 + 2 + 4 + 5
    assert _loop_plan(names, max_chunks=64)["micro_batches"] == [(0, n)]
    assert _loop_plan(names, max_chunks=2)["micro_batches"] == [(k, min(k + 2, n)) for k in range(0, n, 2)]
    assert _loop_plan(names, max_chunks=1)["micro_batches"] == [(k, k + 1) for k in range(n)]
    for mc in (1, 2, 64):
        assert _loop_plan(names, max_chunks=mc)["chunks"] == _loop_plan(names)["chunks"]


def test_plan_errors_and_empty_utterances():
    from seedvc_amd.pipeline import long_batch_plan
    with pytest.raises(ValueError):
        long_batch_plan([100], [20], 60, 16, 8, max_chunks=0)
    with pytest.raises(ValueError):                 # window 36 - 20 = 16 = overlap and more than one chunk: no progress
        long_batch_plan([100], [20], 36, 16, 8)
    with pytest.raises(ValueError):                 # the second utterance's longer prompt leaves no window
        long_batch_plan([30, 30], [20, 50], 50, 16, 8)
    ok = long_batch_plan([16], [20], 36, 16, 8)     # one chunk needs no progress
    assert ok["chunks"] == [(0, 0, 16, True, True)] and ok["out_lens"] == [128]
    empty = long_batch_plan([0], [20], 60, 16, 8)
    assert empty == dict(chunks=[], bodies=[], out_lens=[0], micro_batches=[])
    mid = long_batch_plan([41, 0, 17], [20, 20, 20], 60, 16, 8)
    assert mid["out_lens"] == [328, 0, 136]
    assert mid["chunks"] == [(0, 0, 40, True, False), (0, 24, 17, False, True), (2, 0, 17, True, True)]
    assert mid["micro_batches"] == [(0, 3)]


def test_convert_long_batch_refusals_need_no_gpu():
    from seedvc_amd.pipeline import HotPath
    hp = HotPath(None, None)
    assert hp.convert_long_batch([], 10, 0.7, 8, 60) == []
    c = cases.chunkloop_case("loop2")
    utt = (c["cond"], c["prompt_condition"], c["mel2"], c["style2"])
    with pytest.raises(ValueError, match="vocoder_kwargs_fn"):
        hp.convert_long_batch([utt], 10, 0.7, 8, 60, vocoder_kwargs_fn=lambda s: {}, ragged_vocoder=True)
    with pytest.raises(ValueError, match="would not advance"):
        hp.convert_long_batch([utt], 10, 0.7, 8, 36, ragged_vocoder=False)
    with pytest.raises(ValueError, match="max_chunks"):
        hp.convert_long_batch([utt], 10, 0.7, 8, 60, max_chunks=0, ragged_vocoder=False)


# ----------------------------------------------------------------------------- the model the GPU tests are compared with
@pytest.mark.parametrize("name", list(cases.CHUNKSTREAM_CASES))
def test_assemble_model_equals_the_reference_stream(name, golden):
    waves, lens, first, last = LB.chunkstream_rows(name)
    got = LB.assemble_model(LB.padded_rows(waves, max(lens) + 5), lens, first, last, cases.CHUNK_OVERLAP * cases.CHUNK_HOP)
    assert np.array_equal(got, golden[f"chunkstream.{name}.out"].astype(np.float32).reshape(-1))


@pytest.mark.parametrize("name", list(cases.CHUNKLOOP_CASES))
def test_assemble_model_equals_the_reference_loop(name, golden):
    waves, lens, first, last = LB.chunkloop_rows(name)
    got = LB.assemble_model(LB.padded_rows(waves, max(lens) + 3), lens, first, last, cases.CHUNK_OVERLAP * cases.CHUNK_HOP)
    want = golden[f"chunkloop.{name}.out"].astype(np.float32).reshape(-1)
    assert got.shape == want.shape == (LOOP_SAMPLES[name],)
    assert np.array_equal(got, want)


def test_batched_fakes_equal_the_case_fakes():
    """Row b of the batched stand-ins is the B = 1 stand-in of cases.py on row b, bit for bit (CPU tensors here)."""
    mu = cases.randn("lbc.mu", 7, 3, 30, cases.CHUNK_DC)
    mel = LB.BatchedFakeCFM("cpu").inference(mu, None, None, None, None, 10)
    for b in range(3):
        assert torch.equal(mel[b:b + 1], cases.fake_sampler(mu[b:b + 1], cases.CHUNK_P))
    plain, ragged = LB.FakeVocoder(False), LB.FakeVocoder(True)
    w = plain(mel)
    for b in range(3):
        assert torch.equal(w[b:b + 1], cases.fake_vocoder(mel[b:b + 1]))
    lens = [30, 0, 11]
    wr = ragged(mel, lens=lens)
    for b, n in enumerate(lens):
        assert torch.equal(wr[b, 0, :n * cases.CHUNK_HOP], w[b, 0, :n * cases.CHUNK_HOP]) and not wr[b, 0, n * cases.CHUNK_HOP:].any()
    mu80 = LB.MelMixCFM(80, "cpu").inference(mu, None, None, None, None, 10)
    assert mu80.shape == (3, 80, 30) and mu80.min() >= -11.5 and mu80.max() <= 2.0
    assert torch.equal(mu80[1:2], LB.MelMixCFM(80, "cpu").inference(mu[1:2], None, None, None, None, 10))
