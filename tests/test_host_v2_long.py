"""Host side of whole-file v2 conversion (`V2HotPath.convert_long_batch`): the chunk table, the seam rule of the style
branch against `pipeline.stream_wave_chunks`, the per-chunk seeds, the argument errors (raised before a device is
touched) and the condition the GPU tests rest on -- enough files of v2_long_cases qualify."""
import numpy as np
import pytest
import torch

import v2_long_cases as L
from seedvc_amd.pipeline import V2HotPath, derive_seed, v2_chunk_plan, v2_file_record, v2_seam_plan, v2_target_frames

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------------------ chunk table
def test_chunk_plan_boundaries_and_errors():
    assert v2_chunk_plan(0, 5) == []
    assert v2_chunk_plan(1, 5) == [(0, 1, True)]
    assert v2_chunk_plan(5, 5) == [(0, 5, True)]
    assert v2_chunk_plan(6, 5) == [(0, 5, False), (5, 1, True)]
    assert v2_chunk_plan(10, 5) == [(0, 5, False), (5, 5, True)]
    assert v2_chunk_plan(23, 9) == [(0, 9, False), (9, 9, False), (18, 5, True)]
    assert v2_chunk_plan(3, 1) == [(0, 1, False), (1, 1, False), (2, 1, True)]
    for n in range(0, 40):
        for c in (1, 2, 7, 39, 40, 1000):
            plan = v2_chunk_plan(n, c)
            assert [p[0] for p in plan] == list(range(0, n, c))
            assert sum(p[1] for p in plan) == n and all(1 <= p[1] <= c for p in plan)
            assert [p[2] for p in plan] == [i + c >= n for i in range(0, n, c)]
            assert not plan or (plan[-1][2] and not any(p[2] for p in plan[:-1]))
    for bad in (0, -3):
        with pytest.raises(ValueError, match="chunk_tokens"):
            v2_chunk_plan(10, bad)


def test_file_record():
    tok = dict(wide=torch.zeros(1, 31, dtype=torch.int64), narrow=torch.zeros(1, 31, dtype=torch.int64),
               narrow_reduced=torch.zeros(1, 20, dtype=torch.int64))
    target = dict(P=3)
    r = v2_file_record(tok, 8 * 57 + 5, 8, target, length_adjust=1.1)
    assert r["target"] is target and r["src_narrow"] is tok["narrow_reduced"] and r["src_tokens"] is tok["wide"]
    assert r["frames_per_token"] == 57 / 20 * 1.1 and r["source_frames"] == int(57 * 1.1)
    assert v2_target_frames(r["frames_per_token"], 20) == int(57 / 20 * 1.1 * 20)
    empty = dict(tok, narrow_reduced=torch.zeros(1, 0, dtype=torch.int64))
    assert v2_file_record(empty, 100, 8, target)["frames_per_token"] == 0.0


# -------------------------------------------------------------------------------------------------------------- seam rule
def _check_files(lens_per_file, ov, rng):
    """lens_per_file: chunk wave lengths of every file (the final chunk of a file is its `is_last` chunk)."""
    files, is_last, waves = [], [], []
    for u, lens in enumerate(lens_per_file):
        for i, n in enumerate(lens):
            files.append(u)
            is_last.append(i == len(lens) - 1)
            waves.append(rng.standard_normal(n).astype(np.float32))
    got, plan = L.seam_model(waves, files, is_last, ov, len(lens_per_file))
    for u, lens in enumerate(lens_per_file):
        ks = [k for k in range(len(files)) if files[k] == u]
        want_kept = [len(waves[k]) > 0 and (len(waves[k]) >= 2 * ov or is_last[k]) for k in ks]
        assert [plan["kept"][k] for k in ks] == want_kept
        kept = [k for k, w in zip(ks, want_kept) if w]
        assert [k for k in ks if plan["first"][k]] == kept[:1] and [k for k in ks if plan["last"][k]] == kept[-1:]
        want = L.stream_reference([waves[k] for k in kept], ov, 1)
        assert got[u].dtype == np.float32 and got[u].shape == want.shape == (plan["out_lens"][u],)
        assert np.array_equal(got[u], want), (u, lens, ov)
    return plan


def test_seam_rule_equals_the_stream_over_the_kept_chunks():
    rng = np.random.default_rng(11)
    ov = 8
    # lengths on both sides of 2 ov, an empty last chunk, a short last chunk, a file with nothing kept, an empty file
    plan = _check_files([[16, 15, 40, 17, 5], [30, 16, 0], [15, 7, 0], [], [3], [15, 16], [0], [16, 31, 32, 1]], ov, rng)
    assert plan["kept"] == [True, False, True, True, True, True, True, False, False, False, False, True, False, True, False,
                            True, True, True, True]
    assert plan["out_lens"] == [16 + 40 + 17 - 3 * ov + 5, 30 - ov + 16, 0, 0, 3, 16, 0, 16 + 31 + 32 - 3 * ov + 1]
    for trial in range(60):
        ov = int(rng.integers(1, 12))
        files = []
        for _ in range(int(rng.integers(1, 5))):
            n = int(rng.integers(0, 7))
            files.append([int(rng.choice([0, ov - 1, ov, 2 * ov - 1, 2 * ov, 2 * ov + 1, int(rng.integers(0, 5 * ov))])) for _ in range(n)])
        _check_files(files, ov, rng)


def test_seam_plan_refuses_ragged_arguments():
    with pytest.raises(ValueError):
        v2_seam_plan([0, 0], [10], [False, True], 2, 1)


# ------------------------------------------------------------------------------------------------------------------ seeds
def test_chunk_seeds_are_derived_per_file_and_chunk():
    """What the style branch computes: chunk k of file u draws from derive_seed(seeds[u], k), k counted inside its file."""
    seeds = [7, 2 ** 64 - 1, 0]
    plan = [(u, j) for u, n in enumerate([23, 20, 0]) for j, _ in enumerate(v2_chunk_plan(n, 9))]
    got = [derive_seed(seeds[u], j) for u, j in plan]
    assert plan == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    assert len(set(got)) == len(got) and all(0 <= s < 2 ** 64 for s in got)
    assert got[3] == derive_seed(2 ** 64 - 1, 0) and got[2] == derive_seed(7, 2)


# ------------------------------------------------------------------------------------------------------- argument errors
class _AR:
    cfg = dict(max_seq_len=160)
    max_batch_size = 4


class _CFM:
    device = torch.device("cpu")
    in_channels = 80


def _file(f, **kw):
    u = L.file_inputs(f)
    target = dict(narrow=u["target_narrow"], tokens=u["target_tokens"], mel=u["target_mel"], style=u["style"], P=u["P"],
                  prompt_condition=torch.zeros(1, u["P"], 4))
    return dict(dict(target=target, src_narrow=u["src_narrow"], src_tokens=u["src_tokens"], frames_per_token=u["frames_per_token"],
                     source_frames=30), **kw)


def test_convert_long_batch_refusals_need_no_gpu():
    hp = V2HotPath(_AR(), None, None, _CFM(), None)
    kw = dict(max_context_window=40, hop=8)
    files = [_file(0), _file(1)]
    with pytest.raises(ValueError, match="seeds"):
        hp.convert_long_batch(files, 3, seeds=[1], **kw)
    with pytest.raises(ValueError, match="seeds"):
        hp.convert_long_batch(files, 3, seeds=[1, 2, 3], convert_style=False, **kw)
    with pytest.raises(ValueError, match="2\\^64"):
        hp.convert_long_batch(files, 3, seeds=[1, -2], **kw)
    with pytest.raises(ValueError, match="not both"):
        hp.convert_long_batch(files, 3, seeds=[1, 2], exp_noise_fn=lambda u, k: None, **kw)
    with pytest.raises(ValueError, match="not both"):
        hp.convert_long_batch(files, 3, seeds=[1, 2], noise_fn=lambda u, k, T: None, **kw)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="chunk_tokens"):
            hp.convert_long_batch(files, 3, ar_chunk_tokens=bad, **kw)
        with pytest.raises(ValueError, match="chunk_tokens"):
            hp.convert_long_batch([], 3, ar_chunk_tokens=bad, **kw)
    with pytest.raises(ValueError, match="max_chunks"):
        hp.convert_long_batch(files, 3, max_chunks=0, **kw)
    with pytest.raises(ValueError, match="style branch"):
        hp.convert_long_batch(files, 3, convert_style=False, return_parts=True, **kw)
    # an AR prompt that does not fit the 160-position cache: named by file and chunk, before anything is enqueued
    long_src = torch.zeros(1, 400, dtype=torch.int64)
    with pytest.raises(ValueError, match="file 1, chunk 0"):          # 3 + 154 + 2 + 2 = 161 rows
        hp.convert_long_batch([_file(0), _file(1, src_narrow=long_src)], 3, ar_chunk_tokens=154, **kw)
    with pytest.raises(ValueError, match="file 0, chunk 0"):          # without the target: 159 + 2 rows
        hp.convert_long_batch([_file(0, src_narrow=long_src)], 3, ar_chunk_tokens=159, anonymization_only=True, **kw)
    assert hp.convert_long_batch([], 3, **kw) == []
    assert hp.convert_long_batch([], 3, return_parts=True, **kw) == ([], [])
    assert hp.convert_long_batch([], 3, convert_style=False, **kw) == []


def test_session_close_frees_the_slots():
    """`ARSession.close`, the way out of an error between submit and the end of drain: nothing waits, nothing is in flight."""
    import ar_session_cases as S
    from seedvc_amd.ar import ARSession

    class Backend(S.FakeBackend):
        def session_retire(self, slot, n_tokens):
            return self.slots.pop(slot, None)

    be = Backend(2)
    sess = ARSession(be, steps_per_run=1)
    for name in "abcde":
        sess.submit(name, "", seed=1, max_new=9)
    assert sess.step() == [] and sess.n_active == 2 and sess.n_waiting == 3
    sess.close()
    assert sess.n_active == 0 and sess.n_waiting == 0 and be.slots == {}
    sess.close()                                    # idempotent
    t = sess.submit("f", "", seed=1, max_new=2)
    assert [k for k, _ in sess.drain()] == [t] and be.slots == {}


# ------------------------------------------------------------------------------------------- what the GPU tests rest on
def test_enough_files_qualify():
    q = L.qualified()
    print("qualified files:", q, {f: [c["ref_tokens"].shape[1] for c in L.file_case(f)["chunks"]] for f in L.FILES})
    assert len(q) >= 4
    three = [f for f in q if len(L.file_case(f)["chunks"]) == 3]
    assert len(three) >= 3                                              # the oracle test and the pool test
    assert 4 in q and all(c["ylen"] * L.HOP < 2 * 16 * L.HOP for c in L.file_case(4)["chunks"])      # the short-chunk case
    assert L.anonymized_case() is not None
