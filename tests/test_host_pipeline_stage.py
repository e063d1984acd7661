"""CPU side of the second half every composite call of `pipeline` shares (`_stack_prompts`, `_vocode`, `_row_views`,
`_vocoder_seeds`, `_cos2_windows`) and of the host helpers under it (`_lib.int_list`, `_lib.i32_host`): which vocoder calls a
batch takes, with which rows, keywords and seeds, on CPU tensors with the recording stand-ins of `long_batch_cases`; and that
the stage exists once in the package's source."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import cases
import long_batch_cases as LB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)
LENS = [5, 3, 5, 0, 3, 7]
HOP = cases.CHUNK_HOP


def _mel():
    return cases.randn("stage.mel", 151, len(LENS), cases.CHUNK_C, max(LENS))


def _check_rows(mel, S, rows):
    assert len(rows) == len(S)
    for b, (m, w) in enumerate(rows):
        assert m.shape == (1, mel.size(1), S[b]) and w.shape == (1, S[b] * HOP)
        assert torch.equal(m, mel[b:b + 1, :, :S[b]])
        if S[b]:
            assert torch.equal(w, cases.fake_vocoder(mel[b:b + 1, :, :S[b]]).reshape(1, -1)), b


@pytest.mark.parametrize("ragged,want", [(True, [(6, 7, LENS)]), (False, [(2, 5, None), (2, 3, None), (1, 7, None)])],
                         ids=["ragged", "grouped"])
def test_vocoder_calls_and_rows(ragged, want):
    from seedvc_amd.pipeline import _row_views, _vocode
    mel, voc = _mel(), LB.FakeVocoder(True)
    calls = _vocode(voc, mel, LENS, ragged, "stage", hop=HOP)
    assert voc.calls == want
    assert [c.frames for c in calls] == [w[1] for w in want]
    if not ragged:          # members as slices, in order of first appearance
        assert [c.runs for c in calls] == [[(0, 1), (2, 3)], [(1, 2), (4, 5)], [(5, 6)]]
    _check_rows(mel, LENS, _row_views(mel, LENS, calls))


@pytest.mark.parametrize("ragged", [True, False])
def test_one_length_is_one_plain_call_on_the_input_itself(ragged):
    from seedvc_amd.pipeline import _row_views, _vocode
    mel, seen = _mel()[:3, :, :4].contiguous(), []
    voc = LB.FakeVocoder(True)
    calls = _vocode(lambda m, **kw: seen.append(m) or voc(m, **kw), mel, [4, 4, 4], ragged, "stage", hop=HOP)
    assert voc.calls == [(3, 4, None)] and len(seen) == 1 and seen[0] is mel and calls[0].mel is mel
    _check_rows(mel, [4, 4, 4], _row_views(mel, [4, 4, 4], calls))
    # no frames at all: no call, empty rows
    assert _vocode(voc, mel, [0, 0, 0], ragged, "stage") == [] and len(voc.calls) == 1
    _check_rows(mel, [0, 0, 0], _row_views(mel, [0, 0, 0], []))


def test_row_kwargs_arrive_in_member_order_and_whole_batch_kwargs_need_a_whole_batch_call():
    from seedvc_amd.pipeline import _vocode
    mel, seen = _mel(), []

    def voc(m, tag=None, f0=None):
        seen.append((m.size(0), None if tag is None else tag.reshape(-1).tolist(), f0))
        return LB.FakeVocoder(False)(m)
    _vocode(voc, mel, LENS, False, "stage", row_kwargs=[{"tag": torch.tensor([[b]])} for b in range(len(LENS))])
    assert seen == [(2, [0, 2], None), (2, [1, 4], None), (1, [5], None)]
    del seen[:]
    f0 = torch.zeros(3, 4)
    _vocode(voc, mel[:3, :, :4].contiguous(), [4, 4, 4], False, "stage", vocoder_kwargs={"f0": f0})
    assert len(seen) == 1 and seen[0][2] is f0
    with pytest.raises(ValueError, match="stage: vocoder_kwargs"):
        _vocode(voc, mel, LENS, False, "stage", vocoder_kwargs={"f0": f0})


def test_a_wrong_sample_count_is_refused_with_the_callers_prefix():
    from seedvc_amd.pipeline import _vocode
    for what in ("convert_long_batch", "RealtimeEngine.step"):
        with pytest.raises(ValueError, match=re.escape(f"{what}: the vocoder gave {5 * HOP} samples per row, {5 * (HOP + 1)} expected")):
            _vocode(LB.FakeVocoder(False), _mel()[:2, :, :5].contiguous(), [5, 5], False, what, hop=HOP + 1)


def _recording_hift():
    from seedvc_amd.vocoder import HiFT

    class Recording(HiFT):
        def __call__(self, x, lens=None, **kw):
            self.seen.append((x.size(0), lens, kw))
            return LB.FakeVocoder(True)(x, **({} if lens is None else {"lens": lens}))
    voc = HiFT.__new__(Recording)
    voc._h, voc.seen = None, []
    return voc


def test_seeds_reach_a_hift_only_and_follow_the_members():
    from seedvc_amd.pipeline import HotPath, _vocode, _vocoder_seeds
    mel, seeds = _mel(), [10, 11, 12, 13, 14, 15]
    voc = _recording_hift()
    _vocode(voc, mel, LENS, False, "stage", seeds=seeds)
    assert voc.seen == [(2, None, {"seeds": [10, 12]}), (2, None, {"seeds": [11, 14]}), (1, None, {"seeds": [15]})]
    del voc.seen[:]
    _vocode(voc, mel, LENS, True, "stage", seeds=seeds)
    assert voc.seen == [(6, LENS, {"seeds": seeds})]
    del voc.seen[:]
    _vocode(voc, mel, LENS, False, "stage", seeds=None)
    assert [kw for _, _, kw in voc.seen] == [{}, {}, {}]
    plain = LB.FakeVocoder(True)                     # asserts that it gets no keyword but lens
    _vocode(plain, mel, LENS, True, "stage", seeds=seeds)
    _vocode(plain, mel, LENS, False, "stage", seeds=seeds)
    assert len(plain.calls) == 4
    assert _vocoder_seeds(voc, seeds) == {"seeds": seeds} and _vocoder_seeds(voc, None) == {} and _vocoder_seeds(plain, seeds) == {}
    # a HotPath reaches the rule through its own method: the seam the seeded long-form test hooks
    hp, hooked = HotPath(None, voc), []
    assert hp._vocoder_seeds(seeds) == {"seeds": seeds}
    _vocode(plain, mel, LENS, False, "stage", seeds=seeds, seed_kw=lambda s: hooked.append(s) or {})
    assert hooked == [[10, 12], [11, 14], [15]]


def test_prompt_stacker():
    from seedvc_amd.pipeline import _stack_prompts
    Dc, C, Ds = cases.CHUNK_DC, cases.CHUNK_C, 3
    recs = [(cases.randn(f"stage.pc{P}", 152, 1, P, Dc), cases.randn(f"stage.pm{P}", 152, 1, C, P), cases.randn(f"stage.st{P}", 152, 1, Ds))
            for P in (5, 3)]
    st = _stack_prompts(recs)
    assert st["P"] == [5, 3] and st["Pmax"] == 5
    assert st["prompt_condition"].shape == (2, 5, Dc) and st["mel"].shape == (2, C, 5) and st["style"].shape == (2, Ds)
    for b, (pc, mel, style) in enumerate(recs):
        P = st["P"][b]
        assert torch.equal(st["prompt_condition"][b, :P], pc[0]) and torch.equal(st["mel"][b, :, :P], mel[0])
        assert torch.equal(st["style"][b], style[0])
        assert not st["prompt_condition"][b, P:].any() and not st["mel"][b, :, P:].any()


@pytest.mark.parametrize("n", [1, 64, 4096])
def test_cos2_windows(n):
    from seedvc_amd.pipeline import _cos2_windows
    fade_in, fade_out = _cos2_windows(n)
    assert fade_in.dtype == fade_out.dtype == np.float64
    assert np.array_equal(fade_in, np.cos(np.linspace(np.pi / 2, 0, n)) ** 2)
    assert np.array_equal(fade_out, np.cos(np.linspace(0, np.pi / 2, n)) ** 2)
    assert all(np.array_equal(a, b) for a, b in zip(_cos2_windows(n), LB.fades(n)))


def test_host_integer_helpers():
    from seedvc_amd import _lib
    for v in ([3, 0, 7], torch.LongTensor([3, 0, 7]), np.array([3, 0, 7], np.int64), (3, 0, 7)):
        got = _lib.int_list(v)
        assert got == [3, 0, 7] and all(type(x) is int for x in got)
    assert _lib.int_list([]) == [] and len(_lib.i32_host([])) == 0
    a = _lib.i32_host([1, -2, 2 ** 31 - 1])
    assert list(a) == [1, -2, 2 ** 31 - 1] and a._type_ is _lib.C.c_int32
    assert _lib.seed_ints(torch.tensor([1, 2]), 2, "x") == [1, 2]


def test_hift_refuses_before_anything_touches_a_device():
    from seedvc_amd.vocoder import HiFT
    voc = HiFT.__new__(HiFT)
    voc.cfg, voc.total_up, voc.device, voc._h = dict(nb_harmonics=8), 8, torch.device("cpu"), None
    x = torch.zeros(3, 80, 5)
    with pytest.raises(ValueError, match="seeds or phase0 / noise"):
        voc(x, seeds=[1, 2, 3], noise=torch.zeros(3, 9, 40))
    with pytest.raises(ValueError, match="lens has 2 entries, the batch has 3"):
        voc(x, lens=[5, 4])
    with pytest.raises(ValueError, match="lens has 4 entries"):
        voc(x, lens=torch.LongTensor([5, 4, 3, 2]), seeds=[1, 2, 3])


def test_the_stage_exists_once_in_the_source():
    src = {p: open(p).read() for p in glob.glob(os.path.join(ROOT, "seed-vc_amd", "*.py"))}
    for name in ("svc_mel_strip_prompt", "svc_v2_assemble_cond"):
        assert sum(s.count(f".{name}(") for s in src.values()) == 1, name
    pipeline = src[os.path.join(ROOT, "seed-vc_amd", "pipeline.py")]
    assert len(re.findall(r"isinstance\([^()]*\bHiFT\)", pipeline)) == 1
    assert "lambda v: (C.c_int32" not in pipeline and "tolist() if torch.is_tensor" not in pipeline
