"""CPU side of per-utterance sampler settings (`svc_cfm_sample_rows`, `svc_cfm_rows_plan`, `CFM.inference_rows`,
`CFM.rows_plan`, `RealtimeEngine.set_sampler`, `sampler=` of the long-form entry points): the entry points are declared,
exported and bound; the partition into classes is the documented one; bad rows and NULL arguments are refused before
anything touches a device; and the mirrors hand every utterance its own settings."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import cases
import long_batch_cases as LB
import realtime_cases as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svc_cfm_sample_rows", "svc_cfm_rows_plan")
torch.set_grad_enabled(False)

V1_ROWS = [(4, .7), (4, .3), (2, .7), (4, 0.), (4, 1.)]
V1_PLAN = ([0, 0, 1, 2, 0], [2, 2, 1])
# one row per v2 guidance structure, then a second row of every structure with other rates (and another temperature)
V2_ROWS = [(3, (.7, .7), 1.0, True), (3, (0., 0.)), (3, (0., .7)), (3, (.7, 0.)), (3, (.7, .7)),
           (3, (.3, 1.), .5, True), (3, (0., 0.), .8), (3, (0., .3), .5), (3, (1., 0.), .8), (3, (.4, .9), .5)]
V2_PLAN = ([0, 1, 2, 3, 4, 0, 1, 2, 3, 4], [2, 1, 2, 2, 3])


def _rows(settings):
    from seedvc_amd import _lib
    from seedvc_amd.cfm import sampler_setting
    rows = (_lib.CfmRow * len(settings))()
    for r, e in zip(rows, settings):
        r.n_timesteps, (r.cfg_rate[0], r.cfg_rate[1]), r.temperature, rv = sampler_setting(e)
        r.random_voice = int(rv)
    return rows


def _plan(version, settings):
    from seedvc_amd import _lib
    B = len(settings)
    class_of, n_streams = (ctypes.c_int32 * B)(), (ctypes.c_int32 * B)()
    n = _lib.lib().svc_cfm_rows_plan(version, _rows(settings), B, class_of, n_streams)
    return n, list(class_of), list(n_streams[:max(n, 0)])


def _bare_cfm(version):
    from seedvc_amd.cfm import CFM
    cfm = CFM.__new__(CFM)                         # no handle, no device: the plan needs neither
    cfm.cfg, cfm.in_channels, cfm.device = dict(version=version), 80, torch.device("cpu")
    return cfm


def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline
    from seedvc_amd.cfm import CFM
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
        assert getattr(_lib.lib(), name).argtypes, f"{name} has no prototype"
    assert "svc_cfm_row_t" in header and ctypes.sizeof(_lib.CfmRow) == 20
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert callable(CFM.inference_rows) and callable(CFM.rows_plan) and callable(pipeline.RealtimeEngine.set_sampler)
    for fn in (pipeline.HotPath.convert_long_batch, pipeline.V2HotPath.convert_long_batch):
        p = inspect.signature(fn).parameters["sampler"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__qualname__
    # the signatures that are part of a contract keep their parameter lists
    assert list(inspect.signature(CFM.inference).parameters) == [
        "self", "mu", "x_lens", "prompt", "style", "f0", "n_timesteps", "temperature", "inference_cfg_rate", "random_voice", "z",
        "prompt_lens", "seeds"]
    E = pipeline.RealtimeEngine
    assert list(inspect.signature(E.step).parameters)[1:] == ["slots", "content", "n_timesteps", "inference_cfg_rate", "z",
                                                              "vocoder_kwargs", "return_parts"]
    assert list(inspect.signature(E.step_seeded).parameters)[1:] == ["slots", "content", "n_timesteps", "inference_cfg_rate", "seeds",
                                                                     "vocoder_kwargs", "return_parts"]


def test_plan_v1():
    n, class_of, streams = _plan(1, V1_ROWS)
    assert (n, class_of, streams) == (3, *V1_PLAN)


def test_plan_v2_every_structure_is_a_class_and_rates_do_not_split_it():
    n, class_of, streams = _plan(2, V2_ROWS)
    assert (n, class_of, streams) == (5, *V2_PLAN)
    assert _plan(2, V2_ROWS[:5]) == (5, [0, 1, 2, 3, 4], [2, 1, 2, 2, 3])
    # the step count does split: the same structures at another count are new classes
    n, class_of, _ = _plan(2, V2_ROWS[:5] + [(2,) + r[1:] for r in V2_ROWS[:5]])
    assert n == 10 and class_of == list(range(10))


@pytest.mark.parametrize("version", [1, 2])
def test_temperature_never_splits_a_class(version):
    rows = [(3, .7, t) for t in (1.0, .5, .8, 0.0, 2.0)] + [(3, 0., t) for t in (1.0, .5)]
    n, class_of, streams = _plan(version, rows)
    assert (n, class_of) == (2, [0] * 5 + [1] * 2) and streams == [2 if version == 1 else 3, 1]


@pytest.mark.parametrize("version,rows,msg", [
    (1, [(4, .7), (0, .7)], b"rows[1] has n_timesteps < 1"),
    (2, [(0, .7)], b"rows[0] has n_timesteps < 1"),
    (1, [(4, float("nan"))], b"rows[0] has a non-finite cfg_rate"),
    (2, [(4, .7), (4, (.7, float("inf")))], b"rows[1] has a non-finite cfg_rate"),
    (1, [(4, .7, float("nan"))], b"rows[0] has a non-finite temperature"),
    (1, [(4, .7), (4, .7), (4, .7, 1.0, True)], b"rows[2] sets random_voice, which is v2 only"),
], ids=["steps0_v1", "steps0_v2", "nan_rate", "inf_rate_v2", "nan_temperature", "random_voice_v1"])
def test_plan_refuses_bad_rows_with_a_message(version, rows, msg):
    from seedvc_amd import _lib
    n, _, _ = _plan(version, rows)
    err = _lib.lib().svc_last_error()
    assert n < 0 and b"svc_cfm_rows_plan" in err and msg in err, err
    assert _lib.lib().svc_cfm_rows_plan(version, None, 3, None, None) < 0
    assert _lib.lib().svc_cfm_rows_plan(3, _rows(V1_ROWS), 5, None, None) < 0


def test_sample_rows_argument_checks_need_no_gpu():
    """NULL handle, NULL rows, neither z nor seeds: refused by the checks that come before any HIP call."""
    from seedvc_amd import _lib
    l = _lib.lib()
    rows, seeds = _rows(V1_ROWS), (ctypes.c_uint64 * 5)(1, 2, 3, 4, 5)
    handle = ctypes.c_void_p(16)                   # never dereferenced: the refusals below come first
    a = _lib.CfmArgs()
    a.B, a.T, a.P = 5, 12, 4
    assert l.svc_cfm_sample_rows(None, ctypes.byref(a), rows, seeds, None) != 0 and b"svc_cfm_sample_rows" in l.svc_last_error()
    assert l.svc_cfm_sample_rows(handle, None, rows, seeds, None) != 0
    assert l.svc_cfm_sample_rows(handle, ctypes.byref(a), None, seeds, None) != 0 and b"rows is NULL" in l.svc_last_error()
    assert a.z is None
    assert l.svc_cfm_sample_rows(handle, ctypes.byref(a), rows, None, None) != 0 and b"both NULL" in l.svc_last_error()


def test_mirror_plan_agrees_with_the_library():
    assert _bare_cfm(1).rows_plan(V1_ROWS) == V1_PLAN
    assert _bare_cfm(2).rows_plan(V2_ROWS) == V2_PLAN
    as_dicts = [dict(n_timesteps=n, inference_cfg_rate=r) for n, r in V1_ROWS]
    assert _bare_cfm(1).rows_plan(as_dicts) == V1_PLAN
    with pytest.raises(ValueError, match="n_timesteps < 1"):
        _bare_cfm(1).rows_plan([(0, .7)])
    with pytest.raises(ValueError, match="random_voice"):
        _bare_cfm(1).rows_plan([(3, .7, 1.0, True)])
    with pytest.raises(ValueError, match="an entry"):
        _bare_cfm(1).rows_plan([dict(n_timesteps=3)])
    with pytest.raises(ValueError, match="an entry"):
        _bare_cfm(1).rows_plan([(3,)])


def test_mirror_refuses_a_settings_list_of_the_wrong_length():
    mu, prompt, style = torch.zeros(3, 12, 8), torch.zeros(3, 80, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match="2 settings for 3"):
        _bare_cfm(1).inference_rows(mu, [12] * 3, prompt, style, [(2, .7), (2, .3)], seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="seeds or z"):
        _bare_cfm(1).inference_rows(mu, [12] * 3, prompt, style, [(2, .7)] * 3, seeds=[1, 2, 3], z=torch.zeros(3, 80, 12))
    with pytest.raises(ValueError, match="2 seeds for 3"):
        _bare_cfm(1).inference_rows(mu, [12] * 3, prompt, style, [(2, .7)] * 3, seeds=[1, 2])


# ------------------------------------------------------------------------------------------- the engine and the pool
class RecordingCFM(LB.BatchedFakeCFM):
    """The exact stand-in sampler, recording every call: ("inference", B, n_timesteps, rate, keywords) or
    ("inference_rows", normalised per-row settings, keywords)."""

    def __init__(self, device="cpu"):
        super().__init__(device)
        self.calls = []

    def inference(self, mu, x_lens, prompt, style, f0, n, inference_cfg_rate=0.7, z=None, prompt_lens=None, **kw):
        self.calls.append(("inference", mu.size(0), n, inference_cfg_rate, dict(kw)))
        return super().inference(mu, x_lens, prompt, style, f0, n, inference_cfg_rate, z, prompt_lens)

    def inference_rows(self, mu, x_lens, prompt, style, settings, z=None, prompt_lens=None, **kw):
        from seedvc_amd.cfm import sampler_setting
        assert len(settings) == mu.size(0)
        self.calls.append(("inference_rows", [sampler_setting(e) for e in settings], dict(kw)))
        return super().inference(mu, x_lens, prompt, style, None, 0, 0.0, z, prompt_lens)


def test_set_sampler_is_a_per_slot_setting():
    from seedvc_amd.pipeline import RealtimeEngine
    cfm = RecordingCFM()
    eng = RealtimeEngine(RT.FakeLR(), cfm, RT.FakeVocoder(), max_streams=3, **RT.FAKE_GEOMETRY)
    ref = (torch.zeros(1, 5, cases.CHUNK_DC), torch.zeros(1, cases.CHUNK_C, 5), torch.zeros(1, 3))
    with pytest.raises(ValueError, match="slot 0 is not open"):
        eng.set_sampler(0, n_timesteps=2)
    with pytest.raises(ValueError, match="outside"):
        eng.set_sampler(7, n_timesteps=2)
    assert [eng.open(*ref) for _ in range(3)] == [0, 1, 2]
    for bad in (dict(n_timesteps=0), dict(inference_cfg_rate=float("nan")), dict(temperature=float("inf"))):
        with pytest.raises(ValueError, match="set_sampler"):
            eng.set_sampler(1, **bad)
    assert eng._sampler == {}
    eng.set_sampler(1, n_timesteps=2, inference_cfg_rate=0.0)
    eng.set_sampler(1)                                   # all None: what the step call says
    assert eng._sampler == {}
    eng.set_sampler(1, inference_cfg_rate=0.3)
    eng.close(1)
    with pytest.raises(ValueError, match="slot 1 is not open"):
        eng.set_sampler(1, n_timesteps=2)
    assert eng.open(*ref) == 1 and eng._sampler == {}    # `open` starts without an override
    eng.set_sampler(1, n_timesteps=2)
    eng.close(1)
    assert eng.open(*ref) == 1 and eng._sampler == {}


# The two tests below drive a whole step / a whole pool with the recording stub.  Both end in the library's device calls
# (`svc_sola_step`, `svc_chunks_gather_cond`, `svc_chunks_assemble`), so they carry the gpu mark although the sampler is a stub.
DEV = "cuda:0"


@pytest.mark.gpu
def test_engine_step_calls_inference_as_before_until_a_listed_slot_has_an_override():
    from seedvc_amd.pipeline import RealtimeEngine
    cfm = RecordingCFM(DEV)
    eng = RealtimeEngine(RT.FakeLR(), cfm, RT.FakeVocoder(), max_streams=3, **RT.FAKE_GEOMETRY)
    ref = (torch.zeros(1, 5, cases.CHUNK_DC), torch.zeros(1, cases.CHUNK_C, 5), torch.zeros(1, 3))
    for _ in range(3):
        eng.open(*ref)
    x = cases.randn("rows.engine.x", 7, 3, RT.FAKE_GEOMETRY["S"], cases.CHUNK_DC).to(DEV)
    plain = eng.step([0, 1, 2], x, 3, 0.7)
    assert cfm.calls == [("inference", 3, 3, 0.7, {})]
    eng.set_sampler(1, n_timesteps=2, inference_cfg_rate=0.0)
    eng.step([0, 2], x[[0, 2]], 3, 0.7)                  # slot 1 is not listed: the call made today
    assert cfm.calls[1:] == [("inference", 2, 3, 0.7, {})]
    for s in range(3):
        eng.reset(s)
    out = eng.step_seeded([0, 1, 2], x, 3, 0.7, [5, 6, 7])
    assert cfm.calls[2:] == [("inference_rows", [(3, (.7, .7), 1.0, False), (2, (0., 0.), 1.0, False), (3, (.7, .7), 1.0, False)],
                              dict(seeds=[5, 6, 7]))]
    assert torch.equal(out, plain)                       # the stand-in ignores the settings: same blocks
    eng.set_sampler(1, temperature=0.5)                  # replaces the override: only the temperature is the slot's own
    eng.step([2, 1], x[[2, 1]], 4, 0.3)
    assert cfm.calls[3:] == [("inference_rows", [(4, (.3, .3), 1.0, False), (4, (.3, .3), 0.5, False)], {})]
    eng.set_sampler(1)
    eng.step([0, 1, 2], x, 3, 0.7)
    assert cfm.calls[4:] == [("inference", 3, 3, 0.7, {})]


def _pool(sampler, **kw):
    from seedvc_amd.pipeline import HotPath
    cfm = RecordingCFM(DEV)
    hp = HotPath(cfm, LB.FakeVocoder(ragged=True))
    utts = []
    for name in ("loop2", "loop1", "loop4"):
        c = cases.chunkloop_case(name)
        utts.append(tuple(c[k].to(DEV) for k in ("cond", "prompt_condition", "mel2", "style2")))
    outs = hp.convert_long_batch(utts, 10, 0.7, cases.CHUNK_HOP, cases.CHUNK_WINDOW, overlap_frame_len=cases.CHUNK_OVERLAP,
                                 max_chunks=4, ragged_vocoder=True, sampler=sampler, **kw)
    return cfm.calls, outs, utts


@pytest.mark.gpu
def test_long_pool_hands_every_chunk_its_files_entry():
    from seedvc_amd.pipeline import long_batch_plan
    calls, outs, utts = _pool([(2, 0.3), None, dict(n_timesteps=4, inference_cfg_rate=0.0, temperature=0.5)])
    plan = long_batch_plan([u[0].size(1) for u in utts], [u[2].size(2) for u in utts], cases.CHUNK_WINDOW, cases.CHUNK_OVERLAP,
                           cases.CHUNK_HOP, 4)
    want = {0: (2, (.3, .3), 1.0, False), 1: (10, (.7, .7), 1.0, False), 2: (4, (0., 0.), 0.5, False)}
    assert len(plan["micro_batches"]) > 1 and len({c[0] for c in plan["chunks"]}) == 3
    assert len(calls) == len(plan["micro_batches"])
    for (k0, k1), call in zip(plan["micro_batches"], calls):
        assert call[0] == "inference_rows" and call[2] == {}
        assert call[1] == [want[c[0]] for c in plan["chunks"][k0:k1]]
    # the stand-in ignores the settings, so the audio is that of the call without the keyword
    calls0, outs0, _ = _pool(None)
    assert [c[0] for c in calls0] == ["inference"] * len(calls) and all(c[2:4] == (10, 0.7) and c[4] == {} for c in calls0)
    assert [c[1] for c in calls0] == [k1 - k0 for k0, k1 in plan["micro_batches"]]
    assert all(torch.equal(a, b) for a, b in zip(outs, outs0))
    seeded, _, _ = _pool([None, (2, 0.3), None], seeds=[1, 2, 3])
    assert all(c[0] == "inference_rows" and set(c[2]) == {"seeds"} and len(c[2]["seeds"]) == len(c[1]) for c in seeded)


def test_long_pool_refuses_a_sampler_list_of_the_wrong_length():
    """`_file_settings` runs before the pool touches a device."""
    from seedvc_amd.pipeline import HotPath
    c = cases.chunkloop_case("loop2")
    utts = [(c["cond"], c["prompt_condition"], c["mel2"], c["style2"])] * 3
    hp = HotPath(RecordingCFM(), LB.FakeVocoder(ragged=True))
    for sampler, msg in (([(2, 0.3), None], "2 sampler entries for 3 files"), ([None, (2,), None], r"sampler\[1\]")):
        with pytest.raises(ValueError, match=msg):
            hp.convert_long_batch(utts, 10, 0.7, cases.CHUNK_HOP, cases.CHUNK_WINDOW, ragged_vocoder=True, sampler=sampler)
