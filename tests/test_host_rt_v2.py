"""CPU side of v2 real-time sessions: `svc_astral_tokens_heads` is declared, exported and bound; the stand-ins of
rt_v2_cases.py agree between numpy and torch and their session model is decided by no near tie; every refusal of the engine's
token mode that needs no device leaves `_sampler`, `_audio` and `state` as they were; and `AstralTokenizer.tokens_batch` checks
`heads=` before it touches a device."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import cases
import realtime_cases as RT
import rt_audio_cases as RA
import rt_v2_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


def test_entry_point_is_declared_exported_and_bound():
    from seedvc_amd import _lib, astral, pipeline
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    name = "svc_astral_tokens_heads"
    assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
    assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
    assert hasattr(lib, name), f"{name} is not exported by the library"
    assert len(_lib.lib().svc_astral_tokens_heads.argtypes) == len(_lib.lib().svc_astral_tokens.argtypes) + 1
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sig = lambda f: list(inspect.signature(f).parameters)                              # noqa: E731
    E, T = pipeline.RealtimeEngine, astral.AstralTokenizer
    assert sig(E.step_tokens) == ["self", "slots", "tokens", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts",
                                  "seeds"]
    assert sig(E.set_sampler) == ["self", "slot", "n_timesteps", "inference_cfg_rate", "temperature", "random_voice"]
    assert sig(E.attach_tokens) == ["self", "content", "resample", "Lin", "L16", "ce_dit_difference", "head"]
    assert sig(T.tokens_batch) == ["self", "waves", "lens", "overlap_s", "reduce_head", "heads"]
    assert sig(T.tokens_fn) == ["self", "waves_16k", "head"] and callable(T.codebook_size)
    # existing signatures stay
    assert sig(E.step) == ["self", "slots", "content", "n_timesteps", "inference_cfg_rate", "z", "vocoder_kwargs", "return_parts"]
    assert sig(E.attach_audio) == ["self", "content", "resample", "Lin", "L16", "ce_dit_difference"]


def test_library_refusals_come_before_the_handle_is_read():
    """A handle at address 1 is never read: the mask's own range, the pointers and reduce_head's buffers are checked first."""
    from seedvc_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(1)

    def bad(rc, part):
        assert rc != 0 and part in lib.svc_last_error(), lib.svc_last_error()
        assert lib.svc_last_error().startswith(b"svc_astral_tokens_heads:")

    call = lambda **kw: lib.svc_astral_tokens_heads(*[{**dict(m=one, wave=one, lens=None, B=1, L=4000, ov=20, mask=1, tokens=one,  # noqa: E731
                                                              Rmax=100, rh=-1, red=None, cnt=None, st=None), **kw}[k] for k in
                                                      ("m", "wave", "lens", "B", "L", "ov", "mask", "tokens", "Rmax", "rh", "red", "cnt", "st")])
    bad(call(mask=0), b"head_mask")
    bad(call(mask=4), b"head_mask")
    bad(call(mask=0xffffffff), b"head_mask")
    bad(call(wave=None), b"null wave or tokens")
    bad(call(tokens=None), b"null wave or tokens")
    bad(call(rh=0), b"reduce_head needs reduced and counts")
    bad(call(B=65), b"B must be")
    bad(call(ov=-1), b"overlap_rows")
    bad(call(Rmax=0), b"Rmax")
    bad(call(m=None), b"null handle")


# ------------------------------------------------------------------------------------------------------------ stand-ins
def test_stand_ins_agree_between_numpy_and_torch():
    rng = np.random.default_rng(5)
    ctx = rng.uniform(-1, 1, (3, 8 * 320 + 7)).astype(np.float32)
    ctx[0, 0], ctx[1, 320] = 0.0, -0.75
    tok = V.FakeTokenizer()
    got = tok.tokens_fn(torch.from_numpy(ctx), head=0)
    assert got.dtype == torch.int32 and got.shape == (3, 8) and tok.calls == [(3, 8 * 320 + 7, 0)] and tok.codebook_size(0) == V.K
    for b in range(3):
        assert np.array_equal(got[b].numpy(), V.fake_tokens(ctx[b]))
    assert int(got.min()) >= 0 and int(got.max()) < V.K and len(set(got.reshape(-1).tolist())) > 8
    assert np.array_equal(V.TABLE * 64, np.round(V.TABLE * 64)) and np.abs(V.TABLE).max() <= 2       # dyadic rationals
    lr = V.FakeTokenLR()
    S = RT.FAKE_GEOMETRY["S"]
    cond, ylens = lr(got[:, 2:], ylens=torch.LongTensor([S] * 3))
    assert cond.shape == (3, S, cases.CHUNK_DC) and ylens.tolist() == [S] * 3
    assert lr.cfg == dict(is_discrete=True, codebook_size=V.K, f0_condition=False)
    for b in range(3):
        rows = V.fake_content(V.fake_tokens(ctx[b])[2:])
        assert np.array_equal(cond[b].numpy(), rows[(np.arange(S) * 6) // S] * np.float32(0.5))      # what `fake_wave` starts from


def test_no_block_of_the_session_model_is_a_near_tie():
    sess = V.sessions()                                       # asserts the gap itself
    assert sess["min_gap"] > 1e-4
    assert len(sess["models"]) == 3 and all(len(m) == V.N_BLOCKS for m in sess["models"])
    assert all(t.shape == (6,) and t.dtype == np.int32 for ts in sess["tokens"] for t in ts)
    offsets = [[m[2] for m in ms] for ms in sess["models"]]
    assert len({o for os_ in offsets for o in os_}) > 3, offsets          # the splice moves: the sessions exercise SOLA
    assert any(t.any() for t in sess["tokens"][0]) and len({int(v) for ts in sess["tokens"] for t in ts for v in t}) > 10


# ------------------------------------------------------------------------------------------------------------ the engine
class _Cfm:
    device = torch.device("cpu")
    in_channels = 4

    def __init__(self, version):
        self.cfg = dict(version=version)


def _engine(lr, version=2, **kw):
    from seedvc_amd.pipeline import RealtimeEngine
    return RealtimeEngine(lr, _Cfm(version), None, **{**RT.FAKE_GEOMETRY, "max_streams": 3, **kw})


def _snapshot(eng):
    a = eng._audio
    return (dict(eng._sampler), None if a is None else (id(a), a["content"], a["head"], a["ring"].clone(), a["hist"].clone()), eng.state.clone())


def _same(eng, snap):
    sampler, audio, state = _snapshot(eng)
    assert sampler == snap[0] and torch.equal(state, snap[2])
    assert (audio is None) == (snap[1] is None)
    if audio is not None:
        assert audio[:3] == snap[1][:3] and torch.equal(audio[3], snap[1][3]) and torch.equal(audio[4], snap[1][4])


REF = (torch.zeros(1, 5, cases.CHUNK_DC), torch.zeros(1, cases.CHUNK_C, 5), torch.zeros(1, 3))
RESAMPLE = types.SimpleNamespace(orig_freq=22050, new_freq=16000, _h=None)


def _refused(eng, match, fn, *a, **kw):
    snap = _snapshot(eng)
    with pytest.raises(ValueError, match=match):
        fn(*a, **kw)
    _same(eng, snap)


def test_the_mode_is_the_regulators():
    assert _engine(V.FakeTokenLR()).token_mode is True
    assert _engine(RT.FakeLR()).token_mode is False and _engine(None).token_mode is False
    assert _engine(types.SimpleNamespace(cfg=dict(is_discrete=False))).token_mode is False
    assert "token_mode" not in inspect.signature(type(_engine(None)).__init__).parameters       # not a user option


def test_token_engine_refusals_need_no_gpu():
    eng = _engine(V.FakeTokenLR())
    assert [eng.open(*REF), eng.open(*REF)] == [0, 1]
    eng.state.fill_(3.0)
    eng.set_sampler(1, inference_cfg_rate=(0.7, 0.0), random_voice=True)
    assert eng._sampler == {1: (None, (0.7, 0.0), None, True)}
    x, f0 = torch.zeros(2, 6, cases.CHUNK_DC), torch.zeros(2, 12)
    tok = torch.zeros(2, 6, dtype=torch.int32)
    _refused(eng, "step: the length regulator is discrete", eng.step, [0, 1], x, 3, 0.7)
    _refused(eng, "step_f0: the length regulator is discrete", eng.step_f0, [0, 1], x, f0, None, 3, 0.7)
    for bad in (tok[0], tok[:, :, None], tok[:1], torch.zeros(3, 6, dtype=torch.int32)):             # rank, rank, rows, rows
        _refused(eng, "step_tokens: tokens .* is not", eng.step_tokens, [0, 1], bad, 3, (0.7, 0.5))
    for bad in (tok.float(), tok.double(), tok.bool()):
        _refused(eng, "step_tokens: tokens are .* integer", eng.step_tokens, [0, 1], bad, 3, (0.7, 0.5))
    _refused(eng, "slot 2 is not open", eng.step_tokens, [0, 2], tok, 3, 0.7)
    _refused(eng, "a slot appears twice", eng.step_tokens, [1, 1], tok, 3, 0.7)
    # the input side: a feature encoder, a codebook that is too large, and a head the tokenizer refuses
    good = dict(content=V.FakeTokenizer(), resample=RESAMPLE, Lin=441, L16=2560, ce_dit_difference=0.04)
    _refused(eng, "attach_audio: .*token mode.*tokens_fn", eng.attach_audio, **{**good, "content": RA.FakeContent()})
    _refused(eng, "attach_audio: head 0 has 65 codes, the length regulator's codebook_size is 64", eng.attach_audio,
             **{**good, "content": V.FakeTokenizer(codebook=V.K + 1)})
    _refused(eng, "attach_audio: head 1 has 65 codes", eng.attach_tokens, **{**good, "content": V.FakeTokenizer(codebook=V.K + 1)}, head=1)
    _refused(eng, "attach_audio: Lin", eng.attach_audio, **{**good, "Lin": 440})
    assert eng._audio is None
    eng.attach_tokens(**good, head=1)
    assert eng._audio["head"] == 1 and eng._audio["ce"] == 2 and eng._audio["planes"].shape == (2, 3, 2560)
    eng.attach_audio(**good)
    assert eng._audio["head"] == 0
    _refused(eng, "attach_audio: .*token mode", eng.attach_audio, **{**good, "content": RA.FakeContent()})      # the attached one stays
    _refused(eng, "step_audio: audio", eng.step_audio, [0, 1], torch.zeros(2, 440), 3, (0.7, 0.7))
    # pitch: the regulator is not f0-conditioned
    rmvpe = types.SimpleNamespace(f0_batch=lambda x, thred=0.03: None, frames=lambda n: n // 160 + 1)
    _refused(eng, "attach_pitch: the length regulator is not f0-conditioned", eng.attach_pitch, rmvpe)
    assert eng._pitch is None
    # the sampler's pair
    for bad in (dict(inference_cfg_rate=(0.7, float("nan"))), dict(inference_cfg_rate=(float("inf"), 0.5)), dict(inference_cfg_rate=(0.7,)),
                dict(inference_cfg_rate=[0.7, 0.5, 0.1]), dict(n_timesteps=0, inference_cfg_rate=(0.7, 0.5))):
        _refused(eng, "set_sampler", eng.set_sampler, 1, **bad)
    eng.set_sampler(1, random_voice=False)
    assert eng._sampler == {1: (None, None, None, False)}
    eng.set_sampler(1)
    assert eng._sampler == {}


def test_feature_engine_refusals_need_no_gpu():
    eng = _engine(RT.FakeLR(), version=1)
    assert [eng.open(*REF), eng.open(*REF)] == [0, 1]
    eng.state.fill_(3.0)
    eng.set_sampler(0, inference_cfg_rate=0.3)
    tok = torch.zeros(2, 6, dtype=torch.int32)
    _refused(eng, "step_tokens: the length regulator is not discrete", eng.step_tokens, [0, 1], tok, 3, 0.7)
    good = dict(resample=RESAMPLE, Lin=441, L16=2560, ce_dit_difference=0.04)
    _refused(eng, "attach_audio: content is a tokenizer", eng.attach_audio, content=V.FakeTokenizer(), **good)
    _refused(eng, "attach_tokens needs a discrete length regulator", eng.attach_tokens, content=V.FakeTokenizer(), **good)
    assert eng._audio is None
    # a v1 sampler takes neither a pair nor random_voice
    _refused(eng, "set_sampler: a pair of rates and random_voice need a v2 sampler", eng.set_sampler, 1, inference_cfg_rate=(0.7, 0.5))
    _refused(eng, "set_sampler: a pair of rates and random_voice need a v2 sampler", eng.set_sampler, 1, random_voice=True)
    _refused(eng, "set_sampler: a pair of rates and random_voice need a v2 sampler", eng.set_sampler, 0, random_voice=False)
    assert eng._sampler == {0: (None, 0.3, None, None)}
    eng.attach_audio(content=RA.FakeContent(), **good)
    _refused(eng, "attach_audio: content is a tokenizer", eng.attach_audio, content=V.FakeTokenizer(), **good)


# ------------------------------------------------------------------------------------------------------------ the mirror
def test_heads_argument_checks_need_no_gpu():
    import astral_cases as AC
    from seedvc_amd.astral import AstralTokenizer
    t = AstralTokenizer.__new__(AstralTokenizer)              # no handle: the checks come before anything reads one
    t.cfg, t.n_heads, t.W, t._h = AC.CFG_S, 2, AC.CFG_S["ssl"]["window_samples"], None
    w = torch.zeros(1, 4000)
    for heads, reduce_head, part in (((), None, "distinct"), ((0, 0), None, "distinct"), ((1, 0, 1), None, "distinct"), ((2,), None, "outside"),
                                     ((-1, 0), None, "outside"), ((0,), 1, "reduce_head 1 is not in heads"), ((1,), 0, "reduce_head")):
        with pytest.raises(ValueError, match="tokens_batch.*" + part):
            t.tokens_batch(w, heads=heads, reduce_head=reduce_head)
    with pytest.raises(ValueError, match="tokens_fn: head"):
        t.tokens_fn(w, head=2)
    with pytest.raises(ValueError, match="tokens_fn"):
        t.tokens_fn(torch.zeros(4000))
    assert t.codebook_size(0) == 2048 and t.codebook_size(1) == 32
    with pytest.raises(ValueError, match="codebook_size"):
        t.codebook_size(2)
