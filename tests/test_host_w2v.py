"""CPU side of the wav2vec 2.0 content encoder (csrc/wav2vec2.hip, seedvc_amd/wav2vec2.py): the float64 restatement of w2v_cases.py
(the GPU tests' yardstick) is pinned to transformers' `Wav2Vec2Model`, `HubertModel` and `Wav2Vec2FeatureExtractor`; the row rule
and the window rows agree with the extractor and the literal driver loop; the weight-norm fold is the parametrised conv's weight;
the host checks come before any handle is touched; the spec table is the module tree; the entry points are declared, exported and
bound; the asserted error bounds do not exceed the caps they come from."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import w2v_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

NAMES = ("svc_w2v_create", "svc_w2v_destroy", "svc_w2v_frames", "svc_w2v_n_windows", "svc_w2v_rows", "svc_w2v_set_window_group",
         "svc_w2v_set_timing", "svc_w2v_last_timing", "svc_w2v_normalize", "svc_w2v_features", "svc_w2v_posconv", "svc_w2v_encode",
         "svc_w2v_content", "svc_op_layernorm_gelu")


def _hf_kwargs(c):
    return dict(hidden_size=c["d_model"], num_hidden_layers=c["n_layers"], num_attention_heads=c["n_heads"], intermediate_size=c["ffn_dim"],
                conv_dim=(c["conv_dim"],) * len(c["conv_kernel"]), conv_kernel=c["conv_kernel"], conv_stride=c["conv_stride"],
                feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True, num_conv_pos_embeddings=c["pos_k"],
                num_conv_pos_embedding_groups=c["pos_groups"], hidden_act="gelu", feat_extract_activation="gelu")


def _hf_model(c, sd, kind="wav2vec2"):
    from transformers import HubertConfig, HubertModel, Wav2Vec2Config, Wav2Vec2Model
    m = (Wav2Vec2Model(Wav2Vec2Config(**_hf_kwargs(c))) if kind == "wav2vec2" else HubertModel(HubertConfig(**_hf_kwargs(c)))).eval()
    m.load_state_dict(sd, strict=True)
    return m


def _lib():
    from seedvc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import pipeline, wav2vec2
    _l = _lib()
    lib = ctypes.CDLL(_l.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _l.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    W = wav2vec2.Wav2Vec2Content
    p = inspect.signature(W.__init__).parameters
    assert list(p) == ["self", "state_dict", "cfg", "device", "precision"] and p["precision"].default == 1 and p["cfg"].default is None
    p = inspect.signature(W.content_batch).parameters
    assert list(p) == ["self", "waves", "lens", "overlap_s"] and p["overlap_s"].default == 5.0
    assert list(inspect.signature(W.semantic_fn).parameters) == ["self", "waves_16k"]
    for seam in ("normalize", "features", "posconv", "encode", "rows", "set_window_group", "set_timing", "last_timing", "close"):
        assert callable(getattr(W, seam))
    assert "whisper" in inspect.signature(pipeline.content_conditions).parameters        # the shared entry point, not a fork


def test_state_spec_is_the_module_tree():
    from seedvc_amd import specs
    for c in (VC.CFG_S, dict(specs.wav2vec2_config(), n_layers=1)):
        sd = VC.make_state_dict(c)
        for kind in ("wav2vec2", "hubert"):
            ref = _hf_model(c, sd, kind).state_dict()                                   # the generator's dict loads unchanged (strict)
            spec = specs.wav2vec2_state_spec(c)
            assert list(spec.keys()) == list(ref.keys())
            for k, shp in spec.items():
                assert tuple(shp) == tuple(ref[k].shape), k
    full = specs.wav2vec2_config()
    assert {k: full[k] for k in VC.CFG_F if k != "n_layers"} == {k: v for k, v in VC.CFG_F.items() if k != "n_layers"} and full["n_layers"] == 12


@pytest.mark.parametrize("name", ["S", "F"])
def test_restatement_is_the_hf_model(name):
    """float64 restatement == Wav2Vec2Model.double() == HubertModel.double(); every branch carries weight; the asserted bounds do not
    exceed the caps they are derived from (precision 1: the restatement end to end in float16)"""
    k = VC.case(name)
    c, sd = k["cfg"], k["sd"]
    worst = 0.0
    for kind in ("wav2vec2", "hubert"):
        hf = _hf_model(c, sd, kind).double()
        for xn, ref in zip(k["norm"], k["ref"]):
            want = hf(xn[None]).last_hidden_state[0]
            assert want.shape == ref.shape
            worst = max(worst, (ref - want).abs().max().item())
    print(f"{name}: max |restatement - HF .double()| = {worst:.2e} (bound 1e-13)")
    assert worst <= 1e-13                                       # measured 3.3e-15 (S) and 8.5e-15 (F)
    assert abs(torch.cat(k["ref"]).pow(2).mean().sqrt().item() - 1.0) < 0.2
    wave, ref = k["waves"][0], k["ref"][0]
    assert VC.rms(VC.model(sd, c, wave), ref) == 0.0
    if name == "S":
        br = []
        VC.layers(sd, c, VC.posconv(sd, c, k["h"][0]), branches=br)
        assert len(br) == 2 * c["n_layers"] and all(a >= 0.1 * b for a, b in br), br
        pc = VC.posconv(sd, c, k["h"][0]) - k["h"][0]
        assert pc.pow(2).mean().sqrt() >= 0.1 * k["h"][0].pow(2).mean().sqrt()
    e16 = VC.rms(VC.model(sd, c, wave, attn16=True), ref)
    e_tanh = VC.rms(VC.model(sd, c, wave, gelu="tanh"), ref)
    e_first = VC.rms(VC.layers(sd, c, VC.posconv(sd, c, k["h"][0], drop="first")), ref)
    cap1 = VC.rms(VC.model(sd, c, wave, dtype=torch.float16), ref)
    print(f"{name}: attn16 {e16:.2e}  tanh-GELU {e_tanh:.2e}  first-output-dropped {e_first:.2e}  float16 restatement (precision-1 cap) {cap1:.2e}")
    assert e16 < VC.RMS_BOUND[name][0]                   # what precision 0 rounds by design (fp16 attention operands) fits under 1e-4 ...
    assert e_first > 100 * VC.RMS_BOUND[name][1]         # ... a positional conv that drops the FIRST output does not fit under any bound ...
    assert name == "S" or e_tanh > VC.RMS_BOUND[name][0]  # ... nor a tanh-GELU at XLS-R widths (S has too little FFN to tell: 9.7e-5)
    assert VC.RMS_BOUND[name][0] <= 1e-4 and VC.RMS_BOUND[name][1] <= cap1


def test_normalisation_is_the_feature_extractor():
    from transformers import Wav2Vec2FeatureExtractor
    fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=False)
    for n, seed in ((400, 1), (5000, 2), (16001, 3)):
        w = VC.make_wave(n, seed) + (100.0 if seed == 2 else 0.0)
        want = torch.as_tensor(fe(w.numpy(), sampling_rate=16000, return_tensors="np").input_values[0])
        got = VC.normalize(w)
        e = (got - want.double()).abs().max().item()
        print(f"normalisation n={n}: max |restatement - Wav2Vec2FeatureExtractor (float32)| = {e:.2e}")
        assert e <= (5e-5 if seed == 2 else 1e-6)              # HF computes in float32: a few ulp of 1, and of 100 on the offset clip (measured 2.3e-7, 8.9e-6)
    assert (VC.normalize(torch.zeros(1000)) == 0).all()


def test_frames_is_the_extractor_length():
    from seedvc_amd import wav2vec2
    lib = _host_lib()
    c = VC.CFG_S
    hf = _hf_model(c, VC.make_state_dict(c))
    cc = wav2vec2.c_config(c)
    for n in range(400, 1101):
        want = hf.feature_extractor(torch.zeros(1, n)).shape[-1]
        assert VC.frames(c, n) == wav2vec2.frames(c, n) == want == lib.svc_w2v_frames(ctypes.byref(cc), n), n
        assert int(hf._get_feat_extract_output_lengths(n)) == want
    for n in (400, 719, 720, 1039, 1040, 16000, 32000, 480000):
        assert VC.frames(c, n) == (n - 400) // 320 + 1
    assert VC.frames(c, 399) == 0 and lib.svc_w2v_frames(ctypes.byref(cc), 399) == 0


def _host_lib():
    """the library with the argument types set, loaded without touching a device"""
    return _lib().lib()


def test_weight_norm_fold_is_the_parametrised_weight():
    c = VC.CFG_S
    sd = VC.make_state_dict(c, seed=3)
    hf = _hf_model(c, sd)
    want = hf.encoder.pos_conv_embed.conv.weight.double()
    got = VC.pos_weight(sd)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-6       # HF folds in float32
    old = {k.replace("parametrizations.weight.original0", "weight_g").replace("parametrizations.weight.original1", "weight_v"): v for k, v in sd.items()}
    assert torch.equal(VC.pos_weight(old), got)
    g = sd["encoder.pos_conv_embed.conv.parametrizations.weight.original0"]
    assert g.shape == (1, 1, c["pos_k"]) and (g > 0).all()


@pytest.mark.parametrize("W,O", [(32000, 6400), (480000, 80000)])
def test_window_rows_are_the_driver_loop(W, O):
    from seedvc_amd import wav2vec2
    lib = _host_lib()
    c = dict(VC.CFG_S, window_samples=W)
    cc = wav2vec2.c_config(c)
    ov = O // 320
    step = W - O
    Ls = {400, 401, 719, 720, W - 1, W, W + 1, W + 399, W + 400, W + step - 1, W + step, W + step + 1, W + 2 * step, W + 2 * step + 1, 3 * W + 17}
    for j in (1, 2):                                        # the last window keeps no row, one row, two rows
        for rows_last in (ov - 1, ov, ov + 1, ov + 2):
            Ls.add(j * step + 400 + 320 * (rows_last - 1))
            Ls.add(j * step + 400 + 320 * (rows_last - 1) + 319)
    rng = np.random.RandomState(W % 1000)
    Ls |= {int(v) for v in rng.randint(400, 4 * W, size=40)}
    for L in sorted(v for v in Ls if v >= 400):
        lit = VC.driver_plan(L, W, O)
        rows = sum(max(0, VC.frames(c, n) - drop) for _, n, drop in lit)
        plan = wav2vec2.window_plan(c, L, ov)
        assert [(s, n, d) for s, n, d, _ in plan] == lit, L
        assert lib.svc_w2v_n_windows(ctypes.byref(cc), ov, L) == len(lit) and lib.svc_w2v_rows(ctypes.byref(cc), ov, L) == rows, L
    if W == 32000:
        assert [lib.svc_w2v_n_windows(ctypes.byref(cc), 20, n) for n in (20000, 32000, 32400, 57700)] == [1, 1, 2, 3]
        assert [lib.svc_w2v_rows(ctypes.byref(cc), 20, n) for n in (20000, 32000, 32400, 57700)] == [62, 99, 100, 178]
    else:
        assert lib.svc_w2v_rows(ctypes.byref(cc), 250, 480000) == 1499 and lib.svc_w2v_n_windows(ctypes.byref(cc), 250, 600 * 16000) == 24


def test_arguments_are_checked_before_the_handle():
    from seedvc_amd import wav2vec2
    _l = _lib()
    lib = _host_lib()
    one = ctypes.c_void_p(1)                                  # never dereferenced: every check below fails before the handle is touched
    i32 = lambda *v: _l.i32_host(list(v))                     # noqa: E731
    cc = wav2vec2.c_config(VC.CFG_S)

    def bad(rc, word):
        assert rc != 0 and word in lib.svc_last_error(), lib.svc_last_error()

    bad(lib.svc_w2v_rows(ctypes.byref(cc), 100, 5000), b"overlap_rows")
    bad(lib.svc_w2v_rows(ctypes.byref(cc), -1, 5000), b"overlap_rows")
    bad(lib.svc_w2v_rows(ctypes.byref(cc), 20, 399), b"receptive field")
    bad(lib.svc_w2v_n_windows(ctypes.byref(cc), 20, 0), b"receptive field")
    bad(int(lib.svc_w2v_frames(ctypes.byref(cc), -1) < 0), b"n_samples")
    for fn, name in ((lib.svc_w2v_normalize, b"svc_w2v_normalize"),):
        bad(fn(one, one, None, 2, 4000, one, None), b"lens is NULL")
        bad(fn(one, one, i32(4000, 0), 2, 4000, one, None), b"lens")
        bad(fn(one, one, i32(4000, 4001), 2, 4000, one, None), b"lens")
        bad(fn(one, one, i32(*([4000] * 65)), 65, 4000, one, None), b"B")
        bad(fn(one, None, i32(4000), 1, 4000, one, None), b"null wave")
    bad(lib.svc_w2v_features(one, one, None, 2, 4000, one, 12, None), b"lens is NULL")
    bad(lib.svc_w2v_features(one, one, i32(4000, 4001), 2, 4000, one, 12, None), b"lens")
    bad(lib.svc_w2v_features(one, one, i32(4000), 0, 4000, one, 12, None), b"B")
    for fn in (lib.svc_w2v_posconv, lib.svc_w2v_encode):
        bad(fn(one, one, None, 1, 50, one, None), b"rows is NULL")
        bad(fn(one, one, i32(51), 1, 50, one, None), b"rows outside")
        bad(fn(one, one, i32(0), 1, 50, one, None), b"rows outside")
        bad(fn(one, one, i32(5), 0, 50, one, None), b"B")
        bad(fn(one, None, i32(5), 1, 50, one, None), b"null h")
        bad(fn(None, one, i32(5), 1, 50, one, None), b"null handle")
    bad(lib.svc_w2v_content(one, one, i32(4000, 4001), 2, 4000, 20, one, 100, None), b"lens")
    bad(lib.svc_w2v_content(one, one, i32(0), 1, 4000, 20, one, 100, None), b"lens")
    bad(lib.svc_w2v_content(one, one, None, 0, 4000, 20, one, 100, None), b"B")
    bad(lib.svc_w2v_content(one, one, None, 65, 4000, 20, one, 100, None), b"B")
    bad(lib.svc_w2v_content(one, one, None, 1, 4000, -1, one, 100, None), b"overlap_rows")
    bad(lib.svc_w2v_content(one, one, None, 1, 4000, 20, one, 0, None), b"Rmax")
    bad(lib.svc_w2v_content(None, one, None, 1, 4000, 20, one, 100, None), b"null handle")
    bad(lib.svc_w2v_set_window_group(one, 65), b"windows")
    bad(lib.svc_op_layernorm_gelu(one, one, one, one, 4, 100, 1e-5, None), b"multiple of 64")

    # configurations the encoder does not compute are refused at create time, before any weight is looked at
    def create(**kw):
        c = wav2vec2.c_config(dict(VC.CFG_S, **kw))
        out = ctypes.c_void_p()
        return lib.svc_w2v_create(ctypes.byref(c), one, 0, None, ctypes.byref(out))

    bad(create(feat_extract_norm="group"), b"feat_extract_norm")
    bad(create(do_stable_layer_norm=False), b"do_stable_layer_norm")
    bad(create(conv_bias=False), b"conv_bias")
    bad(create(n_heads=4), b"head dimension 64")
    bad(create(pos_k=15), b"even")
    bad(create(pos_groups=4), b"groups of 64")
    bad(create(window_samples=32001), b"multiple of 320")
    bad(create(conv_stride=(5, 2, 2, 2, 2, 2, 1)), b"multiply to 320")            # another hop would drop the wrong overlap
    bad(create(conv_kernel=(64, 3, 3, 3, 3, 2, 2), conv_dim=512), b"8192")           # conv0's weights would not fit its LDS
    c = wav2vec2.c_config(VC.CFG_S, precision=2)
    bad(lib.svc_w2v_create(ctypes.byref(c), one, 0, None, ctypes.byref(ctypes.c_void_p())), b"precision")
