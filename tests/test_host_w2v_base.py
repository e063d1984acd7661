"""CPU side of the wav2vec 2.0 base family (HuBERT-base / wav2vec2-base; csrc/wav2vec2.hip through svc_w2v_create_ex):
the float64 restatement of w2v_base_cases.py (the GPU tests' yardstick) is pinned to transformers' `HubertModel` and `Wav2Vec2Model`
built with feat_extract_norm = "group", do_stable_layer_norm = False, conv_bias = False; `do_normalize` is the feature extractor's;
the family-aware spec table is the module tree; svc_w2v_create_ex refuses by name, before any weight is looked at; the entry point is
declared, exported and bound; the asserted error bounds do not exceed the caps they come from."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import w2v_base_cases as BC
import w2v_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)


def _hf_kwargs(c):
    return dict(hidden_size=c["d_model"], num_hidden_layers=c["n_layers"], num_attention_heads=c["n_heads"], intermediate_size=c["ffn_dim"],
                conv_dim=(c["conv_dim"],) * len(c["conv_kernel"]), conv_kernel=c["conv_kernel"], conv_stride=c["conv_stride"],
                feat_extract_norm=c["feat_extract_norm"], do_stable_layer_norm=c["do_stable_layer_norm"], conv_bias=c["conv_bias"],
                num_conv_pos_embeddings=c["pos_k"], num_conv_pos_embedding_groups=c["pos_groups"], hidden_act="gelu",
                feat_extract_activation="gelu")


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


def test_create_ex_is_declared_exported_and_bound():
    from seedvc_amd import wav2vec2
    _l = _lib()
    lib = ctypes.CDLL(_l.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    assert "svc_w2v_create_ex" in declared and "svc_w2v_create_ex" in _l.EXPORTS and hasattr(lib, "svc_w2v_create_ex")
    assert re.search(r"typedef struct svc_w2v_ext \{\s*int do_normalize;[^}]*int feat_proj_layer_norm;[^}]*\} svc_w2v_ext_t;", header)
    assert [f[0] for f in _l.W2vExt._fields_] == ["do_normalize", "feat_proj_layer_norm"] and ctypes.sizeof(_l.W2vExt) == 8
    # the header is the contract: what it declares is what the library exports (nm -D), symbol for symbol
    nm = subprocess.run(["nm", "-D", "--defined-only", _l.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("svc_")}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    # which creator a cfg goes through
    assert wav2vec2.c_ext(VC.CFG_S) is None and wav2vec2.c_ext(VC.CFG_F) is None
    e = wav2vec2.c_ext(BC.CFG_BS)
    assert (e.do_normalize, e.feat_proj_layer_norm) == (1, 1)
    assert wav2vec2.c_ext(dict(VC.CFG_S, do_normalize=False)).do_normalize == 0
    cc = wav2vec2.c_config(BC.CFG_BF)
    assert (cc.feat_extract_norm_layer, cc.do_stable_layer_norm, cc.conv_bias, cc.d_model // cc.pos_groups) == (0, 0, 0, 48)


def test_state_spec_is_the_module_tree_in_both_families():
    from seedvc_amd import specs
    full = specs.wav2vec2_base_config()
    assert {k: full[k] for k in BC.CFG_BF if k not in ("n_layers", "window_samples")} == \
        {k: v for k, v in BC.CFG_BF.items() if k not in ("n_layers", "window_samples")} and full["n_layers"] == 12
    assert specs.wav2vec2_is_base(full) and not specs.wav2vec2_is_base(specs.wav2vec2_config())
    cfgs = (BC.CFG_BS, dict(full, n_layers=1), dict(BC.CFG_BS, conv_bias=True),
            dict(VC.CFG_S, conv_bias=False))                                            # conv_bias is free in both families
    for c in cfgs:
        sd = BC.make_state_dict(c)
        spec = specs.wav2vec2_state_spec(c)
        group, bias = c["feat_extract_norm"] == "group", c["conv_bias"]
        assert ("feature_extractor.conv_layers.0.layer_norm.weight" in spec) and ("feature_extractor.conv_layers.1.layer_norm.weight" in spec) == (not group)
        assert ("feature_extractor.conv_layers.0.conv.bias" in spec) == bias
        for kind in ("wav2vec2", "hubert"):
            ref = _hf_model(c, sd, kind).state_dict()                                   # the generator's dict loads unchanged (strict)
            assert list(spec.keys()) == list(ref.keys())
            for k, shp in spec.items():
                assert tuple(shp) == tuple(ref[k].shape), k


@pytest.mark.parametrize("name", ["BS", "BF"])
def test_restatement_is_the_hf_model(name):
    """float64 restatement == Wav2Vec2Model.double() == HubertModel.double() of the base family; every branch carries weight; the
    asserted bounds do not exceed the caps they are derived from (precision 1: the restatement end to end, and at each seam, in
    float16)"""
    k = BC.case(name)
    c, sd = k["cfg"], k["sd"]
    worst = 0.0
    for kind in ("wav2vec2", "hubert"):
        hf = _hf_model(c, sd, kind).double()
        for xn, ref in zip(k["norm"], k["ref"]):
            want = hf(xn[None]).last_hidden_state[0]
            assert want.shape == ref.shape
            worst = max(worst, (ref - want).abs().max().item())
        if kind == "hubert":                                 # the seams, against the modules themselves
            xn = k["norm"][0]
            feats = hf.feature_projection(hf.feature_extractor(xn[None]).transpose(1, 2))
            feats = feats[0] if isinstance(feats, tuple) else feats
            worst = max(worst, (k["h"][0] - feats[0]).abs().max().item())
            pos = k["h"][0] + hf.encoder.pos_conv_embed(k["h"][0][None])[0]
            worst = max(worst, (BC.posconv(sd, c, k["h"][0]) - pos).abs().max().item())
    print(f"{name}: max |restatement - HF .double()| = {worst:.2e} (bound 1e-12)")
    assert worst <= 1e-12                                       # measured 3.6e-15 (BS) and 6.6e-15 (BF)
    assert abs(torch.cat(k["ref"]).pow(2).mean().sqrt().item() - 1.0) < 0.2
    wave, ref = k["waves"][0], k["ref"][0]
    assert BC.rms(BC.model(sd, c, wave), ref) == 0.0
    if name == "BS":
        br = []
        BC.layers(sd, c, BC.posconv(sd, c, k["h"][0]), branches=br)
        assert len(br) == 2 * c["n_layers"] and all(a >= 0.1 * b for a, b in br), br
    # a pre-LN order, a LayerNorm over channels in place of the GroupNorm and a statistic over another window's frames are other networks
    e_pre = BC.rms(VC.layers(sd, c, BC.posconv(sd, c, k["h"][0])), ref)
    e_other = BC.rms(BC.extractor(sd, c, torch.cat([k["norm"][0], 3.0 * k["norm"][0]]))[:ref.shape[0]], k["h"][0])
    e16 = BC.rms(BC.model(sd, c, wave, attn16=True), ref)
    cap1 = BC.rms(BC.model(sd, c, wave, dtype=torch.float16), ref)
    x, want = BC.extractor_case(name, False)
    cap_ext = max(BC.rms(BC.extractor(sd, c, xi, dtype=torch.float16), r) for xi, r in zip(x, want))
    h = torch.randn(100, c["d_model"], generator=torch.Generator().manual_seed(77))
    cap_pos = BC.rms(BC.posconv(sd, c, h, dtype=torch.float16), BC.posconv(sd, c, h))
    print(f"{name}: attn16 {e16:.2e}  pre-LN order {e_pre:.2e}  statistics over a longer window {e_other:.2e}  float16 restatement: model "
          f"{cap1:.2e}, extractor {cap_ext:.2e}, positional conv {cap_pos:.2e} (the precision-1 caps)")
    # fp16 q, k, v and softmax weights (what precision 0 keeps in the pre-LN families) do not fit under 1e-4 in the post-LN order on
    # the short clips of BS (1.38e-4 here; 8.9e-5 on BF): precision 0 of this family runs the attention in fp32
    assert e16 > BC.RMS_BOUND[name][0] and (name != "BS" or e16 > 1e-4)
    assert e_pre > 100 * BC.RMS_BOUND[name][1] and e_other > 100 * BC.RMS_BOUND[name][1]
    assert BC.RMS_BOUND[name][0] <= 1e-4 and BC.RMS_BOUND[name][1] <= cap1
    assert BC.SEAM_BOUND["extractor"][0] <= 1e-4 and BC.SEAM_BOUND["extractor"][1] <= cap_ext
    assert BC.SEAM_BOUND["posconv"][0] <= 1e-4 and BC.SEAM_BOUND["posconv"][1] <= cap_pos
    # the DC-offset input of the extractor seam: the float32 restatement itself stays far inside the precision-0 bound
    xd, wd = BC.extractor_case(name, True)
    e32 = max(BC.rms(BC.extractor(sd, c, xi, dtype=torch.float32), r) for xi, r in zip(xd, wd))
    print(f"{name}: float32 restatement on the DC-offset ({BC.DC_OFFSET}) clips: {e32:.2e}")
    assert e32 <= BC.SEAM_BOUND["extractor"][0]              # inside the asserted precision-0 bound (itself far below the 1e-4 cap)


def test_do_normalize_is_the_feature_extractor():
    from transformers import Wav2Vec2FeatureExtractor
    w = VC.make_wave(5000, 2) + 0.5
    for flag in (True, False):
        fe = Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=flag, return_attention_mask=False)
        want = torch.as_tensor(fe(w.numpy(), sampling_rate=16000, return_tensors="np").input_values[0]).double()
        got = BC.normalize(w) if flag else w.double()
        e = (got - want).abs().max().item()
        print(f"do_normalize={flag}: max |restatement - Wav2Vec2FeatureExtractor (float32)| = {e:.2e}")
        assert e <= (1e-6 if flag else 0.0)
    k = BC.case("BS")
    a, b = BC.model(k["sd"], k["cfg"], w, do_normalize=False), BC.model(k["sd"], k["cfg"], w)
    assert BC.rms(a, b) > 1e-3                                # the flag is not a no-op on the network's output


def test_create_ex_refuses_by_name_before_any_weight():
    from seedvc_amd import wav2vec2
    _l = _lib()
    lib = _l.lib()
    one = ctypes.c_void_p(1)                                  # never dereferenced: every check below fails before a weight is looked at

    def create(base, ext, **kw):
        c = wav2vec2.c_config(dict(base, **kw))
        out = ctypes.c_void_p()
        e = None if ext is None else ctypes.byref(_l.W2vExt(*ext))
        rc = lib.svc_w2v_create_ex(ctypes.byref(c), e, one, 0, None, ctypes.byref(out))
        return rc, lib.svc_last_error()

    def old(**kw):
        c = wav2vec2.c_config(dict(VC.CFG_S, **kw))
        rc = lib.svc_w2v_create(ctypes.byref(c), one, 0, None, ctypes.byref(ctypes.c_void_p()))
        return rc, lib.svc_last_error()

    def bad(res, word):
        assert res[0] != 0 and word in res[1], res

    # ext = NULL: exactly svc_w2v_create's refusals, word for word
    for kw in (dict(feat_extract_norm="group"), dict(do_stable_layer_norm=False), dict(conv_bias=False), dict(n_heads=4), dict(pos_k=15),
               dict(pos_groups=4), dict(window_samples=32001), dict(conv_stride=(5, 2, 2, 2, 2, 2, 1)),
               dict(conv_kernel=(64, 3, 3, 3, 3, 2, 2), conv_dim=512)):
        a, b = create(VC.CFG_S, None, **kw), old(**kw)
        assert a[0] != 0 and a == b, (kw, a, b)
    bad(create(BC.CFG_BS, None), b"feat_extract_norm")
    # with ext: the mixed forms, by name
    bad(create(BC.CFG_BS, (1, 1), do_stable_layer_norm=True), b"mixed form")
    bad(create(BC.CFG_BS, (1, 1), do_stable_layer_norm=True), b"\"group\" with do_stable_layer_norm")
    bad(create(VC.CFG_S, (1, 1), do_stable_layer_norm=False), b"mixed form")
    bad(create(VC.CFG_S, (1, 1), do_stable_layer_norm=False), b"\"layer\" without do_stable_layer_norm")
    bad(create(BC.CFG_BS, (1, 0)), b"feat_proj_layer_norm must be 1")
    bad(create(BC.CFG_BS, (2, 1)), b"do_normalize must be 0 or 1")
    # the group width: a multiple of 16, at most 64
    bad(create(BC.CFG_BS, (1, 1), pos_groups=8), b"groups of 16, 32, 48 or 64 channels")      # 24
    bad(create(BC.CFG_BS, (1, 1), pos_groups=2), b"groups of 16, 32, 48 or 64 channels")      # 96
    bad(create(BC.CFG_BS, (1, 1), pos_groups=5), b"groups of 16, 32, 48 or 64 channels")      # does not divide
    bad(create(VC.CFG_S, (1, 1), pos_groups=1), b"groups of 16, 32, 48 or 64 channels")       # 128
    bad(create(BC.CFG_BS, (1, 1), conv_kernel=(20, 3, 3, 3, 3, 2, 2)), b"conv_kernel[0] <= 16")
    # what passes these checks goes on to the weights: the accepted forms fail on the first missing key, not on the configuration
    for base, kw in ((BC.CFG_BS, {}), (BC.CFG_BF, {}), (BC.CFG_BS, dict(conv_bias=True)), (VC.CFG_S, dict(conv_bias=False)),
                     (BC.CFG_BS, dict(pos_groups=12)), (BC.CFG_BS, dict(pos_groups=6)), (BC.CFG_BS, dict(pos_groups=3))):
        for ext in ((1, 1), (0, 1)):
            bad(create(base, ext, **kw), b"feature_extractor.conv_layers.0.conv.weight")
