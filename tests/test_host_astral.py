"""CPU side of the ASTRAL tokenizer (csrc/astral.hip, seedvc_amd/astral.py): the float64 restatement of astral_cases.py (the GPU
tests' yardstick) is pinned to transformers' `ConvNextV2Layer` and to `HubertModel` with the final LayerNorm replaced by Identity; the
index convention, the duration reduction and the window arithmetic agree with their literal statements; the spec table, the entry
points and the create-time refusals are checked without a device; the token margins leave at most 5 % of the bits unchecked."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import astral_cases as AC
import w2v_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

NAMES = ("svc_astral_create", "svc_astral_destroy", "svc_astral_n_windows", "svc_astral_rows", "svc_astral_set_window_group",
         "svc_astral_set_timing", "svc_astral_last_timing", "svc_astral_ssl", "svc_astral_convnext", "svc_astral_logits",
         "svc_astral_tokens", "svc_op_bsq_index", "svc_tokens_reduce")


def _lib():
    from seedvc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_block_is_convnextv2_layer():
    """the 1-D block == ConvNextV2Layer.double() on a (1, D, 1, T) input with the 7 taps in the middle row of the 7 x 7 kernel"""
    from transformers import ConvNextV2Config
    from transformers.models.convnextv2.modeling_convnextv2 import ConvNextV2Layer
    D, T = 64, 37
    c = dict(ssl=dict(VC.CFG_S, d_model=D), heads=[dict(dim=D, intermediate_dim=4 * D, n_blocks=1, bits=5, dw_kernel=7)])
    sd = AC.make_head_sd(c, 0, seed=5)
    layer = ConvNextV2Layer(ConvNextV2Config(hidden_act="gelu", layer_norm_eps=1e-6), dim=D).double().eval()
    p = "encoder.blocks.0."
    w = torch.zeros(D, 1, 7, 7, dtype=torch.float64)
    w[:, :, 3, :] = sd[p + "dwconv.weight"].double()
    hf = {"dwconv.weight": w, "dwconv.bias": sd[p + "dwconv.bias"], "layernorm.weight": sd[p + "norm.weight"], "layernorm.bias": sd[p + "norm.bias"],
          "pwconv1.weight": sd[p + "pwconv1.weight"], "pwconv1.bias": sd[p + "pwconv1.bias"], "pwconv2.weight": sd[p + "pwconv2.weight"],
          "pwconv2.bias": sd[p + "pwconv2.bias"], "grn.weight": sd[p + "grn.gamma"].reshape(1, 1, 1, -1), "grn.bias": sd[p + "grn.beta"].reshape(1, 1, 1, -1)}
    missing = layer.load_state_dict({k: v.double() for k, v in hf.items()}, strict=False)
    assert not missing.unexpected_keys and all("drop_path" in k or "layer_scale" in k for k in missing.missing_keys), missing
    assert getattr(layer, "layer_scale_parameter", None) is None
    x = torch.randn(T, D, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    want = layer(x.T[None, :, None, :])[0, :, 0, :].T
    e = (AC.block(sd, 0, x) - want).abs().max().item()
    print(f"ConvNeXt V2 block: max |1-D restatement - ConvNextV2Layer.double()| = {e:.2e} (bound 1e-12)")
    assert e <= 1e-12


def test_ssl_restatement_is_hubert_without_the_final_layernorm():
    from transformers import HubertConfig, HubertModel
    k = AC.case("S")
    c, sd = k["cfg"]["ssl"], k["ssl_sd"]
    full = HubertModel(HubertConfig(
        hidden_size=c["d_model"], num_hidden_layers=c["n_layers"] + 1, num_attention_heads=c["n_heads"], intermediate_size=c["ffn_dim"],
        conv_dim=(c["conv_dim"],) * len(c["conv_kernel"]), conv_kernel=c["conv_kernel"], conv_stride=c["conv_stride"], feat_extract_norm="layer",
        do_stable_layer_norm=True, conv_bias=True, num_conv_pos_embeddings=c["pos_k"], num_conv_pos_embedding_groups=c["pos_groups"],
        hidden_act="gelu", feat_extract_activation="gelu")).eval()
    more = VC.make_state_dict(dict(c, n_layers=c["n_layers"] + 1), seed=21)            # one layer more than the tokenizer keeps
    full.load_state_dict(more, strict=True)
    full.encoder.layers = full.encoder.layers[:c["n_layers"]]
    full.encoder.layer_norm = torch.nn.Identity()
    full = full.double()
    worst = 0.0
    for n in (5123, 16000):
        wave = AC.make_wave(n, 40)
        xn = VC.normalize(wave)
        want = full(xn[None]).last_hidden_state[0]
        got = AC.ssl(more, dict(k["cfg"], ssl=c), wave)
        assert got.shape == want.shape == (AC.window_rows(k["cfg"], n), c["d_model"])
        worst = max(worst, (got - want).abs().max().item())
    print(f"SSL front: max |restatement - HubertModel.double() cut, Identity final norm| = {worst:.2e} (bound 1e-13)")
    assert worst <= 1e-13
    ln = torch.nn.functional.layer_norm(AC.ssl(sd, k["cfg"], AC.make_wave(5123, 40)), (c["d_model"],), sd["encoder.layer_norm.weight"].double(),
                                        sd["encoder.layer_norm.bias"].double(), 1e-5)
    assert VC.rms(ln, VC.model(sd, c, AC.make_wave(5123, 40))) <= 1e-13            # the only difference from the w2v yardstick


def test_branches_carry_weight_and_margins_leave_few_bits():
    for name in ("S", "F"):
        k = AC.case(name)
        for hk, sd in enumerate(k["heads"]):
            br = []
            AC.convnext(sd, k["cfg"]["heads"][hk], k["h"][-1], branches=br)
            assert len(br) == k["cfg"]["heads"][hk]["n_blocks"] and all(a >= 0.1 * b for a, b in br), br
            assert sd["encoder.blocks.0.grn.gamma"].mean() > 0.3                    # GRN matters
        for p in (0, 1):
            m = AC.MARGIN[name][p]
            if m is None:
                continue
            for hk in range(2):
                frac = AC.excluded_fraction(torch.cat(k["z"][hk]), m)
                print(f"{name} head {hk} precision {p}: margin {m:.2e} excludes {100 * frac:.2f} % of the bits (at most 5 %)")
                assert frac <= AC.MAX_EXCLUDED
    for p in (0, 1):
        m = AC.MARGIN["S"][p]
        if m is None:
            continue
        for zs in AC.token_case()["z"]:
            assert AC.excluded_fraction(torch.cat(zs), m) <= AC.MAX_EXCLUDED
        for zc in AC.clip_case()["z"]:
            for z in zc:
                assert AC.excluded_fraction(z, m) <= AC.MAX_EXCLUDED


def test_caps_and_measured_bounds():
    """precision 1's cap is the float16 restatement's own error (computed, not typed in); an asserted bound never exceeds its cap"""
    for name in ("S", "F"):
        cap = AC.cap16(name)
        print(f"{name}: float16 restatement rel RMS x {cap['x']:.2e}, z {cap['z']:.2e}, max |z16 - z64| {cap['zmax']:.2e}")
        assert 1e-5 < cap["x"] < 1e-2 and 1e-5 < cap["z"] < 2e-2
        for what in ("x", "z"):
            assert AC.rms_bound(name, 0, what) <= 1e-4 and AC.rms_bound(name, 1, what) <= cap[what]
        one = AC.seam_case(name)["cap16"]                    # the block seam is held to ONE block's figures, below the whole head's
        print(f"{name}: one block in float16, rel RMS x {one:.2e}")
        assert 1e-5 < one < cap["x"] and AC.block_bound(name, 1) <= one
        assert AC.block_bound(name, 0) == 4 * AC.MEASURED_BLOCK[name][0] < AC.rms_bound(name, 0, "x")


def test_index_convention():
    from seedvc_amd import astral
    pats = torch.tensor([[1.0 if (i >> (4 - j)) & 1 else -1.0 for j in range(5)] for i in range(32)])
    assert AC.bsq_index(pats).tolist() == list(range(32)) == astral.bsq_index(pats).tolist()
    explicit = sum((pats[:, j] > 0).long() * 2 ** (5 - 1 - j) for j in range(5))
    assert torch.equal(AC.bsq_index(pats), explicit)
    z = torch.tensor([[0.0, -0.0, 1e-30, -1e-30, 1.0], [1e-30, 0.0, 0.0, -0.0, -1.0]])
    assert AC.bsq_index(z).tolist() == [0b00101, 0b10000] == astral.bsq_index(z).tolist()
    assert torch.equal(AC.index_bits(AC.bsq_index(pats), 5), pats > 0)


def test_reduction_restatement():
    W = 99                                                  # a run crossing what will be a window seam of config S
    cases = [torch.full((17,), 3), torch.arange(40) % 2, torch.tensor([7]), torch.cat([torch.arange(W - 3) % 5, torch.full((9,), 4), torch.arange(20) % 3]),
             torch.randint(0, 2, (500,), generator=torch.Generator().manual_seed(1)), torch.randint(0, 32, (500,), generator=torch.Generator().manual_seed(2))]
    for seq in cases:
        want = torch.unique_consecutive(seq)
        assert torch.equal(AC.reduce_unfold(seq), want) and torch.equal(AC.reduce_ref(seq), want)
    assert AC.reduce_unfold(cases[0]).tolist() == [3] and AC.reduce_unfold(cases[1]).tolist() == (torch.arange(40) % 2).tolist()


def test_rows_and_windows_are_the_window_plan():
    from seedvc_amd import astral, content
    lib = _lib().lib()
    c = AC.CFG_S
    cc = astral.c_config(c)
    W, O = c["ssl"]["window_samples"], AC.OV * 320
    for n in (400, 719, 720, W - 1, W, W + 1, W + (W - O) - 1, W + (W - O), W + (W - O) + 1, 57700):
        plan = content.window_plan(n, W, O)
        rows = sum(max(0, min(VC.frames(c["ssl"], ns), ns // 320) - d) for _, ns, d, _ in plan)
        assert [(s, ns, d) for s, ns, d, _ in astral.window_plan(c, n, AC.OV)] == VC.driver_plan(n, W, O)
        assert sum(max(0, r - d) for _, _, d, r in astral.window_plan(c, n, AC.OV)) == rows
        assert lib.svc_astral_n_windows(ctypes.byref(cc), AC.OV, n) == len(plan) and lib.svc_astral_rows(ctypes.byref(cc), AC.OV, n) == rows, n
    assert [lib.svc_astral_rows(ctypes.byref(cc), AC.OV, n) for n in AC.CLIP_LENS] == [62, 99, 100, 178]
    assert AC.window_rows(c, 400) == 1 and AC.window_rows(c, 719) == 1 and AC.window_rows(c, 720) == 2
    assert lib.svc_astral_rows(ctypes.byref(cc), AC.OV, 399) == -1 and b"receptive field" in lib.svc_last_error()
    assert lib.svc_astral_rows(ctypes.byref(cc), 100, 5000) == -1 and b"overlap_rows" in lib.svc_last_error()


def test_state_spec_and_presets():
    from seedvc_amd import specs
    c = specs.astral_config()
    assert c["ssl"]["n_layers"] == 18 and c["ssl"]["d_model"] == 1024 and len(c["heads"]) == 2
    assert c["heads"][0] == specs.ASTRAL_WIDE and c["heads"][1] == specs.ASTRAL_NARROW
    assert specs.ASTRAL_WIDE["bits"] == 11 and specs.ASTRAL_NARROW["bits"] == 5 and specs.ASTRAL_WIDE["dim"] == 512
    assert specs.ASTRAL_WIDE["intermediate_dim"] == 1536 and specs.ASTRAL_WIDE["n_blocks"] == 12
    s = specs.astral_head_state_spec(c, 1)
    keys = list(s)
    assert keys[:2] == ["encoder.input_projection.weight", "encoder.input_projection.bias"] and s[keys[0]] == (512, 1024, 1)
    blk = ["dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "grn.gamma", "grn.beta", "pwconv2.weight", "pwconv2.bias"]
    for i in range(12):
        assert keys[2 + 10 * i:12 + 10 * i] == [f"encoder.blocks.{i}.{n}" for n in blk]
    assert keys[122:] == ["quantizer.project_in.weight", "quantizer.project_in.bias", "quantizer.project_out.weight", "quantizer.project_out.bias"]
    assert s["encoder.blocks.3.dwconv.weight"] == (512, 1, 7) and s["encoder.blocks.3.pwconv1.weight"] == (1536, 512)
    assert s["encoder.blocks.3.grn.gamma"] == (1, 1, 1536) and s["quantizer.project_in.weight"] == (5, 512) and s["quantizer.project_out.weight"] == (512, 5)


def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import astral, pipeline
    _l = _lib()
    lib = ctypes.CDLL(_l.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _l.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1
    A = astral.AstralTokenizer
    p = inspect.signature(A.__init__).parameters
    assert list(p) == ["self", "ssl_state_dict", "head_state_dicts", "cfg", "device", "precision"] and p["precision"].default == 1
    assert list(inspect.signature(A.tokens_batch).parameters)[:4] == ["self", "waves", "lens", "overlap_s"]
    for seam in ("tokenize", "ssl", "convnext", "logits", "reduce", "rows", "set_window_group", "set_timing", "last_timing", "close"):
        assert callable(getattr(A, seam))
    assert list(inspect.signature(pipeline.v2_content_tokens).parameters) == ["astral", "waves_16k", "lens", "overlap_s"]


def test_bad_configs_and_arguments_are_refused_with_a_message():
    from seedvc_amd import astral
    _l = _lib()
    lib = _l.lib()
    one = ctypes.c_void_p(1)                                  # never dereferenced: every check below fails before it would be
    i32 = lambda *v: _l.i32_host(list(v))                     # noqa: E731

    def bad(rc, word):
        assert rc != 0 and word in lib.svc_last_error(), lib.svc_last_error()

    def create(head=None, n_heads=None, **ssl):
        c = dict(ssl=dict(VC.CFG_S, **ssl), heads=[dict(h) for h in AC.HEADS_S])
        c["heads"][1].update(head or {})
        cc = astral.c_config(c)
        if n_heads is not None:
            cc.n_heads = n_heads
        hp, hn = (ctypes.c_void_p * 2)(1, 1), (ctypes.c_int * 2)(0, 0)
        return lib.svc_astral_create(ctypes.byref(cc), one, 0, hp, hn, None, ctypes.byref(ctypes.c_void_p()))

    bad(create(head=dict(dim=96)), b"dim must be a multiple of 64")
    bad(create(head=dict(dim=4096)), b"dim must be a multiple of 64")
    bad(create(head=dict(intermediate_dim=100)), b"intermediate_dim")
    bad(create(head=dict(bits=0)), b"bits")
    bad(create(head=dict(bits=17)), b"bits")
    bad(create(head=dict(dw_kernel=5)), b"7 taps")
    bad(create(head=dict(n_blocks=0)), b"n_blocks")
    bad(create(n_heads=3), b"n_heads")
    bad(create(pos_k=15), b"even")                            # the SSL front's own refusals come through, under this entry point's name
    assert lib.svc_last_error().startswith(b"svc_astral_create: the SSL front:")
    for fn in (lib.svc_astral_convnext, lib.svc_astral_logits):
        bad(fn(one, 0, one, None, 1, 50, one, None), b"rows is NULL")
        bad(fn(one, 0, one, i32(51), 1, 50, one, None), b"rows outside")
        bad(fn(one, 0, one, i32(5), 65, 50, one, None), b"B")
        bad(fn(None, 0, one, i32(5), 1, 50, one, None), b"null handle")
    bad(lib.svc_astral_ssl(one, one, None, 1, 4000, one, 12, None), b"lens is NULL")
    bad(lib.svc_astral_ssl(one, one, i32(4001), 1, 4000, one, 12, None), b"lens")
    bad(lib.svc_astral_tokens(one, one, i32(0), 1, 4000, 20, one, 100, -1, None, None, None), b"lens")
    bad(lib.svc_astral_tokens(one, one, None, 65, 4000, 20, one, 100, -1, None, None, None), b"B")
    bad(lib.svc_astral_tokens(one, one, None, 1, 4000, -1, one, 100, -1, None, None, None), b"overlap_rows")
    bad(lib.svc_astral_tokens(one, one, None, 1, 4000, 20, one, 0, -1, None, None, None), b"Rmax")
    bad(lib.svc_astral_tokens(one, one, None, 1, 4000, 20, one, 100, 1, None, None, None), b"reduce_head")
    bad(lib.svc_astral_tokens(None, one, None, 1, 4000, 20, one, 100, -1, None, None, None), b"null handle")
    bad(lib.svc_tokens_reduce(one, None, 1, 10, one, one, None), b"rows is NULL")
    bad(lib.svc_tokens_reduce(one, i32(11), 1, 10, one, one, None), b"rows outside")
    bad(lib.svc_tokens_reduce(one, i32(5), 1, 10, one, None, None), b"null tokens")
    for out in (4096, 4096 - 76, 4096 + 76):                  # tokens [2][10] at 4096: out on it, and sharing one element below and above
        bad(lib.svc_tokens_reduce(ctypes.c_void_p(4096), i32(5, 5), 2, 10, ctypes.c_void_p(out), one, None), b"must not overlap")
    bad(lib.svc_op_bsq_index(one, one, 4, 17, None), b"bits")
    bad(lib.svc_astral_set_window_group(one, 65), b"windows")
