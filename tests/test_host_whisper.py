"""CPU side of the Whisper content encoder (csrc/whisper.hip, seedvc_amd/whisper.py): the float64 restatement of whisper_cases.py
(the GPU tests' yardstick) is pinned to transformers' `WhisperEncoder`, `WhisperFeatureExtractor` and `mel_filter_bank`; the
window plan agrees with the literal driver loop; the host checks come before any handle is touched; the spec table is the module
tree; the entry points are declared, exported and bound; the asserted error bounds do not exceed the caps they come from."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import whisper_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

NAMES = ("svc_whisper_create", "svc_whisper_destroy", "svc_whisper_n_windows", "svc_whisper_rows", "svc_whisper_set_window_group",
         "svc_whisper_set_timing", "svc_whisper_last_timing", "svc_whisper_mel", "svc_whisper_encode", "svc_whisper_content",
         "svc_op_layernorm")


def _hf_encoder(c, sd):
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    hc = WhisperConfig(num_mel_bins=c["n_mels"], d_model=c["d_model"], encoder_attention_heads=c["n_heads"], encoder_layers=c["n_layers"],
                       encoder_ffn_dim=c["ffn_dim"], max_source_positions=c["max_source_positions"])
    m = WhisperEncoder(hc).eval()
    m.load_state_dict(sd, strict=True)
    return m


def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline, whisper
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    p = inspect.signature(whisper.WhisperContent.__init__).parameters
    assert list(p) == ["self", "state_dict", "cfg", "mel_basis", "device", "precision"] and p["precision"].default == 1
    p = inspect.signature(whisper.WhisperContent.content_batch).parameters
    assert list(p) == ["self", "waves", "lens", "overlap_s"] and p["overlap_s"].default == 5.0
    assert list(inspect.signature(whisper.WhisperContent.semantic_fn).parameters) == ["self", "waves_16k"]
    for seam in ("mel", "encode"):
        assert callable(getattr(whisper.WhisperContent, seam))
    p = inspect.signature(pipeline.content_conditions).parameters
    assert list(p)[:10] == ["whisper", "length_regulator", "src_16k", "src_lens", "src_ylens", "ref_16k", "ref_lens", "ref_ylens", "f0_src", "f0_ref"]
    assert p["f0_src"].default is None and p["f0_ref"].default is None


def test_state_spec_is_the_module_tree():
    from seedvc_amd import specs
    for c, n_par in ((WC.CFG_S, None), (specs.whisper_config(), 88.15)):
        ref = _hf_encoder(c, WC.make_state_dict(c)).state_dict()
        spec = specs.whisper_state_spec(c)
        assert list(spec.keys()) == list(ref.keys())
        for k, shp in spec.items():
            assert tuple(shp) == tuple(ref[k].shape), k
        if n_par:
            assert round(sum(int(np.prod(s)) for s in spec.values()) / 1e6, 2) == n_par
    assert specs.whisper_config() == WC.CFG_F
    sd = WC.make_state_dict(WC.CFG_S, seed=1)
    hf = _hf_encoder(WC.CFG_S, sd)                                                 # the generator's dict loads unchanged (strict)
    assert torch.equal(WC.sinusoids(100, 128).float(), type(hf)(hf.config).state_dict()["embed_positions.weight"])   # what HF builds


@pytest.mark.parametrize("name", ["S", "F"])
def test_restatement_is_the_hf_encoder(name):
    """float64 restatement == WhisperEncoder.double() to 1e-10; every branch carries weight; the rounded-operand restatement stays
    inside 7e-5 on these inputs; the asserted bounds do not exceed the caps they are derived from"""
    k = WC.case(name)
    c, sd, feats = k["cfg"], k["sd"], k["feats"]
    hf = _hf_encoder(c, sd)
    want = hf.double()(feats).last_hidden_state
    e = (k["ref"] - want).abs().max().item()
    print(f"{name}: max |restatement - WhisperEncoder.double()| = {e:.2e}")
    assert e <= 1e-10
    assert abs(k["ref"].pow(2).mean().sqrt().item() - 1.0) < 0.2
    if name == "S":
        br = []
        WC.encoder(sd, c, feats, branches=br)
        assert len(br) == 2 * c["n_layers"] and all(a >= 0.1 * b for a, b in br), br
    e16 = WC.rms(WC.encoder(sd, c, feats, attn16=True), k["ref"])
    e_tanh = WC.rms(WC.encoder(sd, c, feats, gelu="tanh"), k["ref"])
    cap1 = WC.rms(WC.encoder(sd, c, feats.half(), dtype=torch.float16), k["ref"])
    e_hf16 = WC.rms(hf.half()(feats.half()).last_hidden_state, k["ref"])
    print(f"{name}: attn16 {e16:.2e}  tanh-GELU {e_tanh:.2e}  float16 restatement {cap1:.2e}  HF .half() {e_hf16:.2e}")
    assert e16 <= 7e-5                                   # what precision 0 rounds by design leaves room under 1e-4 ...
    assert e_tanh > WC.RMS_BOUND[0]                      # ... and a tanh-GELU does not fit under it
    assert 0.5 * e_hf16 <= cap1 <= 2.0 * e_hf16          # the float16 restatement is the reference's own arithmetic
    assert WC.RMS_BOUND[0] <= 1e-4 and WC.RMS_BOUND[1] <= cap1


def test_log_mel_restatement_is_the_hf_feature_extractor():
    from transformers import WhisperFeatureExtractor
    from transformers.audio_utils import mel_filter_bank
    from seedvc_amd.audio import whisper_mel_basis
    ref = mel_filter_bank(201, 80, 0.0, 8000.0, 16000, "slaney", "slaney")
    basis = whisper_mel_basis(80)
    assert basis.dtype == torch.float64 and basis.shape == (80, 201)
    assert np.abs(basis.numpy() - ref.T).max() <= 1e-9
    for P, lens in ((100, WC.S_LENS), (1500, (301234,))):
        fe = WhisperFeatureExtractor(feature_size=80, chunk_length=P * 320 // 16000)
        assert fe.n_samples == P * 320 and fe.nb_max_frames == 2 * P
        for i, n in enumerate(lens):
            w = WC.make_wave(n, i)
            want = torch.from_numpy(fe(w.numpy(), sampling_rate=16000, return_tensors="np").input_features[0]).double()
            got = WC.log_mel(w, P, basis)
            d = (got - want).abs()
            print(f"log-mel P={P} n={n}: max {d.max().item():.2e} mean {d.mean().item():.2e}")
            assert got.shape == want.shape == (80, 2 * P) and d.max().item() <= 5e-5 and d.mean().item() <= 1e-6


def test_window_plan_is_the_driver_loop():
    from seedvc_amd import _lib
    from seedvc_amd.whisper import window_plan
    lib = _lib.lib()
    for P, ov in ((100, 20), (1500, 250)):
        W, O = P * 320, ov * 320
        edge = [1, 319, 320, 321, W - 1, W, W + 1, W + O, 2 * W - O - 1, 2 * W - O, 2 * W - O + 1, 3 * W - 2 * O, 3 * W - 2 * O + 1, 3 * W - 2 * O + 319]
        sweep = edge + list(range(5, 4 * W, 7919 if P == 100 else 104729))
        for L in sweep:
            lit = WC.driver_plan(L, W, O)
            mine = window_plan(L, W, O)
            assert [(s, n, d) for s, n, d, _ in mine] == lit, L
            rows = sum(min(P, n // 320 + 1) - d for s, n, d in lit)
            assert all(r == min(P, n // 320 + 1) and r > d for _, n, d, r in mine), L       # every window keeps at least one row
            assert lib.svc_whisper_n_windows(P, ov, L) == len(lit) and lib.svc_whisper_rows(P, ov, L) == rows, L
    assert lib.svc_whisper_rows(1500, 250, 480000) == 1500 and lib.svc_whisper_rows(1500, 250, 16000) == 51
    assert [lib.svc_whisper_n_windows(100, 20, n) for n in (20000, 32000, 32001, 57605)] == [1, 1, 2, 3]
    assert [lib.svc_whisper_rows(100, 20, n) for n in (20000, 32000, 32001, 57605)] == [63, 100, 101, 181]
    assert lib.svc_whisper_n_windows(1500, 250, 600 * 16000) == 24


def test_argument_errors_need_no_gpu():
    """The host checks come first, name the offending argument and touch no handle."""
    from seedvc_amd import _lib
    lib, err = _lib.lib(), _lib.lib().svc_last_error
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks come first

    def bad(rc, word):
        assert rc != 0 and word in err(), err()

    # window plan: (P, overlap_rows, n_samples)
    bad(lib.svc_whisper_rows(100, 100, 5000), b"overlap_rows")
    bad(lib.svc_whisper_rows(100, -1, 5000), b"overlap_rows")
    bad(lib.svc_whisper_n_windows(100, 20, 0), b"n_samples")
    # mel: (m, wave, lens, B, L, feat, stream)
    bad(lib.svc_whisper_mel(one, one, None, 2, 4000, one, None), b"lens is NULL")
    bad(lib.svc_whisper_mel(one, one, i32(4000, 0), 2, 4000, one, None), b"lens")
    bad(lib.svc_whisper_mel(one, one, i32(4000, 4001), 2, 4000, one, None), b"lens")
    bad(lib.svc_whisper_mel(one, one, i32(*([4000] * 65)), 65, 4000, one, None), b"B")
    bad(lib.svc_whisper_mel(one, one, i32(4000), 0, 4000, one, None), b"B")
    # encode: (m, feat, B, out, stream)
    bad(lib.svc_whisper_encode(one, one, 0, one, None), b"B")
    # content: (m, wave, lens, B, L, overlap_rows, out, Rmax, stream)
    bad(lib.svc_whisper_content(one, one, i32(4000, 4001), 2, 4000, 20, one, 100, None), b"lens")
    bad(lib.svc_whisper_content(one, one, i32(0), 1, 4000, 20, one, 100, None), b"lens")
    bad(lib.svc_whisper_content(one, one, None, 0, 4000, 20, one, 100, None), b"B")
    bad(lib.svc_whisper_content(one, one, None, 65, 4000, 20, one, 100, None), b"B")
    bad(lib.svc_whisper_content(one, one, None, 1, 4000, -1, one, 100, None), b"overlap_rows")
    bad(lib.svc_whisper_content(one, one, None, 1, 4000, 20, one, 0, None), b"Rmax")
    bad(lib.svc_whisper_set_window_group(one, 65), b"windows")
    # create: (cfg, weights, n, mel_basis, stream, out): geometry and keys are checked before anything touches the device
    c = WC.CFG_S
    sd = WC.make_state_dict(c)
    out = ctypes.c_void_p()

    def create(cfg, state):
        wc = _lib.WhisperConfig()
        for k, v in cfg.items():
            setattr(wc, k, int(v))
        wc.precision = cfg.get("precision", 1)
        descs, n, keep = _lib.make_descs(state, "cpu")                      # host tensors: never read, the checks fail first
        return lib.svc_whisper_create(ctypes.byref(wc), descs, n, one, None, ctypes.byref(out))

    bad(create(dict(c, n_heads=3), sd), b"n_heads")
    bad(create(dict(c, d_model=96, n_heads=1), sd), b"d_model")
    bad(create(dict(c, n_mels=84), sd), b"n_mels")
    bad(create(dict(c, precision=2), sd), b"precision")
    bad(create(c, {k: v for k, v in sd.items() if k != "layers.1.fc2.bias"}), b"missing layers.1.fc2.bias")
    bad(create(c, {("model.encoder." + k): v for k, v in sd.items() if k != "layer_norm.weight"}), b"missing model.encoder.layer_norm.weight")
    bad(create(c, dict(sd, **{"layers.0.self_attn.k_proj.weight": torch.zeros(128, 64)})), b"shape mismatch for layers.0.self_attn.k_proj.weight")
    assert not out.value
