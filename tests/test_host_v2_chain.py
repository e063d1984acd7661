"""CPU side of the v2 chain (`pipeline.V2HotPath`, seeded AR sampling, the ragged assembly calls): the C ABI, `_lib.EXPORTS`
and the library agree on the new entry points; the frame-count arithmetic and the equal-length grouping; the AR prompts the
GPU chain test compares token for token survive the logit error the kernels are allowed; and the statistics the seeded
draws are held to on the GPU are sound (numpy's own Exp(1) passes them, the Philox reference gives the published
known answers)."""
import ctypes
import os
import re

import numpy as np
import torch

import v2_chain_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svc_ar_generate_batch_seeded", "svc_ar_exp_draws", "svc_v2_assemble_cond", "svc_mel_strip_prompt")
torch.set_grad_enabled(False)


def test_v2_chain_abi_agrees():
    from seedvc_amd import _lib, pipeline
    from seedvc_amd.ar import ARModel
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
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header
    for name in ("exp_draws", "generate_batch", "generate_batch_raw"):
        assert callable(getattr(ARModel, name, None)), name
    for name in ("prepare_target", "convert_batch"):
        assert callable(getattr(pipeline.V2HotPath, name, None)), name


def test_ragged_argument_errors_need_no_gpu():
    """Lengths are checked on the host before anything is launched."""
    from seedvc_amd import _lib
    lib = _lib.lib()
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks come first
    assert lib.svc_v2_assemble_cond(one, i32(3), one, i32(4), 1, 2, 4, 8, 7, one, None) != 0        # P_b > Pmax
    assert b"assemble_cond" in lib.svc_last_error()
    assert lib.svc_v2_assemble_cond(one, i32(2), one, i32(4), 1, 2, 4, 8, 5, one, None) != 0        # P_b + S_b > T
    assert lib.svc_mel_strip_prompt(one, i32(2), i32(9), 1, 4, 8, 6, ctypes.c_float(0), one, None) != 0     # x_len > T
    assert b"strip_prompt" in lib.svc_last_error()
    assert lib.svc_mel_strip_prompt(one, i32(1), i32(8), 1, 4, 8, 6, ctypes.c_float(0), one, None) != 0     # 7 frames > Smax
    assert lib.svc_ar_exp_draws(None, ctypes.c_uint64(1), 0, 1, one, None) != 0


def test_target_frames_arithmetic():
    """int(frames_per_token * n) in Python doubles: hand-computed cases, one where float32 arithmetic gives another frame
    count (0.29 * 100 = 28.999999999999996 in double -> 28; 29.0 in float32 -> 29)."""
    from seedvc_amd.pipeline import v2_target_frames
    assert v2_target_frames(1.5, 7) == 10
    assert v2_target_frames(2.0, 160) == 320
    assert v2_target_frames(0.02, 40) == 0
    assert v2_target_frames(860 / 322, 256) == 683          # 683.726...
    assert v2_target_frames(0.29, 100) == 28
    assert int(np.float32(0.29) * np.float32(100)) == 29
    assert v2_target_frames(4.35, 100) == 434 and int(np.float32(4.35) * np.float32(100)) == 435
    assert v2_target_frames(np.float32(1.5), torch.tensor(7)) == 10


def test_equal_length_grouping():
    from seedvc_amd.pipeline import group_by_length
    assert group_by_length([30, 12, 30, 0, 12, 7]) == {30: [0, 2], 12: [1, 4], 7: [5]}
    assert list(group_by_length([30, 12, 30, 0, 12, 7])) == [30, 12, 7]
    assert group_by_length([5, 5, 5]) == {5: [0, 1, 2]}
    assert group_by_length([0, 0]) == {} and group_by_length([]) == {}


def test_chain_prompts_survive_the_allowed_logit_error():
    """The probe of test_host_ar_batch.py on the AR prompts the chain builds (out of the AR length regulator): candidates
    that fail are dropped; at least three must remain, with different source lengths, prompt lengths and ratios."""
    ok = V.qualified()
    print("qualified candidates:", ok, {k: (V.utterance(k)["ref_tokens"].shape[1], V.utterance(k)["ylen"]) for k in ok})
    assert len(ok) >= 3
    first = [V.CANDIDATES[k] for k in ok[:3]]
    for col in (1, 3, 4):
        assert len({c[col] for c in first}) == 3
    for k in ok[:3]:
        u = V.utterance(k)
        assert u["ylen"] > 0 and u["ref_tokens"].shape[1] >= 10 and int(u["ref_tokens"].max()) < 32


def test_philox_reference_known_answers():
    """The numpy Philox4x32-10 the GPU test compares with gives the known answers of the Random123 distribution."""
    kat = lambda c, k: [int(x) for x in V.philox4x32_10(np.full((1, 4), c), (k, k))[0]]       # noqa: E731
    assert kat(0, 0) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert kat(0xffffffff, 0xffffffff) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    got = V.philox4x32_10(np.array([[0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]]), (0xa4093822, 0x299f31d0))[0]
    assert [int(x) for x in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    u = V.reference_uniforms(0x1234567812345678, 3, 2, 2049)
    assert u.shape == (2, 2049) and u.min() > 0.0 and u.max() <= 1.0


def test_ks_bound_is_sound():
    """1.95 / sqrt(n) is the 0.1 % critical value: numpy's own Exp(1) sample of the size the GPU test uses passes it, and
    so does the reference construction of the seeded draws; a mis-scaled sample does not."""
    n = 64 * 2049
    q = np.random.default_rng(0).exponential(size=n)
    d = V.ks_exp1(q)
    print(f"numpy Exp(1), n = {n}: KS {d:.5f} (bound {V.ks_critical(n):.5f})")
    assert d < V.ks_critical(n)
    d_ref = V.ks_exp1(-np.log(V.reference_uniforms(77, 0, 64, 2049)))
    print(f"reference construction: KS {d_ref:.5f}")
    assert d_ref < V.ks_critical(n)
    assert V.ks_exp1(q * 1.02) > V.ks_critical(n)
    a, b = -np.log(V.reference_uniforms(77, 0, 64, 2049)), -np.log(V.reference_uniforms(78, 0, 64, 2049))
    assert abs(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1]) < 4 / np.sqrt(n)
    assert abs(np.corrcoef(a[:-1].reshape(-1), a[1:].reshape(-1))[0, 1]) < 4 / np.sqrt(a[1:].size)
