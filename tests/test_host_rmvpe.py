"""CPU side of the RMVPE pitch extractor (csrc/rmvpe.hip, seedvc_amd/rmvpe.py): the entry points are declared, exported and
bound and the ABI is still 1; `specs.rmvpe_state_spec` is the restated module tree's state dict key for key; the HTK mel basis
has the shape, support and areas librosa documents; the host checks come before any handle is touched; and the numpy decode of
rmvpe_cases.py (the GPU tests' yardstick) agrees with a frame worked out by hand."""
import ctypes
import inspect
import os
import re

import numpy as np
import torch

import rmvpe_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

NAMES = ("svc_rmvpe_create", "svc_rmvpe_destroy", "svc_rmvpe_frames", "svc_rmvpe_min_len", "svc_rmvpe_set_plane_budget", "svc_rmvpe_set_timing",
         "svc_rmvpe_last_timing", "svc_rmvpe_mel",
         "svc_rmvpe_salience", "svc_rmvpe_decode", "svc_rmvpe_f0", "svc_f0_adjust")


def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline, rmvpe
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
    assert lib.svc_rmvpe_min_len() == 513 and lib.svc_rmvpe_frames(16000) == 101 and lib.svc_rmvpe_frames(513) == 4
    p = inspect.signature(rmvpe.RMVPE.infer_from_audio).parameters
    assert list(p) == ["self", "audio", "thred"] and p["thred"].default == 0.03          # the reference's signature
    p = inspect.signature(rmvpe.RMVPE.f0_batch).parameters
    assert list(p) == ["self", "waves", "lens", "thred"] and p["lens"].default is None
    for seam in ("mel", "salience", "decode"):
        assert callable(getattr(rmvpe.RMVPE, seam))
    p = inspect.signature(pipeline.f0_conditions).parameters
    assert list(p) == ["rmvpe", "src_16k", "src_lens", "ref_16k", "ref_lens", "auto_f0_adjust", "pitch_shift"]
    assert p["auto_f0_adjust"].default is True and p["pitch_shift"].default == 0


def test_state_spec_is_the_module_tree():
    from seedvc_amd import specs
    for over, n_tensors in ((dict(), 741), (R.SHALLOW, None)):
        c = specs.rmvpe_config(**over)
        ref = R.E2E(c).state_dict()
        spec = specs.rmvpe_state_spec(c)
        assert list(spec.keys()) == list(ref.keys())
        for k, shp in spec.items():
            assert tuple(shp) == tuple(ref[k].shape), k
        if n_tensors:
            assert len(spec) == n_tensors
            n_par = sum(int(np.prod(s)) for k, s in spec.items() if not k.endswith(("running_mean", "running_var", "num_batches_tracked")))
            assert n_par == sum(p.numel() for p in R.E2E(c).parameters()) and round(n_par / 1e6, 2) == 90.42
    for k in ("unet.encoder.layers.0.conv.0.conv.0.weight", "unet.decoder.layers.0.conv1.0.weight", "fc.0.gru.weight_hh_l0_reverse", "fc.1.bias"):
        assert k in spec or k in specs.rmvpe_state_spec(specs.rmvpe_config())
    sd = R.make_state_dict(specs.rmvpe_config(**R.SHALLOW), seed=1)
    R.E2E(specs.rmvpe_config(**R.SHALLOW)).load_state_dict(sd, strict=True)              # the generator's dict loads unchanged
    bn = sd["unet.encoder.layers.0.conv.0.conv.1.running_var"]
    assert bn.min() > 0.4 and bn.std() > 0.1 and sd["unet.encoder.bn.running_mean"].abs().item() > 0     # statistics are not the defaults


def test_htk_mel_basis_shape_support_and_areas():
    from seedvc_amd.audio import htk_mel_basis
    sr, n_fft, n_mels, fmin, fmax = 16000, 1024, 128, 30, 8000
    w = htk_mel_basis(sr, n_fft, n_mels, fmin, fmax).double().numpy()
    assert w.shape == (128, 513) and (w >= 0).all()
    mel = lambda f: 2595.0 * np.log10(1.0 + f / 700.0)   # noqa: E731
    inv = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)  # noqa: E731
    edges = inv(np.linspace(mel(fmin), mel(fmax), n_mels + 2))
    freqs = np.linspace(0, sr / 2, 513)
    for i in (0, 1, 40, 127):
        nz = np.nonzero(w[i])[0]
        inside = (freqs > edges[i]) & (freqs < edges[i + 2])
        assert set(nz) == set(np.nonzero(inside)[0])       # support = the open interval between the neighbouring centres
    # Slaney normalisation: every continuous triangle has unit area, height 2 / width at its centre frequency
    for i in (5, 60, 127):
        peak = 2.0 / (edges[i + 2] - edges[i])
        assert w[i].max() <= peak * (1 + 1e-6)
        fine = np.linspace(edges[i], edges[i + 2], 20001)
        tri = np.maximum(0, np.minimum((fine - edges[i]) / (edges[i + 1] - edges[i]), (edges[i + 2] - fine) / (edges[i + 2] - edges[i + 1]))) * peak
        assert abs(((tri[1:] + tri[:-1]) * np.diff(fine)).sum() / 2 - 1.0) < 1e-6
        k = int(np.argmin(np.abs(freqs - edges[i + 1])))
        want = max(0.0, min((freqs[k] - edges[i]) / (edges[i + 1] - edges[i]), (edges[i + 2] - freqs[k]) / (edges[i + 2] - edges[i + 1]))) * peak
        assert abs(w[i, k] - want) < 1e-6 * peak
    # wide filters (many DFT bins per triangle): the sampled area times the bin spacing is the unit area
    assert abs(w[127].sum() * (sr / n_fft) - 1.0) < 0.02


def test_argument_errors_need_no_gpu():
    """The host checks come first, name the offending argument and touch no handle."""
    from seedvc_amd import _lib
    lib, err = _lib.lib(), _lib.lib().svc_last_error
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)      # noqa: E731
    one = ctypes.c_void_p(16)                           # never dereferenced: the checks come first

    def bad(rc, word):
        assert rc != 0 and word in err(), err()

    mn = lib.svc_rmvpe_min_len()
    # mel: (m, wave, lens, B, L, mel_out, stream)
    bad(lib.svc_rmvpe_mel(one, one, None, 2, 4000, one, None), b"lens is NULL")
    bad(lib.svc_rmvpe_mel(one, one, i32(4000, mn - 1), 2, 4000, one, None), b"lens")        # a clip under svc_rmvpe_min_len()
    bad(lib.svc_rmvpe_mel(one, one, i32(4000, 4001), 2, 4000, one, None), b"lens")
    bad(lib.svc_rmvpe_mel(one, one, i32(*([4000] * 65)), 65, 4000, one, None), b"B")        # more than 64 clips
    # f0: (m, wave, lens, B, L, thred, f0_out, stream): lens may be NULL, the other rules hold
    bad(lib.svc_rmvpe_f0(one, one, i32(4000, mn - 1), 2, 4000, 0.03, one, None), b"lens")
    bad(lib.svc_rmvpe_f0(one, one, None, 65, 4000, 0.03, one, None), b"B")
    bad(lib.svc_rmvpe_f0(one, one, None, 1, mn - 1, 0.03, one, None), b"L")
    # salience: (m, mel, frame_lens, B, T, out, stream); decode: (salience, frame_lens, B, T, thred, f0_out, stream)
    bad(lib.svc_rmvpe_salience(one, one, None, 2, 70, one, None), b"frame_lens is NULL")
    bad(lib.svc_rmvpe_salience(one, one, i32(70, 71), 2, 70, one, None), b"frame_lens")
    bad(lib.svc_rmvpe_salience(one, one, i32(70, 0), 2, 70, one, None), b"frame_lens")
    bad(lib.svc_rmvpe_decode(one, None, 2, 70, 0.03, one, None), b"frame_lens is NULL")
    bad(lib.svc_rmvpe_decode(one, i32(*([70] * 65)), 65, 70, 0.03, one, None), b"B")
    # f0_adjust: (f0_alt, alt_lens, f0_ori, ori_lens, B, Talt, Tori, auto_adjust, semitones, out, medians, stream)
    bad(lib.svc_f0_adjust(one, None, one, i32(5), 1, 10, 10, 1, None, one, None, None), b"alt_lens is NULL")
    bad(lib.svc_f0_adjust(one, i32(5), one, None, 1, 10, 10, 1, None, one, None, None), b"ori_lens is NULL")
    bad(lib.svc_f0_adjust(one, i32(11), one, i32(5), 1, 10, 10, 1, None, one, None, None), b"alt_lens")
    bad(lib.svc_f0_adjust(one, i32(5), one, i32(-1), 1, 10, 10, 1, None, one, None, None), b"ori_lens")


def test_numpy_decode_agrees_with_a_hand_computed_frame():
    s = np.zeros((4, 360))
    # frame 0: a peak at bin 100 with neighbours: cents = sum(s_k * c_k) / sum(s_k) over bins 96 .. 104
    s[0, 99:102] = (0.2, 0.6, 0.4)
    c = lambda k: 20.0 * k + R.CENTS0                    # noqa: E731
    cents0 = (0.2 * c(99) + 0.6 * c(100) + 0.4 * c(101)) / 1.2
    # frame 1: a peak at bin 0: the window's bins -4 .. -1 do not exist and contribute nothing
    s[1, 0:3] = (0.5, 0.25, 0.25)
    cents1 = (0.5 * c(0) + 0.25 * c(1) + 0.25 * c(2)) / 1.0
    # frame 2: an exact tie between bins 50 and 200: the first maximum wins, bin 200 is outside its window
    s[2, 50] = s[2, 200] = 0.7
    # frame 3: the maximum is exactly the threshold: unvoiced
    s[3, 10] = 0.03
    f0 = R.np_decode(s, thred=0.03)
    want = [10 * 2 ** (cents0 / 1200), 10 * 2 ** (cents1 / 1200), 10 * 2 ** (c(50) / 1200), 0.0]
    assert np.allclose(f0, want, rtol=1e-12, atol=0) and f0[3] == 0.0
    assert abs(f0[2] - 10 * 2 ** ((20.0 * 50 + 1997.3794084376191) / 1200)) < 1e-9
    tr = R.f0_tracks()
    assert [(r[:n] > 1).sum().item() for r, n in zip(tr[0], tr[1])] == [21, 16, 1, 0, 7]   # odd, even, one and no voiced frames
    assert [(r[:n] > 1).sum().item() for r, n in zip(tr[2], tr[3])] == [14, 9, 4, 6, 0]
