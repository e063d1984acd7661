"""CPU side of per-utterance noise seeds (`svc_cfm_sample_seeded`, `svc_hift_forward_seeded`, `svc_cfm_noise_draws`,
`svc_hift_noise_draws`, `pipeline.derive_seed` and the `seeds=` keywords): the entry points are declared, exported and
bound; seeds are refused before anything touches a device; `derive_seed` is the documented function; and the numpy
restatement of the draw layout the GPU tests compare the device with gives N(0, 1) draws with the prefix property."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cases
import seeded_noise_cases as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("svc_cfm_sample_seeded", "svc_hift_forward_seeded", "svc_cfm_noise_draws", "svc_hift_noise_draws")
torch.set_grad_enabled(False)


def test_entry_points_are_declared_exported_and_bound():
    from seedvc_amd import _lib, pipeline
    from seedvc_amd.cfm import CFM
    from seedvc_amd.vocoder import HiFT
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
        assert getattr(_lib.lib(), name).argtypes, f"{name} has no prototype (64-bit seeds need one)"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    for fn, kw in ((CFM.inference, "seeds"), (HiFT.__call__, "seeds"), (pipeline.HotPath.convert_batch, "seeds"),
                   (pipeline.HotPath.convert_long_batch, "seeds"),
                   (pipeline.V2HotPath.convert_batch, "noise_seeds")):
        assert inspect.signature(fn).parameters[kw].default is None, (fn.__qualname__, kw)
    assert callable(CFM.noise_draws) and callable(HiFT.noise_draws)


def test_c_argument_checks_need_no_gpu():
    """NULL handle / seeds / output: refused by the checks that come before any device call."""
    from seedvc_amd import _lib
    l = _lib.lib()
    one = ctypes.c_void_p(16)
    assert l.svc_cfm_sample_seeded(None, None, None, None) != 0
    assert l.svc_hift_forward_seeded(None, one, None, None, (ctypes.c_uint64 * 1)(3), 1, 4, one, None, None) != 0
    assert l.svc_cfm_noise_draws(1234, 80, 16, None, None) != 0 and b"null" in l.svc_last_error()
    assert l.svc_cfm_noise_draws(1234, 0, 16, one, None) != 0 and b"svc_cfm_noise_draws" in l.svc_last_error()
    assert l.svc_hift_noise_draws(1234, 9, 0, one, one, None) != 0 and b"svc_hift_noise_draws" in l.svc_last_error()
    assert l.svc_hift_noise_draws(1234, 9, 2 ** 31, one, one, None) != 0
    assert l.svc_hift_noise_draws(1234, 9, 64, None, one, None) != 0


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1, 1234])
@pytest.mark.parametrize("index", [0, 1, 63])
def test_derive_seed_equals_its_restatement(seed, index):
    from seedvc_amd.pipeline import derive_seed
    got = derive_seed(seed, index)
    assert isinstance(got, int) and 0 <= got < 2 ** 64
    assert got == SN.derive_seed_reference(seed, index)


def test_derive_seed_is_injective_in_the_index_and_checks_its_arguments():
    from seedvc_amd.pipeline import derive_seed
    vals = [derive_seed(1234, i) for i in range(10000)]
    assert len(set(vals)) == 10000 and all(0 <= v < 2 ** 64 for v in vals)
    assert derive_seed(1234, 0) != derive_seed(1235, 0) and derive_seed(0, 0) != 0
    for bad in ((-1, 0), (2 ** 64, 0), (5, -1)):
        with pytest.raises(ValueError, match="derive_seed"):
            derive_seed(*bad)


# ----------------------------------------------------------------------------------------- refusals before any device
def _bare_cfm():
    from seedvc_amd.cfm import CFM
    cfm = CFM.__new__(CFM)                         # no handle, no device: the refusals come before either is touched
    cfm.cfg, cfm.in_channels, cfm.device = dict(version=1), 80, torch.device("cpu")
    return cfm


def _bare_hift():
    from seedvc_amd.vocoder import HiFT
    voc = HiFT.__new__(HiFT)
    voc.cfg, voc.total_up, voc.device, voc._h = dict(nb_harmonics=8), 8, torch.device("cpu"), None
    return voc


BAD_SEEDS = [([1, 2], "2 seeds for 3"), ([1, -1, 2], "outside"), ([1, 2 ** 64, 2], "outside")]


@pytest.mark.parametrize("seeds,msg", BAD_SEEDS, ids=["count", "negative", "too_large"])
def test_mirrors_refuse_bad_seeds(seeds, msg):
    mu, prompt, style = torch.zeros(3, 12, 8), torch.zeros(3, 80, 4), torch.zeros(3, 4)
    with pytest.raises(ValueError, match=msg):
        _bare_cfm().inference(mu, [12] * 3, prompt, style, None, 2, seeds=seeds)
    with pytest.raises(ValueError, match=msg):
        _bare_hift()(torch.zeros(3, 80, 5), seeds=seeds)
    with pytest.raises(ValueError, match=msg):
        _bare_hift()(torch.zeros(3, 80, 5), seeds=seeds, lens=[5, 4, 0])


def test_mirrors_refuse_seeds_with_the_tensors_they_stand_for():
    mu, prompt, style = torch.zeros(2, 12, 8), torch.zeros(2, 80, 4), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="seeds or z"):
        _bare_cfm().inference(mu, [12] * 2, prompt, style, None, 2, seeds=[1, 2], z=torch.zeros(2, 80, 12))
    for kw in (dict(phase0=torch.zeros(2, 9, 1)), dict(noise=torch.zeros(2, 9, 40))):
        with pytest.raises(ValueError, match="seeds or phase0"):
            _bare_hift()(torch.zeros(2, 80, 5), seeds=[1, 2], **kw)
    for fn in (_bare_cfm().noise_draws, _bare_hift().noise_draws):
        for bad in (-1, 2 ** 64):
            with pytest.raises(ValueError, match="outside"):
                fn(bad, 8)


def test_pipeline_refusals_need_no_gpu():
    from seedvc_amd.pipeline import HotPath, RealtimeEngine, V2HotPath
    assert callable(HotPath.convert_batch_ragged_seeded) and callable(RealtimeEngine.step_seeded)
    hp = HotPath(None, None)
    mu, prompt, style = torch.zeros(3, 12, 8), torch.zeros(3, 80, 4), torch.zeros(3, 4)
    z = torch.zeros(3, 80, 12)
    with pytest.raises(ValueError, match="seeds or z"):
        hp.convert_batch(mu, prompt, style, 2, 0.7, seeds=[1, 2, 3], z=z)
    with pytest.raises(ValueError, match="seeds is None"):
        hp.convert_batch_ragged_seeded(mu, prompt, style, [12, 10, 9], [4, 3, 2], 2, 0.7, None)
    for call in (lambda seeds, **kw: hp.convert_batch(mu, prompt, style, 2, 0.7, seeds=seeds, **kw),
                 lambda seeds, **kw: hp.convert_batch_ragged_seeded(mu, prompt, style, [12, 10, 9], [4, 3, 2], 2, 0.7, seeds, **kw)):
        with pytest.raises(ValueError, match="phase0 / noise"):
            call([1, 2, 3], vocoder_kwargs=dict(noise=torch.zeros(3, 9, 64)))
        with pytest.raises(ValueError, match="phase0 / noise"):
            call([1, 2, 3], vocoder_kwargs=dict(phase0=torch.zeros(3, 9, 1)))
        for seeds, msg in BAD_SEEDS:
            with pytest.raises(ValueError, match=msg):
                call(seeds)
    c = cases.chunkloop_case("loop2")
    utt = (c["cond"], c["prompt_condition"], c["mel2"], c["style2"])
    with pytest.raises(ValueError, match="noise_fn"):
        hp.convert_long_batch([utt], 10, 0.7, 8, 60, seeds=[5], noise_fn=lambda T: torch.zeros(1, 80, T))
    with pytest.raises(ValueError, match="vocoder_kwargs_fn"):
        hp.convert_long_batch([utt], 10, 0.7, 8, 60, seeds=[5], vocoder_kwargs_fn=lambda s: {})
    for seeds, msg in (([1, 2], "2 seeds for 1"), ([-1], "outside"), ([2 ** 64], "outside")):
        with pytest.raises(ValueError, match=msg):
            hp.convert_long_batch([utt], 10, 0.7, 8, 60, seeds=seeds)
    import realtime_cases as RT
    import long_batch_cases as LB
    eng = RealtimeEngine(RT.FakeLR(), LB.BatchedFakeCFM("cpu"), RT.FakeVocoder(), max_streams=2, **RT.FAKE_GEOMETRY)
    slot = eng.open(torch.zeros(1, 5, cases.CHUNK_DC), torch.zeros(1, cases.CHUNK_C, 5), torch.zeros(1, 3))
    x = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="seeds is None"):
        eng.step_seeded([slot], x, 2, 0.7, None)
    with pytest.raises(ValueError, match="phase0 / noise"):
        eng.step_seeded([slot], x, 2, 0.7, [1], vocoder_kwargs=dict(noise=torch.zeros(1, 9, 96)))
    for seeds, msg in (([1, 2], "2 seeds for 1"), ([-1], "outside"), ([2 ** 64], "outside")):
        with pytest.raises(ValueError, match=msg):
            eng.step_seeded([slot], x, 2, 0.7, seeds)
    v2 = V2HotPath.__new__(V2HotPath)
    v2.device = torch.device("cpu")
    with pytest.raises(ValueError, match="seeds or z"):
        v2.convert_batch([x], [{}], [1.0], 2, noise_seeds=[1], z=[torch.zeros(1, 80, 9)])
    with pytest.raises(ValueError, match="outside"):
        v2.convert_batch([x], [{}], [1.0], 2, noise_seeds=[-1])


# ----------------------------------------------------------------------------------------- the restatement of the layout
SHAPES = [(80, 512, SN.DOMAIN_Z), (9, 4096, SN.DOMAIN_HIFT_NOISE)]


@pytest.mark.parametrize("seed", SN.STAT_SEEDS)
@pytest.mark.parametrize("rows,n,domain", SHAPES, ids=["sampler_z", "hift_noise"])
def test_restated_draws_are_standard_normal(seed, rows, n, domain):
    x = SN.reference_normals(seed, domain, rows, n)
    assert x.shape == (rows, n)
    SN.check_statistics(x, f"seed {seed}, {rows} x {n}, domain {domain}")
    assert abs(x.mean()) < 0.02 and 0.95 < x.var() < 1.05


@pytest.mark.parametrize("rows,n,domain", SHAPES, ids=["sampler_z", "hift_noise"])
def test_restated_draws_have_the_prefix_property_and_depend_on_seed_and_domain(rows, n, domain):
    x = SN.reference_normals(1234, domain, rows, n)
    assert np.array_equal(SN.reference_normals(1234, domain, rows - 3, n), x[:rows - 3])       # fewer rows (not a multiple of 4)
    assert np.array_equal(SN.reference_normals(1234, domain, rows, n - 67), x[:, :n - 67])     # fewer positions
    assert np.array_equal(SN.reference_normals(1234, domain, 1, 1), x[:1, :1])
    for other in (SN.reference_normals(1235, domain, rows, n), SN.reference_normals(1234, domain + 1, rows, n),
                  SN.reference_normals(1234 + 2 ** 32, domain, rows, n)):                      # the high key word counts
        assert not np.array_equal(other, x)
        assert abs(np.corrcoef(other.reshape(-1), x.reshape(-1))[0, 1]) < 4.5 / np.sqrt(x.size)
    u = SN.reference_uniforms(1234, domain, rows, n)
    assert u.min() > 0.0 and u.max() <= 1.0 and np.array_equal(u * 2.0 ** 24, np.round(u * 2.0 ** 24))
    ph = SN.reference_phase0(1234, 9)
    assert ph.shape == (9,) and np.abs(ph).max() <= np.pi and len(set(ph.tolist())) == 9
    assert not np.array_equal(ph, SN.reference_phase0(77, 9))
