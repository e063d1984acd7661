"""CPU side of the fp16p8 precision plan (svc_*_plan_*, svc_*_calibrate, BigVGAN / HiFT .calibrate / .precision_plan):
the entry points are declared, exported and bound; the CPU statement of both range censuses (voc_plan_cases.py) reproduces the
window the design rests on, with torch.float8_e4m3fn as the yardstick; plan get / set / reset and the OR-accumulation work on
a handle that needs no device; and every refusal comes before anything is launched and leaves the plan untouched."""
import ctypes as C
import inspect
import math
import os
import re

import pytest
import torch

import cases
import voc_plan_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)

NEW = ["svc_bigvgan_plan_size", "svc_bigvgan_plan_name", "svc_bigvgan_plan_get", "svc_bigvgan_plan_set", "svc_bigvgan_plan_reset",
       "svc_bigvgan_calibrate", "svc_hift_plan_size", "svc_hift_plan_name", "svc_hift_plan_get", "svc_hift_plan_set",
       "svc_hift_plan_reset", "svc_hift_calibrate", "svc_op_range_census", "svc_op_weight_census", "svc_op_plan_fake",
       "svc_op_plan_apply"]


def _L():
    from seedvc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def _fields(header, struct):
    body = re.search(r"\{([^{}]*)\}\s*" + struct + ";", header).group(1)
    return re.findall(r"\**\s*([A-Za-z_0-9]+)\s*(?:\[\d+\])?\s*[,;]", body)


def test_plan_entry_points_are_declared_exported_and_bound():
    _lib = _L()
    from seedvc_amd import ops, vocoder
    lib = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "seedvc_hip.h")).read()
    declared = set(re.findall(r"\b(svc_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/seedvc_hip.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert lib.svc_abi_version() == 1 and "#define SVC_ABI_VERSION 1" in header        # additive
    assert header.index("op-level entry points") < header.index("svc_op_range_census")
    assert _fields(header, "svc_census_t") == [f[0] for f in _lib.Census._fields_] and C.sizeof(_lib.Census) == 80
    assert _fields(header, "svc_plan_row_t") == [f[0] for f in _lib.PlanRow._fields_] and C.sizeof(_lib.PlanRow) == 128
    assert _fields(header, "svc_range_census_t") == [f[0] for f in _lib.RangeCensus._fields_]
    for cls in (vocoder.BigVGAN, vocoder.HiFT):
        p = inspect.signature(cls.calibrate).parameters
        assert p["lens"].default is None and p["tau"].default == 2.0 ** -6
        assert isinstance(cls.precision_plan, property) and cls.precision_plan.fset is not None and callable(cls.reset_plan)
        assert inspect.signature(cls.__init__).parameters["precision"].default == "fp16p8"
    assert callable(ops.range_census) and callable(ops.weight_census)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8w" in design and "svc_bigvgan_calibrate" in design
    assert "precision_plan" in open(os.path.join(ROOT, "README.md")).read()
    assert "svc_op_range_census" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_census_statement_counts_by_hand():
    #            zero  clamp   subnormal  in range  lo flushes          lo clamps
    hi = torch.tensor([0.0, 500.0, 2.0 ** -7, 1.0, 0.5, 4.0]).half().reshape(1, 1, 6)
    lo = torch.tensor([0.0, 0.125, 0.0, 2.0 ** -12, 2.0 ** -21, 0.25]).half().reshape(1, 1, 6)
    d = V.census_ref(hi, lo, 6)
    assert (d["n"], d["n_hi_clamp"], d["n_hi_sub"], d["n_lo_flush"], d["n_lo_clamp"]) == (5, 1, 1, 1, 1)
    assert d["max_hi"] == 500.0
    # 2^-7 is an e4m3 subnormal (kept exactly), 500 clamps to 448; 2^11 2^-21 = 2^-10 is half the smallest subnormal: flushed
    assert d["s_hi_err2"] == (500.0 - 448.0) ** 2
    assert d["s_lo_err2"] == (2.0 ** -21) ** 2 + (0.25 - 448.0 / 2048.0) ** 2
    # rows at and above lens and channels at and above C are not part of the census
    hi2 = torch.cat([hi, torch.full((1, 1, 6), float("nan")).half()], 1)
    lo2 = torch.cat([lo, torch.full((1, 1, 6), float("nan")).half()], 1)
    assert V.census_ref(hi2, lo2, 6, [1]) == d
    assert V.census_ref(hi, lo, 4)["n"] == 3


@pytest.mark.parametrize("log2_rms,rho,eta", [(0, 6e-4, 7e-4), (-6, 6.9e-3, 1.5e-3), (-8, 9.6e-2, 2.1e-2), (-10, 0.75, 0.33),
                                              (8, 1.5e-3, 2.4e-2), (9, 6.2e-2, 0.20), (10, 0.25, 0.47)])
def test_census_statement_reproduces_the_window(log2_rms, rho, eta):
    """The loss ratios of Gaussian planes against the CPU simulation the design quotes: flat over the
    window, rising to 1 below 2^-10 and above 2^9."""
    v = cases.randn("voc_plan.window", 7300 + log2_rms, 1, 512, 128) * 2.0 ** log2_rms
    hi, lo = V.split_planes(v)
    r, e = V.ratios(V.census_ref(hi, lo, 128))
    print(f"RMS 2^{log2_rms}: rho {r:.3g} (table {rho:.3g}), eta {e:.3g} (table {eta:.3g})")
    assert rho / 1.5 < r < rho * 1.5 and eta / 1.5 < e < eta * 1.5
    assert (max(r, e) > V.TAU) == (log2_rms in (-8, -10, 8, 9, 10))     # what the default tau vetoes (2^8: the clamp's tail)


def test_census_case_covers_every_count():
    hi, lo = V.census_planes()
    d = V.census_ref(hi, lo, V.CENSUS_SHAPE[2], list(V.CENSUS_LENS))
    live = sum(V.CENSUS_LENS) * V.CENSUS_SHAPE[2]
    assert all(d[k] > 50 for k in V.COUNTS) and d["n"] < live and d["max_hi"] > 448
    assert torch.isnan(hi[1, 1:]).all() and torch.isnan(hi[:, :, V.CENSUS_SHAPE[2]:]).all()      # what the kernel must not read


def test_weight_census_statement():
    w = V.census_weight()
    s, ex = V.weight_census_ref(w)
    assert ex == math.floor(math.log2(224.0 / w.abs().max().item()))
    assert (s[5] == 0).all() and (s[40] == 0).all()                     # all-zero channels: exempt (ratio 0)
    live = s[:, 0] > 0
    om_hi, om_lo = s[live, 1] / s[live, 0], s[live, 3] / s[live, 2]
    # one scale per layer from max|w|: the loudest channel sits inside the window, the quietest ones lose their correction
    # bytes -- the per-channel omega is what tells them apart
    gain = w.reshape(64, -1).abs().amax(1)[live]
    assert om_hi[gain.argmax()] < 1e-3 and om_lo[gain.argmax()] < 1e-3
    assert om_lo[gain.argmin()] > V.TAU and om_hi.max() > V.TAU
    # the fp16x3 planes themselves hold the weight to ~2^-22
    assert ((s[live, 2] / s[live, 0]).sqrt() < 2.0 ** -11).all()


def _fake(n=8, precision=3):
    lib = _L().lib()
    h = C.c_void_p()
    assert lib.svc_op_plan_fake(precision, n, C.byref(h)) == 0
    return lib, h


def _get(lib, h, n):
    v = (C.c_uint8 * n)()
    assert lib.svc_bigvgan_plan_get(h, v, n) == 0
    return list(v)


def test_plan_get_set_reset_and_or_accumulation():
    _lib = _L()
    lib, h = _fake(8)
    try:
        assert lib.svc_bigvgan_plan_size(h) == 8
        names = [lib.svc_bigvgan_plan_name(h, i).decode() for i in range(8)]
        assert names == ["resblocks.0.convs1.0", "resblocks.0.convs2.0", "resblocks.0.convs1.1", "resblocks.0.convs2.1",
                         "resblocks.0.convs1.2", "resblocks.0.convs2.2", "resblocks.1.convs1.0", "resblocks.1.convs2.0"]
        assert lib.svc_bigvgan_plan_name(h, 8) is None and lib.svc_bigvgan_plan_name(h, -1) is None
        assert _get(lib, h, 8) == [0] * 8                                   # the default plan is empty
        want = [0, 1, 0, 0, 1, 0, 0, 1]
        assert lib.svc_bigvgan_plan_set(h, (C.c_uint8 * 8)(*want), 8) == 0 and _get(lib, h, 8) == want
        # calibrate's decision: a ratio above tau vetoes, and the plan takes the OR with what it held
        rows = (_lib.PlanRow * 8)()
        rows[0].rho, rows[2].eta, rows[3].omega_hi, rows[6].omega_lo = 0.02, 0.5, 1.0, 0.016
        rows[5].rho = rows[5].eta = rows[5].omega_hi = rows[5].omega_lo = 2.0 ** -6       # AT tau: not above it
        assert lib.svc_op_plan_apply(h, rows, 8, 2.0 ** -6) == 0
        assert [r.veto for r in rows] == [1, 0, 1, 1, 0, 0, 1, 0]
        assert _get(lib, h, 8) == [1, 1, 1, 1, 1, 0, 1, 1]
        rows = (_lib.PlanRow * 8)()                                         # a later call that finds nothing removes nothing
        assert lib.svc_op_plan_apply(h, rows, 8, 2.0 ** -6) == 0 and _get(lib, h, 8) == [1, 1, 1, 1, 1, 0, 1, 1]
        assert lib.svc_bigvgan_plan_reset(h) == 0 and _get(lib, h, 8) == [0] * 8
    finally:
        lib.svc_bigvgan_destroy(h)


def test_plan_and_calibrate_refusals_leave_the_plan_untouched():
    _lib = _L()
    lib, h = _fake(8)
    lib3, h2 = _fake(8, precision=2)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)      # noqa: E731
    one = C.c_void_p(16)                           # never dereferenced: the checks come first
    rows = (_lib.PlanRow * 8)()
    want = [1, 0, 0, 1, 0, 0, 0, 1]
    try:
        assert lib.svc_bigvgan_plan_set(h, (C.c_uint8 * 8)(*want), 8) == 0

        def refused(rc, word):
            assert rc != 0 and word in lib.svc_last_error(), (rc, lib.svc_last_error())
            assert _get(lib, h, 8) == want

        v8, v7 = (C.c_uint8 * 8)(*([1] * 8)), (C.c_uint8 * 7)(*([1] * 7))
        refused(lib.svc_bigvgan_plan_set(h, v7, 7), b"plan size")
        refused(lib.svc_bigvgan_plan_set(h, None, 8), b"NULL")
        refused(lib.svc_bigvgan_plan_get(h, v7, 7), b"plan size")
        refused(lib.svc_bigvgan_plan_get(h, None, 8), b"NULL")
        refused(lib.svc_bigvgan_plan_set(None, v8, 8), b"null handle")
        refused(lib.svc_bigvgan_plan_reset(None), b"null handle")
        # a handle of another precision has no plan
        assert lib.svc_bigvgan_plan_size(h2) == -1 and lib.svc_bigvgan_plan_size(None) == -1
        refused(lib.svc_bigvgan_plan_set(h2, v8, 8), b"fp16p8")
        refused(lib.svc_bigvgan_plan_get(h2, v8, 8), b"fp16p8")
        refused(lib.svc_bigvgan_plan_reset(h2), b"fp16p8")
        tau = 2.0 ** -6
        refused(lib.svc_bigvgan_calibrate(h2, one, None, 2, 64, tau, rows, 8, None), b"fp16p8")
        refused(lib.svc_bigvgan_calibrate(None, one, None, 2, 64, tau, rows, 8, None), b"null handle")
        refused(lib.svc_bigvgan_calibrate(h, None, None, 2, 64, tau, rows, 8, None), b"mel and rows")
        refused(lib.svc_bigvgan_calibrate(h, one, None, 2, 64, tau, None, 8, None), b"mel and rows")
        refused(lib.svc_bigvgan_calibrate(h, one, None, 2, 64, tau, rows, 7, None), b"plan size")
        for bad in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            refused(lib.svc_bigvgan_calibrate(h, one, None, 2, 64, bad, rows, 8, None), b"tau")
        refused(lib.svc_bigvgan_calibrate(h, one, None, 0, 64, tau, rows, 8, None), b"B and S")
        refused(lib.svc_bigvgan_calibrate(h, one, None, 2, 0, tau, rows, 8, None), b"B and S")
        refused(lib.svc_bigvgan_calibrate(h, one, None, 1 << 15, 1 << 15, tau, rows, 8, None), b"2^31")
        refused(lib.svc_bigvgan_calibrate(h, one, i32(64, 0), 2, 64, tau, rows, 8, None), b"lens")
        refused(lib.svc_bigvgan_calibrate(h, one, i32(65, 3), 2, 64, tau, rows, 8, None), b"lens")
        # the HiFT mirror checks its handle first as well
        assert lib.svc_hift_plan_size(None) == -1 and lib.svc_hift_plan_name(None, 0) is None
        for rc in (lib.svc_hift_plan_get(None, v8, 8), lib.svc_hift_plan_set(None, v8, 8), lib.svc_hift_plan_reset(None),
                   lib.svc_hift_calibrate(None, one, None, None, one, one, 2, 32, tau, rows, 8, None)):
            refused(rc, b"null handle")
    finally:
        lib.svc_bigvgan_destroy(h)
        lib.svc_bigvgan_destroy(h2)


def test_census_seams_refuse_before_any_launch():
    _lib = _L()
    lib = _lib.lib()
    out = _lib.Census()
    i32 = lambda *v: (C.c_int32 * len(v))(*v)      # noqa: E731

    def census(**kw):
        e = _lib.RangeCensus()
        e.hi, e.lo, e.B, e.L, e.C, e.ld, e.out = 16, 16, 3, 200, 72, 128, C.pointer(out)
        for k, v in kw.items():
            setattr(e, k, v)
        return lib.svc_op_range_census(C.byref(e), None)

    assert lib.svc_op_range_census(None, None) != 0
    for kw in (dict(hi=None), dict(lo=None), dict(out=None), dict(B=0), dict(L=0), dict(C=0), dict(ld=71), dict(ld=74), dict(hi=20),
               dict(lo=12), dict(lens=i32(200, 1, 201)), dict(lens=i32(-1, 1, 1)), dict(B=1 << 16, L=1 << 15)):
        assert census(**kw) != 0, kw
        assert b"svc_op_range_census" in lib.svc_last_error()
    o = (C.c_double * 4)()
    for args in ((None, 4, 4, 7, o), (16, 4, 4, 7, None), (16, 0, 4, 7, o), (16, 4, 0, 7, o), (16, 4, 4, 1, o), (16, 4, 4, 17, o)):
        assert lib.svc_op_weight_census(*args, None, None) != 0, args
        assert b"svc_op_weight_census" in lib.svc_last_error()
