"""GPU tests of the DiT's full-precision mode (svc_dit_create_ex precision 2, fp16x3): the split-precision attention at
op level against float64, estimator and sampler against the float64 yardstick beside a precision-1 handle of the same weights, the
sampler's contracts bit for bit on precision-2 handles, precision 1 unchanged, the refusals, and V2HotPath(cfm_timbre=)."""
import ctypes as C
import functools

import pytest
import torch

import cases
import dit_precision_cases as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"


# --------------------------------------------------------------------------------------------------- 1. attention op
@functools.lru_cache(maxsize=None)
def _attn(name):
    """(inputs, device output, float64 reference, float32 reference) of one launch; computed once."""
    from seedvc_amd import ops
    q, k, v, lens, q_start = P.attention_case(name)
    out = ops.attention_x3(q.to(DEV), k.to(DEV), v.to(DEV), lens, Tq=P.ATTN_TQ, q_start=q_start).cpu()
    return (q, k, v, lens, q_start), out, P.attention_ref(q, k, v, lens, torch.float64), P.attention_ref(q, k, v, lens, torch.float32)


@pytest.mark.parametrize("name", list(P.ATTN_LAUNCHES))
def test_attention_x3_against_float64(name):
    (q, k, v, lens, q_start), out, ref64, ref32 = _attn(name)
    rows = slice(q_start, P.ATTN_TQ)
    got = out[:, rows]
    assert not torch.isnan(got).any(), "NaN from k / v rows at or above kv_len reached the output"
    assert torch.isnan(out[:, :q_start]).all() and torch.isnan(out[:, P.ATTN_TQ:]).all(), "rows outside [q_start, Tq) were written"
    err = (got.double() - ref64[:, rows]).abs()
    noise32 = (ref32[:, rows].double() - ref64[:, rows]).abs().amax(dim=(1, 3), keepdim=True)       # per (sequence, head)
    tol = 4 * noise32 + P.attention_x3_level(q, k, v, lens)
    worst = (err.amax(dim=(1, 3), keepdim=True) / tol).flatten().tolist()
    print(f"attention_x3 {name}: max err {err.max().item():.3e}, max noise32 {noise32.max().item():.3e}, err / tol per (seq, head) "
          + " ".join(f"{w:.2f}" for w in worst))
    assert (err <= tol).all(), worst


@pytest.mark.parametrize("name", list(P.ATTN_LAUNCHES))
def test_attention_x3_sequence_alone_equals_in_batch(name):
    from seedvc_amd import ops
    (q, k, v, lens, q_start), out, _, _ = _attn(name)
    for s in range(len(lens)):
        alone = ops.attention_x3(q[s:s + 1].to(DEV), k[s:s + 1].to(DEV), v[s:s + 1].to(DEV), lens[s:s + 1], Tq=P.ATTN_TQ,
                                 q_start=q_start).cpu()
        assert torch.equal(alone[0, q_start:P.ATTN_TQ], out[s, q_start:P.ATTN_TQ]), f"sequence {s} depends on its batch"


def test_attention_x3_refusals_and_zero_length():
    from seedvc_amd import ops
    q = torch.randn(1, 16, 1, 64, device=DEV)
    for kw, lens in ((dict(Tq=17), [4]), (dict(q_start=16), [4]), (dict(q_start=-1), [4]), (dict(), [17]), (dict(), [-1])):
        with pytest.raises(RuntimeError, match="svc_op_attention_x3"):
            ops.attention_x3(q, q, q, lens, **kw)
    assert ops.attention_x3(q, q, q, [0]).abs().max().item() == 0.0          # no keys: zero rows


# --------------------------------------------------------------------------------------------------- 2. estimator and sampler
@functools.lru_cache(maxsize=None)
def _pair(name):
    """(precision-1 CFM, precision-2 CFM) packed from the weights of cases.dit_case(name)."""
    from seedvc_amd.cfm import CFM
    cfg, sd = cases.dit_case(name)[:2]
    return CFM(cfg, sd, DEV), CFM(cfg, sd, DEV, precision="fp16x3")


def _check(name, what, e1, e2, eg, bound, measured, golden_bound=None):
    print(f"{name}: {what} vs float64: precision 1 {e1:.3e}, precision 2 {e2:.3e} (ratio {e2 / e1:.2e}); precision 2 vs fp32 golden {eg:.3e}")
    assert e2 <= P.P2_CAP * e1, f"{name}: precision 2 {what} {e2:.3e} is above 1/50 of precision 1's {e1:.3e}"
    assert bound is not None and abs(bound - 4 * measured) <= 1e-12 * bound, "the committed bound is 4 x the committed measurement"
    assert e2 <= bound, f"{name}: precision 2 {what} {e2:.3e} is above the committed bound {bound:.3e}"
    if golden_bound is not None:
        assert eg < golden_bound, f"{name}: precision 2 vs the reference's fp32 golden {eg:.3e}"


@pytest.mark.parametrize("name", list(cases.DIT_CASES))
def test_estimator_against_float64(name, golden):
    cfg, sd, inp, meta, est64, _ = P.dit_reference(name)
    p1, p2 = _pair(name)
    assert (p1.precision, p2.precision, p2.estimator.precision) == (1, 2, 2)
    T, Pl = meta["T"], meta["P"]
    prompt_x = torch.zeros(1, cfg["C"], T)
    prompt_x[..., :Pl] = inp["prompt"]
    y = [m.estimator(inp["x"].to(DEV), prompt_x.to(DEV), torch.LongTensor([T]), inp["t"], inp["style"].to(DEV), inp["mu"].to(DEV)).cpu()
         for m in (p1, p2)]
    e1, e2 = ((t.double() - est64).abs().max().item() for t in y)
    eg = (y[1] - torch.from_numpy(golden[name + ".est"])).abs().mean().item()
    _check(name, "estimator max-abs", e1, e2, eg, P.P2_EST_MAXABS_BOUND, P.P2_EST_MAXABS_MEASURED, P.GOLDEN_MEL_L1)


@pytest.mark.parametrize("name", list(cases.DIT_CASES))
def test_sampler_against_float64(name, golden):
    cfg, sd, inp, meta, _, smp64 = P.dit_reference(name)
    p1, p2 = _pair(name)
    y = [m.inference(inp["mu"].to(DEV), torch.LongTensor([meta["T"]]), inp["prompt"].to(DEV), inp["style"].to(DEV), None, meta["n_steps"],
                     inference_cfg_rate=meta["cfg_rate"], z=inp["z"].to(DEV), random_voice=meta["random_voice"]).cpu() for m in (p1, p2)]
    e1, e2 = ((t.double() - smp64).abs().mean().item() for t in y)
    eg = (y[1] - torch.from_numpy(golden[name + ".sample"])).abs().mean().item()
    _check(name, "sampler mel L1", e1, e2, eg, P.P2_SAMPLE_L1_BOUND, P.P2_SAMPLE_L1_MEASURED, P.GOLDEN_MEL_L1)
    assert float(y[1][..., :meta["P"]].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------- 3. contracts, bit for bit
CONTRACT_T, CONTRACT_P = 100, 16
HANDLES = ["tiny_r", "v2_r"]                      # a v1 handle and the v2 handle (prefix tokens, three guidance streams)


@functools.lru_cache(maxsize=None)
def _contract_inputs(name):
    cfg = cases.dit_case(name)[0]
    T, Pl, B = CONTRACT_T, CONTRACT_P, 3
    return dict(cfg=cfg, T=T, lens=[T, T - 17, 65], plens=[Pl, 9, 3],
                mu=cases.randn(name + ".p2.mu", 3, B, T, cfg["Dc"]), z=cases.randn(name + ".p2.z", 3, B, cfg["C"], T),
                prompt=cases.logmel(name + ".p2.prompt", 3, B, cfg["C"], Pl), style=cases.randn(name + ".p2.style", 3, B, cfg["style_dim"]),
                rate=[0.7, 0.5] if cfg["version"] == 2 else 0.7, steps=3)


def _run(cfm, c, rows=None, lens=None, plens=None, T=None, **kw):
    """cfm.inference on the rows `rows` of the contract inputs, cut to T frames."""
    rows = list(range(3)) if rows is None else rows
    T = T or c["T"]
    lens = [c["lens"][b] for b in rows] if lens is None else lens
    plens = [c["plens"][b] for b in rows] if plens is None else plens
    Pm = max(plens)
    args = dict(inference_cfg_rate=c["rate"], prompt_lens=plens)
    if "seeds" not in kw and "z" not in kw:
        kw["z"] = c["z"][rows][:, :, :T].to(DEV)
    args.update(kw)
    steps = args.pop("steps", c["steps"])
    return cfm.inference(c["mu"][rows][:, :T].to(DEV), torch.LongTensor(lens), c["prompt"][rows][:, :, :Pm].to(DEV), c["style"][rows].to(DEV),
                         None, steps, **args).cpu()


@pytest.mark.parametrize("name", HANDLES)
def test_p2_ragged_batch_equals_runs_alone(name):
    p2, c = _pair(name)[1], _contract_inputs(name)
    got = _run(p2, c)
    for b in range(3):
        Tb = c["lens"][b]
        alone = _run(p2, c, rows=[b], T=Tb)
        assert alone.shape[-1] == Tb and torch.isfinite(alone).all()
        assert torch.equal(got[b:b + 1, :, :Tb], alone), f"utterance {b} of the ragged batch differs from its run alone"


@pytest.mark.parametrize("name", HANDLES)
def test_p2_microbatch_graph_and_seeds(name):
    p2, c = _pair(name)[1], _contract_inputs(name)
    est = p2.estimator
    est.set_microbatch(3)
    base = _run(p2, c)
    est.set_microbatch(1)
    assert torch.equal(_run(p2, c), base), "micro-batch 1 differs from 3"
    # hipGraph: eager, capture + first replay, replay (micro-batch 1: three groups of one key inside each call)
    uniform = dict(lens=[c["T"]] * 3, plens=[CONTRACT_P] * 3)
    eager = _run(p2, c, **uniform)
    est.set_graphs(True)
    try:
        for i in range(3):
            assert torch.equal(_run(p2, c, **uniform), eager), f"graph call {i}"
    finally:
        est.set_graphs(False)
        est.set_microbatch(0)
    # seeds against the same draws handed in
    seeds = [5, 2 ** 63 + 11, 7]
    z = torch.cat([p2.noise_draws(s, c["T"]) for s in seeds])
    assert torch.equal(_run(p2, c, seeds=seeds), _run(p2, c, z=z))


@pytest.mark.parametrize("name", HANDLES)
def test_p2_rows_with_two_classes_equal_the_uniform_calls(name):
    p2, c = _pair(name)[1], _contract_inputs(name)
    v2 = c["cfg"]["version"] == 2
    sa = (3, [0.7, 0.5] if v2 else 0.7, 1.0)
    sb = (2, [0.0, 0.0] if v2 else 0.0, 0.8)
    settings = [sa, sb, sa]
    class_of, n_streams = p2.rows_plan(settings)
    assert class_of == [0, 1, 0] and n_streams == [3 if v2 else 2, 1]
    got = p2.inference_rows(c["mu"].to(DEV), torch.LongTensor(c["lens"]), c["prompt"].to(DEV), c["style"].to(DEV), settings,
                            z=c["z"].to(DEV), prompt_lens=c["plens"]).cpu()
    want_a = _run(p2, c, rows=[0, 2], steps=sa[0], inference_cfg_rate=sa[1], temperature=sa[2])
    want_b = _run(p2, c, rows=[1], steps=sb[0], inference_cfg_rate=sb[1], temperature=sb[2])
    assert torch.equal(got[[0, 2]], want_a) and torch.equal(got[1:2], want_b)


@pytest.mark.parametrize("name", HANDLES)
def test_p2_nan_in_padded_mu_rows_stays_out(name):
    p2, c = _pair(name)[1], _contract_inputs(name)
    clean = _run(p2, c)
    mu = c["mu"].clone()
    for b, L in enumerate(c["lens"]):
        mu[b, L:] = float("nan")
    got = p2.inference(mu.to(DEV), torch.LongTensor(c["lens"]), c["prompt"].to(DEV), c["style"].to(DEV), None, c["steps"],
                       inference_cfg_rate=c["rate"], z=c["z"].to(DEV), prompt_lens=c["plens"]).cpu()
    for b, L in enumerate(c["lens"]):
        assert torch.isfinite(got[b, :, :L]).all() and torch.equal(got[b, :, :L], clean[b, :, :L]), f"utterance {b}"


# --------------------------------------------------------------------------------------------------- 4. precision 1 unchanged
def _legacy_cfm(cfg, sd):
    """A CFM whose handle comes from svc_dit_create itself (the wrapper calls svc_dit_create_ex)."""
    from seedvc_amd import _lib
    from seedvc_amd.cfm import CFM, _cfg_struct
    m = CFM(cfg, sd, DEV)
    m.estimator.close()
    with torch.cuda.device(m.device):
        descs, n, keep = _lib.make_descs(sd, m.device)
        cs = _cfg_struct(cfg)
        _lib.check(_lib.lib().svc_dit_create(C.byref(cs), descs, n, _lib.stream_ptr(), C.byref(m.estimator._h)))
        torch.cuda.current_stream().synchronize()
    del keep
    assert _lib.lib().svc_dit_precision(m.estimator._h) == 1
    return m


@pytest.mark.parametrize("min_rows", [0, 1 << 40], ids=["fused", "tap-gemm"])
def test_create_ex_1_is_create(min_rows):
    cfg, sd, inp, meta = cases.dit_case("tiny_full")          # hidden_dim 384: the fused row-panel kernel exists
    T, Pl = meta["T"], meta["P"]
    prompt_x = torch.zeros(1, cfg["C"], T)
    prompt_x[..., :Pl] = inp["prompt"]
    a, b = _pair("tiny_full")[0], _legacy_cfm(cfg, sd)
    outs = []
    for m in (a, b):
        assert m.estimator.fused_available
        m.estimator.set_fused_min_rows(min_rows)
        est = m.estimator(inp["x"].to(DEV), prompt_x.to(DEV), torch.LongTensor([T]), inp["t"], inp["style"].to(DEV), inp["mu"].to(DEV)).cpu()
        smp = m.inference(inp["mu"].to(DEV), torch.LongTensor([T]), inp["prompt"].to(DEV), inp["style"].to(DEV), None, meta["n_steps"],
                          inference_cfg_rate=meta["cfg_rate"], z=inp["z"].to(DEV)).cpu()
        m.estimator.set_fused_min_rows(-1)
        outs.append((est, smp))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# --------------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("precision", [0, 3, -1])
def test_create_refuses_other_precisions(precision):
    from seedvc_amd import _lib
    from seedvc_amd.cfm import _cfg_struct
    cfg, sd = cases.dit_case("tiny_r")[:2]
    with torch.cuda.device(DEV):
        descs, n, keep = _lib.make_descs(sd, torch.device(DEV))
        cs, out = _cfg_struct(cfg), C.c_void_p()
        rc = _lib.lib().svc_dit_create_ex(C.byref(cs), descs, n, precision, _lib.stream_ptr(), C.byref(out))
    assert rc != 0 and out.value is None and b"precision" in _lib.lib().svc_last_error()


def test_fused_setters_on_a_precision_2_handle():
    p2, c = _pair("tiny_r")[1], _contract_inputs("tiny_r")
    est = p2.estimator
    assert not est.fused_available
    base = _run(p2, c)
    for rows, mask in ((0, 0), (1 << 40, 1), (-1, 3)):
        est.set_fused_min_rows(rows)
        est.set_fused_seams(mask)
        assert not est.fused_available and torch.equal(_run(p2, c), base)


# --------------------------------------------------------------------------------------------------- 6. V2HotPath(cfm_timbre=)
def test_v2_hotpath_timbre_cfm():
    """The timbre branch runs on cfm_timbre (equal to a chain whose cfm is that handle, pool and stream); the style branch does not
    see it (equal to the chain without it).  Exact stand-in models of v2_long_cases."""
    import ar_batch_cases as A
    import v2_long_cases as L
    from seedvc_amd.ar import ARModel
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath, collect_stream
    M = L.models()
    ar = ARModel(*M["ar"], DEV)
    ar.setup_caches(max_batch_size=4)
    parts = (ar, InterpolateRegulator(*M["ar_lr"], DEV), InterpolateRegulator(*M["cfm_lr"], DEV))
    from seedvc_amd.vocoder import BigVGAN
    voc = BigVGAN(*M["voc"], DEV)
    c1, c2 = CFM(*M["dit"], DEV), CFM(*M["dit"], DEV, precision=2)
    both, only2, only1 = V2HotPath(*parts, c1, voc, cfm_timbre=c2), V2HotPath(*parts, c2, voc), V2HotPath(*parts, c1, voc)
    assert only1.cfm_timbre is None
    fa, fb = L.qualified()[:2]

    def record(hp, f, frames):
        u = L.file_inputs(f)
        target = hp.prepare_target(u["target_narrow"], u["target_tokens"], u["target_mel"], u["style"])
        return dict(target=target, src_narrow=u["src_narrow"].to(DEV), src_tokens=u["src_tokens"].to(DEV),
                    frames_per_token=u["frames_per_token"], source_frames=frames)

    recs = [record(both, fa, 30), record(both, fb, 9)]
    window = recs[0]["target"]["P"] + 12
    kw = dict(convert_style=False, max_context_window=window, hop=L.HOP, overlap_frame_len=2, seeds=[21, 22])
    got = both.convert_long_batch(recs, L.N_STEPS, L.CFG_RATES, **kw)
    want = only2.convert_long_batch(recs, L.N_STEPS, L.CFG_RATES, **kw)
    plain = only1.convert_long_batch(recs, L.N_STEPS, L.CFG_RATES, **kw)
    streamed = collect_stream(both.convert_long_stream(recs, L.N_STEPS, L.CFG_RATES, **kw), len(recs))
    for g, w, p, s in zip(got, want, plain, streamed):
        assert torch.isfinite(g).all() and torch.equal(g, w) and torch.equal(s.to(g.device), g)
        assert not torch.equal(g, p), "the timbre branch did not change hands"
    skw = dict(max_context_window=64, hop=L.HOP, max_new=A.MAX_NEW, seeds=[31])
    srec = [record(both, fa, 0)]
    a = both.convert_long_batch(srec, L.N_STEPS, L.CFG_RATES, **skw)
    b = only1.convert_long_batch(srec, L.N_STEPS, L.CFG_RATES, **skw)
    assert torch.equal(a[0], b[0]), "the style branch saw cfm_timbre"
