"""GPU parity of the v2 AR decode step (row a20): prefill, eager and hipGraph-replayed one-token steps, and the
sampler, against the committed reference outputs."""
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
# logits of the fp16-weight / fp32-cache HIP model vs the reference's fp32 run, relative to mean |logit|
LOGIT_TOL = 5e-3
UNASSISTED_PREFIX_MIN = 160    # ar_gen_full with the PLAIN draws: all 160 tokens equal the reference run (measured; a near-tie flipped by a kernel change would show here)


# prefill_split = n: the prefill runs as two calls, the last n tokens second (n <= 8: the GEMV-pair layers on a cache that
# already holds the first part).  Split 0 keeps the ids the test had before the parameter.
AR_STEP_PARAMS = [pytest.param(name, use_graph, split, id=f"{name}-{use_graph}" + (f"-split{split}" if split else ""))
                  for name in cases.AR_CASES for use_graph in (False, True) for split in (0, 5)]


@pytest.mark.parametrize("name,use_graph,prefill_split", AR_STEP_PARAMS)
def test_ar_generate_steps(name, use_graph, prefill_split, golden):
    from seedvc_amd.ar import ARModel
    c, sd, x_prefill, input_pos, x_steps, exp_noise, meta = cases.ar_case(name)
    ar = ARModel(c, sd, "cuda:0")
    ar.setup_caches()
    ref_logits = torch.from_numpy(golden[name + ".logits"])
    ip = torch.tensor(input_pos)
    kv = torch.arange(meta["n_prefill"])
    if prefill_split:
        n = meta["n_prefill"] - prefill_split
        ar.forward_generate(x_prefill[:, :n].cuda(), ip[:n], kv[:n])
        lg = ar.forward_generate(x_prefill[:, n:].cuda(), ip[n:], kv[n:]).cpu()
    else:
        lg = ar.forward_generate(x_prefill.cuda(), ip, kv).cpu()
    scale = ref_logits.abs().mean().item()
    err0 = (lg[0] - ref_logits[0]).abs().max().item()
    print(f"{name}: prefill logits max err {err0:.3e} (|logits| mean {scale:.3f})")
    assert err0 < LOGIT_TOL * max(scale, 1.0)
    prev = []
    worst = err0
    for s in range(meta["n_decode"]):
        ip, kv = ip[-1:] + 1, kv[-1:] + 1
        if use_graph:
            lg = ar.decode_step(x_steps[s].cuda(), int(ip[0]) if s == 0 else None, int(kv[0]) if s == 0 else None).cpu()
        else:
            lg = ar.forward_generate(x_steps[s].cuda(), ip, kv).cpu()
        err = (lg[0] - ref_logits[s + 1]).abs().max().item()
        assert err < LOGIT_TOL * max(scale, 1.0), f"step {s}: {err:.3e}"
        worst = max(worst, err)
        # sampler parity on the REFERENCE logits (isolates the sampler from fp16 logit noise)
        pt = torch.tensor(prev, dtype=torch.int32) if prev else None
        idx, probs = ar.sample(ref_logits[s + 1].cuda(), pt, [c["vocab_size"] - 1], 0.7, 0.7, 1.5, exp_noise=exp_noise[s].cuda(),
                               return_probs=True)
        assert (probs.cpu() - torch.from_numpy(golden[name + ".probs"][s])).abs().max().item() < 1e-5
        assert int(idx) == int(golden[name + ".idx"][s])
        prev.append(int(idx))
    print(f"{name}: worst logit error over prefill + {meta['n_decode']} steps {worst:.3e} = {worst / max(scale, 1.0):.2e} x mean |logit|")


@pytest.mark.parametrize("name", list(cases.AR_GEN_CASES))
@pytest.mark.parametrize("check_every", [1, 16])
def test_generate_loop_matches_reference(name, check_every, golden):
    """8f row 4: the on-device token loop (`svc_ar_generate`: captured decode step + device sampler, EOS looked at every
    `check_every` tokens) reproduces the reference's NaiveWrapper.generate token for token with the same Exp(1) draws."""
    from seedvc_amd.ar import ARModel
    c, sd, text, target, exp_noise = cases.ar_gen_case(name)
    m = ARModel(c, sd, "cuda:0")
    codes = m.generate(text.cuda(), target.cuda(), top_p=0.7, temperature=0.7, repetition_penalty=1.5,
                       exp_noise=exp_noise.cuda(), check_every=check_every).cpu()
    ref = torch.from_numpy(golden[name + ".codes"])
    print(f"{name}: {codes.shape[-1]} tokens (reference {ref.shape[-1]})")
    assert codes.shape == ref.shape and torch.equal(codes, ref)
    # a second call on the same handle starts from a clean cache / positions
    again = m.generate(text.cuda(), target.cuda(), exp_noise=exp_noise.cuda(), check_every=check_every).cpu()
    assert torch.equal(again, ref)


def test_generate_loop_full_size(golden):
    """BASELINE configs[4] size through `svc_ar_generate`: the full ar_base model, 120 condition frames + 200 prompt
    tokens, 160 generated tokens, token for token against the reference run (HIP logits -> same tokens, not only the
    sampler on reference logits).  ASSISTED: the Exp(1) draw of every reference token is divided by AR_GEN_FULL_BOOST = 4
    (cases.ar_gen_full_case), so a HIP token only flips if the logit error moves the winner by more than 4x or pushes it
    out of the top-p set; the unassisted run with the plain draws is reported below through its identical prefix."""
    from seedvc_amd.ar import ARModel
    ref = torch.from_numpy(golden["ar_gen_full.codes"])
    c, sd, text, target, exp_noise = cases.ar_gen_full_case(winners=ref)
    m = ARModel(c, sd, "cuda:0")
    codes = m.generate(text.cuda(), target.cuda(), top_p=0.7, temperature=0.7, repetition_penalty=1.5,
                       exp_noise=exp_noise.cuda(), max_new=cases.AR_GEN_FULL_TOKENS, check_every=16).cpu()
    n_same = int((codes[0, :ref.shape[1]] == ref[0, :codes.shape[1]]).long().cumprod(0).sum()) if codes.numel() else 0
    print(f"ar_gen_full: {codes.shape[-1]} tokens, first {n_same} identical to the reference")
    assert codes.shape == ref.shape and torch.equal(codes, ref)
    # unassisted: the plain Exp(1) rows (the draws the reference run itself used).  A near-tie in the exponential race may
    # flip on fp16-weight logits, after which the trajectories differ by construction: the identical prefix is the figure.
    c, sd, text, target, plain = cases.ar_gen_full_case()
    codes_p = m.generate(text.cuda(), target.cuda(), top_p=0.7, temperature=0.7, repetition_penalty=1.5,
                         exp_noise=plain.cuda(), max_new=cases.AR_GEN_FULL_TOKENS, check_every=16).cpu()
    n_plain = int((codes_p[0, :ref.shape[1]] == ref[0, :codes_p.shape[1]]).long().cumprod(0).sum())
    print(f"ar_gen_full, plain draws (unassisted): first {n_plain} of {ref.shape[1]} tokens identical to the reference")
    assert n_plain >= UNASSISTED_PREFIX_MIN


# intermediate_size 2624 > 64 * 8 * DEC_MAXC: the decode-step kernels refuse the shape, so S = 1 runs the GEMV-pair layers
AR_GEMV_STEP = dict(dim=128, n_head=2, n_local_heads=1, n_layer=3, intermediate_size=2624, vocab_size=65, max_seq_len=64)


@pytest.mark.parametrize("use_graph", [False, True])
def test_ar_one_token_gemv_pair_steps(use_graph):
    """S = 1 on a shape the decode step does not hold goes through the GEMV-pair layers: prefill, then eager or
    hipGraph-replayed one-token steps against the oracle (pinned to the reference by test_oracle_golden.py)."""
    import seedvc_oracle as O
    from seedvc_amd import specs, weights
    from seedvc_amd.ar import ARModel
    seed, n_prefill, n_decode = 65, 9, 4
    c = specs.ar_config(**AR_GEMV_STEP)
    sd = weights.make_state_dict(specs.ar_state_spec(c), seed=seed, prefix="ar.")
    x_prefill = cases.randn("ar_gemv_step.prefill", seed, 1, n_prefill, c["dim"])
    x_steps = cases.randn("ar_gemv_step.steps", seed, n_decode, 1, 1, c["dim"])
    caches = O.ar_new_cache(c)
    ar = ARModel(c, sd, "cuda:0")
    ar.setup_caches()
    ip = torch.tensor(list(range(n_prefill // 2 + 1)) + list(range(n_prefill - n_prefill // 2 - 1)))
    kv = torch.arange(n_prefill)
    ref = O.ar_forward_generate(sd, c, x_prefill, ip, kv, caches)
    lg = ar.forward_generate(x_prefill.cuda(), ip, kv).cpu()
    scale = max(ref.abs().mean().item(), 1.0)
    err = (lg - ref).abs().max().item()
    assert err < LOGIT_TOL * scale, f"prefill: {err:.3e}"
    for s in range(n_decode):
        ip, kv = ip[-1:] + 1, kv[-1:] + 1
        ref = O.ar_forward_generate(sd, c, x_steps[s], ip, kv, caches)
        if use_graph:
            lg = ar.decode_step(x_steps[s].cuda(), int(ip[0]) if s == 0 else None, int(kv[0]) if s == 0 else None).cpu()
        else:
            lg = ar.forward_generate(x_steps[s].cuda(), ip, kv).cpu()
        err = (lg - ref).abs().max().item()
        assert err < LOGIT_TOL * scale, f"step {s}: {err:.3e}"
