"""GPU tests of continuous batching: the ragged prefill (`svc_ar_prefill_batch`) against the oracle and against itself
(alone / in company / another slot / another place / split into passes / on a poisoned cache: bit for bit), and sessions
(`svc_ar_admit / _run / _retire`, `ARSession`) token for token against the reference and against the same request alone."""
import pytest
import torch

import ar_batch_cases as A
import ar_session_cases as S
import cases

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOGIT_TOL = A.LOGIT_TOL            # 5e-3 x max(mean |reference|, 1): the project's bound (tests/test_gpu_ar.py)
PARAMS = dict(top_p=0.7, temperature=0.7, repetition_penalty=1.5)


def _model(c, sd, max_batch):
    from seedvc_amd.ar import ARModel
    m = ARModel(c, sd, "cuda:0")
    m.setup_caches(max_batch_size=max_batch)
    return m


def _prefill(m, lengths, slots):
    seqs = [S.rows(n) for n in lengths]
    return m.prefill_batch(list(slots), [x.cuda() for x, _, _ in seqs], [ip for _, ip, _ in seqs], [kv for _, _, kv in seqs]).cpu()


def _decode(m, lengths, slots, n_slots):
    """N_DECODE batched steps on slots 0 .. n_slots - 1; the slots of `lengths` get their sequences' step inputs and
    positions, the others a zero row at position 0: (len(lengths), N_DECODE, vocab), CPU."""
    c, _ = S.model_g()
    ips, kvs = [0] * n_slots, [0] * n_slots
    for n, slot in zip(lengths, slots):
        _, ip, kv = S.rows(n)
        ips[slot], kvs[slot] = int(ip[-1]) + 1, int(kv[-1]) + 1
    out = []
    for t in range(S.N_DECODE):
        x = torch.zeros(n_slots, c["dim"])
        for n, slot in zip(lengths, slots):
            x[slot] = S.step_inputs(n)[t]
        lg = m.decode_step_batch(x.cuda(), ips if t == 0 else None, kvs if t == 0 else None).cpu()
        out.append(lg[list(slots)])
    return torch.stack(out, dim=1)


@pytest.fixture(scope="module")
def one_call():
    """All ten sequences in one ragged call into permuted slots, then two batched decode steps: (prefill logits
    (10, vocab), decode logits (10, N_DECODE, vocab))."""
    c, sd = S.model_g()
    m = _model(c, sd, len(S.LENGTHS))
    pre = _prefill(m, S.LENGTHS, S.SLOTS)
    assert m.prefill_passes() == 1
    return pre, _decode(m, S.LENGTHS, S.SLOTS, len(S.LENGTHS))


# ------------------------------------------------------------------------------------- 3. ragged prefill against the oracle
def test_ragged_prefill_matches_the_oracle(one_call):
    c, sd = S.model_g()
    pre, dec = one_call
    fresh = _model(c, sd, 1)
    for i, n in enumerate(S.LENGTHS):
        ref_pre, ref_dec = S.reference(n)
        scale = max(ref_pre.abs().mean().item(), 1.0)
        err = (pre[i] - ref_pre).abs().max().item()
        x, ip, kv = S.rows(n)
        old = fresh.prefill_slot(0, x.cuda(), ip, kv).cpu().reshape(-1)
        print(f"S = {n:3d} (slot {S.SLOTS[i]}): prefill max err {err:.3e} (bound {LOGIT_TOL * scale:.3e}); "
              f"distance from prefill_slot {(pre[i] - old).abs().max().item():.3e}")
        assert err < LOGIT_TOL * scale, f"S = {n}: {err:.3e}"
        for t in range(S.N_DECODE):
            scale = max(ref_dec[t].abs().mean().item(), 1.0)
            err = (dec[i, t] - ref_dec[t]).abs().max().item()
            print(f"S = {n:3d}: decode step {t} max err {err:.3e} (bound {LOGIT_TOL * scale:.3e})")
            assert err < LOGIT_TOL * scale, f"S = {n}, step {t}: {err:.3e}"


# ----------------------------------------------------------------------------------------------------- 4. independence
@pytest.mark.parametrize("n", [1, 65, 130])
def test_a_sequence_does_not_depend_on_its_company(n, one_call):
    """Alone, with the nine others, in another slot, at another place in the concatenation: the same bits, for the prefill
    logits and for the batched decode steps that follow (which read the cache rows the prefill wrote)."""
    c, sd = S.model_g()
    pre, dec = one_call
    i = S.LENGTHS.index(n)
    m = _model(c, sd, len(S.LENGTHS))
    alone = _prefill(m, [n], [S.SLOTS[i]])
    alone_dec = _decode(m, [n], [S.SLOTS[i]], len(S.LENGTHS))
    assert torch.equal(alone[0], pre[i]), f"alone vs in company: {(alone[0] - pre[i]).abs().max():.3e}"
    assert torch.equal(alone_dec[0], dec[i])
    other = (S.SLOTS[i] + 3) % len(S.LENGTHS)
    moved = _prefill(m, [n], [other])
    assert torch.equal(moved[0], pre[i])
    assert torch.equal(_decode(m, [n], [other], len(S.LENGTHS))[0], dec[i])
    order = list(reversed(S.LENGTHS))                  # another place in the concatenation, other slots for everybody
    slots = [(s + 5) % len(S.LENGTHS) for s in reversed(S.SLOTS)]
    again = _prefill(m, order, slots)
    assert torch.equal(again[order.index(n)], pre[i])
    assert torch.equal(_decode(m, order, slots, len(S.LENGTHS))[order.index(n)], dec[i])


# ----------------------------------------------------------------------------------------------------- 5. pass splitting
def test_passes_of_whole_sequences_give_the_single_pass(one_call):
    c, sd = S.model_g()
    pre, dec = one_call
    m = _model(c, sd, len(S.LENGTHS))
    m.set_prefill_rows(c["max_seq_len"])               # 607 rows, at most 320 per pass
    got = _prefill(m, S.LENGTHS, S.SLOTS)
    print(f"{sum(S.LENGTHS)} rows in {m.prefill_passes()} passes")
    assert m.prefill_passes() >= 3
    assert torch.equal(got, pre)
    assert torch.equal(_decode(m, S.LENGTHS, S.SLOTS, len(S.LENGTHS)), dec)
    with pytest.raises(RuntimeError, match="rows"):
        m.set_prefill_rows(c["max_seq_len"] - 1)


# --------------------------------------------------------------------------------------------- 6. stale and poisoned rows
def test_poisoned_rows_above_the_prefix_do_not_reach_the_result(one_call):
    """NaN arithmetic only: a 257-row sequence whose rows from 40 up are NaN leaves NaN keys and values in cache rows >= 40
    of every layer; a 33-row sequence prefilled into that slot afterwards, with no reset, must not see them."""
    c, sd = S.model_g()
    pre, dec = one_call
    i = S.LENGTHS.index(33)
    m = _model(c, sd, 4)
    x, ip, kv = S.rows(257)
    x = x.clone()
    x[:, 40:] = float("nan")
    assert torch.isnan(m.prefill_slot(2, x.cuda(), ip, kv)).all()
    got = _prefill(m, [33], [2])
    assert torch.isfinite(got).all()
    assert torch.equal(got[0], pre[i])
    got_dec = _decode(m, [33], [2], 4)
    assert torch.isfinite(got_dec).all() and torch.equal(got_dec[0], dec[i])


# ------------------------------------------------------------------------------------------------------------ 7. sessions
def _filler(k):
    """A sequence that is none of the qualified ones (candidate 3's generator with other lengths), plain draws."""
    return A.prompt(3, 2 + (k * 5) % 9, (k * 3) % 7)


def _session_run(m, order, steps_per_run, up_front=5):
    """Submits order[:up_front] before the first step and one more request between steps: with four slots the later ones
    wait, reuse freed slots and are admitted while others are in mid-sequence.  -> {request key: tokens (1, n) CPU}."""
    from seedvc_amd.ar import ARSession
    s = ARSession(m, steps_per_run=steps_per_run)
    tickets, out = {}, {}

    def submit(key):
        kind, k = key
        text, target, noise = A.sequence(k)[:3] if kind == "q" else _filler(k)
        tickets[s.submit(text.cuda(), target.cuda(), exp_noise=noise.cuda(), max_new=A.MAX_NEW, **PARAMS)] = key

    pending = list(order)
    for _ in range(up_front):
        submit(pending.pop(0))
    while pending or s.n_active or s.n_waiting:
        for t, toks in s.step():
            out[tickets[t]] = toks.cpu()
        if pending:
            submit(pending.pop(0))
    assert s.n_active == 0 and s.n_waiting == 0
    return out


def test_session_tokens_match_the_reference_whatever_else_is_in_flight():
    c, sd = A.model()
    m = _model(c, sd, 4)
    order = [x for pair in zip([("q", b) for b in A.ORDER], [("f", k) for k in range(6)]) for x in pair]
    runs = [_session_run(m, order, spr) for spr in (1, 5, 16)] + [_session_run(m, order[::-1], 5)]
    for b in A.ORDER:
        text, target, noise, ref = A.sequence(b)
        alone = m.generate_batch([text.cuda()], [target.cuda()], exp_noise=[noise.cuda()], max_new=A.MAX_NEW, prefill="ragged", **PARAMS)[0].cpu()
        print(f"sequence {b}: {alone.shape[1]} tokens (reference {ref.shape[1]})")
        assert alone.shape == ref.shape and torch.equal(alone, ref), f"sequence {b} alone: {alone.tolist()} vs {ref.tolist()}"
        for r, run in enumerate(runs):
            assert torch.equal(run[("q", b)], ref), f"sequence {b}, run {r}: {run[('q', b)].tolist()} vs {ref.tolist()}"
    for k in range(6):      # the fillers have thin margins: not held to the oracle, but the same in every run
        for run in runs[1:]:
            assert torch.equal(run[("f", k)], runs[0][("f", k)]), f"filler {k}"


# --------------------------------------------------------------------------------------------- 8. per-request parameters
def test_per_request_parameters():
    from seedvc_amd.ar import ARSession
    c, sd = A.model()
    m = _model(c, sd, 4)
    text, target, noise = A.prompt(5)
    kw = [dict(max_new=7, temperature=0.7, top_p=0.7, repetition_penalty=1.5),
          dict(max_new=40, temperature=1.1, top_p=0.95, repetition_penalty=1.2)]
    alone = [m.generate_batch([text.cuda()], [target.cuda()], exp_noise=[noise.cuda()], prefill="ragged", **k)[0].cpu() for k in kw]
    assert alone[0].shape[1] <= 7
    s = ARSession(m, steps_per_run=3)
    f = _filler(1)
    s.submit(f[0].cuda(), f[1].cuda(), exp_noise=f[2].cuda(), max_new=A.MAX_NEW)
    t = [s.submit(text.cuda(), target.cuda(), exp_noise=noise.cuda(), **k) for k in kw]
    got = dict(s.drain())
    for j in range(2):
        assert torch.equal(got[t[j]].cpu(), alone[j]), f"request {j}: {got[t[j]].tolist()} vs {alone[j].tolist()}"
    # the same two in ONE generate_batch call with per-sequence parameters
    both = m.generate_batch([text.cuda()] * 2, [target.cuda()] * 2, exp_noise=[noise.cuda()] * 2, prefill="ragged", max_new=40,
                            temperature=[k["temperature"] for k in kw], top_p=[k["top_p"] for k in kw],
                            repetition_penalty=[k["repetition_penalty"] for k in kw])
    assert torch.equal(both[1].cpu(), alone[1]) and torch.equal(both[0].cpu()[:, :alone[0].shape[1]], alone[0])


# ------------------------------------------------------------------------------------------------------------- 9. seeded
def test_seeded_requests():
    from seedvc_amd.ar import ARSession
    c, sd = A.model()
    m = _model(c, sd, 4)
    seeds = {0: 12345, 2: 2 ** 63 + 17, 5: 7}
    alone = {}
    for b, seed in seeds.items():
        text, target, _ = A.prompt(b)
        alone[b] = m.generate_batch([text.cuda()], [target.cuda()], seeds=[seed], max_new=A.MAX_NEW, prefill="ragged", **PARAMS)[0].cpu()
        fed = m.generate_batch([text.cuda()], [target.cuda()], exp_noise=[m.exp_draws(seed, 0, A.MAX_NEW)], max_new=A.MAX_NEW,
                               prefill="ragged", **PARAMS)[0].cpu()
        assert torch.equal(fed, alone[b]), f"sequence {b}: draws fed back"
    s = ARSession(m, steps_per_run=4)
    tickets, out = {}, []
    for k in range(3):
        f = _filler(k)
        s.submit(f[0].cuda(), f[1].cuda(), exp_noise=f[2].cuda(), max_new=A.MAX_NEW)
    for b, seed in seeds.items():           # one more per step: admitted while the others are in mid-sequence
        text, target, _ = A.prompt(b)
        tickets[s.submit(text.cuda(), target.cuda(), seed=seed, max_new=A.MAX_NEW, **PARAMS)] = b
        out += s.step()
    out += s.drain()
    got = {tickets[t]: toks.cpu() for t, toks in out if t in tickets}
    assert sorted(got) == sorted(seeds)
    for b in seeds:
        assert torch.equal(got[b], alone[b]), f"sequence {b}: {got[b].tolist()} vs {alone[b].tolist()}"


# --------------------------------------------------------------------------------------------- 10. existing paths untouched
def test_existing_paths_after_and_during_a_session(golden):
    from seedvc_amd.ar import ARModel, ARSession
    c, sd, text, target, noise = cases.ar_gen_case("ar_gen_r2")
    ref = torch.from_numpy(golden["ar_gen_r2.codes"])
    max_new = c["max_seq_len"]
    fresh = _model(c, sd, 3)
    want = [t.cpu() for t in fresh.generate_batch([text.cuda()] * 3, [target.cuda()] * 3, exp_noise=[noise.cuda()] * 3, max_new=max_new)]
    m = _model(c, sd, 3)
    s = ARSession(m, steps_per_run=1)          # one step: nobody can be finished yet (EOS is suppressed for ten tokens)
    for _ in range(5):
        s.submit(text.cuda(), target.cuda(), exp_noise=noise.cuda(), max_new=max_new)
    assert s.step() == [] and s.n_active == 3
    # a session is active (slots 0 .. 2 occupied): the closed-batch calls, the B = 1 calls and set_max_batch are refused
    x = torch.zeros(3, c["dim"], device="cuda")
    with pytest.raises(RuntimeError, match="session is active"):
        m.generate_batch([text.cuda()], [target.cuda()], exp_noise=[noise.cuda()], max_new=max_new)
    with pytest.raises(RuntimeError, match="session is active"):
        m.decode_step_batch(x, [1, 1, 1], [1, 1, 1])
    with pytest.raises(RuntimeError, match="session is active"):
        m.setup_caches(max_batch_size=2)
    with pytest.raises(RuntimeError, match="session is active"):
        m.generate(text.cuda(), target.cuda(), exp_noise=noise.cuda())
    with pytest.raises(RuntimeError, match="session is active"):
        m.forward_generate(x[None, :2], torch.arange(2), torch.arange(2))
    with pytest.raises(RuntimeError, match="occupied"):
        m.prefill_slot(1, x[None, :2], torch.arange(2), torch.arange(2))
    with pytest.raises(RuntimeError, match="occupied"):
        m.prefill_batch([1], [x[None, :2]], [torch.arange(2)], [torch.arange(2)])
    got = dict(s.drain())
    assert len(got) == 5 and all(torch.equal(t, got[0]) for t in got.values())     # five times the same request
    # drained: everything as on a fresh handle
    again = [t.cpu() for t in m.generate_batch([text.cuda()] * 3, [target.cuda()] * 3, exp_noise=[noise.cuda()] * 3, max_new=max_new)]
    assert all(torch.equal(a, w) for a, w in zip(again, want))
    codes = m.generate(text.cuda(), target.cuda(), exp_noise=noise.cuda(), **PARAMS).cpu()
    assert codes.shape == ref.shape and torch.equal(codes, ref)


def test_session_argument_errors():
    c, sd = A.model()
    m = _model(c, sd, 4)
    L = c["max_seq_len"]
    x = torch.zeros(1, 3, c["dim"], device="cuda")
    pos = torch.arange(3)
    with pytest.raises(RuntimeError, match="slot outside"):
        m.prefill_batch([4], [x], [pos], [pos])
    with pytest.raises(RuntimeError, match="slot outside"):
        m.prefill_batch([-1], [x], [pos], [pos])
    with pytest.raises(RuntimeError, match="duplicate slot"):
        m.prefill_batch([1, 1], [x, x], [pos, pos], [pos, pos])
    with pytest.raises(RuntimeError, match="position out of range"):
        m.prefill_batch([0, 1], [x, x], [pos, pos], [pos, torch.tensor([0, 1, L])])
    with pytest.raises(RuntimeError, match="position out of range"):
        m.prefill_batch([0], [x], [torch.tensor([0, -1, 2])], [pos])
    with pytest.raises(RuntimeError, match="n outside"):
        m.prefill_batch([], [], [], [])
    with pytest.raises(RuntimeError, match="max_batch"):
        m.prefill_batch([0, 1, 2, 3, 0], [x] * 5, [pos] * 5, [pos] * 5)
    text, target, noise = A.sequence(0)[:3]
    reqs = [m.session_request(text.cuda(), target.cuda(), None, noise.cuda(), A.MAX_NEW, 0.7, 0.7, 1.5) for _ in range(5)]
    with pytest.raises(RuntimeError, match="max_batch"):
        m.session_admit(list(enumerate(reqs)))
    with pytest.raises(RuntimeError, match="slot outside"):
        m.session_admit([(4, reqs[0])])
    with pytest.raises(RuntimeError, match="duplicate slot"):
        m.session_admit([(2, reqs[0]), (2, reqs[1])])
    with pytest.raises(RuntimeError, match="no session is active"):
        m.session_run(1)
    m.session_admit([(1, reqs[0])])
    with pytest.raises(RuntimeError, match="occupied"):
        m.session_admit([(1, reqs[1])])
    n, done = m.session_run(A.MAX_NEW)
    assert done[1] and torch.equal(m.session_retire(1, n[1]).cpu(), A.sequence(0)[3])
    # the handle still works after the refusals
    seqs = [A.sequence(b) for b in A.ORDER[:4]]
    got = m.generate_batch([q[0].cuda() for q in seqs], [q[1].cuda() for q in seqs], exp_noise=[q[2].cuda() for q in seqs], max_new=A.MAX_NEW,
                           **PARAMS)
    assert all(torch.equal(g.cpu(), q[3]) for g, q in zip(got, seqs))


# ----------------------------------------------------------------------------------------------------------- 11. full size
def test_session_full_size(golden):
    """ar_base, 40 slots: ar_gen_full (boosted draws) submitted three times among 37 truncated companions with plain draws,
    half of the companions only after the first step; the three give the committed 160 tokens."""
    from seedvc_amd.ar import ARSession
    ref = torch.from_numpy(golden["ar_gen_full.codes"])
    c, sd, text, target, boosted = cases.ar_gen_full_case(winners=ref)
    plain = cases.ar_gen_full_case()[4]
    held = (0, 17, 39)
    m = _model(c, sd, 40)
    s = ARSession(m, steps_per_run=16)
    text_d, boosted_d, plain_d = text.cuda(), boosted.cuda(), plain.cuda()
    tickets = {}

    def submit(b):
        t = s.submit(text_d, (target if b in held else target[:, :200 - b]).cuda(), exp_noise=boosted_d if b in held else plain_d,
                     max_new=cases.AR_GEN_FULL_TOKENS, **PARAMS)
        if b in held:
            tickets[t] = b

    late = [b for b in range(40) if b not in held][::2]
    for b in range(40):
        if b not in late:
            submit(b)
    out = s.step()
    print(f"first admission of {40 - len(late)} prompts: {m.prefill_passes()} prefill passes")
    for b in late:
        submit(b)
    out += s.drain()
    got = {tickets[t]: toks.cpu() for t, toks in out if t in tickets}
    assert len(out) == 40 and sorted(got) == list(held)
    for b in held:
        codes = got[b]
        n_same = int((codes[0, :ref.shape[1]] == ref[0, :codes.shape[1]]).long().cumprod(0).sum())
        print(f"ar_gen_full submitted as request {b}: {codes.shape[1]} tokens, first {n_same} identical")
        assert codes.shape == ref.shape and torch.equal(codes, ref)
