"""GPU tests of the batched AR path (`svc_ar_set_max_batch`, `svc_ar_prefill_slot`, `svc_ar_decode_step_batch`,
`svc_ar_generate_batch`): teacher-forced logits per slot against the oracle, ragged batches token for token against the
reference, and the invariances a caller relies on -- a sequence's result depends neither on B, nor on its slot, nor on
what the other slots hold or held before.  The batched kernels have one form for every B (the number of 16-row M tiles
is the only thing that changes at B = 17, 33 and 49), so the invariance tests run at B = 6 (one tile) and B = 40 (three)."""
import pytest
import torch

import ar_batch_cases as A
import cases
import seedvc_oracle as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
LOGIT_TOL = A.LOGIT_TOL
SPREAD_40 = (0, 9, 17, 26, 33, 39)     # slots of the six qualified sequences in a B = 40 batch: all three M tiles


def _model(c, sd, max_batch):
    from seedvc_amd.ar import ARModel
    m = ARModel(c, sd, "cuda:0")
    m.setup_caches(max_batch_size=max_batch)
    return m


def _generate(m, seqs, check_every=16, max_new=A.MAX_NEW):
    """seqs: list of (text, target, noise, ...) -> list of (1, n) CPU token tensors."""
    out = m.generate_batch([s[0].cuda() for s in seqs], [s[1].cuda() for s in seqs], exp_noise=[s[2].cuda() for s in seqs],
                           top_p=0.7, temperature=0.7, repetition_penalty=1.5, max_new=max_new, check_every=check_every)
    return [t.cpu() for t in out]


def _prompt_rows(sd, text, target):
    """The prefill of NaiveWrapper.generate (ar.py:390-396): rows (1, S, dim), input_pos, kv_pos."""
    sep = sd["sep_token_emb"].reshape(1, 1, -1)
    tgt = sd["model.embeddings.weight"][target[0]][None]
    x = torch.cat([sep, text, sep, tgt], dim=1)
    ip = torch.cat([torch.arange(text.size(1) + 1), torch.tensor([0]), torch.arange(tgt.size(1)) + 1])
    return x, ip, torch.arange(x.size(1))


def _step_logits(m, sd, seqs, n_steps=4):
    """Prefill every slot with its sequence's prompt, then n_steps batched one-token steps fed with the embeddings of the
    sequences' own reference tokens: logits (B, n_steps, vocab), CPU."""
    emb = sd["model.embeddings.weight"]
    ips, kvs = [], []
    for slot, s in enumerate(seqs):
        x, ip, kv = _prompt_rows(sd, s[0], s[1])
        m.prefill_slot(slot, x.cuda(), ip, kv)
        ips.append(int(ip[-1]) + 1)
        kvs.append(int(kv[-1]) + 1)
    out = []
    for t in range(n_steps):
        x = torch.stack([emb[int(s[3][0, min(t, s[3].shape[1] - 1)])] for s in seqs])
        out.append(m.decode_step_batch(x.cuda(), ips if t == 0 else None, kvs if t == 0 else None).cpu())
    return torch.stack(out, dim=1)


def _filler(b, tag):
    """A sequence that is none of the qualified ones (candidate 3's generator with other lengths); its own oracle tokens
    feed `_step_logits`, nothing is compared with them."""
    _, sd = A.model()
    text, target, noise = A.prompt(3, 2 + (b * 5 + tag) % 9, (b * 3 + tag) % 7)
    return text, target, noise, torch.zeros(1, 1, dtype=torch.long) + (b + tag) % 32


# ------------------------------------------------------------------------------------------------ 3. teacher-forced logits
@pytest.mark.parametrize("name", list(cases.AR_CASES))
def test_batched_step_logits_match_the_oracle(name, golden):
    """Three slots hold the case's prefill with its last 0, 2 and 5 rows dropped (three different kv_pos), then the case's
    decode inputs go through `decode_step_batch`; every slot, every step against the oracle on the slot's own cache, and
    the untruncated slot against the committed reference logits as well."""
    c, sd, x_prefill, input_pos, x_steps, _, meta = cases.ar_case(name)
    drops = (0, 2, 5)
    m = _model(c, sd, len(drops))
    ip_all, kv_all = torch.tensor(input_pos), torch.arange(meta["n_prefill"])
    gold = torch.from_numpy(golden[name + ".logits"])
    caches, ips, kvs = [], [], []
    worst = 0.0
    for slot, d in enumerate(drops):
        n = meta["n_prefill"] - d
        caches.append(O.ar_new_cache(c))
        ref = O.ar_forward_generate(sd, c, x_prefill[:, :n], ip_all[:n], kv_all[:n], caches[slot])
        lg = m.prefill_slot(slot, x_prefill[:, :n].cuda(), ip_all[:n], kv_all[:n]).cpu()
        scale = max(ref.abs().mean().item(), 1.0)
        err = (lg - ref).abs().max().item()
        print(f"{name}: slot {slot} prefill ({n} rows) max err {err:.3e} (bound {LOGIT_TOL * scale:.3e})")
        assert err < LOGIT_TOL * scale
        ips.append(ip_all[n - 1:n] + 1)
        kvs.append(kv_all[n - 1:n] + 1)
    for s in range(meta["n_decode"]):
        x = x_steps[s].reshape(1, -1).repeat(len(drops), 1)
        lg = m.decode_step_batch(x.cuda(), [int(p) for p in ips] if s == 0 else None, [int(p) for p in kvs] if s == 0 else None).cpu()
        for slot in range(len(drops)):
            ref = O.ar_forward_generate(sd, c, x_steps[s], ips[slot], kvs[slot], caches[slot])[0, 0]
            scale = max(ref.abs().mean().item(), 1.0)
            err = (lg[slot] - ref).abs().max().item()
            worst = max(worst, err / scale)
            print(f"{name}: step {s} slot {slot} max err {err:.3e} (bound {LOGIT_TOL * scale:.3e})")
            assert err < LOGIT_TOL * scale, f"step {s} slot {slot}: {err:.3e}"
            ips[slot], kvs[slot] = ips[slot] + 1, kvs[slot] + 1
        gscale = max(gold.abs().mean().item(), 1.0)
        gerr = (lg[0] - gold[s + 1, 0]).abs().max().item()
        assert gerr < LOGIT_TOL * gscale, f"step {s} vs committed logits: {gerr:.3e}"
    print(f"{name}: worst batched-step logit error {worst:.2e} x mean |logit|")


# ------------------------------------------------------------------------------------- 4. ragged batch vs the reference
@pytest.mark.parametrize("check_every", [1, 16])
def test_generate_batch_matches_reference(check_every):
    """Six sequences with ragged prompts (four end by EOS at three different steps, two at the cap) in one call."""
    c, sd = A.model()
    seqs = [A.sequence(b) for b in A.ORDER]
    m = _model(c, sd, len(seqs))
    got = _generate(m, seqs, check_every)
    for b, g, s in zip(A.ORDER, got, seqs):
        print(f"sequence {b}: {g.shape[1]} tokens (reference {s[3].shape[1]})")
        assert g.shape == s[3].shape and torch.equal(g, s[3]), f"sequence {b}: {g.tolist()} vs {s[3].tolist()}"


def _spread_batch():
    seqs = [A.sequence(A.ORDER[j % len(A.ORDER)]) for j in range(40)]
    for slot, b in zip(SPREAD_40, A.ORDER):
        seqs[slot] = A.sequence(b)
    return seqs


def test_generate_batch_of_40_matches_reference():
    """The same six spread over a B = 40 batch (three M tiles) whose other slots repeat them."""
    c, sd = A.model()
    seqs = _spread_batch()
    m = _model(c, sd, 40)
    got = _generate(m, seqs)
    for slot, (g, s) in enumerate(zip(got, seqs)):
        assert g.shape == s[3].shape and torch.equal(g, s[3]), f"slot {slot}: {g.tolist()} vs {s[3].tolist()}"


# --------------------------------------------------------------------------------------------------- 5. batch invariance
@pytest.mark.parametrize("B", [6, 40])
def test_permuting_slots_permutes_results(B):
    c, sd = A.model()
    seqs = [A.sequence(A.ORDER[j % len(A.ORDER)]) for j in range(B)]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B)).tolist()
    m = _model(c, sd, B)
    toks = _generate(m, seqs)
    logits = _step_logits(m, sd, seqs)
    toks_p = _generate(m, [seqs[j] for j in perm])
    logits_p = _step_logits(m, sd, [seqs[j] for j in perm])
    for i, j in enumerate(perm):
        assert torch.equal(toks_p[i], toks[j]), f"slot {i} <- {j}"
        assert torch.equal(logits_p[i], logits[j]), f"slot {i} <- {j}: step logits differ by {(logits_p[i] - logits[j]).abs().max():.3e}"


@pytest.mark.parametrize("B", [6, 40])
def test_result_does_not_depend_on_other_slots(B):
    """Same B, same slot for the sequence under test, every other slot replaced by a different sequence: bit-identical."""
    c, sd = A.model()
    m = _model(c, sd, B)
    for k, b in enumerate(A.ORDER):
        slot = SPREAD_40[k] if B == 40 else k
        runs = []
        for tag in (0, 1):
            seqs = [_filler(j, tag) for j in range(B)]
            seqs[slot] = A.sequence(b)
            runs.append((_generate(m, seqs)[slot], _step_logits(m, sd, seqs)[slot]))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][0], A.sequence(b)[3]), f"sequence {b}"
        assert torch.equal(runs[0][1], runs[1][1]), f"sequence {b}: step logits differ by {(runs[0][1] - runs[1][1]).abs().max():.3e}"


@pytest.mark.parametrize("name", list(cases.AR_GEN_CASES))
def test_thin_margin_cases_do_not_depend_on_other_slots(name):
    """ar_gen_r / ar_gen_r2 have near-ties the fp16 logits may flip, so they are not held to their reference here; what
    they must be is the same whatever the other slots hold, and the same as alone."""
    c, sd, text, target, noise = cases.ar_gen_case(name)
    m = _model(c, sd, 5)
    max_new = c["max_seq_len"]
    alone = m.generate_batch([text.cuda()], [target.cuda()], exp_noise=[noise.cuda()], max_new=max_new)[0].cpu()
    runs = []
    for tag in (0, 1):
        texts, targets, noises = [], [], []
        for j in range(5):
            tt, tp = 2 + (3 * j + 4 * tag) % 8, (2 * j + tag) % 5
            texts.append(cases.randn(f"{name}.fill{tag}.{j}.text", 7, 1, tt, c["dim"]))
            targets.append((cases.rand(f"{name}.fill{tag}.{j}.tgt", 7, 1, tp) * (c["vocab_size"] - 1)).long())
            noises.append(-torch.log(cases.rand(f"{name}.fill{tag}.{j}.expn", 7, max_new, c["vocab_size"]).clamp_min(1e-9)))
        texts[2], targets[2], noises[2] = text, target, noise
        out = m.generate_batch([t.cuda() for t in texts], [t.cuda() for t in targets], exp_noise=[q.cuda() for q in noises], max_new=max_new)
        runs.append(out[2].cpu())
    print(f"{name}: {alone.shape[1]} tokens")
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], alone)


def test_alone_equals_in_batch():
    """Each qualified sequence through `generate_batch` with B = 1 gives the tokens it gives inside B = 6 and B = 40."""
    c, sd = A.model()
    m = _model(c, sd, 40)
    in6 = _generate(m, [A.sequence(b) for b in A.ORDER])
    in40 = _generate(m, _spread_batch())
    for k, b in enumerate(A.ORDER):
        alone = _generate(m, [A.sequence(b)])[0]
        assert torch.equal(alone, in6[k]) and torch.equal(alone, in40[SPREAD_40[k]]) and torch.equal(alone, A.sequence(b)[3]), f"sequence {b}"


# ------------------------------------------------------------------------------------------------------------ 6. full size
def test_generate_batch_full_size(golden):
    """ar_base, B = 40: slots 0, 17 and 39 hold ar_gen_full (boosted draws) and must give the committed 160 tokens; the
    other slots hold the same prompt with a shorter target and plain draws (near-ties: not compared), once truncated to
    200 - b and once to 100 - b tokens, and must not change what slots 0, 17 and 39 give."""
    ref = torch.from_numpy(golden["ar_gen_full.codes"])
    c, sd, text, target, boosted = cases.ar_gen_full_case(winners=ref)
    plain = cases.ar_gen_full_case()[4]
    held = (0, 17, 39)
    m = _model(c, sd, 40)
    for keep in (200, 100):
        texts = [text.cuda()] * 40
        targets = [(target if b in held else target[:, :keep - b]).cuda() for b in range(40)]
        noises = [(boosted if b in held else plain).cuda() for b in range(40)]
        out = m.generate_batch(texts, targets, exp_noise=noises, top_p=0.7, temperature=0.7, repetition_penalty=1.5,
                               max_new=cases.AR_GEN_FULL_TOKENS, check_every=16)
        for b in held:
            codes = out[b].cpu()
            n_same = int((codes[0, :ref.shape[1]] == ref[0, :codes.shape[1]]).long().cumprod(0).sum())
            print(f"ar_gen_full in slot {b} (others truncated to {keep} - b): {codes.shape[1]} tokens, first {n_same} identical")
            assert codes.shape == ref.shape and torch.equal(codes, ref)


# ------------------------------------------------------------------------------------------------------- 7. stale cache rows
def test_stale_cache_rows_do_not_reach_a_shorter_sequence():
    """Slot 1 generates the 40-token sequence 2 and then, with no reset in between, the 13-token sequence 1: the rows the
    longer run left above the shorter one's kv_pos must not matter."""
    c, sd = A.model()
    m = _model(c, sd, 3)
    first = _generate(m, [A.sequence(0), A.sequence(2), A.sequence(4)])
    second = _generate(m, [A.sequence(0), A.sequence(1), A.sequence(4)])
    fresh = _generate(_model(c, sd, 3), [A.sequence(0), A.sequence(1), A.sequence(4)])
    assert torch.equal(first[1], A.sequence(2)[3])
    assert torch.equal(second[1], fresh[1]) and torch.equal(second[1], A.sequence(1)[3])
    for k in (0, 2):
        assert torch.equal(second[k], first[k]) and torch.equal(second[k], fresh[k])


# ------------------------------------------------------------------------------------------------------- 8. B = 1 untouched
def test_b1_generate_after_set_max_batch(golden):
    """Slot 0 is the cache of the B = 1 calls: `generate` on a handle with eight slots still gives the reference tokens."""
    c, sd, text, target, noise = cases.ar_gen_case("ar_gen_r2")
    m = _model(c, sd, 8)
    ref = torch.from_numpy(golden["ar_gen_r2.codes"])
    codes = m.generate(text.cuda(), target.cuda(), top_p=0.7, temperature=0.7, repetition_penalty=1.5, exp_noise=noise.cuda()).cpu()
    assert codes.shape == ref.shape and torch.equal(codes, ref)
    m.generate_batch([text.cuda()] * 8, [target.cuda()] * 8, exp_noise=[noise.cuda()] * 8, max_new=c["max_seq_len"])
    codes = m.generate(text.cuda(), target.cuda(), top_p=0.7, temperature=0.7, repetition_penalty=1.5, exp_noise=noise.cuda()).cpu()
    assert torch.equal(codes, ref)


# ------------------------------------------------------------------------------------------------------- 9. argument errors
def test_batch_argument_errors():
    c, sd = A.model()
    from seedvc_amd.ar import ARModel
    m = ARModel(c, sd, "cuda:0")
    x = torch.zeros(5, c["dim"], device="cuda")
    with pytest.raises(RuntimeError, match="max_batch"):
        m.setup_caches(max_batch_size=65)
    with pytest.raises(RuntimeError, match="max_batch"):       # one slot until setup_caches asks for more
        m.decode_step_batch(x[:2], [1, 1], [1, 1])
    m.setup_caches(max_batch_size=4)
    with pytest.raises(RuntimeError, match="max_batch"):
        m.decode_step_batch(x, [1] * 5, [1] * 5)
    with pytest.raises(RuntimeError, match="max_batch"):
        m.decode_step_batch(x[:0], [], [])
    with pytest.raises(RuntimeError, match="position out of range"):
        m.decode_step_batch(x[:2], [1, c["max_seq_len"]], [1, 1])
    with pytest.raises(RuntimeError, match="position out of range"):
        m.decode_step_batch(x[:2], [1, 1], [c["max_seq_len"], 1])
    with pytest.raises(RuntimeError, match="set_pos"):
        m.decode_step_batch(x[:2])
    with pytest.raises(RuntimeError, match="max_batch"):
        m.prefill_slot(4, x[None, :3], torch.arange(3), torch.arange(3))
    with pytest.raises(RuntimeError, match="position out of range"):
        m.prefill_slot(1, x[None, :3], torch.arange(3), torch.tensor([0, 1, c["max_seq_len"]]))
    seqs = [A.sequence(b) for b in A.ORDER[:5]]
    with pytest.raises(RuntimeError, match="max_batch"):
        _generate(m, seqs)
    # the handle still works after the refusals
    got = _generate(m, seqs[:4])
    assert all(torch.equal(g, s[3]) for g, s in zip(got, seqs))
