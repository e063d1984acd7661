"""Inputs shared by the continuous-batching tests (test_host_ar_session.py, test_gpu_ar_session.py).

Model G is small and GQA (6 query heads on 2 KV heads), so one workgroup of the ragged prefill attention really shares
its K / V tiles among three heads.  Its sequences are plain `cases.randn` rows of the lengths at which a 16- or 32-row
tiling changes shape (1, 9, 15, 16, 17, 33, 64, 65) plus two that need a multi-tile key loop (130, 257); the positions are
laid out like a prompt: input_pos restarts after the second separator, kv_pos counts on.  The oracle references (prefill
logits, then two decode steps on the same cache) are computed once per length and shared.

`FakeBackend` is what `ARSession` needs from an ARModel, with sequences that end after scripted token counts."""
import functools

import torch

import cases
import seedvc_oracle as O
from seedvc_amd import specs, weights

SEED_G = 191
CFG_G = dict(dim=384, n_head=6, n_local_heads=2, n_layer=2, intermediate_size=256, vocab_size=33, max_seq_len=320)
LENGTHS = (1, 9, 15, 16, 17, 33, 64, 65, 130, 257)
SLOTS = (7, 2, 9, 0, 4, 1, 8, 3, 6, 5)      # slot of each sequence in the one-call tests: a permutation
N_DECODE = 2


@functools.lru_cache(maxsize=None)
def model_g():
    c = specs.ar_config(**CFG_G)
    sd = weights.make_state_dict(specs.ar_state_spec(c), seed=SEED_G, prefix="ar.")
    return c, sd


def rows(S):
    """(x (1, S, dim), input_pos (S,), kv_pos (S,)) of the sequence of S rows."""
    c, _ = model_g()
    x = cases.randn(f"ars.{S}.rows", SEED_G + S, 1, S, c["dim"])
    nt = S // 2
    ip = torch.tensor(list(range(nt + 1)) + list(range(S - nt - 1)))
    return x, ip, torch.arange(S)


def step_inputs(S):
    """(N_DECODE, dim): the inputs of the decode steps that follow the prefill of the sequence of S rows."""
    c, _ = model_g()
    return cases.randn(f"ars.{S}.steps", SEED_G + S, N_DECODE, c["dim"])


@functools.lru_cache(maxsize=None)
def reference(S):
    """Oracle: (prefill logits (vocab,), decode logits (N_DECODE, vocab)) of the sequence of S rows on its own cache."""
    c, sd = model_g()
    x, ip, kv = rows(S)
    cache = O.ar_new_cache(c)
    pre = O.ar_forward_generate(sd, c, x, ip, kv, cache)[0, 0]
    xs = step_inputs(S)
    dec = []
    for t in range(N_DECODE):
        dec.append(O.ar_forward_generate(sd, c, xs[t].reshape(1, 1, -1), ip[-1:] + 1 + t, kv[-1:] + 1 + t, cache)[0, 0])
    return pre, torch.stack(dec)


class FakeBackend:
    """The backend interface of ARSession without a device.  A request is scripted by its `max_new`: the sequence is done
    once it holds that many tokens (one from the admission, one per step after it)."""

    def __init__(self, n_slots, max_seq_len=100):
        self.max_batch_size, self.max_seq_len = n_slots, max_seq_len
        self.slots = {}            # slot -> [request, tokens so far]
        self.admit_calls = []      # one list of (slot, request name) per admit call
        self.steps = 0

    def session_request(self, prompt_text, prompt_target, seed, exp_noise, max_new, top_p, temperature, repetition_penalty):
        S = len(prompt_text) + 2 + len(prompt_target)
        if S > self.max_seq_len:
            raise ValueError("prompt does not fit the cache")
        return dict(name=prompt_text, max_new=min(max_new, self.max_seq_len - S + 1), seed=seed, exp_noise=exp_noise)

    def session_admit(self, entries):
        assert entries
        for slot, r in entries:
            assert slot not in self.slots and 0 <= slot < self.max_batch_size
            self.slots[slot] = [r, 1]
        self.admit_calls.append([(slot, r["name"]) for slot, r in entries])

    def session_run(self, n_steps):
        assert self.slots
        self.steps += n_steps
        n, done = [0] * self.max_batch_size, [True] * self.max_batch_size
        for slot, st in self.slots.items():
            st[1] = min(st[0]["max_new"], st[1] + n_steps)
            n[slot], done[slot] = st[1], st[1] >= st[0]["max_new"]
        return n, done

    def session_retire(self, slot, n_tokens):
        r, n = self.slots.pop(slot)
        assert n == n_tokens
        return (r["name"], n_tokens)
