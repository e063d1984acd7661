"""Host-side mirror of the v2 AR model's generation step over the C ABI (modules/v2/ar.py).

`ARModel.forward_generate(x, input_pos, kv_pos)` mirrors `NaiveTransformer.forward_generate` (B = 1) and returns the
last token's logits; `decode_step` is the hipGraph-captured one-token step (the reference's `compiled_decode_fn`);
`sample(...)` mirrors `sample()/logits_to_probs()` with the Exp(1) noise drawn here unless supplied.
`setup_caches(max_batch_size=B)` gives the handle B slots (one KV cache each); `generate_batch`, `prefill_slot` and
`decode_step_batch` run up to 64 sequences per decode step on them.  Without `exp_noise`, `generate` / `generate_batch`
draw inside the sampler kernel from one 64-bit seed per sequence (`seed=` / `seeds=`, or fresh ones from torch's CPU
generator): no noise tensor is allocated; `exp_draws` returns the draws a seed stands for.

Continuous batching: `prefill_batch` prefills n sequences into n slots in one ragged pass; `generate_batch(...,
prefill="ragged")` admits all B sequences with it and runs them on the session entry points (`svc_ar_admit / _run /
_retire`); `ARSession` keeps the batch open -- requests are submitted at any time, enter free slots while others are in
mid-sequence and leave when they finish.  A request's tokens do not depend on what else is in flight.
"""
import collections
import ctypes as C

import torch

from . import _lib


class ARModel:
    def __init__(self, cfg, state_dict, device="cuda:0"):
        self.cfg = cfg
        self.device = torch.device(device)
        c = _lib.ArConfig()
        for k in ("dim", "n_head", "n_local_heads", "head_dim", "n_layer", "intermediate_size", "vocab_size", "max_seq_len"):
            setattr(c, k, int(cfg[k]))
        c.rope_base, c.norm_eps = float(cfg["rope_base"]), float(cfg["norm_eps"])
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            descs, n, keep = _lib.make_descs(state_dict, self.device)
            _lib.check(_lib.lib().svc_ar_create(C.byref(c), descs, n, _lib.stream_ptr(), C.byref(self._h)))
            torch.cuda.current_stream().synchronize()
        del keep
        # host-side pieces of NaiveWrapper.generate's prompt assembly (ar.py:390-396)
        self._sep = state_dict["sep_token_emb"].detach().to(self.device, torch.float32) if "sep_token_emb" in state_dict else None
        self._emb = (state_dict["model.embeddings.weight"].detach().to(self.device, torch.float32)
                     if "model.embeddings.weight" in state_dict else None)
        self.max_batch_size = 1
        self._admitted = {}            # slot -> the admitted request (keeps its device tensors alive until it is retired)

    def setup_caches(self, max_batch_size=1, max_seq_len=None, dtype=None, device=None):
        """vc_wrapper.py:328-329.  The caches live in the handle: max_batch_size > 1 allocates one per slot
        (`svc_ar_set_max_batch`; the default leaves the slots as they are); resets slot 0, the cache of the B = 1 calls."""
        with torch.cuda.device(self.device):
            if max_batch_size > 1:
                _lib.check(_lib.lib().svc_ar_set_max_batch(self._h, int(max_batch_size), _lib.stream_ptr()))
                self.max_batch_size = int(max_batch_size)
            _lib.check(_lib.lib().svc_ar_reset(self._h, _lib.stream_ptr()))

    @torch.inference_mode()
    def forward_generate(self, x, input_pos, kv_pos):
        """x (1, S, dim) -> logits (1, 1, vocab) of the last token."""
        S = x.shape[1]
        with torch.cuda.device(self.device):
            xx = _lib.f32c(x, self.device).reshape(S, -1)
            out = torch.empty(self.cfg["vocab_size"], device=self.device)
            ip, kp = _lib.i64_host(input_pos.tolist()), _lib.i64_host(kv_pos.tolist())
            _lib.check(_lib.lib().svc_ar_forward_generate(self._h, _lib.ptr(xx), S, ip, kp, _lib.ptr(out), _lib.stream_ptr()))
        return out.reshape(1, 1, -1)

    @torch.inference_mode()
    def decode_step(self, x, input_pos=None, kv_pos=None):
        """One-token step from the captured hipGraph; pass positions on the first step only (then they auto-advance)."""
        with torch.cuda.device(self.device):
            xx = _lib.f32c(x, self.device).reshape(-1)
            out = torch.empty(self.cfg["vocab_size"], device=self.device)
            set_pos = int(input_pos is not None)
            _lib.check(_lib.lib().svc_ar_decode_step(self._h, _lib.ptr(xx), set_pos, C.c_int64(int(input_pos or 0)),
                                                     C.c_int64(int(kv_pos or 0)), _lib.ptr(out), _lib.stream_ptr()))
        return out.reshape(1, 1, -1)

    @torch.inference_mode()
    def sample(self, logits, previous_tokens=None, suppress_tokens=None, temperature=0.7, top_p=0.7, repetition_penalty=1.5,
               exp_noise=None, return_probs=False):
        V = self.cfg["vocab_size"]
        if suppress_tokens is not None and len(suppress_tokens) > 1:
            raise ValueError(f"ARModel.sample suppresses one token, not {len(suppress_tokens)}: the sampler kernel takes a single index")
        with torch.cuda.device(self.device):
            lg = _lib.f32c(logits, self.device).reshape(-1)[-V:].contiguous()
            if exp_noise is None:
                exp_noise = torch.empty(V, device=self.device).exponential_(1)      # ar.py:726
            q = _lib.f32c(exp_noise, self.device)
            prev = previous_tokens.to(self.device, torch.int32).contiguous() if previous_tokens is not None else None
            sup = int(suppress_tokens[0]) if suppress_tokens else -1
            idx = torch.empty(1, device=self.device, dtype=torch.int32)
            probs = torch.empty(V, device=self.device) if return_probs else None
            _lib.check(_lib.lib().svc_ar_sample(self._h, _lib.ptr(lg), _lib.ptr(prev), 0 if prev is None else prev.numel(), sup,
                                                C.c_float(temperature), C.c_float(top_p), C.c_float(repetition_penalty),
                                                _lib.ptr(q), _lib.ptr(idx), _lib.ptr(probs), _lib.stream_ptr()))
        return (idx, probs) if return_probs else idx

    @torch.inference_mode()
    def generate(self, prompt_text, prompt_target, compiled_decode_fn=None, top_p=0.7, temperature=0.7,
                 repetition_penalty=1.5, exp_noise=None, max_new=4001, check_every=16, seed=None):
        """`NaiveWrapper.generate` (modules/v2/ar.py:382-422): prompt_text (1, Tt, dim) condition embeddings,
        prompt_target (1, Tp) tokens -> (1, n) generated tokens.  The token loop runs on the device
        (`svc_ar_generate`); exp_noise (max_new, vocab) pins the Exp(1) draws.  Without it the draws come from `seed`
        (a fresh one from torch's CPU generator when None) inside the sampler: `generate_batch` with one sequence.
        compiled_decode_fn is accepted and ignored: the captured hipGraph step is always used."""
        if exp_noise is None:
            return self.generate_batch([prompt_text], [prompt_target], seeds=None if seed is None else [seed], top_p=top_p,
                                       temperature=temperature, repetition_penalty=repetition_penalty, max_new=max_new,
                                       check_every=check_every)[0]
        assert seed is None, "give exp_noise or seed, not both"
        V, D = self.cfg["vocab_size"], self.cfg["dim"]
        with torch.cuda.device(self.device):
            text = _lib.f32c(prompt_text, self.device)
            sep = self._sep.reshape(1, 1, D)
            tgt = prompt_target.to(self.device).long()
            tgt_emb = self._emb[tgt[0]][None] if tgt.numel() else torch.zeros(1, 0, D, device=self.device)
            emb_seq = torch.cat([sep, text, sep, tgt_emb], dim=1)[0].contiguous()
            S = emb_seq.shape[0]
            input_pos = list(range(text.size(1) + 1)) + [0] + [i + 1 for i in range(tgt_emb.size(1))]
            kv_pos = list(range(S))
            max_new = min(int(max_new), self.cfg["max_seq_len"] - S + 1)
            q = _lib.f32c(exp_noise, self.device)
            assert q.shape[0] >= max_new and q.shape[1] == V
            toks = torch.zeros(max_new, device=self.device, dtype=torch.int32)
            n = C.c_int32(0)
            self.setup_caches()
            _lib.check(_lib.lib().svc_ar_generate(self._h, _lib.ptr(emb_seq), S, _lib.i64_host(input_pos), _lib.i64_host(kv_pos),
                                                  _lib.ptr(q), max_new, 10, C.c_float(temperature), C.c_float(top_p),
                                                  C.c_float(repetition_penalty), int(check_every), _lib.ptr(toks), C.byref(n),
                                                  _lib.stream_ptr()))
        return toks[:n.value].long()[None, :]

    @torch.inference_mode()
    def prefill_slot(self, slot, x, input_pos, kv_pos):
        """`forward_generate` on the cache of one slot (0 <= slot < max_batch_size): x (1, S, dim) -> logits (1, 1, vocab)."""
        S = x.shape[1]
        with torch.cuda.device(self.device):
            xx = _lib.f32c(x, self.device).reshape(S, -1)
            out = torch.empty(self.cfg["vocab_size"], device=self.device)
            ip, kp = _lib.i64_host(input_pos.tolist()), _lib.i64_host(kv_pos.tolist())
            _lib.check(_lib.lib().svc_ar_prefill_slot(self._h, int(slot), _lib.ptr(xx), S, ip, kp, _lib.ptr(out), _lib.stream_ptr()))
        return out.reshape(1, 1, -1)

    @torch.inference_mode()
    def prefill_batch(self, slots, xs, input_pos, kv_pos):
        """`prefill_slot` for n sequences in one ragged pass (`svc_ar_prefill_batch`): slots n distinct free slots, xs a list
        of n (1, S_i, dim) tensors, input_pos / kv_pos lists of n position sequences -> logits (n, vocab)."""
        n = len(slots)
        if not (n == len(xs) == len(input_pos) == len(kv_pos)):
            raise ValueError("prefill_batch: slots, xs, input_pos and kv_pos must have one entry per sequence")
        with torch.cuda.device(self.device):
            rows = [_lib.f32c(x, self.device).reshape(-1, self.cfg["dim"]) for x in xs]
            S = [r.shape[0] for r in rows]
            xx = torch.cat(rows, dim=0).contiguous() if n else torch.empty(1, self.cfg["dim"], device=self.device)
            ip = [int(v) for p in input_pos for v in torch.as_tensor(p).reshape(-1).tolist()]
            kp = [int(v) for p in kv_pos for v in torch.as_tensor(p).reshape(-1).tolist()]
            if len(ip) != sum(S) or len(kp) != sum(S):
                raise ValueError("prefill_batch: one input_pos and one kv_pos per row")
            out = torch.empty(max(n, 1), self.cfg["vocab_size"], device=self.device)
            _lib.check(_lib.lib().svc_ar_prefill_batch(self._h, n, (C.c_int32 * max(n, 1))(*[int(v) for v in slots]), _lib.ptr(xx),
                                                       (C.c_int32 * max(n, 1))(*S), _lib.i64_host(ip + [0] * (not ip)),
                                                       _lib.i64_host(kp + [0] * (not kp)), _lib.ptr(out), _lib.stream_ptr()))
        return out[:n]

    def set_prefill_rows(self, rows):
        """Rows of one ragged-prefill pass (max_seq_len .. 8192, the default); a call with more rows runs as several passes."""
        _lib.check(_lib.lib().svc_ar_set_prefill_rows(self._h, int(rows)))

    def prefill_passes(self):
        """Passes the last ragged prefill ran as."""
        return int(_lib.lib().svc_ar_prefill_passes(self._h))

    @torch.inference_mode()
    def decode_step_batch(self, x, input_pos=None, kv_pos=None):
        """One token for each of slots 0 .. B-1 from the captured batched step: x (B, dim) -> logits (B, vocab).  Pass the
        B input_pos / kv_pos on the first step of a batch only (then they auto-advance)."""
        xx = _lib.f32c(x, self.device)
        xx = xx.reshape(-1, self.cfg["dim"])
        B = xx.shape[0]
        with torch.cuda.device(self.device):
            out = torch.empty(B, self.cfg["vocab_size"], device=self.device)
            set_pos = int(input_pos is not None)
            ip = _lib.i64_host(torch.as_tensor(input_pos).reshape(-1).tolist()) if set_pos else None
            kp = _lib.i64_host(torch.as_tensor(kv_pos).reshape(-1).tolist()) if set_pos else None
            assert not set_pos or (len(ip) == B and len(kp) == B)
            _lib.check(_lib.lib().svc_ar_decode_step_batch(self._h, B, _lib.ptr(xx), set_pos, ip, kp, _lib.ptr(out), _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def exp_draws(self, seed, step0, n):
        """(n, vocab) device tensor: the Exp(1) draws the seeded sampler uses for `seed` at token steps step0 .. step0 + n - 1
        (`svc_ar_exp_draws`).  Given back as `exp_noise`, they reproduce the seeded run bit for bit."""
        with torch.cuda.device(self.device):
            out = torch.empty(int(n), self.cfg["vocab_size"], device=self.device)
            _lib.check(_lib.lib().svc_ar_exp_draws(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1)), int(step0), int(n), _lib.ptr(out),
                                                   _lib.stream_ptr()))
        return out

    @torch.inference_mode()
    def generate_batch(self, prompt_texts, prompt_targets, exp_noise=None, top_p=0.7, temperature=0.7, repetition_penalty=1.5,
                       max_new=4001, check_every=16, seeds=None, prefill="slot"):
        """`generate` for B sequences at once (`svc_ar_generate_batch`; B <= the max_batch_size given to setup_caches):
        lists of B prompt_text (1, Tt_b, dim) and prompt_target (1, Tp_b) tensors, exp_noise a list of B (>= n_b, vocab)
        tensors of Exp(1) draws -> list of B (1, n_b) token tensors, each what `generate` gives for that sequence alone.
        Without exp_noise the sampler generates the draws from `seeds` (B integers; fresh ones from torch's CPU generator
        when None, so `torch.manual_seed` governs them) and no noise tensor exists (`svc_ar_generate_batch_seeded`).
        prefill: "slot" prefills slot after slot inside that call; "ragged" admits all B at once with one ragged prefill and
        runs them to completion on the session entry points (temperature, top_p and repetition_penalty may then be lists of B)."""
        toks, n = self.generate_batch_raw(prompt_texts, prompt_targets, exp_noise, top_p, temperature, repetition_penalty, max_new,
                                          check_every, seeds, prefill)
        return [toks[b, :n[b]].long()[None, :] for b in range(len(n))]

    @torch.inference_mode()
    def generate_batch_raw(self, prompt_texts, prompt_targets, exp_noise=None, top_p=0.7, temperature=0.7, repetition_penalty=1.5,
                           max_new=4001, check_every=16, seeds=None, prefill="slot"):
        """`generate_batch` without the per-sequence slicing: (tokens (B, max_new) int32 on the device, list of B counts);
        row b holds its sequence's tokens in [:n_b]."""
        V, D, Lmax = self.cfg["vocab_size"], self.cfg["dim"], self.cfg["max_seq_len"]
        B = len(prompt_texts)
        if prefill not in ("slot", "ragged"):
            raise ValueError('generate_batch: prefill must be "slot" or "ragged"')
        if B != len(prompt_targets) or (exp_noise is not None and len(exp_noise) != B) or (seeds is not None and len(seeds) != B):
            raise ValueError("generate_batch: prompt_texts, prompt_targets and exp_noise / seeds must have one entry per sequence")
        if exp_noise is not None and seeds is not None:
            raise ValueError("generate_batch: give exp_noise or seeds, not both")
        with torch.cuda.device(self.device):
            emb_seq, S, input_pos, kv_pos = self._prompt_layout(prompt_texts, prompt_targets)
            cap = [min(int(max_new), Lmax - s + 1) for s in S]      # what `generate` allows each sequence
            max_new = max(cap)
            toks = torch.zeros(B, max_new, device=self.device, dtype=torch.int32)
            if prefill == "ragged":
                if exp_noise is None and seeds is None:
                    seeds = torch.randint(0, 2 ** 62, (B,), dtype=torch.int64).tolist()
                q = None if exp_noise is None else self._noise_layout(exp_noise, B, max_new, cap)
                per = [v if isinstance(v, (list, tuple)) else [v] * B for v in (temperature, top_p, repetition_penalty)]
                reqs, r0 = [], 0
                for b in range(B):
                    reqs.append(_Request(emb_seq[r0:r0 + S[b]], S[b], input_pos[r0:r0 + S[b]], kv_pos[r0:r0 + S[b]],
                                         None if q is None else q[b], None if q is not None else seeds[b], max_new,
                                         per[0][b], per[1][b], per[2][b], toks[b]))
                    r0 += S[b]
                self.session_admit(list(enumerate(reqs)), x=emb_seq)
                try:
                    while True:
                        n, done = self.session_run(int(check_every) if check_every >= 1 else 16)
                        if all(done[:B]):
                            break
                finally:
                    for b in range(B):
                        self.session_retire(b, 0)
                return toks, list(n[:B])
            if any(isinstance(v, (list, tuple)) for v in (temperature, top_p, repetition_penalty)):
                raise ValueError('generate_batch: per-sequence sampling parameters need prefill="ragged"')
            n = (C.c_int32 * B)()
            tail = (max_new, 10, C.c_float(temperature), C.c_float(top_p), C.c_float(repetition_penalty), int(check_every),
                    _lib.ptr(toks), n, _lib.stream_ptr())
            head = (self._h, B, _lib.ptr(emb_seq), (C.c_int32 * B)(*S), _lib.i64_host(input_pos), _lib.i64_host(kv_pos))
            if exp_noise is None:
                if seeds is None:
                    seeds = torch.randint(0, 2 ** 62, (B,), dtype=torch.int64).tolist()
                sd = (C.c_uint64 * B)(*[int(v) & (2 ** 64 - 1) for v in seeds])
                _lib.check(_lib.lib().svc_ar_generate_batch_seeded(*head, sd, *tail))
            else:
                q = self._noise_layout(exp_noise, B, max_new, cap)
                _lib.check(_lib.lib().svc_ar_generate_batch(*head, _lib.ptr(q), *tail))
        return toks, list(n)

    def _prompt_layout(self, prompt_texts, prompt_targets):
        """The prompt of NaiveWrapper.generate (ar.py:390-396) for every sequence, concatenated: rows (sum S, dim) =
        [sep, text, sep, embeddings of the target tokens] per sequence, list of S, input_pos and kv_pos of all rows."""
        D = self.cfg["dim"]
        sep = self._sep.reshape(1, D)
        rows, S, input_pos, kv_pos = [], [], [], []
        for text, tgt in zip(prompt_texts, prompt_targets):
            text = _lib.f32c(text, self.device)[0]
            tgt = tgt.to(self.device).long().reshape(-1)
            rows += [sep, text, sep, self._emb[tgt]]
            S.append(text.size(0) + 2 + tgt.numel())
            input_pos += list(range(text.size(0) + 1)) + [0] + [i + 1 for i in range(tgt.numel())]
            kv_pos += list(range(S[-1]))
        return torch.cat(rows, dim=0).contiguous(), S, input_pos, kv_pos

    def _noise_layout(self, exp_noise, B, max_new, cap):
        """exp_noise (a list of B (>= cap_b, vocab) tensors, or one (B, max_new, vocab) tensor) as (B, max_new, vocab)."""
        V = self.cfg["vocab_size"]
        if torch.is_tensor(exp_noise) and tuple(exp_noise.shape) == (B, max_new, V):
            return _lib.f32c(exp_noise, self.device)       # already in the call's layout: used as it is
        q = torch.ones(B, max_new, V, device=self.device)
        for b, e in enumerate(exp_noise):
            assert e.shape[0] >= cap[b] and e.shape[1] == V
            k = min(e.shape[0], max_new)
            q[b, :k] = _lib.f32c(e, self.device)[:k]
        return q

    # ---- the backend of ARSession: requests, admit, run, retire
    @torch.inference_mode()
    def session_request(self, prompt_text, prompt_target, seed, exp_noise, max_new, top_p, temperature, repetition_penalty):
        """One request as `session_admit` takes it; ValueError if its prompt does not fit the cache."""
        V, Lmax = self.cfg["vocab_size"], self.cfg["max_seq_len"]
        with torch.cuda.device(self.device):
            rows, S, input_pos, kv_pos = self._prompt_layout([prompt_text], [prompt_target])
            if S[0] > Lmax:
                raise ValueError(f"ARSession: a prompt of {S[0]} rows does not fit the cache ({Lmax} positions)")
            max_new = min(int(max_new), Lmax - S[0] + 1)
            q = None
            if exp_noise is not None:
                e = _lib.f32c(exp_noise, self.device)
                if e.dim() != 2 or e.shape[0] < max_new or e.shape[1] != V:
                    raise ValueError("ARSession: exp_noise must be (>= max_new, vocab)")
                q = e[:max_new].contiguous()
            toks = torch.zeros(max_new, device=self.device, dtype=torch.int32)
        return _Request(rows, S[0], input_pos, kv_pos, q, seed, max_new, temperature, top_p, repetition_penalty, toks)

    @torch.inference_mode()
    def session_admit(self, entries, x=None):
        """entries: list of (slot, request) -> one `svc_ar_admit`.  x: the requests' rows already concatenated."""
        n = len(entries)
        with torch.cuda.device(self.device):
            if x is None:
                x = torch.cat([r.rows for _, r in entries], dim=0).contiguous()
            reqs = (_lib.ArRequest * max(n, 1))()
            ip, kp = [], []
            for i, (slot, r) in enumerate(entries):
                q = reqs[i]
                q.slot, q.S, q.max_new, q.min_tokens_before_eos = int(slot), int(r.S), int(r.max_new), 10
                q.exp_noise = r.noise.data_ptr() if r.noise is not None else None
                q.seed = 0 if r.seed is None else int(r.seed) & (2 ** 64 - 1)
                q.temperature, q.top_p, q.repetition_penalty = float(r.temperature), float(r.top_p), float(r.repetition_penalty)
                q.tokens_out = r.toks.data_ptr()
                ip += r.input_pos
                kp += r.kv_pos
            _lib.check(_lib.lib().svc_ar_admit(self._h, n, reqs, _lib.ptr(x), _lib.i64_host(ip), _lib.i64_host(kp), _lib.stream_ptr()))
        for slot, r in entries:
            self._admitted[int(slot)] = r

    def session_run(self, n_steps):
        """n_steps batched steps over the occupied slots -> (tokens so far, done flags), one entry per slot."""
        nb = self.max_batch_size
        n, done = (C.c_int32 * nb)(), (C.c_int32 * nb)()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().svc_ar_run(self._h, int(n_steps), n, done, _lib.stream_ptr()))
        return list(n), [bool(d) for d in done]

    @torch.inference_mode()
    def session_retire(self, slot, n_tokens):
        """Frees `slot` and returns its first n_tokens tokens, (1, n_tokens); None if the slot holds no request."""
        r = self._admitted.pop(int(slot), None)
        if r is None:
            return None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().svc_ar_retire(self._h, int(slot), _lib.stream_ptr()))
            return r.toks[:int(n_tokens)].long()[None, :]

    def close(self):
        if self._h:
            _lib.lib().svc_ar_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Request:
    """One waiting or admitted sequence: its prompt rows and positions, draws (`noise` or `seed`), limits, sampling
    parameters and token buffer."""
    __slots__ = ("rows", "S", "input_pos", "kv_pos", "noise", "seed", "max_new", "temperature", "top_p", "repetition_penalty", "toks")

    def __init__(self, rows, S, input_pos, kv_pos, noise, seed, max_new, temperature, top_p, repetition_penalty, toks):
        self.rows, self.S, self.input_pos, self.kv_pos = rows, S, input_pos, kv_pos
        self.noise, self.seed, self.max_new = noise, seed, max_new
        self.temperature, self.top_p, self.repetition_penalty, self.toks = temperature, top_p, repetition_penalty, toks


class ARSession:
    """Continuous batching over the slots of one ARModel: FIFO, lowest free slot first.

    `submit` queues a request and returns its ticket; `step` admits ALL waiting requests that fit into free slots in ONE
    admit call (one ragged prefill), runs `steps_per_run` batched steps, retires what has finished and returns
    [(ticket, tokens (1, n))]; `drain` steps until nothing is left.  A request's tokens do not depend on the other requests,
    on its slot, on `steps_per_run` or on when it was admitted.  The class is plain Python: everything that touches the
    device is the backend's (`ar.max_batch_size`, `ar.session_request / _admit / _run / _retire`)."""

    def __init__(self, ar, steps_per_run=16):
        if steps_per_run < 1:
            raise ValueError("ARSession: steps_per_run must be at least 1")
        self.ar, self.steps_per_run = ar, int(steps_per_run)
        self._waiting = collections.deque()        # (ticket, request)
        self._active = {}                          # slot -> ticket
        self._next_ticket = 0

    @property
    def n_active(self):
        return len(self._active)

    @property
    def n_waiting(self):
        return len(self._waiting)

    def submit(self, prompt_text, prompt_target, *, seed=None, exp_noise=None, max_new=4001, top_p=0.7, temperature=0.7,
               repetition_penalty=1.5):
        if (seed is None) == (exp_noise is None):
            raise ValueError("ARSession.submit: give exactly one of seed / exp_noise")
        req = self.ar.session_request(prompt_text, prompt_target, seed, exp_noise, max_new, top_p, temperature, repetition_penalty)
        ticket = self._next_ticket
        self._next_ticket += 1
        self._waiting.append((ticket, req))
        return ticket

    def step(self):
        free = [b for b in range(self.ar.max_batch_size) if b not in self._active]
        entries = []
        while self._waiting and free:
            ticket, req = self._waiting.popleft()
            slot = free.pop(0)
            self._active[slot] = ticket
            entries.append((slot, req))
        if entries:
            self.ar.session_admit(entries)
        if not self._active:
            return []
        n_tokens, done = self.ar.session_run(self.steps_per_run)
        out = []
        for slot in sorted(self._active):
            if done[slot]:
                out.append((self._active.pop(slot), self.ar.session_retire(slot, n_tokens[slot])))
        return out

    def drain(self):
        out = []
        while self._waiting or self._active:
            out += self.step()
        return out

    def close(self):
        """Drops what is waiting and retires what is in flight, so that the model is free again (a caller's way out of an
        error between `submit` and the end of `drain`)."""
        self._waiting.clear()
        for slot in sorted(self._active):
            self.ar.session_retire(slot, 0)
        self._active.clear()
