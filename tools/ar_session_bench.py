"""Continuous batching of the AR model, measured: ar_base with synthetic weights (as tools/v2_bench.py builds them), every
comparison in ONE process with the two paths alternating run by run, HIP events, median and spread (max - min).

prefill     The 64 prompts of BASELINE config 5 (120 condition frames + 200 prompt tokens = 322 rows each) through ONE
            `svc_ar_prefill_batch` against 64 calls of `svc_ar_prefill_slot` (the closed batch's way); also n = 1, 4, 16.
            Both are timed at the C entry points on prepared inputs, host synchronisations included.
mixed       256 requests whose lengths come from a fixed seeded list spread over 64 ... 1024 tokens: four consecutive
            `generate_batch` calls of 64 in arrival order against one 64-slot `ARSession`.  A random-weight model would
            draw EOS at random, so the lengths are pinned through the draws, the same way in both paths: top_p = 1 (no
            entry is cut, EOS keeps a positive probability), the Exp(1) draw of EOS is 1e30 in every row (EOS never wins
            the race) except 1e-30 in the row of token L (it wins there): request i ends by EOS with exactly L_i tokens.
            Reported: tokens/s, decode steps run, mean slot occupancy (tokens recorded by the steps / (steps x 64)),
            per-request completion time p50 / p95 (all 256 arrive at t = 0; host clock, the calls synchronise).
v2          (--v2) the tools/v2_bench.py composite at B = 64 with V2HotPath(ar_prefill="ragged") beside "slot".
--prefill-once   one warm ragged pass and one more, nothing else: the run to put under a kernel trace.

`--out FILE` writes one JSON document."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import _pkgload
_pkgload.load_package()
import torch
from seedvc_amd import _lib, specs, weights
from seedvc_amd.ar import ARModel, ARSession

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--mixed-repeats", type=int, default=3)
ap.add_argument("--requests", type=int, default=256)
ap.add_argument("--steps-per-run", type=int, default=16)
ap.add_argument("--sections", default="prefill,mixed")
ap.add_argument("--v2", action="store_true")
ap.add_argument("--prefill-once", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
R = args.repeats

torch.set_grad_enabled(False)
torch.manual_seed(0)
dev = "cuda:0"
NB = 64
ac = specs.ar_config()
V, D, EOS = ac["vocab_size"], ac["dim"], ac["vocab_size"] - 1
ar = ARModel(ac, weights.make_state_dict(specs.ar_state_spec(ac), seed=7, prefix="ar."), dev)
ar.setup_caches(max_batch_size=NB)
lib = _lib.lib()


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "spread_ms": round(ts[-1] - ts[0], 3)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(paths, repeats, warm=2):
    """{name: fn} -> {name: [ms]}: `warm` untimed rounds, then `repeats` rounds with the paths taking turns."""
    for _ in range(warm):
        for f in paths.values():
            f()
    ts = {k: [] for k in paths}
    for _ in range(repeats):
        for k, f in paths.items():
            ts[k].append(event_ms(f))
    return ts


g = torch.Generator().manual_seed(5)
texts = [torch.randn(1, 120, D, generator=g).to(dev) for _ in range(NB)]
tgts = [torch.randint(0, 2048, (1, 200), generator=g).to(dev) for _ in range(NB)]
record = {"tool": "tools/ar_session_bench.py", "model": "ar_base, synthetic weights", "slots": NB, "prompt_rows": 322}


def prefill_paths(n):
    x, S, ip, kp = ar._prompt_layout(texts[:n], tgts[:n])
    S32, ipc, kpc = (C.c_int32 * n)(*S), _lib.i64_host(ip), _lib.i64_host(kp)
    slots = (C.c_int32 * n)(*range(n))
    out = torch.empty(n, V, device=dev)
    offs = [sum(S[:i]) for i in range(n)]
    per = [(_lib.i64_host(ip[o:o + s]), _lib.i64_host(kp[o:o + s])) for o, s in zip(offs, S)]

    def ragged():
        _lib.check(lib.svc_ar_prefill_batch(ar._h, n, slots, _lib.ptr(x), S32, ipc, kpc, _lib.ptr(out), _lib.stream_ptr()))

    def slot_by_slot():
        for i in range(n):
            _lib.check(lib.svc_ar_prefill_slot(ar._h, i, C.c_void_p(x.data_ptr() + offs[i] * D * 4), S[i], per[i][0], per[i][1],
                                               C.c_void_p(out.data_ptr() + i * V * 4), _lib.stream_ptr()))

    return {"ragged": ragged, "slot": slot_by_slot}, out


if args.prefill_once:
    paths, _ = prefill_paths(NB)
    paths["ragged"]()
    torch.cuda.synchronize()
    paths["ragged"]()
    torch.cuda.synchronize()
    print(json.dumps({"prefill_once": True, "passes": ar.prefill_passes()}))
    sys.exit(0)

if "prefill" in args.sections:
    record["prefill"] = []
    for n in (1, 4, 16, 64):
        paths, out = prefill_paths(n)
        paths["slot"]()
        a = out.clone()
        paths["ragged"]()
        dist = (out - a).abs().max().item()
        ts = alternate(paths, R)
        rec = {"n": n, "rows": 322 * n, "passes": ar.prefill_passes(), "ragged": stats(ts["ragged"]), "slot": stats(ts["slot"]),
               "max_logit_distance": round(dist, 6), "mean_abs_logit": round(a.abs().mean().item(), 4)}
        rec["speedup"] = round(rec["slot"]["ms"] / rec["ragged"]["ms"], 3)
        rec["beats_by_more_than_both_spreads"] = bool(rec["slot"]["ms"] - rec["ragged"]["ms"] > rec["slot"]["spread_ms"] + rec["ragged"]["spread_ms"])
        print(json.dumps(rec), flush=True)
        record["prefill"].append(rec)

if "mixed" in args.sections:
    NREQ, CAP = args.requests, 1024
    lg = torch.Generator().manual_seed(11)
    lengths = (64 + torch.randint(0, CAP - 64 + 1, (NREQ,), generator=lg)).tolist()
    groups = [list(range(k, min(k + NB, NREQ))) for k in range(0, NREQ, NB)]
    noise = []
    for grp in groups:           # one (64, CAP, V) tensor per arrival group, already in generate_batch's layout
        q = torch.empty(len(grp), CAP, V, device=dev).exponential_(1)
        q[:, :, EOS] = 1e30
        for j, i in enumerate(grp):
            if lengths[i] < CAP:
                q[j, lengths[i], EOS] = 1e-30
        noise.append(q)
    kw = dict(top_p=1.0, temperature=0.7, repetition_penalty=1.5)
    state = {}

    def closed():
        t0, done_at, counts, steps = time.perf_counter(), [], [], 0
        for grp, q in zip(groups, noise):
            _, n = ar.generate_batch_raw([texts[i % NB] for i in grp], [tgts[i % NB] for i in grp], exp_noise=q, max_new=CAP, check_every=16, **kw)
            done_at += [time.perf_counter() - t0] * len(grp)
            counts += n
            steps += min(CAP - 1, -(-max(n) // 16) * 16)        # a sequence of L tokens draws EOS in step L
        state["closed"] = (done_at, counts, steps)

    def session():
        t0, done_at, counts = time.perf_counter(), {}, {}
        s = ARSession(ar, steps_per_run=args.steps_per_run)
        runs = 0
        for grp, q in zip(groups, noise):
            for j, i in enumerate(grp):
                s.submit(texts[i % NB], tgts[i % NB], exp_noise=q[j], max_new=CAP, **kw)
        while s.n_active or s.n_waiting:
            for t, toks in s.step():
                done_at[t], counts[t] = time.perf_counter() - t0, int(toks.shape[1])
            runs += 1
        state["session"] = ([done_at[t] for t in range(NREQ)], [counts[t] for t in range(NREQ)], runs * args.steps_per_run)

    ts = alternate({"closed": closed, "session": session}, args.mixed_repeats, warm=1)
    rec = {"requests": NREQ, "lengths": {"min": min(lengths), "max": max(lengths), "mean": round(sum(lengths) / NREQ, 1)},
           "steps_per_run": args.steps_per_run, "repeats": args.mixed_repeats}
    for k in ("closed", "session"):
        done_at, counts, steps = state[k]
        assert counts == lengths, (k, [(a, b) for a, b in zip(counts, lengths) if a != b][:5])
        d = sorted(done_at)
        st = stats(ts[k])
        rec[k] = {"total": st, "tokens": sum(counts), "tokens_per_s": round(sum(counts) / st["ms"] * 1e3, 1), "decode_steps": steps,
                  "mean_slot_occupancy": round(sum(c - 1 for c in counts) / (steps * NB), 4),
                  "completion_s": {"p50": round(d[len(d) // 2], 3), "p95": round(d[int(len(d) * 0.95)], 3)}}
    rec["speedup"] = round(rec["closed"]["total"]["ms"] / rec["session"]["total"]["ms"], 3)
    rec["beats_by_more_than_both_spreads"] = bool(rec["closed"]["total"]["ms"] - rec["session"]["total"]["ms"] >
                                                  rec["closed"]["total"]["spread_ms"] + rec["session"]["total"]["spread_ms"])
    print(json.dumps(rec), flush=True)
    record["mixed_lengths"] = rec
    del noise

if args.v2:
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath
    from seedvc_amd.vocoder import BigVGAN
    sd_of = lambda spec, seed, prefix: weights.make_state_dict(spec, seed=seed, prefix=prefix)      # noqa: E731
    alc, clc, dc, vh = specs.lr_config("v2_ar"), specs.lr_config("v2_cfm"), specs.dit_config("v2"), specs.bigvgan_config("22k")
    hp = V2HotPath(ar, InterpolateRegulator(alc, sd_of(specs.lr_state_spec(alc), 5, "lr."), dev),
                   InterpolateRegulator(clc, sd_of(specs.lr_state_spec(clc), 6, "lr."), dev),
                   CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.v2."), dev),
                   BigVGAN(vh, sd_of(specs.bigvgan_state_spec(vh), 1234, "bigvgan."), dev))
    P, N_TOK, STEPS = 430, 256, 25
    gg = torch.Generator().manual_seed(NB)
    target = hp.prepare_target(torch.randint(0, 32, (1, 40), generator=gg), torch.randint(0, 2048, (1, 200), generator=gg),
                               (torch.randn(1, dc["C"], P, generator=gg) * 2 - 4).clamp(-11.5, 2), torch.randn(1, dc["style_dim"], generator=gg))
    src = [torch.randint(0, 32, (1, 80), generator=gg).to(dev) for _ in range(NB)]
    seeds = list(range(1000, 1000 + NB))

    def composite(mode):
        def run():
            hp.ar_prefill = mode
            hp.convert_batch(src, [target] * NB, [P / N_TOK] * NB, STEPS, cfg_rates=(0.7, 0.7), max_new=N_TOK, seeds=seeds)
        return run

    ts = alternate({"slot": composite("slot"), "ragged": composite("ragged")}, R, warm=2)
    hp.ar_prefill = "slot"
    rec = {"workload": "BASELINE config 5 as one call", "B": NB, "slot": stats(ts["slot"]), "ragged": stats(ts["ragged"])}
    print(json.dumps(rec), flush=True)
    record["v2_composite"] = rec

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
