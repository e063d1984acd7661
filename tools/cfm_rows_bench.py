"""Per-utterance sampler settings (`CFM.inference_rows` / `svc_cfm_sample_rows`), full-size DiTs, seeded, B
utterances with B distinct guidance rates, at two shapes:

  realtime  tiny, 10 steps, prompt 258 + 232 source frames: one engine step of tools/rt_bench.py's geometry;
  small     small, 25 steps, prompt 430 + 430 source frames: bench.py's shape.

Variants, alternating round by round in one process after `--warmup` rounds:
  (i)   rows_distinct    one `inference_rows` call, B distinct rates in (0, 1];
  (ii)  b1_calls         B `inference` calls at B = 1, one per rate: the only way before `inference_rows`;
  (iii) uniform_call     `inference` at B with one rate: the floor;
  (iv)  rows_uniform     `inference_rows` with that one rate on every row: the launches of (iii) plus one table load per element;
and a mixed-steps case, B / 2 rows at the shape's step count and B / 2 at 4 steps, as one `inference_rows` call
(mixed_steps_rows) against the two grouped `inference` calls it is defined as (mixed_steps_grouped).

Per variant: host-clock milliseconds around the call(s), ending in a device synchronisation; median and spread (max - min)
over `--repeats` rounds.  `--out FILE` writes the JSON document."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
import torch
from seedvc_amd import specs, weights
from seedvc_amd.cfm import CFM

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="realtime:tiny:10:258:232,small:small:25:430:430", help="name:preset:steps:P:S, comma separated")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()

torch.set_grad_enabled(False)
dev = "cuda:0"
B = args.batch


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "spread_ms": round(ts[-1] - ts[0], 3)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


records = []
for spec in args.cases.split(","):
    name, preset, steps, P, S = spec.split(":")
    steps, P, S = int(steps), int(P), int(S)
    T = P + S
    cfg = specs.dit_config(preset)
    cfm = CFM(cfg, weights.make_state_dict(specs.dit_state_spec(cfg), seed=1234, prefix=f"dit.{preset}."), dev)
    g = torch.Generator().manual_seed(0)
    mu = torch.randn(B, T, cfg["Dc"], generator=g).to(dev)
    prompt = (torch.randn(B, cfg["C"], P, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev)
    style = torch.randn(B, cfg["style_dim"], generator=g).to(dev)
    seeds = [(0x9E3779B97F4A7C15 * (b + 1)) % 2 ** 64 for b in range(B)]
    rates = [(b + 1) / B for b in range(B)]
    lens = [T] * B
    h = B // 2

    def b1_calls():
        for b in range(B):
            cfm.inference(mu[b:b + 1], [T], prompt[b:b + 1], style[b:b + 1], None, steps, inference_cfg_rate=rates[b], seeds=seeds[b:b + 1])

    def grouped():
        cfm.inference(mu[:h], lens[:h], prompt[:h], style[:h], None, steps, inference_cfg_rate=0.7, seeds=seeds[:h])
        cfm.inference(mu[h:], lens[h:], prompt[h:], style[h:], None, 4, inference_cfg_rate=0.7, seeds=seeds[h:])

    paths = {
        "rows_distinct": lambda: cfm.inference_rows(mu, lens, prompt, style, [(steps, r) for r in rates], seeds=seeds),
        "b1_calls": b1_calls,
        "uniform_call": lambda: cfm.inference(mu, lens, prompt, style, None, steps, inference_cfg_rate=0.7, seeds=seeds),
        "rows_uniform": lambda: cfm.inference_rows(mu, lens, prompt, style, [(steps, 0.7)] * B, seeds=seeds),
        "mixed_steps_rows": lambda: cfm.inference_rows(mu, lens, prompt, style, [(steps, 0.7)] * h + [(4, 0.7)] * (B - h), seeds=seeds),
        "mixed_steps_grouped": grouped,
    }
    for _ in range(args.warmup):
        for fn in paths.values():
            fn()
    ts = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            ts[k].append(timed(fn))
    rec = {"case": name, "model": preset, "B": B, "steps": steps, "P": P, "S": S}
    for k in paths:
        rec[k] = stats(ts[k])
    rec["b1_calls_over_rows_distinct"] = round(rec["b1_calls"]["ms"] / rec["rows_distinct"]["ms"], 2)
    d = rec["rows_uniform"]["ms"] - rec["uniform_call"]["ms"]
    rec["rows_uniform_minus_uniform_call_ms"] = round(d, 3)
    rec["rows_uniform_within_the_spreads"] = bool(abs(d) <= rec["rows_uniform"]["spread_ms"] + rec["uniform_call"]["spread_ms"])
    rec["mixed_steps_rows_minus_grouped_ms"] = round(rec["mixed_steps_rows"]["ms"] - rec["mixed_steps_grouped"]["ms"], 3)
    y = cfm.inference_rows(mu, lens, prompt, style, [(steps, 0.7)] * B, seeds=seeds)
    rec["rows_uniform_equals_uniform_call_bit_for_bit"] = bool(torch.equal(
        y, cfm.inference(mu, lens, prompt, style, None, steps, inference_cfg_rate=0.7, seeds=seeds)))
    del y, mu, prompt, style
    cfm.estimator.close()
    torch.cuda.empty_cache()
    records.append(rec)
    print(json.dumps(rec), flush=True)
doc = {"tool": "tools/cfm_rows_bench.py", "timing": "host clock around calls that end in a device synchronisation",
       "repeats": args.repeats, "warmup": args.warmup, "records": records}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
