"""BigVGAN 22k on a batch of 64 utterances of 64 DIFFERENT lengths (120 ... 430 frames, evenly spread, fixed shuffled
order), fp16p8, vocoder alone:

  (a) grouped: 64 calls `voc(mel[b:b+1, :, :S_b])` -- what one call per distinct length costs on such a batch;
  (b) ragged:  one call `voc(mel, lens=S)`;
  (c) uniform: one call `voc(mel)` at B = 64, S = 430 -- the ceiling a batch padded to its longest member would cost
      (its result is not the utterances' own: see tests/test_host_vocoder_ragged.py).

HIP events, 2 warm-up + `--repeats` (5) timed runs of each, median and spread (max - min); the share of padded rows in (b)
(sum over micro-batches of longest member x members / sum of lengths - 1, utterances sorted longest first, micro-batch 32).
(a) and (c) use nothing but `BigVGAN.__call__(mel)`, so the tool also runs on a commit without the ragged call, where it
reports those two only.  `--parent FILE` embeds such a record, labelled, with the differences to this run.
`--out FILE` writes the JSON document."""
import argparse
import inspect
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
import torch
from seedvc_amd import specs, weights
from seedvc_amd.vocoder import BigVGAN

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--min-frames", type=int, default=120)
ap.add_argument("--max-frames", type=int, default=430)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--precision", default="fp16p8")
ap.add_argument("--microbatch", type=int, default=32)
ap.add_argument("--label", default="this commit")
ap.add_argument("--parent", default="", help="JSON written by this tool on the parent commit")
ap.add_argument("--out", default="")
args = ap.parse_args()
B, R = args.batch, args.repeats

torch.set_grad_enabled(False)
dev = "cuda:0"
LOG_MEL_FLOOR = -11.512925464970229
vh = specs.bigvgan_config("22k")
voc = BigVGAN(vh, weights.make_state_dict(specs.bigvgan_state_spec(vh), seed=1234, prefix="bigvgan."), dev, precision=args.precision)
voc.set_microbatch(args.microbatch)
has_ragged = "lens" in inspect.signature(BigVGAN.__call__).parameters

lens = [args.min_frames + round((args.max_frames - args.min_frames) * i / max(B - 1, 1)) for i in range(B)]
random.Random(0).shuffle(lens)
Smax = max(lens)
g = torch.Generator().manual_seed(0)
mel = torch.full((B, vh["num_mels"], Smax), LOG_MEL_FLOOR)
for b, n in enumerate(lens):
    mel[b, :, :n] = (torch.randn(vh["num_mels"], n, generator=g) * 2 - 4).clamp(-11.5, 2)
mel = mel.to(dev)


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "spread_ms": round(ts[-1] - ts[0], 3)}


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(R):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return stats(ts)


grouped = lambda: [voc(mel[b:b + 1, :, :lens[b]]) for b in range(B)]      # noqa: E731
rec = {"label": args.label, "model": "BigVGAN 22k", "precision": args.precision, "B": B, "frames": [min(lens), max(lens)],
       "distinct_lengths": len(set(lens)), "sum_frames": sum(lens), "microbatch": args.microbatch, "repeats": R,
       "a_grouped": timed(grouped)}
if has_ragged:
    rec["b_ragged"] = timed(lambda: voc(mel, lens=lens))
    order = sorted(lens, reverse=True)
    rows = sum(order[i] * len(order[i:i + args.microbatch]) for i in range(0, B, args.microbatch))
    rec["b_padded_row_share"] = round(rows / sum(lens) - 1, 4)
    ya, yb = grouped(), voc(mel, lens=lens)
    up = yb.shape[2] // Smax
    same = [torch.equal(ya[b].reshape(-1), yb[b, 0, :lens[b] * up]) for b in range(B)]
    rec["b_equals_a_bit_for_bit_from_192_frames"] = bool(all(s for s, n in zip(same, lens) if n >= 192))
    rec["b_vs_a_below_192_frames"] = {"utterances": sum(n < 192 for n in lens), "bit_identical": sum(s for s, n in zip(same, lens) if n < 192),
                                      "max_rms": max([(ya[b].reshape(-1) - yb[b, 0, :lens[b] * up]).pow(2).mean().sqrt().item()
                                                      for b in range(B) if lens[b] < 192] or [0.0])}
    rec["b_tails_zero"] = bool(all((yb[b, 0, lens[b] * up:] == 0).all().item() for b in range(B)))
    rec["a_over_b"] = round(rec["a_grouped"]["ms"] / rec["b_ragged"]["ms"], 3)
    rec["b_below_a_by_more_than_the_spreads"] = bool(
        rec["a_grouped"]["ms"] - rec["b_ragged"]["ms"] > rec["a_grouped"]["spread_ms"] + rec["b_ragged"]["spread_ms"])
rec["c_uniform_B_x_Smax"] = timed(lambda: voc(mel))
doc = {"tool": "tools/vocoder_ragged_bench.py", "records": [rec]}
if args.parent:
    with open(args.parent) as f:
        prec = json.load(f)["records"][0]
    doc["records"].append(prec)
    doc["this_minus_parent_ms"] = {k: round(rec[k]["ms"] - prec[k]["ms"], 3) for k in ("a_grouped", "c_uniform_B_x_Smax")}
print(json.dumps(doc), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
