"""Full-size HiFT on a batch of 64 utterances of 64 DIFFERENT lengths (120 ... 430 frames, evenly spread, fixed shuffled
order), fp16p8, vocoder alone, f0 / phase0 / noise pinned (drawn once):

  (a) grouped: 64 calls `voc(mel[b:b+1, :, :S_b], ...)` -- what one call per distinct length costs on such a batch;
  (b) ragged:  one call `voc(mel, ..., lens=S)`;
  (c) uniform: one call `voc(mel, ...)` at B = 64, S = 430 -- the ceiling a batch padded to its longest member would cost
      (its result is not the utterances' own: see tests/test_host_hift_ragged.py).

HIP events, 2 warm-up + `--repeats` (5) timed runs of each, median and spread (max - min); the share of padded rows in (b)
(sum over micro-batches of longest member x members / sum of lengths - 1; utterances sorted longest first, a micro-batch ends
after 32 members or where the next utterance's stage lengths fall on another side of the 192-row kernel-choice boundary).
(a) and (c) use nothing but the plain `HiFT.__call__`, so the tool also runs on a commit without the ragged call, where it
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
from seedvc_amd.vocoder import HiFT

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
c = specs.hift_config()
voc = HiFT(c, weights.make_state_dict(specs.hift_state_spec(c), seed=1234, prefix="hift."), dev, precision=args.precision)
voc.set_microbatch(args.microbatch)
has_ragged = "lens" in inspect.signature(HiFT.__call__).parameters

lens = [args.min_frames + round((args.max_frames - args.min_frames) * i / max(B - 1, 1)) for i in range(B)]
random.Random(0).shuffle(lens)
Smax = max(lens)
up, nh = specs.hift_total_upsample(c), c["nb_harmonics"] + 1
g = torch.Generator().manual_seed(0)
mel = torch.full((B, c["in_channels"], Smax), LOG_MEL_FLOOR)
for b, n in enumerate(lens):
    mel[b, :, :n] = (torch.randn(c["in_channels"], n, generator=g) * 2 - 4).clamp(-11.5, 2)
mel = mel.to(dev)
f0 = (120.0 + 80.0 * torch.rand(B, Smax, generator=g)).to(dev)
phase0 = ((torch.rand(B, nh, 1, generator=g) * 2 - 1) * 3.141592653589793).to(dev)
noise = torch.randn(B, nh, Smax * up, generator=g).to(dev)
alone = [(mel[b:b + 1, :, :n].contiguous(), f0[b:b + 1, :n].contiguous(), phase0[b:b + 1], noise[b:b + 1, :, :n * up].contiguous())
         for b, n in enumerate(lens)]


def kernel_class(n):      # svc_hift::kernel_class: stages of an utterance that reach the resident-tile conv's 192 rows
    rows, k = [n], n
    for i, u in enumerate(c["upsample_rates"]):
        k = k * u + (1 if i == len(c["upsample_rates"]) - 1 and n else 0)
        rows.append(k)
    return sum(r >= 192 for r in rows)


def padded_rows():
    order, total, i = sorted(lens, reverse=True), 0, 0
    while i < B:
        j = i
        while j < B and j - i < args.microbatch and kernel_class(order[j]) == kernel_class(order[i]):
            j += 1
        total += order[i] * (j - i)
        i = j
    return total


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


grouped = lambda: [voc(m, f0=f, phase0=p, noise=z) for m, f, p, z in alone]      # noqa: E731
rec = {"label": args.label, "model": "HiFT (full size)", "precision": args.precision, "B": B, "frames": [min(lens), max(lens)],
       "distinct_lengths": len(set(lens)), "sum_frames": sum(lens), "microbatch": args.microbatch, "repeats": R,
       "a_grouped": timed(grouped)}
if has_ragged:
    ragged = lambda: voc(mel, f0=f0, phase0=phase0, noise=noise, lens=lens)      # noqa: E731
    rec["b_ragged"] = timed(ragged)
    rec["b_padded_row_share"] = round(padded_rows() / sum(lens) - 1, 4)
    ya, yb = grouped(), ragged()
    same = [torch.equal(ya[b].reshape(-1), yb[b, :lens[b] * up]) for b in range(B)]
    rec["b_equals_a_bit_for_bit"] = {"utterances": B, "bit_identical": sum(same),
                                     "max_rms": max((ya[b].reshape(-1) - yb[b, :lens[b] * up]).pow(2).mean().sqrt().item() for b in range(B))}
    rec["b_tails_zero"] = bool(all((yb[b, lens[b] * up:] == 0).all().item() for b in range(B)))
    rec["a_over_b"] = round(rec["a_grouped"]["ms"] / rec["b_ragged"]["ms"], 3)
    rec["b_below_a_by_more_than_the_spreads"] = bool(
        rec["a_grouped"]["ms"] - rec["b_ragged"]["ms"] > rec["a_grouped"]["spread_ms"] + rec["b_ragged"]["spread_ms"])
rec["c_uniform_B_x_Smax"] = timed(lambda: voc(mel, f0=f0, phase0=phase0, noise=noise))
doc = {"tool": "tools/hift_ragged_bench.py", "records": [rec]}
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
