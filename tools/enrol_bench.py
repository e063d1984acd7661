"""Enrolment of B reference voices (the full-size CAMPPlus, the 22 kHz mel preset: n_fft 1024, hop 256, 80 mels) for
B = 1, 8, 64 clips whose lengths are spread evenly over 3 ... 25 s (fixed shuffled order), random weights, noise clips:

  (a) loop:     per clip `mel_fn(wave[b:b+1, :n_b])` and `campplus.style(wave_16k[b, :n16_b])` -- the one-clip entry points
                (mel; fbank, mean in torch, embedding), B times;
  (b) one call: `pipeline.enrol_references(mel_fn, campplus, waves, lens, waves_16k, lens_16k)` -- three library calls for
                the whole batch.

HIP events, 2 warm-up + `--repeats` (5) timed runs of each, median and spread (max - min), per batch size; (b)'s rows are
compared with (a)'s (max |diff| of the styles, bit equality of the prompt frames).  The share of padded rows in (b) is
reported too: the one-call form computes every row of the B x Tmax rectangle.  `--out FILE` writes the JSON document.
`--only loop|one` runs that form alone (no comparison): the command to put after `rocprofv3 --kernel-trace --stats --`, so
that the kernel statistics are one form's."""
import argparse
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
from seedvc_amd.audio import MelSpectrogram
from seedvc_amd.campplus import CAMPPlus
from seedvc_amd.pipeline import enrol_references

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,8,64")
ap.add_argument("--min-seconds", type=float, default=3.0)
ap.add_argument("--max-seconds", type=float, default=25.0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only", choices=["both", "loop", "one"], default="both")
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
args = ap.parse_args()
R = args.repeats

torch.set_grad_enabled(False)
dev = "cuda:0"
SR, SR16 = 22050, 16000
c = specs.campplus_config()
cp = CAMPPlus(c, weights.make_state_dict(specs.campplus_state_spec(c), seed=1234, prefix="campplus."), dev)
mel_fn = MelSpectrogram(1024, 80, SR, 256, 1024, 0, None, center=False, device=dev)


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


records = []
for B in [int(v) for v in args.batches.split(",")]:
    secs = [args.min_seconds + (args.max_seconds - args.min_seconds) * i / max(B - 1, 1) for i in range(B)]
    random.Random(0).shuffle(secs)
    lens, lens16 = [int(s * SR) for s in secs], [int(s * SR16) for s in secs]
    g = torch.Generator().manual_seed(B)
    waves = (0.1 * torch.randn(B, max(lens), generator=g)).to(dev)
    waves16 = (0.1 * torch.randn(B, max(lens16), generator=g)).to(dev)
    alone = [(waves[b:b + 1, :lens[b]].contiguous(), waves16[b, :lens16[b]].contiguous()) for b in range(B)]
    loop = lambda: [(mel_fn(w), cp.style(w16)) for w, w16 in alone]                     # noqa: E731
    one = lambda: enrol_references(mel_fn, cp, waves, lens, waves16, lens16)            # noqa: E731
    rec = {"B": B, "seconds": [round(min(secs), 2), round(max(secs), 2)], "sum_seconds": round(sum(secs), 1),
           "padded_row_share": round(B * max(secs) / sum(secs) - 1, 4)}
    if args.only != "one":
        rec["a_loop"] = timed(loop)
    if args.only != "loop":
        rec["b_one_call"] = timed(one)
    if args.only != "both":
        records.append(rec)
        print(json.dumps(rec), flush=True)
        continue
    ya, yb = loop(), one()
    P = yb["prompt_lens"]
    rec["b_vs_a"] = {"style_max_abs_diff": max((ya[b][1] - yb["style"][b:b + 1]).abs().max().item() for b in range(B)),
                     "prompts_bit_identical": sum(torch.equal(ya[b][0], yb["prompt"][b:b + 1, :, :P[b]]) for b in range(B)),
                     "finite": bool(torch.isfinite(yb["style"]).all().item())}
    rec["a_over_b"] = round(rec["a_loop"]["ms"] / rec["b_one_call"]["ms"], 3)
    rec["b_below_a_by_more_than_the_spreads"] = bool(
        rec["a_loop"]["ms"] - rec["b_one_call"]["ms"] > rec["a_loop"]["spread_ms"] + rec["b_one_call"]["spread_ms"])
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del waves, waves16, alone, ya, yb

doc = {"tool": "tools/enrol_bench.py", "label": args.label, "model": "CAMPPlus (full size) + 22 kHz log-mel", "repeats": R,
       "records": records}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
