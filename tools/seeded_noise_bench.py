"""Full-size HiFT, fp16p8, f0 pinned: the vocoder call with its SineGen draws made by torch (`torch.rand` (B, nh, 1) +
`torch.randn` (B, nh, S * up), then the explicit call -- what `HiFT.__call__` does without seeds, the only path before the
seeded call existed) against `HiFT.__call__(seeds=...)`, which draws inside the source kernel, at two shapes:

  realtime     64 rows of S = 65 frames: one engine step of tools/rt_bench.py's geometry at 64 streams;
  long_chunks  64 rows of S = 2580 frames: the vocoder call of one 64-chunk micro-batch of tools/long_bench.py's 30 s windows.

Per case and path: HIP-event milliseconds of `--inner` back-to-back calls per sample (divided back to one call), median
and spread (max - min) over `--repeats` samples, the two paths alternating sample by sample after `--warmup` calls of each;
and the peak rise of `torch.cuda.max_memory_allocated` over one call (the caching allocator's view: the (B, nh, S * up)
noise tensor is in it, the library's workspace is not, in either path).  `--out FILE` writes the JSON document."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
import torch
from seedvc_amd import specs, weights
from seedvc_amd.vocoder import HiFT

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="realtime:64:65:20,long_chunks:64:2580:1", help="name:B:S:inner, comma separated")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--precision", default="fp16p8")
ap.add_argument("--out", default="")
args = ap.parse_args()

torch.set_grad_enabled(False)
dev = "cuda:0"
c = specs.hift_config()
voc = HiFT(c, weights.make_state_dict(specs.hift_state_spec(c), seed=1234, prefix="hift."), dev, precision=args.precision)
up, nh = specs.hift_total_upsample(c), c["nb_harmonics"] + 1


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "spread_ms": round(ts[-1] - ts[0], 3)}


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def peak_rise(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    del y
    return torch.cuda.max_memory_allocated() - before


records = []
for spec in args.cases.split(","):
    name, B, S, inner = spec.split(":")
    B, S, inner = int(B), int(S), int(inner)
    g = torch.Generator().manual_seed(0)
    mel = (torch.randn(B, c["in_channels"], S, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev)
    f0 = (120.0 + 80.0 * torch.rand(B, S, generator=g)).to(dev)
    seeds = [(0x9E3779B97F4A7C15 * (b + 1)) % 2 ** 64 for b in range(B)]
    paths = {"torch_draws_explicit_call": lambda: voc(mel, f0=f0), "seeded_call": lambda: voc(mel, f0=f0, seeds=seeds)}
    for fn in paths.values():
        for _ in range(args.warmup):
            fn()
    ts = {k: [] for k in paths}
    for _ in range(args.repeats):
        for k, fn in paths.items():
            ts[k].append(sample(fn, inner))
    rec = {"case": name, "B": B, "S": S, "samples_per_row": S * up, "inner_calls_per_sample": inner,
           "noise_tensor_bytes": B * nh * S * up * 4, "wave_bytes": B * S * up * 4}
    for k, fn in paths.items():
        rec[k] = dict(stats(ts[k]), peak_rise_bytes=peak_rise(fn))
    d = rec["torch_draws_explicit_call"]["ms"] - rec["seeded_call"]["ms"]
    rec["explicit_minus_seeded_ms"] = round(d, 3)
    rec["difference_exceeds_the_spreads"] = bool(abs(d) > rec["torch_draws_explicit_call"]["spread_ms"] + rec["seeded_call"]["spread_ms"])
    rec["seeded_peak_below_noise_tensor"] = bool(rec["seeded_call"]["peak_rise_bytes"] < rec["noise_tensor_bytes"])
    y1, y2 = voc(mel, f0=f0, seeds=seeds), voc(mel, f0=f0, seeds=seeds)
    rec["seeded_call_repeats_bit_for_bit"] = bool(torch.equal(y1, y2))
    del y1, y2, mel, f0
    torch.cuda.empty_cache()
    records.append(rec)
    print(json.dumps(rec), flush=True)
doc = {"tool": "tools/seeded_noise_bench.py", "model": "HiFT (full size)", "precision": args.precision, "repeats": args.repeats,
       "warmup": args.warmup, "records": records}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
