"""The fp16p8 precision plan at full size (informational, no speed claim): BigVGAN 22k, B = 32 x S = 430, vocoder alone.

  (a) p8_empty:  `voc(mel)` with the empty plan -- the launches of fp16p8 as it always was;
  (b) p8_full:   the same handle with every candidate vetoed -- the launches of fp16x3;
  (c) x3:        a precision="fp16x3" handle on the same weights (what (b) must cost);
  (d) calibrate: one `voc.calibrate(mel)` (an fp16x3 forward + one census per candidate conv + the weight census; host clock
      around the call, which ends in a stream synchronise).

HIP events, 2 warm-up + `--repeats` (5) timed runs of each, the three forwards alternating inside every repeat, median and
spread (max - min).  (a) and (c) use nothing but `BigVGAN.__call__`, so the tool also runs on a commit without the plan, where
it reports those two only; `--parent FILE` embeds such a record, labelled, with the differences to this run.
`--fixtures` adds the error table of the test fixtures (tests/voc_plan_cases.py: E_p8, E_plan, E_x3 against the oracle).
`--out FILE` writes the JSON document."""
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
from seedvc_amd.vocoder import BigVGAN

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=430)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--label", default="this commit")
ap.add_argument("--parent", default="", help="JSON written by this tool on the parent commit")
ap.add_argument("--fixtures", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
B, S, R = args.batch, args.frames, args.repeats

torch.set_grad_enabled(False)
assert torch.cuda.is_available(), "this tool measures on the GPU"
dev = "cuda:0"
vh = specs.bigvgan_config("22k")
sd = weights.make_state_dict(specs.bigvgan_state_spec(vh), seed=1234, prefix="bigvgan.")
p8 = BigVGAN(vh, sd, dev, precision="fp16p8")
x3 = BigVGAN(vh, sd, dev, precision="fp16x3")
has_plan = hasattr(p8, "calibrate")
g = torch.Generator().manual_seed(0)
mel = (torch.randn(B, vh["num_mels"], S, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev)


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


def set_full(on):
    if on:
        p8.precision_plan = {k: True for k in p8.plan_names()}
    else:
        p8.reset_plan()


runs = {"p8_empty": lambda: p8(mel), "x3": lambda: x3(mel)}
if has_plan:
    runs["p8_full"] = lambda: p8(mel)
times = {k: [] for k in runs}
for rep in range(2 + R):
    for k, fn in runs.items():
        if has_plan:
            set_full(k == "p8_full")
        t = event_ms(fn)
        if rep >= 2:
            times[k].append(t)
doc = {"label": args.label, "model": "bigvgan 22k", "batch": B, "frames": S, "repeats": R,
       "method": "HIP events, forwards alternating inside every repeat, median and max - min; vocoder alone"}
doc.update({k: stats(v) for k, v in times.items()})
if has_plan:
    set_full(False)
    y0 = p8(mel)
    cal = []
    for rep in range(1 + 3):
        p8.reset_plan()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = p8.calibrate(mel)
        torch.cuda.synchronize()
        if rep >= 1:
            cal.append((time.perf_counter() - t0) * 1e3)
    doc["calibrate"] = stats(cal)
    doc["calibrate"]["clock"] = "host, around a call that ends in a stream synchronise; 1 warm-up + 3 runs"
    doc["candidates"] = len(rows)
    doc["vetoed_at_default_tau"] = sum(r["veto"] for r in rows)
    doc["rho_max"], doc["eta_max"] = max(r["rho"] for r in rows), max(r["eta"] for r in rows)
    doc["omega_hi_max"], doc["omega_lo_max"] = max(r["omega_hi"] for r in rows), max(r["omega_lo"] for r in rows)
    doc["empty_plan_after_calibrate_bit_equal"] = bool(torch.equal(p8(mel), y0)) if not doc["vetoed_at_default_tau"] else None
    set_full(True)
    doc["full_plan_equals_fp16x3_bits"] = bool(torch.equal(p8(mel), x3(mel)))
    set_full(False)

if args.fixtures and has_plan:
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle")):
        sys.path.insert(0, p)
    import voc_plan_cases as V
    from seedvc_amd.vocoder import HiFT
    table = []
    for voc_name, variants in (("bigvgan", V.VARIANTS), ("hift", ("in_range", "gains"))):
        for variant in variants:
            if voc_name == "bigvgan":
                h, fsd, fmel, ref = V.bigvgan_fixture(variant)
                a, b = BigVGAN(h, fsd, dev), BigVGAN(h, fsd, dev, precision="fp16x3")
                kw = dict(mel=fmel.to(dev))
                run = lambda v: v(kw["mel"]).cpu()                       # noqa: E731
            else:
                c, fsd, fmel, f0, ph, nz, ref = V.hift_fixture(variant)
                a, b = HiFT(c, fsd, dev), HiFT(c, fsd, dev, precision="fp16x3")
                kw = dict(x=fmel.to(dev), f0=f0.to(dev), phase0=ph.to(dev), noise=nz.to(dev))
                run = lambda v: v(**kw).cpu()                            # noqa: E731
            e_p8 = V.rel_rms(run(a), ref)
            frows = a.calibrate(**kw)
            table.append({"vocoder": voc_name, "fixture": variant, "candidates": len(frows), "vetoed": sum(r["veto"] for r in frows),
                          "E_p8": e_p8, "E_plan": V.rel_rms(run(a), ref), "E_x3": V.rel_rms(run(b), ref),
                          "rho_max": max(r["rho"] for r in frows), "eta_max": max(r["eta"] for r in frows),
                          "omega_max": max(max(r["omega_hi"], r["omega_lo"]) for r in frows)})
    doc["fixtures"] = {"errors": "RMS(err) / RMS(oracle), fp32 oracle", "tau": V.TAU, "rows": table}

if args.parent:
    parent = json.load(open(args.parent))
    doc["parent"] = parent
    doc["vs_parent_ms"] = {k: round(doc[k]["ms"] - parent[k]["ms"], 3) for k in ("p8_empty", "x3") if k in parent}
print(json.dumps(doc))
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
