"""What the DiT's full-precision mode costs (precision 2, fp16x3: DESIGN.md 8v): `CFM.inference` of a precision-1 and a
precision-2 handle packed from the same weights, timed in the same run, alternating round by round after `--warmup` rounds.

Shapes (name:preset:B:steps:P:S): full-size tiny and small at B = 1 and B = 64, v2 at B = 64; 25 steps, prompt 430 + 430 source
frames (bench.py's shape), seeded noise.  v1 runs one guidance rate (two streams), v2 both (three streams).

Per shape and precision: host-clock milliseconds around the call, ending in a device synchronisation; median and spread (max -
min) over `--repeats` rounds; then ONE more call under the launch timer (`svc_prof_*`: HIP events around every tap-GEMM,
attention and row-panel launch) for the breakdown by class -- gemm (fp16 and fp32 tap-GEMMs), attention, fused (the row-panel
kernel, precision 1 only) and rest (the timed call minus the classes: norms, RoPE / split rows, state update, layout changes,
launch gaps; the timer's own events inflate it, so it is an upper bound).  `ratio` = precision 2 over precision 1.
`--out FILE` writes the JSON document (profiles/dit_precision.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
import torch
from seedvc_amd import _lib, specs, weights
from seedvc_amd.cfm import CFM

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="tiny_b1:tiny:1:25:430:430,tiny_b64:tiny:64:25:430:430,small_b1:small:1:25:430:430,"
                                   "small_b64:small:64:25:430:430,v2_b64:v2:64:25:430:430", help="name:preset:B:steps:P:S, comma separated")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default="")
args = ap.parse_args()

torch.set_grad_enabled(False)
dev = "cuda:0"
CLASSES = ("gemm_f16", "gemm_f32", "attention", "fused")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def breakdown(fn):
    L = _lib.lib()
    buf = (C.c_double * (4 * len(CLASSES)))()
    L.svc_prof_enable(1)
    L.svc_prof_collect(buf, len(CLASSES))          # clear
    ms = timed(fn)
    L.svc_prof_collect(buf, len(CLASSES))
    L.svc_prof_enable(0)
    cls = {c: buf[4 * i + 1] for i, c in enumerate(CLASSES)}
    out = {"timed_call_ms": round(ms, 3), "gemm_ms": round(cls["gemm_f16"] + cls["gemm_f32"], 3), "attention_ms": round(cls["attention"], 3),
           "fused_ms": round(cls["fused"], 3)}
    out["rest_ms"] = round(ms - out["gemm_ms"] - out["attention_ms"] - out["fused_ms"], 3)
    out["launches"] = {c: int(buf[4 * i]) for i, c in enumerate(CLASSES)}
    return out


records = []
for spec in args.cases.split(","):
    name, preset, B, steps, P, S = spec.split(":")
    B, steps, P, S = int(B), int(steps), int(P), int(S)
    T = P + S
    cfg = specs.dit_config(preset)
    sd = weights.make_state_dict(specs.dit_state_spec(cfg), seed=1234, prefix=f"dit.{preset}.")
    models = {1: CFM(cfg, sd, dev, precision=1), 2: CFM(cfg, sd, dev, precision=2)}
    g = torch.Generator().manual_seed(0)
    mu = torch.randn(B, T, cfg["Dc"], generator=g).to(dev)
    prompt = (torch.randn(B, cfg["C"], P, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev)
    style = torch.randn(B, cfg["style_dim"], generator=g).to(dev)
    seeds = [(0x9E3779B97F4A7C15 * (b + 1)) % 2 ** 64 for b in range(B)]
    rate = [0.7, 0.7] if cfg["version"] == 2 else 0.7
    run = {p: (lambda m=m: m.inference(mu, [T] * B, prompt, style, None, steps, inference_cfg_rate=rate, seeds=seeds)) for p, m in models.items()}
    for _ in range(args.warmup):
        for fn in run.values():
            fn()
    ts = {p: [] for p in run}
    for _ in range(args.repeats):
        for p, fn in run.items():
            ts[p].append(timed(fn))
    rec = {"case": name, "model": preset, "B": B, "steps": steps, "P": P, "S": S, "streams": 3 if cfg["version"] == 2 else 2}
    for p in run:
        t = sorted(ts[p])
        rec[f"precision_{p}"] = {"ms": round(t[len(t) // 2], 3), "spread_ms": round(t[-1] - t[0], 3),
                                 "frames_per_s": round(B * T / (t[len(t) // 2] * 1e-3), 1), "fused_path": bool(models[p].estimator.fused_available),
                                 "classes": breakdown(run[p])}
    rec["ratio"] = round(rec["precision_2"]["ms"] / rec["precision_1"]["ms"], 2)
    y1, y2 = run[1](), run[2]()
    rec["mel_l1_between_precisions"] = float((y1 - y2).abs().mean())
    del y1, y2, mu, prompt, style
    for m in models.values():
        m.estimator.close()
    torch.cuda.empty_cache()
    records.append(rec)
    print(json.dumps(rec), flush=True)
doc = {"tool": "tools/dit_precision_bench.py", "timing": "host clock around calls that end in a device synchronisation; classes from the launch timer on one extra call",
       "repeats": args.repeats, "warmup": args.warmup, "records": records}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
