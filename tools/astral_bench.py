"""ASTRAL tokenizer (csrc/astral.hip), released sizes (HuBERT-large cut to 18 layers, two heads of 12 ConvNeXt V2 blocks, 2048 and 32
codes), random weights, precision 1: audio at 16 kHz -> content tokens, on five cases:

  one real-time context (the GUI's extra + block + right context, `realtime_geometry`), 64 such clips, one 30 s clip, 8 ragged clips
  of 3 ... 25 s, one 600 s file (24 windows).

For each case, alternated in the same run with a rotating order (HIP events, 2 warm-up + `--repeats` timed rounds, median and
spread = max - min): the one call `AstralTokenizer.tokens_batch` with both heads; the same on a handle with the narrow head only; the
SSL seam alone (18 layers, all windows in one call), so that the heads' added cost is visible; the loop over one-window calls; and
the heads alone (ConvNeXt + BSQ seams of both heads over all windows' rows in one ragged call) against a torch float16 statement of
the same heads on the same GPU, fed the same rows one window at a time.  The stage split (SSL, ConvNeXt, BSQ, assemble) comes from the
library's own events and covers the LAST window group of the call.  Nothing is gated on these numbers.  `--out FILE` writes the JSON
document."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _pkgload
_pkgload.load_package()
import torch
import astral_cases as AC
import w2v_cases as VC
from seedvc_amd import pipeline, specs
from seedvc_amd.astral import AstralTokenizer, bsq_index, window_plan

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--precision", type=int, default=1)
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
args = ap.parse_args()
R = args.repeats
torch.set_grad_enabled(False)
dev = "cuda:0"
c = specs.astral_config()
ssl_sd = VC.make_state_dict(c["ssl"], seed=22)
heads = [AC.make_head_sd(c, k, seed=60 + k) for k in range(2)]
m2 = AstralTokenizer(ssl_sd, heads, cfg=c, device=dev, precision=args.precision)
m1 = AstralTokenizer(ssl_sd, heads[1:], cfg=dict(c, heads=c["heads"][1:]), device=dev, precision=args.precision)
heads16 = [{k: v.half().to(dev) for k, v in sd.items()} for sd in heads]
GROUP = 16
geo = pipeline.realtime_geometry(22050, 256, 0.18, 0.04, 2.5, 0.2, 2.0)
RT_SECONDS = (geo["skip_head"] + geo["return_length"] + geo["skip_tail"]) * 320 / 16000


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "spread_ms": round(ts[-1] - ts[0], 3)}


def timed_alternated(fns, warm=2):
    for _ in range(warm):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    names = list(fns)
    for r in range(R):
        for k in names[r % len(names):] + names[:r % len(names)]:      # the order rotates
            f = fns[k]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: stats(v) for k, v in ts.items()}


def torch_heads(rows16):
    for h in rows16:
        for hk, sd in enumerate(heads16):
            bsq_index(AC.logits(sd, AC.convnext(sd, c["heads"][hk], h, torch.float16), torch.float16))


def case(name, secs):
    lens = [int(s * 16000) for s in secs]
    B, L = len(lens), max(lens)
    waves = torch.zeros(B, L)
    for b, n in enumerate(lens):
        src = VC.make_wave(min(n, 30 * 16000), b)
        waves[b, :n] = src.repeat(-(-n // src.numel()))[:n]
    waves = waves.to(dev)
    wins = [(b, s, n, r) for b, L_b in enumerate(lens) for s, n, d, r in window_plan(c, L_b, 250) if r > d]
    one = [waves[b:b + 1, s:s + n].contiguous() for b, s, n, _ in wins]
    wl = [n for _, _, n, _ in wins]
    wbuf = torch.zeros(len(wins), max(wl), device=dev)
    for i, w in enumerate(one):
        wbuf[i, :w.size(1)] = w[0]
    rows_t, wr = m2.ssl(wbuf, wl)
    rows16 = [rows_t[i, :r].half() for i, r in enumerate(wr)]
    rec = {"case": name, "clips": B, "seconds": [round(s, 3) for s in secs], "windows": len(wins), "tokens": [m2.rows(n) for n in lens]}

    def device_heads():
        for hk in range(2):
            m2.logits(hk, m2.convnext(hk, rows_t, wr), wr)

    fns = {"tokens_batch_both_heads": lambda: m2.tokens_batch(waves, lens, reduce_head=1),
           "tokens_batch_one_head": lambda: m1.tokens_batch(waves, lens, reduce_head=0),
           "ssl_seam_18_layers": lambda: m2.ssl(wbuf, wl, out=rows_t),
           "loop_of_one_window_calls": lambda: [m2.tokens_batch(w, None, overlap_s=0.0) for w in one],
           "heads_alone_device": device_heads,
           "heads_alone_torch_fp16": lambda: torch_heads(rows16)}
    rec.update(timed_alternated(fns))
    m2.set_timing(True)
    split = []
    for _ in range(R):
        m2.tokens_batch(waves, lens, reduce_head=1)
        split.append(m2.last_timing())
    m2.set_timing(False)
    for k in m2.STAGES:
        rec["stage_" + k + "_last_group"] = stats([s[k] for s in split])
    rec["last_group_windows"] = len(wins) - ((len(wins) - 1) // GROUP) * GROUP
    rec["heads_added_ms"] = round(rec["tokens_batch_both_heads"]["ms"] - rec["ssl_seam_18_layers"]["ms"], 3)
    rec["loop_over_one_call"] = round(rec["loop_of_one_window_calls"]["ms"] / rec["tokens_batch_both_heads"]["ms"], 3)
    rec["torch_heads_over_device_heads"] = round(rec["heads_alone_torch_fp16"]["ms"] / rec["heads_alone_device"]["ms"], 3)
    rec["realtime_factor"] = round(sum(secs) * 1e3 / rec["tokens_batch_both_heads"]["ms"], 1)
    print(json.dumps(rec), flush=True)
    return rec


doc = {"tool": "tools/astral_bench.py", "label": args.label, "precision": args.precision,
       "model": "hubert-large geometry cut to 18 layers + 2 heads (12 ConvNeXt V2 blocks, dim 512 / 1536; 11 and 5 bits), random weights",
       "repeats": R, "torch": torch.__version__, "device": torch.cuda.get_device_name(0), "window_group": GROUP,
       "realtime_context_seconds": RT_SECONDS, "launches_per_block": 6,
       "records": [case("one real-time context", [RT_SECONDS]), case("64 real-time contexts", [RT_SECONDS] * 64),
                   case("one 30 s clip", [30.0]), case("8 ragged clips, 3 ... 25 s", [3.0, 25.0, 7.5, 12.0, 18.5, 5.0, 21.0, 9.0]),
                   case("one 600 s file (24 windows)", [600.0])]}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
