"""Long-form conversion, small+WaveNet + BigVGAN-22k, 25 steps, P = 430 prompt frames, 30 s window:

  host loop    `HotPath.convert_long`:        one B = 1 sampler + vocoder call per chunk, crossfade on the host;
  device loop  `HotPath.convert_long_device`: the same calls, crossfade on the device, vocoder of chunk k beside the
               sampler of chunk k + 1 on a second stream;
  batched      `HotPath.convert_long_batch`:  the chunks of all utterances as ragged batches of `--max-chunks` chunks,
               one launch to cross-fade and concatenate them.

A case is `--seconds` of source audio x `--utterances` files (several cases: give several values to both).  The two loops
convert the files one after the other.  Per case: 2 warm-up rounds, then `--repeats` rounds in which the paths ALTERNATE
(device events around each call; the calls end in a synchronisation of their own), median and spread (max - min) per path,
and the RMS difference of the batched output to the device loop's on the same pinned noise.  `--no-host-loop` leaves the
host loop out.  On a commit without `convert_long_batch` the tool reports the loops only; `--parent FILE` embeds such a
record, labelled.  `--out FILE` writes the JSON document."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
import cases
from seedvc_amd import specs, weights
from seedvc_amd.cfm import CFM
from seedvc_amd.vocoder import BigVGAN
from seedvc_amd.pipeline import HotPath, chunk_plan

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, nargs="+", default=[70.0])
ap.add_argument("--utterances", type=int, nargs="+", default=[1])
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--max-chunks", type=int, default=8,
                help="chunks per micro-batch of the batched path (8 x 30 s windows: about the rows per pass of the B = 64 benchmark)")
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--no-host-loop", action="store_true")
ap.add_argument("--label", default="this commit")
ap.add_argument("--parent", default="", help="JSON written by this tool on the parent commit")
ap.add_argument("--out", default="")
a = ap.parse_args()
if len(a.seconds) != len(a.utterances):
    ap.error("--seconds and --utterances need one value per case")
torch.set_grad_enabled(False)
dev = "cuda:0"
cfg = specs.dit_config("small")
cfm = CFM(cfg, weights.make_state_dict(specs.dit_state_spec(cfg), seed=1234, prefix="dit.small."), dev)
vc = specs.bigvgan_config("22k")
voc = BigVGAN(vc, weights.make_state_dict(specs.bigvgan_state_spec(vc), seed=1234, prefix="bigvgan."), dev)
hop, P = 256, 430
window = 22050 // hop * 30
hp = HotPath(cfm, voc)
has_batch = hasattr(HotPath, "convert_long_batch")
noise = lambda T: torch.randn(1, cfg["C"], T, device=dev, generator=torch.Generator(device=dev).manual_seed(T))      # noqa: E731


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 2), "spread_ms": round(ts[-1] - ts[0], 2), "runs_ms": [round(t, 2) for t in ts]}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


records = []
for seconds, U in zip(a.seconds, a.utterances):
    S = int(seconds * 22050 / hop)
    utts = [(cases.randn(f"lb.cond{u}", 1, 1, S, cfg["Dc"]).to(dev), cases.randn(f"lb.pc{u}", 1, 1, P, cfg["Dc"]).to(dev),
             cases.logmel(f"lb.mel2{u}", 1, 1, cfg["C"], P).to(dev), cases.randn(f"lb.style{u}", 1, 1, cfg["style_dim"]).to(dev))
            for u in range(U)]
    loop = lambda fn: [fn(*t, a.steps, 0.7, hop, window, noise_fn=noise) for t in utts]      # noqa: E731
    paths = {}
    if not a.no_host_loop:
        paths["host_loop"] = lambda: loop(hp.convert_long)
    paths["device_loop"] = lambda: loop(hp.convert_long_device)
    if has_batch:
        paths["batched"] = lambda: hp.convert_long_batch(utts, a.steps, 0.7, hop, window, noise_fn=noise, max_chunks=a.max_chunks)
    times, outs = {k: [] for k in paths}, {}
    for r in range(2 + a.repeats):
        for k, fn in paths.items():
            ms, outs[k] = timed(fn)
            if r >= 2:
                times[k].append(ms)
    n_chunks = len(chunk_plan(S, window - P, 16))
    rec = {"label": a.label, "model": "small + WaveNet, BigVGAN 22k", "steps": a.steps, "prompt_frames": P, "window_frames": window,
           "seconds": seconds, "utterances": U, "source_frames": S, "chunks": n_chunks * U, "repeats": a.repeats,
           "samples_per_utterance": int(outs["device_loop"][0].shape[-1])}
    for k in paths:
        rec[k] = stats(times[k])
        rec[k]["x_real_time"] = round(seconds * U / (rec[k]["ms"] * 1e-3), 1)
    if has_batch:
        rec["max_chunks"] = a.max_chunks
        d, b = torch.cat(outs["device_loop"], dim=1), torch.cat(outs["batched"], dim=1)
        rec["batched_vs_device_loop"] = {"same_shape": d.shape == b.shape, "rms_difference": (d - b).pow(2).mean().sqrt().item(),
                                         "signal_rms": d.pow(2).mean().sqrt().item(), "bit_identical": bool(torch.equal(d, b))}
        gain = rec["device_loop"]["ms"] - rec["batched"]["ms"]
        rec["device_loop_over_batched"] = round(rec["device_loop"]["ms"] / rec["batched"]["ms"], 3)
        rec["batched_below_device_loop_by_more_than_the_spreads"] = bool(
            gain > rec["device_loop"]["spread_ms"] + rec["batched"]["spread_ms"])
    records.append(rec)
    print(json.dumps(rec), flush=True)
doc = {"tool": "tools/long_bench.py", "records": records}
if a.parent:
    with open(a.parent) as f:
        doc["parent_records"] = json.load(f)["records"]
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
