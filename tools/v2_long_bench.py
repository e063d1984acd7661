"""Whole-file v2 conversion, `V2HotPath.convert_long_batch`, on the full-size models and the token-count arrangement of
tools/v2_bench.py: ar_base (40 target + 80 source narrow tokens per chunk = 120 condition frames, 200 prompt tokens, up to
256 new tokens, seeded), v2 length regulators, v2 DiT with 25 steps and CFG (0.7, 0.7), 430 prompt frames, BigVGAN 22k.

Style branch, two workloads: one file of 8 chunks, and eight files of 4 chunks.  The pool against the reference's loop
structure, which is NOT the code under test: the same chunks converted one after the other with `V2HotPath.convert_batch` at
B = 1 (same derived seeds) and spliced by host `stream_wave_chunks`.  Timbre branch: one 600 s file (30000 wide tokens ->
51679 frames, 30 s windows) against `HotPath.convert_long_batch` fed the regulator's output of the same tokens.

Per workload one JSON line: the two variants timed alternately by a host clock around calls that end in a device
synchronisation, two warm-up runs and `--repeats` (5) timed runs each, median and spread (max - min); the stages of the pool
from HIP events inside the call (`V2HotPath.marks`); in how many chunks the loop produced the pool's tokens (the session's
ragged prefill and the per-slot prefill agree to the logit bound, not bit for bit, and with random weights a near-tie can
flip a free-running token: the count is given for the loop with either prefill), and the difference of the waves.  The
timbre baseline is handed the regulator's output, so the record also compares it with the pool's share of the call alone.
`--out FILE` writes the lines to FILE as one JSON document."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
import numpy as np
import torch
from seedvc_amd import specs, weights
from seedvc_amd.ar import ARModel
from seedvc_amd.cfm import CFM
from seedvc_amd.length_regulator import InterpolateRegulator
from seedvc_amd.pipeline import HotPath, V2HotPath, derive_seed, stream_wave_chunks, v2_chunk_plan, v2_seam_plan
from seedvc_amd.vocoder import BigVGAN

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tokens", type=int, default=256, help="cap of new tokens per chunk")
ap.add_argument("--chunk-tokens", type=int, default=80, help="source narrow tokens per chunk")
ap.add_argument("--frames", type=int, default=430, help="prompt frames; generated frames of a chunk that reaches the cap")
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--style", default="1x8,8x4", help="files x chunks of the style workloads")
ap.add_argument("--seconds", type=float, default=600.0, help="length of the timbre workload's file (0: skip it)")
ap.add_argument("--out", default="")
args = ap.parse_args()
R, N_TOK, CT, P, STEPS = args.repeats, args.tokens, args.chunk_tokens, args.frames, args.steps
style_loads = [tuple(int(v) for v in w.split("x")) for w in args.style.split(",") if w]

torch.set_grad_enabled(False)
torch.manual_seed(0)
dev = "cuda:0"
SR, HOP, OV = 22050, 256, 16
WINDOW = SR // HOP * 30


def sd_of(spec, seed, prefix):
    return weights.make_state_dict(spec, seed=seed, prefix=prefix)


ac = specs.ar_config()
ar = ARModel(ac, sd_of(specs.ar_state_spec(ac), 7, "ar."), dev)
ar.setup_caches(max_batch_size=max([min(f * c, 64) for f, c in style_loads] + [2]))
alc, clc = specs.lr_config("v2_ar"), specs.lr_config("v2_cfm")
dc = specs.dit_config("v2")
vh = specs.bigvgan_config("22k")
assert specs.bigvgan_total_upsample(vh) == HOP
cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.v2."), dev)
voc = BigVGAN(vh, sd_of(specs.bigvgan_state_spec(vh), 1234, "bigvgan."), dev)
cfm_lr = InterpolateRegulator(clc, sd_of(specs.lr_state_spec(clc), 6, "lr."), dev)
hp = V2HotPath(ar, InterpolateRegulator(alc, sd_of(specs.lr_state_spec(alc), 5, "lr."), dev), cfm_lr, cfm, voc)
Cm = dc["C"]
FPT = P / N_TOK
g = torch.Generator().manual_seed(1)
target = hp.prepare_target(torch.randint(0, 32, (1, 40), generator=g), torch.randint(0, 2048, (1, 200), generator=g),
                           (torch.randn(1, Cm, P, generator=g) * 2 - 4).clamp(-11.5, 2), torch.randn(1, dc["style_dim"], generator=g))


def stats(ts):
    s = sorted(ts)
    return {"ms": round(s[len(s) // 2], 2), "spread_ms": round(s[-1] - s[0], 2), "runs_ms": [round(t, 2) for t in s]}


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def alternate(variants):
    """{name: fn} -> ({name: [ms]}, {name: last result}): two warm-up rounds, then R timed rounds, the variants in turn."""
    ts, outs = {k: [] for k in variants}, {}
    for i in range(2 + R):
        for k, fn in variants.items():
            ms, outs[k] = clocked(fn)
            if i >= 2:
                ts[k].append(ms)
    return ts, outs


def stages(fn, names):
    """Median HIP-event time of the pool's stages over R runs (micro-batches add up)."""
    per = {k: [] for k in names}
    for _ in range(R):
        torch.cuda.synchronize()
        hp.marks = []
        fn()
        torch.cuda.synchronize()
        marks, hp.marks = hp.marks, None
        acc = dict.fromkeys(names, 0.0)
        for (_, a), (name, b) in zip(marks, marks[1:]):
            acc[name] += a.elapsed_time(b)
        for k in names:
            per[k].append(acc[k])
    return {k: {"ms": round(sorted(v)[len(v) // 2], 2), "spread_ms": round(max(v) - min(v), 2)} for k, v in per.items()}


def compare(a, b):
    a, b = a.reshape(-1).double().cpu(), b.reshape(-1).double().cpu()
    if a.shape != b.shape:
        return {"same_shape": False, "samples": [a.numel(), b.numel()]}
    return {"same_shape": True, "bit_identical": bool(torch.equal(a, b)), "rms_difference": float((a - b).pow(2).mean().sqrt()),
            "signal_rms": float(b.pow(2).mean().sqrt())}


records = []
for n_files, n_chunks in style_loads:
    files = [dict(target=target, src_narrow=torch.randint(0, 32, (1, CT * n_chunks), generator=g).to(dev), src_tokens=None,
                  frames_per_token=FPT, source_frames=0) for _ in range(n_files)]
    seeds = list(range(2000, 2000 + n_files))
    kw = dict(max_context_window=WINDOW, hop=HOP, ar_chunk_tokens=CT, overlap_frame_len=OV, max_new=N_TOK, seeds=seeds)
    pool = lambda: hp.convert_long_batch(files, STEPS, (0.7, 0.7), **kw)      # noqa: E731
    tokens = {}

    def loop():
        """The reference's loop structure: chunk after chunk at B = 1, host splice; the seam rule applied to the lengths."""
        out = []
        for u, f in enumerate(files):
            plan = v2_chunk_plan(f["src_narrow"].size(1), CT)
            parts = [hp.convert_batch([f["src_narrow"][:, p0:p0 + n]], [target], [FPT], STEPS, cfg_rates=(0.7, 0.7), max_new=N_TOK,
                                      seeds=[derive_seed(seeds[u], k)], noise_seeds=[derive_seed(seeds[u], k)])[0]
                     for k, (p0, n, _) in enumerate(plan)]
            tokens[u] = [p["tokens"] for p in parts]
            seam = v2_seam_plan([0] * len(parts), [p["wave"].size(1) for p in parts], [c[2] for c in plan], OV * HOP, 1)
            kept = [p for p, keep in zip(parts, seam["kept"]) if keep]
            chunks, previous, processed = [], None, 0
            for i, p in enumerate(kept):
                processed, previous, _ = stream_wave_chunks(p["wave"], processed, p["mel"].size(2), OV * HOP, OV, chunks, previous,
                                                            i == len(kept) - 1)
            out.append(torch.from_numpy(np.concatenate(chunks))[None] if chunks else torch.zeros(1, 0))
        return out

    ts, outs = alternate({"pool": pool, "loop_b1": loop})
    _, parts = hp.convert_long_batch(files, STEPS, (0.7, 0.7), return_parts=True, **kw)
    n_tok = [int(p["tokens"].size(1)) for ps in parts for p in ps]
    pool_tokens = [p["tokens"] for ps in parts for p in ps]
    same = {}
    for prefill in ("slot", "ragged"):          # untimed: the loop's tokens with either prefill of `convert_batch` (the timed loop ran the default)
        hp.ar_prefill = prefill
        loop()
        same[prefill] = sum(int(torch.equal(a, b)) for a, b in zip(pool_tokens, [t for u in range(n_files) for t in tokens[u]]))
    hp.ar_prefill = "slot"
    samples = sum(int(w.size(1)) for w in outs["pool"])
    rec = {"workload": f"style branch: {n_files} file(s) of {n_chunks} chunks", "files": n_files, "chunks": n_files * n_chunks,
           "ar_slots": ar.max_batch_size, "repeats": R, "sampler_steps": STEPS, "tokens_per_chunk": [min(n_tok), max(n_tok)],
           "chunks_kept": sum(int(p["kept"]) for ps in parts for p in ps), "output_seconds": round(samples / SR, 2),
           "pool": stats(ts["pool"]), "loop_b1": stats(ts["loop_b1"]),
           "pool_stages": stages(pool, ("ar", "lr_assembly", "cfm", "strip_vocoder", "assemble")),
           "chunks_with_the_pools_tokens": {"loop_slot_prefill": same["slot"], "loop_ragged_prefill": same["ragged"]},
           "pool_vs_loop": [compare(a, b) for a, b in zip(outs["pool"], outs["loop_b1"])][:2]}
    rec["loop_over_pool"] = round(rec["loop_b1"]["ms"] / rec["pool"]["ms"], 3)
    rec["pool_below_loop_by_more_than_the_spreads"] = bool(rec["loop_b1"]["ms"] - rec["pool"]["ms"] > rec["loop_b1"]["spread_ms"] + rec["pool"]["spread_ms"])
    rec["pool_x_real_time"] = round(samples / SR / rec["pool"]["ms"] * 1e3, 1)
    print(json.dumps(rec), flush=True)
    records.append(rec)

if args.seconds > 0:
    frames = int(args.seconds * SR) // HOP
    wide = torch.randint(0, 2048, (1, int(args.seconds * 50)), generator=g).to(dev)
    files = [dict(target=target, src_narrow=None, src_tokens=wide, frames_per_token=0.0, source_frames=frames)]
    kw = dict(convert_style=False, max_context_window=WINDOW, hop=HOP, overlap_frame_len=OV, seeds=[77], max_chunks=8)
    pool = lambda: hp.convert_long_batch(files, STEPS, (0.7, 0.7), **kw)      # noqa: E731
    cond = cfm_lr(wide, ylens=torch.LongTensor([frames]))[0]
    v1 = HotPath(cfm, voc)
    base = lambda: v1.convert_long_batch([(cond, target["prompt_condition"], target["mel"], target["style"])], STEPS, [0.7, 0.7], HOP,      # noqa: E731
                                         WINDOW, overlap_frame_len=OV, seeds=[77], max_chunks=8, ragged_vocoder=True)
    ts, outs = alternate({"pool": pool, "v1_pool_given_cond": base})
    rec = {"workload": f"timbre branch: one file of {args.seconds:g} s", "wide_tokens": int(wide.size(1)), "source_frames": frames,
           "window_frames": WINDOW, "max_chunks": 8, "repeats": R, "sampler_steps": STEPS,
           "pool": stats(ts["pool"]), "v1_pool_given_cond": stats(ts["v1_pool_given_cond"]),
           "pool_stages": stages(pool, ("lr_assembly", "pool")), "pool_vs_v1": compare(outs["pool"][0], outs["v1_pool_given_cond"][0])}
    d = abs(rec["pool"]["ms"] - rec["v1_pool_given_cond"]["ms"])
    rec["equal_inside_the_spreads"] = bool(d <= rec["pool"]["spread_ms"] + rec["v1_pool_given_cond"]["spread_ms"])
    share = rec["pool_stages"]["pool"]
    rec["pool_stage_equal_inside_the_spreads"] = bool(abs(share["ms"] - rec["v1_pool_given_cond"]["ms"])
                                                      <= share["spread_ms"] + rec["v1_pool_given_cond"]["spread_ms"])
    rec["pool_x_real_time"] = round(args.seconds / rec["pool"]["ms"] * 1e3, 1)
    print(json.dumps(rec), flush=True)
    records.append(rec)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/v2_long_bench.py", "records": records}, f, indent=1)
        f.write("\n")
