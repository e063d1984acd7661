"""Time to the first audio of long-form conversion: `convert_long_stream` (this commit) against `convert_long_batch` (the
parent commit's code path, whose first audio arrives when the call returns), in one run.

    python tools/long_stream_bench.py --out profiles/long_stream.json

v1 shapes, those of profiles/long_batched.json (small + WaveNet, BigVGAN 22 kHz, 25 steps, 430 prompt frames, 30 s windows,
max_chunks 8): one 70 s file, one 600 s file, eight 70 s files.  v2 shapes, those of profiles/v2_long.json (tools/v2_long_bench.py's
models, seeded): style branch one file of 8 chunks and eight files of 4; timbre branch one file of 8 windows and eight of 4.

Per shape: every variant is run twice untimed, then `--repeats` rounds in which the pool and the stream ALTERNATE.  The pool is
timed by HIP events around the call and by the host clock (the call ends in its own synchronisation).  The stream is timed by
the host clock only, in the consumer: the call, every piece in the consumer's hands (the consumer does nothing with it), the
last piece; the generator waits on its own events, the run ends in a device synchronisation that is not part of any figure.
    first_ms   call -> the first piece that holds samples
    every_file_ms  call -> the moment every file has had its first piece
    last_ms    call -> the last piece (compare with the pool's whole call)
    lag_ms     the largest time by which a piece comes later than a player that started a file at its first piece and plays
               at the sample rate would need it: max over pieces of (arrival - first arrival) - offset / rate, 0 if never late
medians and spreads (max - min) over the rounds.  Then the ramp, `first_chunks` x `growth` around the defaults, and `lookahead`
0 / 1 / 2 at the defaults: each configuration run twice untimed and `--sweep-repeats` times in rounds that alternate the
configurations.  Both paths draw from the same seeds, and the record gives the difference of their audio."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch
import cases
from seedvc_amd import specs, weights
from seedvc_amd.ar import ARModel
from seedvc_amd.cfm import CFM
from seedvc_amd.length_regulator import InterpolateRegulator
from seedvc_amd.pipeline import HotPath, V2HotPath, collect_stream
from seedvc_amd.vocoder import BigVGAN

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--sweep-repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--max-chunks", type=int, default=8, help="chunks per micro-batch, both paths (profiles/long_batched.json: 8)")
ap.add_argument("--v1", default="70x1,600x1,70x8", help="seconds x files of the v1 shapes")
ap.add_argument("--v2", default="1x8,8x4", help="files x chunks of the v2 shapes, each run on both branches ('' skips v2)")
ap.add_argument("--out", default="")
a = ap.parse_args()
R, STEPS = a.repeats, a.steps
torch.set_grad_enabled(False)
torch.manual_seed(0)
dev = "cuda:0"
SR, HOP, P, OV = 22050, 256, 430, 16
WINDOW = SR // HOP * 30


def sd_of(spec, seed, prefix):
    return weights.make_state_dict(spec, seed=seed, prefix=prefix)


def stats(ts):
    s = sorted(ts)
    return {"ms": round(s[len(s) // 2], 2), "spread_ms": round(s[-1] - s[0], 2), "runs_ms": [round(t, 2) for t in s]}


def run_pool(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    return dict(host_ms=host, event_ms=e0.elapsed_time(e1)), out


def run_stream(fn, n_files):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = [(p, time.perf_counter()) for p in fn()]
    torch.cuda.synchronize()
    first = {}
    lag, t_first = 0.0, None
    for p, t in got:
        if p.wave.size(1) and t_first is None:
            t_first = t
        start = first.setdefault(p.file, t)
        lag = max(lag, (t - start) - p.offset / SR)
    return dict(first_ms=((t_first if t_first is not None else got[-1][1]) - t0) * 1e3, every_file_ms=(max(first.values()) - t0) * 1e3,
                last_ms=(got[-1][1] - t0) * 1e3, lag_ms=lag * 1e3, pieces=len(got)), collect_stream([p for p, _ in got], n_files)


def measure(shape, n_files, seconds_out, pool, stream, defaults, sweep):
    """pool() -> waves; stream(first_chunks, growth, lookahead=1) -> generator.  -> the shape's record."""
    looks = [defaults + (la,) for la in (0, 1, 2)]
    for _ in range(2):
        pool()
        for cfg in [defaults] + sweep + looks:
            for _ in stream(*cfg):
                pass
    runs = {"pool": [], "stream": []}
    for _ in range(R):
        m, pool_out = run_pool(pool)
        runs["pool"].append(m)
        m, stream_out = run_stream(lambda: stream(*defaults), n_files)
        runs["stream"].append(m)
    col = lambda k, key: stats([r[key] for r in runs[k]])      # noqa: E731
    rec = dict(shape, files=n_files, output_seconds=round(seconds_out, 2), repeats=R, max_chunks=a.max_chunks, sampler_steps=STEPS,
               pool={"whole_call_host": col("pool", "host_ms"), "whole_call_events": col("pool", "event_ms")},
               stream={"first_chunks": defaults[0], "growth": defaults[1], "lookahead": 1, "first": col("stream", "first_ms"),
                       "every_file": col("stream", "every_file_ms"), "last": col("stream", "last_ms"), "lag": col("stream", "lag_ms"),
                       "pieces": runs["stream"][0]["pieces"]})
    a_, b_ = torch.cat([w.cpu() for w in pool_out], dim=1).double(), torch.cat(stream_out, dim=1).double()
    rec["stream_vs_pool_audio"] = ({"same_shape": True, "bit_identical": bool(torch.equal(a_, b_)),
                                    "rms_difference": float((a_ - b_).pow(2).mean().sqrt()), "signal_rms": float(a_.pow(2).mean().sqrt())}
                                   if a_.shape == b_.shape else {"same_shape": False, "samples": [a_.numel(), b_.numel()]})
    pw, sf, sl = rec["pool"]["whole_call_host"], rec["stream"]["first"], rec["stream"]["last"]
    rec["first_audio_pool_over_stream"] = round(pw["ms"] / sf["ms"], 2)
    rec["first_audio_before_the_pool_returns_by_more_than_the_spreads"] = bool(pw["ms"] - sf["ms"] > pw["spread_ms"] + sf["spread_ms"])
    rec["stream_total_over_pool_total"] = round(sl["ms"] / pw["ms"], 3)
    rec["stream_total_within_the_spreads_of_the_pool"] = bool(sl["ms"] - pw["ms"] <= pw["spread_ms"] + sl["spread_ms"])
    ts = {cfg: [] for cfg in sweep + looks}
    for _ in range(a.sweep_repeats):
        for cfg in sweep + looks:
            ts[cfg].append(run_stream(lambda: stream(*cfg), n_files)[0])
    row = lambda cfg: {k: stats([r[k + "_ms"] for r in ts[cfg]]) for k in ("first", "every_file", "last", "lag")}      # noqa: E731
    rec["ramp_sweep"] = [dict({"first_chunks": cfg[0], "growth": cfg[1]}, **row(cfg)) for cfg in sweep]
    rec["lookahead_sweep"] = [dict({"lookahead": cfg[2]}, **row(cfg)) for cfg in looks]
    print(json.dumps(rec), flush=True)
    return rec


def sweep_of(n_files):
    firsts = sorted({1, n_files, min(2 * n_files, a.max_chunks)})
    return [(fc, gr) for fc in firsts for gr in (1, 2, 4, 8)]


records = []
# ---------------------------------------------------------------------------------------------------------------- v1
cfg = specs.dit_config("small")
cfm = CFM(cfg, sd_of(specs.dit_state_spec(cfg), 1234, "dit.small."), dev)
vc = specs.bigvgan_config("22k")
voc = BigVGAN(vc, sd_of(specs.bigvgan_state_spec(vc), 1234, "bigvgan."), dev)
hp1 = HotPath(cfm, voc)
for shape in [s for s in a.v1.split(",") if s]:
    seconds, U = (float(v) for v in shape.split("x"))
    U = int(U)
    S = int(seconds * SR / HOP)
    utts = [(cases.randn(f"lb.cond{u}", 1, 1, S, cfg["Dc"]).to(dev), cases.randn(f"lb.pc{u}", 1, 1, P, cfg["Dc"]).to(dev),
             cases.logmel(f"lb.mel2{u}", 1, 1, cfg["C"], P).to(dev), cases.randn(f"lb.style{u}", 1, 1, cfg["style_dim"]).to(dev))
            for u in range(U)]
    seeds = list(range(100, 100 + U))
    pool = lambda: hp1.convert_long_batch(utts, STEPS, 0.7, HOP, WINDOW, max_chunks=a.max_chunks, seeds=seeds)      # noqa: E731
    stream = lambda fc, gr, la=1: hp1.convert_long_stream(utts, STEPS, 0.7, HOP, WINDOW, max_chunks=a.max_chunks, seeds=seeds,      # noqa: E731
                                                          first_chunks=fc, growth=gr, lookahead=la)
    records.append(measure({"workload": f"v1: {U} file(s) of {seconds:g} s", "model": "small + WaveNet, BigVGAN 22k"}, U, seconds * U,
                           pool, stream, (None, 4), sweep_of(U)))
del cfm, hp1

# ---------------------------------------------------------------------------------------------------------------- v2
v2_loads = [tuple(int(v) for v in w.split("x")) for w in a.v2.split(",") if w]
if v2_loads:
    N_TOK, CT = 256, 80
    ac = specs.ar_config()
    ar = ARModel(ac, sd_of(specs.ar_state_spec(ac), 7, "ar."), dev)
    ar.setup_caches(max_batch_size=max([min(f * c, 64) for f, c in v2_loads] + [2]))
    alc, clc = specs.lr_config("v2_ar"), specs.lr_config("v2_cfm")
    dc = specs.dit_config("v2")
    cfm2 = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.v2."), dev)
    cfm_lr = InterpolateRegulator(clc, sd_of(specs.lr_state_spec(clc), 6, "lr."), dev)
    hp2 = V2HotPath(ar, InterpolateRegulator(alc, sd_of(specs.lr_state_spec(alc), 5, "lr."), dev), cfm_lr, cfm2, voc)
    g = torch.Generator().manual_seed(1)
    target = hp2.prepare_target(torch.randint(0, 32, (1, 40), generator=g), torch.randint(0, 2048, (1, 200), generator=g),
                                (torch.randn(1, dc["C"], P, generator=g) * 2 - 4).clamp(-11.5, 2), torch.randn(1, dc["style_dim"], generator=g))
    for n_files, n_chunks in v2_loads:
        seeds = list(range(2000, 2000 + n_files))
        frames = (WINDOW - P) + (n_chunks - 1) * (WINDOW - P - OV) - 7          # n_chunks windows, the last one nearly full
        files = [dict(target=target, src_narrow=torch.randint(0, 32, (1, CT * n_chunks), generator=g).to(dev),
                      src_tokens=torch.randint(0, 2048, (1, frames * 50 * HOP // SR), generator=g).to(dev), frames_per_token=P / N_TOK,
                      source_frames=frames) for _ in range(n_files)]
        for branch, style in (("style", True), ("timbre", False)):
            kw = dict(convert_style=style, max_context_window=WINDOW, hop=HOP, overlap_frame_len=OV, seeds=seeds, max_chunks=a.max_chunks)
            if style:
                kw.update(ar_chunk_tokens=CT, max_new=N_TOK)
            pool = lambda: hp2.convert_long_batch(files, STEPS, (0.7, 0.7), **kw)      # noqa: E731
            stream = lambda fc, gr, la=1: hp2.convert_long_stream(files, STEPS, (0.7, 0.7), first_chunks=fc, growth=gr,      # noqa: E731
                                                                  lookahead=la, **kw)
            out_s = sum(int(w.size(1)) for w in pool()) / SR
            records.append(measure({"workload": f"v2 {branch} branch: {n_files} file(s) of {n_chunks} chunks", "ar_slots": ar.max_batch_size,
                                    "model": "ar_base, v2 DiT, BigVGAN 22k"}, n_files, out_s, pool, stream, (None, 4), sweep_of(n_files)))

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/long_stream_bench.py", "command": "python tools/long_stream_bench.py --out profiles/long_stream.json",
                   "records": records}, f, indent=1)
        f.write("\n")
