"""One block step of a real-time session with RMVPE on the context's tail: the configuration of
tools/rt_pitch_bench.py (XLS-R-size wav2vec 2.0, f0-conditioned regulator, tiny DiT + HiFT, 10 sampler steps, cfg 0.7, model at
22.05 kHz, block 0.18 s, 48 kHz in, full-size RMVPE, random weights).

For every B of `--batch` (default 1,64) one JSON line.
(a) Engines that alternate step by step in one process, on the same audio, noise and HiFT draws:
  full       `step_audio` after `attach_pitch`: `rmvpe.f0_batch` on the whole 16 kHz context, one `svc_rt_pitch` (the baseline)
  win<W>     the same after `set_pitch_window(W, --guard)` for every W of `--windows` (64,96,128): `f0_batch` on the last W frames,
             one `svc_rt_pitch_win`
  pitch_off  the same engine without `attach_pitch`
  Per step and path: HIP-event time, host wall time up to the final synchronise, host time until the call returned.
  The timed steps run with return_parts=False, as a block loop does.  `--warmup` (2) untimed rounds, `--rounds` (5) timed ones, the
  order of the variants rotating from round to round; median and spread (max - min).  No target was fixed in advance.
(b) The stages alone, around `--inner` (20) back-to-back calls / `--inner`: `f0_batch` on the context and on each tail,
  `svc_rt_pitch` and `svc_rt_pitch_win` (window 64, with and without a memory of 300 frames); HIP-event time and host time until
  the calls returned; the same rounds and warm-ups, in turn.
`--out FILE` writes the lines to FILE as one JSON document."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _pkgload
_pkgload.load_package()
import numpy as np
import torch
import rmvpe_cases as RV
import w2v_cases as VC
from seedvc_amd import specs, weights
from seedvc_amd.audio import Resample
from seedvc_amd.cfm import CFM
from seedvc_amd.length_regulator import InterpolateRegulator
from seedvc_amd.pipeline import RealtimeEngine, realtime_geometry, realtime_input_geometry
from seedvc_amd.rmvpe import RMVPE, rt_pitch, rt_pitch_cache, rt_pitch_ring, rt_pitch_state, rt_pitch_win
from seedvc_amd.vocoder import HiFT
from seedvc_amd.wav2vec2 import Wav2Vec2Content

ap = argparse.ArgumentParser()
ap.add_argument("--batch", default="1,64")
ap.add_argument("--windows", default="64,96,128")
ap.add_argument("--guard", type=int, default=16)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--prompt", type=int, default=258)
ap.add_argument("--out", default="")
args = ap.parse_args()
sizes, windows = [int(b) for b in args.batch.split(",")], [int(w) for w in args.windows.split(",")]
R, STEPS, P, CFG = args.rounds, args.steps, args.prompt, 0.7

assert torch.cuda.is_available(), "rt_pitch_win_bench.py measures on the GPU; there is no fallback"
torch.set_grad_enabled(False)
dev = "cuda:0"
SR, SR_IO, CE_DIT = 22050, 48000, 2.0
dc, hc, wc = specs.dit_config("tiny"), specs.hift_config(), specs.wav2vec2_config()
lc = specs.lr_config("tiny", in_channels=wc["d_model"], f0_condition=True, n_f0_bins=256)
HOP = specs.hift_total_upsample(hc)
GEO = realtime_geometry(SR, HOP, 0.18, 0.04, 2.5, 0.02, CE_DIT)
GIN = realtime_input_geometry(SR_IO, 0.18, 0.04, 2.5, 0.02)
S, BLOCK, LB, LS = (GEO[k] for k in ("S", "block", "Lb", "Ls"))
ZC, Z16, LIN, L16 = (GIN[k] for k in ("zc", "z16", "Lin", "L16"))
sd_of = lambda spec, seed, prefix: weights.make_state_dict(spec, seed=seed, prefix=prefix)      # noqa: E731
cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.tiny."), dev)
lr = InterpolateRegulator(lc, sd_of(specs.lr_state_spec(lc), 6, "lr."), dev)
voc = HiFT(hc, sd_of(specs.hift_state_spec(hc), 1234, "hift."), dev)
w2v = Wav2Vec2Content(VC.make_state_dict(wc, seed=22), cfg=wc, device=dev, precision=1)
rcfg, rsd, _ = RV.model("full")
rm = RMVPE(rsd, mel_basis=RV.basis(), device=dev, cfg=rcfg)
rs_in = Resample(SR_IO, 16000, device=dev)
Cm, Dc, NH = dc["C"], dc["Dc"], hc["nb_harmonics"] + 1


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 4), "spread_ms": round(ts[-1] - ts[0], 4)}


def measure(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return out, a.elapsed_time(b), (t2 - t0) * 1e3, (t1 - t0) * 1e3


records = []
for B in sizes:
    g = torch.Generator().manual_seed(B)
    ref = ((torch.randn(1, P, Dc, generator=g)).to(dev), (torch.randn(1, Cm, P, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev),
           torch.randn(1, dc["style_dim"], generator=g).to(dev))
    f0_ref = rm.f0_batch(RV.clip(1, 3 * 16000)[None].to(dev))
    names = ["full"] + [f"win{w}" for w in windows] + ["pitch_off"]
    engines = {}
    for name in names:
        eng = RealtimeEngine(lr, cfm, voc, S, HOP, BLOCK, LB, LS, tail=GEO["tail"], max_streams=B)
        eng.attach_audio(w2v, rs_in, LIN, L16, CE_DIT)
        if name != "pitch_off":
            eng.attach_pitch(rm)
        if name.startswith("win"):
            eng.set_pitch_window(int(name[3:]), args.guard)
        slots = [eng.open(*ref) for _ in range(B)]
        if name != "pitch_off":
            for s in slots:
                eng.set_reference_f0(s, f0_ref)
                eng.set_pitch(s, semitones=2.0)
        engines[name] = eng
    # four blocks in turn: a gliding harmonic tone per stream (voiced for RMVPE) at 48 kHz
    t = torch.arange(4 * LIN).double() / SR_IO
    hz = 110.0 * (1.0 + torch.arange(B).double()[:, None] % 5) * (1.0 + 0.2 * torch.sin(2 * np.pi * 1.5 * t)[None, :])
    ph = 2 * np.pi * torch.cumsum(hz, 1) / SR_IO
    tone = (sum(torch.sin(h * ph) / h for h in range(1, 6)) * 0.2).float() + torch.randn(B, 4 * LIN, generator=g) * 0.02
    audio = [tone[:, k * LIN:(k + 1) * LIN].contiguous().to(dev) for k in range(4)]
    zs = [torch.randn(B, Cm, P + S, generator=g).to(dev) for _ in range(4)]
    draws = dict(phase0=((torch.rand(B, NH, 1, generator=g) * 2 - 1) * float(np.pi)).to(dev), noise=torch.randn(B, NH, S * HOP, generator=g).to(dev))

    per = {p: {"event": [], "wall": [], "enqueue": []} for p in names}
    for k in range(args.warmup + R):
        x, z = audio[k % 4], zs[k % 4]
        for path in names[k % len(names):] + names[:k % len(names)]:
            out, ev, wall, enq = measure(lambda: engines[path].step_audio(slots, x, STEPS, CFG, z=z, vocoder_kwargs=draws))
            if k >= args.warmup:
                per[path]["event"].append(ev)
                per[path]["wall"].append(wall)
                per[path]["enqueue"].append(enq)
    k = args.warmup + R
    parts = {n: engines[n].step_audio(slots, audio[k % 4], STEPS, CFG, z=zs[k % 4], vocoder_kwargs=draws, return_parts=True)[1] for n in names}
    voiced_share = float((parts["full"]["f0_raw"] > 1).float().mean())

    # ---- (b) the stages alone
    ctx = parts["full"]["ctx"]
    p = engines["full"]._pitch
    Tf = p["Tf"]
    raw = rm.f0_batch(ctx)
    tails = {w: ctx[:, 160 * (Tf - w):].contiguous() for w in windows}
    W0 = windows[0]
    win0 = rm.f0_batch(tails[W0])
    own = {m: dict(state=rt_pitch_state(B, dev), cache=rt_pitch_cache(B, Tf, dev), ring=rt_pitch_ring(B, m, dev)) for m in (0, 300)}
    state = rt_pitch_state(B, dev)

    def f0_rounds(x):
        return lambda n: [rm.f0_batch(x) for _ in range(n)] and None

    def pitch_rounds(n):
        for _ in range(n):
            rt_pitch(raw, p["n_new"], p["lag"], slots, state, p["ref_median"], [1] * B, [2.0] * B, warmup=p["warmup"], max_step=p["max_step"])

    def win_rounds(m):
        def run(n):
            o = own[m]
            for _ in range(n):
                rt_pitch_win(win0, args.guard, p["n_new"], p["lag"], slots, o["cache"], o["ring"], o["state"], p["ref_median"], [1] * B,
                             [2.0] * B, warmup=p["warmup"], max_step=p["max_step"])
        return run

    stages = {f"f0_batch_on_the_context_{Tf}_frames": f0_rounds(ctx)}
    stages.update({f"f0_batch_on_the_last_{w}_frames": f0_rounds(tails[w]) for w in windows})
    stages.update({"svc_rt_pitch": pitch_rounds, f"svc_rt_pitch_win_window_{W0}": win_rounds(0),
                   f"svc_rt_pitch_win_window_{W0}_memory_300": win_rounds(300)})
    alone = {n: {"event": [], "host": []} for n in stages}
    for r in range(args.warmup + R):
        for name, fn in stages.items():
            _, ev, _, enq = measure(lambda: fn(args.inner))
            if r >= args.warmup:
                alone[name]["event"].append(ev / args.inner)
                alone[name]["host"].append(enq / args.inner)
    steps = {n: {k: stats(v) for k, v in per[n].items()} for n in names}
    block_ms = round(LIN / SR_IO * 1e3, 2)
    rec = {"workload": "real-time block step with pitch: 48 kHz in, XLS-R-size wav2vec 2.0 (12 layers) + f0-conditioned regulator + tiny DiT + "
                       "HiFT at 22.05 kHz, 10 steps, cfg 0.7, block 0.18 s, full-size RMVPE on the whole 16 kHz context or on its tail",
           "B": B, "rounds": R, "warmup": args.warmup, "sampler_steps": STEPS, "prompt_frames": P, "geometry": GEO, "input_geometry": GIN,
           "context_samples_16k": L16, "f0_frames_per_context": Tf, "frames_counted_per_block": p["n_new"], "lag_frames": p["lag"],
           "guard_frames": args.guard, "windows": windows, "block_ms_of_audio": block_ms, "step_audio": steps,
           "minus_full_ms": {n: {k: round(steps[n][k]["ms"] - steps["full"][k]["ms"], 4) for k in ("event", "wall", "enqueue")} for n in names},
           "share_of_the_block": {n: round(steps[n]["wall"]["ms"] / block_ms, 4) for n in names},
           "voiced_share_of_the_last_track": round(voiced_share, 4),
           "stages_alone_per_call": {n: {k: stats(v) for k, v in d.items()} for n, d in alone.items()},
           "note": "stages alone: HIP events around back-to-back calls / their number, host = time until the calls returned / their "
                   "number; the same rounds and warm-ups, in turn"}
    print(json.dumps(rec), flush=True)
    records.append(rec)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        command = (f"python tools/rt_pitch_win_bench.py --batch {args.batch} --windows {args.windows} --guard {args.guard} --rounds {R} "
                   f"--warmup {args.warmup} --inner {args.inner} --steps {STEPS} --prompt {P}")
        json.dump({"tool": "tools/rt_pitch_win_bench.py", "command": command, "records": records}, f, indent=1)
