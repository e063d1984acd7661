"""One block step of a real-time session FROM AUDIO, the published configuration of the reference GUI (tools/rt_bench.py: tiny
DiT + HiFT, 10 sampler steps, cfg 0.7, 22.05 kHz, block 0.18 s, crossfade 0.04 s, extra context 2.5 s / 0.02 s, ce_dit_difference
2.0) with an XLS-R-size wav2vec 2.0 content encoder (12 layers, random weights) in front: `realtime_input_geometry` gives blocks of
3969 samples and a 16 kHz context of 44160.

For every B of `--batch` (default 1,64) one JSON line with two paths that alternate step by step in one process, on the same audio,
noise and HiFT draws:
  engine  `RealtimeEngine.step_audio`: `svc_rt_push`, `semantic_fn`, `step`
  torch   what a user of the library writes without it: the GUI's `input_wav` / `input_wav_res` lines on device tensors (one row
          per stream, every statement once for all streams: the kindest reading for torch), `audio.Resample` as the resampler,
          then `semantic_fn` on the ring and `RealtimeEngine.step`
Per step and path: HIP-event time, host wall time up to the final synchronise, and the host time until the call returned
(enqueue).  `--warmup` (3) untimed steps per path, `--repeats` (30) timed ones; median and spread (max - min) of each figure, and
whether the difference of the medians exceeds the sum of the spreads.  `push_alone`: the input stage by itself, `svc_rt_push` against
the torch lines for all streams at once and against the same lines stream by stream (HIP events around 50 back-to-back rounds / 50,
and the host time of one round).  `same_output`: the two paths' contexts and last blocks compared.  `--out FILE` writes the lines to
FILE as one JSON document."""
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
import w2v_cases as VC
from seedvc_amd import _lib, specs, weights
from seedvc_amd.audio import Resample
from seedvc_amd.cfm import CFM
from seedvc_amd.length_regulator import InterpolateRegulator
from seedvc_amd.pipeline import RealtimeEngine, gui_fade_windows, realtime_geometry, realtime_input_geometry
from seedvc_amd.vocoder import HiFT
from seedvc_amd.wav2vec2 import Wav2Vec2Content

ap = argparse.ArgumentParser()
ap.add_argument("--batch", default="1,64")
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--prompt", type=int, default=258)
ap.add_argument("--out", default="")
args = ap.parse_args()
sizes = [int(b) for b in args.batch.split(",")]
R, STEPS, P, CFG = args.repeats, args.steps, args.prompt, 0.7

assert torch.cuda.is_available(), "rt_audio_bench.py measures on the GPU; there is no fallback"
torch.set_grad_enabled(False)
dev = "cuda:0"
SR, CE_DIT = 22050, 2.0
dc, hc, wc = specs.dit_config("tiny"), specs.hift_config(), specs.wav2vec2_config()
lc = specs.lr_config("tiny", in_channels=wc["d_model"])
HOP = specs.hift_total_upsample(hc)
GEO = realtime_geometry(SR, HOP, 0.18, 0.04, 2.5, 0.02, CE_DIT)
GIN = realtime_input_geometry(SR, 0.18, 0.04, 2.5, 0.02)
S, BLOCK, LB, LS = (GEO[k] for k in ("S", "block", "Lb", "Ls"))
ZC, Z16, LIN, L16 = (GIN[k] for k in ("zc", "z16", "Lin", "L16"))
M = LIN // ZC
TOTAL = L16 // Z16 * ZC                                      # len(input_wav)
CE = int(CE_DIT * 50)
sd_of = lambda spec, seed, prefix: weights.make_state_dict(spec, seed=seed, prefix=prefix)      # noqa: E731
cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.tiny."), dev)
lr = InterpolateRegulator(lc, sd_of(specs.lr_state_spec(lc), 6, "lr."), dev)
voc = HiFT(hc, sd_of(specs.hift_state_spec(hc), 1234, "hift."), dev)
w2v = Wav2Vec2Content(VC.make_state_dict(wc, seed=22), cfg=wc, device=dev, precision=1)
resample = Resample(SR, 16000, device=dev)
Cm, Dc, NH = dc["C"], dc["Dc"], hc["nb_harmonics"] + 1
FADE_IN, FADE_OUT = (w.to(dev) for w in gui_fade_windows(LB))


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 4), "spread_ms": round(ts[-1] - ts[0], 4)}


def torch_push(input_wav, input_wav_res, indata):
    """The GUI's lines, every statement once for all rows (streams)."""
    input_wav[:, :-LIN] = input_wav[:, LIN:].clone()
    input_wav[:, -LIN:] = indata
    input_wav_res[:, :-M * Z16] = input_wav_res[:, M * Z16:].clone()
    input_wav_res[:, -Z16 * (M + 1):] = resample(input_wav[:, -LIN - 2 * ZC:])[:, Z16:]


def torch_push_per_stream(input_wav, input_wav_res, indata):
    """The same lines as the GUI has them: one stream at a time."""
    for b in range(indata.size(0)):
        w, r = input_wav[b], input_wav_res[b]
        w[:-LIN] = w[LIN:].clone()
        w[-LIN:] = indata[b]
        r[:-M * Z16] = r[M * Z16:].clone()
        r[-Z16 * (M + 1):] = resample(w[-LIN - 2 * ZC:])[0, Z16:]


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
    mk = lambda: RealtimeEngine(lr, cfm, voc, S, HOP, BLOCK, LB, LS, tail=GEO["tail"], max_streams=B, fade_in=FADE_IN, fade_out=FADE_OUT)   # noqa: E731
    eng, eng_t = mk(), mk()
    eng.attach_audio(w2v, resample, LIN, L16, CE_DIT)
    slots = [eng.open(*ref) for _ in range(B)]
    assert [eng_t.open(*ref) for _ in range(B)] == slots
    input_wav, input_wav_res = torch.zeros(B, TOTAL, device=dev), torch.zeros(B, L16, device=dev)
    audio = [((torch.rand(B, LIN, generator=g) * 2 - 1) * 0.5).to(dev) for _ in range(4)]            # four blocks, in turn
    zs = [torch.randn(B, Cm, P + S, generator=g).to(dev) for _ in range(4)]
    draws = dict(phase0=((torch.rand(B, NH, 1, generator=g) * 2 - 1) * float(np.pi)).to(dev), noise=torch.randn(B, NH, S * HOP, generator=g).to(dev))

    @torch.inference_mode()
    def torch_step(x, z):
        torch_push(input_wav, input_wav_res, x)
        content = w2v.semantic_fn(input_wav_res)[:, CE:]
        return eng_t.step(slots, content, STEPS, CFG, z=z, vocoder_kwargs=draws)

    per = {p: {"event": [], "wall": [], "enqueue": []} for p in ("engine", "torch")}
    last = {}
    for k in range(args.warmup + R):
        x, z = audio[k % 4], zs[k % 4]
        for path in (("engine", "torch") if k % 2 == 0 else ("torch", "engine")):
            if path == "engine":
                fn = lambda: eng.step_audio(slots, x, STEPS, CFG, z=z, vocoder_kwargs=draws, return_parts=True)    # noqa: E731
            else:
                fn = lambda: torch_step(x, z)                                                                     # noqa: E731
            out, ev, wall, enq = measure(fn)
            last[path] = out
            if k >= args.warmup:
                per[path]["event"].append(ev)
                per[path]["wall"].append(wall)
                per[path]["enqueue"].append(enq)
    out_e, parts = last["engine"]
    same_ctx = bool(torch.equal(parts["ctx"], input_wav_res))
    diff = (out_e - last["torch"]).abs().max().item()
    same_state = bool(torch.equal(eng.state, eng_t.state))

    # the input stage alone: fresh state, the same block every round
    hist = torch.zeros(B, 2 * ZC, device=dev)
    ring = torch.zeros(int(_lib.lib().svc_rt_ring_floats(B, L16)), device=dev)
    ctx = torch.empty(B, L16, device=dev)
    cslots = _lib.i32_host(list(range(B)))
    x0 = audio[0]
    wav2, res2 = torch.zeros(B, TOTAL, device=dev), torch.zeros(B, L16, device=dev)

    def push_rounds(n=50):
        for _ in range(n):
            _lib.check(_lib.lib().svc_rt_push(resample._h, _lib.ptr(x0), LIN, LIN, B, cslots, B, ZC, Z16, _lib.ptr(hist), _lib.ptr(ring), L16,
                                              _lib.ptr(ctx), _lib.stream_ptr()))

    @torch.inference_mode()
    def torch_rounds(n=50):
        for _ in range(n):
            torch_push(wav2, res2, x0)

    @torch.inference_mode()
    def torch_stream_rounds(n=50):
        for _ in range(n):
            torch_push_per_stream(wav2, res2, x0)
    n_stream = 50 if B == 1 else 5                           # 64 streams x 7 statements x 50 rounds is host time only
    alone = {"kernel": [], "torch": [], "torch_per_stream": [], "kernel_host": [], "torch_host": [], "torch_per_stream_host": []}
    for r in range(7):
        for name, fn, n in (("kernel", push_rounds, 50), ("torch", torch_rounds, 50), ("torch_per_stream", torch_stream_rounds, n_stream)):
            _, ev, _, enq = measure(lambda: fn(n))
            if r >= 2:
                alone[name].append(ev / n)
                alone[name + "_host"].append(enq / n)
    same_alone = bool(torch.equal(ctx, res2))
    e, t = stats(per["engine"]["event"]), stats(per["torch"]["event"])
    ew, tw = stats(per["engine"]["wall"]), stats(per["torch"]["wall"])
    rec = {"workload": "real-time block step from audio: XLS-R-size wav2vec 2.0 (12 layers) + tiny DiT + HiFT, 10 steps, cfg 0.7, "
                       "22.05 kHz, block 0.18 s", "B": B, "repeats": R, "warmup": args.warmup, "sampler_steps": STEPS, "prompt_frames": P,
           "geometry": GEO, "input_geometry": GIN, "content_rows_after_ce": GIN["rows"] - CE, "hop": HOP,
           "block_ms_of_audio": round(BLOCK / SR * 1e3, 2), "reference_ms_per_block": 150,
           "engine_step_audio": {"event": e, "wall": ew, "enqueue": stats(per["engine"]["enqueue"])},
           "torch_statement": {"event": t, "wall": tw, "enqueue": stats(per["torch"]["enqueue"])},
           "event_difference_ms": round(t["ms"] - e["ms"], 4),
           "event_difference_exceeds_spreads": bool(abs(t["ms"] - e["ms"]) > e["spread_ms"] + t["spread_ms"]),
           "wall_difference_ms": round(tw["ms"] - ew["ms"], 4),
           "wall_difference_exceeds_spreads": bool(abs(tw["ms"] - ew["ms"]) > ew["spread_ms"] + tw["spread_ms"]),
           "push_alone": {"svc_rt_push": {"event": stats(alone["kernel"]), "host": stats(alone["kernel_host"])},
                          "torch_lines_all_streams": {"event": stats(alone["torch"]), "host": stats(alone["torch_host"])},
                          "torch_lines_per_stream": {"event": stats(alone["torch_per_stream"]), "host": stats(alone["torch_per_stream_host"])},
                          "same_context": same_alone,
                          "note": "per round: HIP events around back-to-back rounds / their number (50; 5 for the per-stream lines "
                                  "at B = 64), host = time until the calls returned / their number; 5 repeats after 2 warm-ups"},
           "push_share_of_engine_step": round(stats(alone["kernel"])["ms"] / e["ms"], 6),
           "same_output": {"context_bit_identical": same_ctx, "last_block_max_abs_diff": diff, "bit_identical": bool(diff == 0.0),
                           "same_sola_buffers": same_state}}
    print(json.dumps(rec), flush=True)
    records.append(rec)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        command = f"python tools/rt_audio_bench.py --batch {args.batch} --repeats {R} --warmup {args.warmup} --steps {STEPS} --prompt {P}"
        json.dump({"tool": "tools/rt_audio_bench.py", "command": command, "records": records}, f, indent=1)
