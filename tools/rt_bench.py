"""One block step of a real-time session, the published configuration of the reference GUI: tiny DiT + HiFT,
10 sampler steps, cfg 0.7, 22.05 kHz, block 0.18 s, crossfade 0.04 s, extra context 2.5 s / 0.02 s, ce_dit_difference 2.0
(`pipeline.realtime_geometry`: S = 65 frames, block 3969, Lb 882, Ls 441), a 258-frame reference, random weights.

For every B of `--batch` (default 1,64) one JSON line with two paths that alternate step by step in one process, on the same
content, noise and HiFT draws:
  engine  `RealtimeEngine.step`: six enqueues from host integers, the SOLA splice in `svc_sola_step`
  torch   the same step as a user of the library without the engine writes it: one batched length-regulator, sampler and
          vocoder call through the public mirrors (torch.cat for the condition, a slice for the prompt), then the GUI's own
          SOLA lines per stream on the device (two conv1d, argmax, a slice at the device-resident index, the in-place fade)
Per step and path: HIP-event time, host wall time up to the final synchronise, and the host time until the call returned
(enqueue).  `--warmup` (3) untimed steps per path, `--repeats` (30) timed ones; median and spread (max - min) of each figure, and
whether the difference of the medians exceeds the sum of the spreads.  `sola_alone`: the SOLA stage by itself on a fixed
waveform, `svc_sola_step` (HIP events around 50 launches) against the torch lines.  `same_output`: the two paths' last blocks
compared.  `--out FILE` writes the lines to FILE as one JSON document."""
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
import torch.nn.functional as F
from seedvc_amd import _lib, specs, weights
from seedvc_amd.cfm import CFM
from seedvc_amd.length_regulator import InterpolateRegulator
from seedvc_amd.pipeline import RealtimeEngine, gui_fade_windows, realtime_geometry
from seedvc_amd.vocoder import HiFT

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

assert torch.cuda.is_available(), "rt_bench.py measures on the GPU; there is no fallback"
torch.set_grad_enabled(False)
dev = "cuda:0"
SR = 22050
dc, lc, hc = specs.dit_config("tiny"), specs.lr_config("tiny"), specs.hift_config()
HOP = specs.hift_total_upsample(hc)
GEO = realtime_geometry(SR, HOP, 0.18, 0.04, 2.5, 0.02, 2.0)
S, BLOCK, LB, LS, START, N_INF = (GEO[k] for k in ("S", "block", "Lb", "Ls", "start", "n_inf"))
TIN = GEO["skip_head"] + GEO["return_length"] + GEO["skip_tail"] - 100          # 50 content frames per second, 2.0 s dropped
sd_of = lambda spec, seed, prefix: weights.make_state_dict(spec, seed=seed, prefix=prefix)      # noqa: E731
cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.tiny."), dev)
lr = InterpolateRegulator(lc, sd_of(specs.lr_state_spec(lc), 6, "lr."), dev)
voc = HiFT(hc, sd_of(specs.hift_state_spec(hc), 1234, "hift."), dev)
Cm, Dc, NH = dc["C"], dc["Dc"], hc["nb_harmonics"] + 1
FADE_IN, FADE_OUT = (w.to(dev) for w in gui_fade_windows(LB))


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 4), "spread_ms": round(ts[-1] - ts[0], 4)}


def torch_sola(infer_wav, sola_buffer):
    """The GUI's lines for one stream; sola_buffer (Lb,) is updated in place."""
    conv_input = infer_wav[None, None, :LB + LS]
    cor_nom = F.conv1d(conv_input, sola_buffer[None, None, :])
    cor_den = torch.sqrt(F.conv1d(conv_input ** 2, torch.ones(1, 1, LB, device=dev)) + 1e-8)
    sola_offset = torch.argmax(cor_nom[0, 0] / cor_den[0, 0])
    infer_wav = infer_wav[sola_offset:]
    infer_wav[:LB] *= FADE_IN
    infer_wav[:LB] += sola_buffer * FADE_OUT
    sola_buffer[:] = infer_wav[BLOCK:BLOCK + LB]
    return infer_wav[:BLOCK]


@torch.inference_mode()
def torch_step(x, pc, mel2, style, z, draws, buffers):
    B = x.size(0)
    cond = lr(x, ylens=torch.LongTensor([S] * B), n_quantizers=3, f0=None)[0]
    cat_condition = torch.cat([pc, cond], dim=1)
    vc_target = cfm.inference(cat_condition, torch.LongTensor([P + S] * B), mel2, style, None, STEPS, inference_cfg_rate=CFG, z=z)[:, :, P:]
    vc_wave = voc(vc_target, **draws).reshape(B, -1)
    tail = GEO["tail"]
    out = torch.empty(B, BLOCK, device=dev)
    for b in range(B):
        out[b] = torch_sola(vc_wave[b, -N_INF - tail:-tail], buffers[b])
    return out


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
    eng = RealtimeEngine(lr, cfm, voc, S, HOP, BLOCK, LB, LS, tail=GEO["tail"], max_streams=max(B, 1), fade_in=FADE_IN, fade_out=FADE_OUT)
    slots = [eng.open(*ref) for _ in range(B)]
    pc, mel2, style = ref[0].expand(B, -1, -1).contiguous(), ref[1].expand(B, -1, -1).contiguous(), ref[2].expand(B, -1).contiguous()
    buffers = torch.zeros(B, LB, device=dev)
    n_steps = args.warmup + R
    xs = [torch.randn(B, TIN, lc["in_channels"], generator=g).to(dev) for _ in range(4)]       # content of four blocks, in turn
    zs = [torch.randn(B, Cm, P + S, generator=g).to(dev) for _ in range(4)]
    draws = dict(phase0=((torch.rand(B, NH, 1, generator=g) * 2 - 1) * float(np.pi)).to(dev), noise=torch.randn(B, NH, S * HOP, generator=g).to(dev))
    per = {p: {"event": [], "wall": [], "enqueue": []} for p in ("engine", "torch")}
    last = {}
    for k in range(n_steps):
        x, z = xs[k % 4], zs[k % 4]
        for path in (("engine", "torch") if k % 2 == 0 else ("torch", "engine")):
            if path == "engine":
                fn = lambda: eng.step(slots, x, STEPS, CFG, z=z, vocoder_kwargs=draws)                      # noqa: E731
            else:
                fn = lambda: torch_step(x, pc, mel2, style, z, draws, buffers)                             # noqa: E731
            out, ev, wall, enq = measure(fn)
            last[path] = out
            if k >= args.warmup:
                per[path]["event"].append(ev)
                per[path]["wall"].append(wall)
                per[path]["enqueue"].append(enq)
    diff = (last["engine"] - last["torch"]).abs().max().item()
    same_state = bool(torch.equal(eng.state[:B], buffers))
    # the SOLA stage alone, on the last step's kind of input: a fixed waveform and a fixed buffer per stream
    wave = torch.randn(B, S * HOP, generator=g).to(dev)
    state0 = torch.randn(B, LB, generator=g).to(dev)
    out = torch.empty(B, BLOCK, device=dev)
    import ctypes as C
    cslots = (C.c_int32 * B)(*range(B))

    def sola_launches(n=50):
        for _ in range(n):
            _lib.check(_lib.lib().svc_sola_step(_lib.ptr(wave), S * HOP, START, B, _lib.ptr(st), B, cslots, _lib.ptr(FADE_IN),
                                                _lib.ptr(FADE_OUT), BLOCK, LB, LS, _lib.ptr(out), None, _lib.stream_ptr()))

    @torch.inference_mode()
    def sola_torch():
        for b in range(B):
            out[b] = torch_sola(wave[b, START:START + N_INF].clone(), st[b])
    sola = {"kernel": [], "torch": []}
    for r in range(7):
        st = state0.clone()
        _, ev, _, _ = measure(sola_launches)
        if r >= 2:
            sola["kernel"].append(ev / 50)
        st = state0.clone()
        _, ev, _, _ = measure(sola_torch)
        if r >= 2:
            sola["torch"].append(ev)
    e, t = stats(per["engine"]["event"]), stats(per["torch"]["event"])
    ew, tw = stats(per["engine"]["wall"]), stats(per["torch"]["wall"])
    rec = {"workload": "real-time block step: tiny DiT + HiFT, 10 steps, cfg 0.7, 22.05 kHz, block 0.18 s", "B": B, "repeats": R,
           "warmup": args.warmup, "sampler_steps": STEPS, "prompt_frames": P, "content_frames": TIN, "geometry": GEO, "hop": HOP,
           "block_ms_of_audio": round(BLOCK / SR * 1e3, 2),
           "engine": {"event": e, "wall": ew, "enqueue": stats(per["engine"]["enqueue"])},
           "torch_statement": {"event": t, "wall": tw, "enqueue": stats(per["torch"]["enqueue"])},
           "event_difference_ms": round(t["ms"] - e["ms"], 4),
           "event_difference_exceeds_spreads": bool(abs(t["ms"] - e["ms"]) > e["spread_ms"] + t["spread_ms"]),
           "wall_difference_ms": round(tw["ms"] - ew["ms"], 4),
           "wall_difference_exceeds_spreads": bool(abs(tw["ms"] - ew["ms"]) > ew["spread_ms"] + tw["spread_ms"]),
           "sola_alone": {"svc_sola_step_per_launch": stats(sola["kernel"]), "torch_lines_all_streams": stats(sola["torch"]),
                          "note": "svc_sola_step: HIP events around 50 back-to-back launches / 50; 5 repeats after 2 warm-ups"},
           "sola_share_of_engine_step": round(stats(sola["kernel"])["ms"] / e["ms"], 5),
           "same_output": {"last_block_max_abs_diff": diff, "bit_identical": bool(diff == 0.0), "same_sola_buffers": same_state}}
    print(json.dumps(rec), flush=True)
    records.append(rec)
    for s in slots:
        eng.close(s)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        # the command without --out: where the record is written is not part of the measurement
        command = f"python tools/rt_bench.py --batch {args.batch} --repeats {R} --warmup {args.warmup} --steps {STEPS} --prompt {P}"
        json.dump({"tool": "tools/rt_bench.py", "command": command, "records": records}, f, indent=1)
