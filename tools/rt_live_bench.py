"""One LIVE block step of a real-time session: the configuration of tools/rt_audio_bench.py (XLS-R-size wav2vec 2.0,
tiny DiT + HiFT, 10 sampler steps, cfg 0.7, model at 22.05 kHz, block 0.18 s, crossfade 0.04 s, extra context 2.5 s / 0.02 s,
ce_dit_difference 2.0) behind a 48 kHz sound card: audio comes in and goes out at 48 kHz (blocks of 8640 samples either way), every
stream has its noise gate at -40 dB and stream 0 is without speech.

For every B of `--batch` (default 1,64) one JSON line.
(a) Two paths that alternate step by step in one process, on the same audio, noise and HiFT draws:
  live       `RealtimeEngine.step_audio` after `attach_output`, `set_gate` and `set_speech`: `svc_rt_push_gated`, `semantic_fn`, the
             model, `svc_rt_out`
  statement  the same step written with the calls the library had before: `svc_rt_push` on host-gated audio (the audio is noise
             far above the threshold, so the host-gated audio is the audio itself and gating it costs the statement nothing),
             `semantic_fn`, the model, `audio.Resample` of the slice SOLA gets, a torch multiply by the speech flags, `svc_sola_step`
  Per step and path: HIP-event time, host wall time up to the final synchronise, host time until the call returned (enqueue).
  `--warmup` (3) untimed steps per path, `--repeats` (30) timed ones; median and spread (max - min), and whether the difference of
  the medians exceeds the sum of the spreads.  `same_output`: the two paths' contexts, blocks and SOLA buffers compared.
(b) The two calls alone, per call (HIP events around 50 back-to-back rounds / 50, host time of a round / 50; 5 repeats after 2
  warm-ups, the variants alternated): `svc_rt_out` against `svc_resample` + `svc_sola_step` on a contiguous slice, and
  `svc_rt_push_gated` (gate off: gate_pow NULL; gate on) against `svc_rt_push`.
`--out FILE` writes the lines to FILE as one JSON document."""
import argparse
import ctypes as C
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
from seedvc_amd import _lib, pipeline, specs, weights
from seedvc_amd.audio import Resample
from seedvc_amd.cfm import CFM
from seedvc_amd.length_regulator import InterpolateRegulator
from seedvc_amd.pipeline import (RealtimeEngine, gate_power, gui_fade_windows, realtime_geometry, realtime_input_geometry,
                                 realtime_output_geometry)
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

assert torch.cuda.is_available(), "rt_live_bench.py measures on the GPU; there is no fallback"
torch.set_grad_enabled(False)
dev = "cuda:0"
SR, SR_IO, CE_DIT, GATE_DB = 22050, 48000, 2.0, -40.0
dc, hc, wc = specs.dit_config("tiny"), specs.hift_config(), specs.wav2vec2_config()
lc = specs.lr_config("tiny", in_channels=wc["d_model"])
HOP = specs.hift_total_upsample(hc)
GEO = realtime_geometry(SR, HOP, 0.18, 0.04, 2.5, 0.02, CE_DIT)
GIN = realtime_input_geometry(SR_IO, 0.18, 0.04, 2.5, 0.02)
GOUT = realtime_output_geometry(GEO, SR, SR_IO)
S, BLOCK, LB, LS, START, N_INF = (GEO[k] for k in ("S", "block", "Lb", "Ls", "start", "n_inf"))
ZC, Z16, LIN, L16 = (GIN[k] for k in ("zc", "z16", "Lin", "L16"))
CE = int(CE_DIT * 50)
sd_of = lambda spec, seed, prefix: weights.make_state_dict(spec, seed=seed, prefix=prefix)      # noqa: E731
cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.tiny."), dev)
lr = InterpolateRegulator(lc, sd_of(specs.lr_state_spec(lc), 6, "lr."), dev)
voc = HiFT(hc, sd_of(specs.hift_state_spec(hc), 1234, "hift."), dev)
w2v = Wav2Vec2Content(VC.make_state_dict(wc, seed=22), cfg=wc, device=dev, precision=1)
rs_in, rs_out = Resample(SR_IO, 16000, device=dev), Resample(SR, SR_IO, device=dev)
Cm, Dc, NH = dc["C"], dc["Dc"], hc["nb_harmonics"] + 1
FADE_IN, FADE_OUT = (w.to(dev) for w in gui_fade_windows(GOUT["Lb"]))
POWER = gate_power(GATE_DB, ZC)
L = _lib.lib()


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


def compare(a, b):
    d = {"ms": round(b["ms"] - a["ms"], 4)}
    d["exceeds_spreads"] = bool(abs(d["ms"]) > a["spread_ms"] + b["spread_ms"])
    return d


records = []
for B in sizes:
    g = torch.Generator().manual_seed(B)
    ref = ((torch.randn(1, P, Dc, generator=g)).to(dev), (torch.randn(1, Cm, P, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev),
           torch.randn(1, dc["style_dim"], generator=g).to(dev))
    eng = RealtimeEngine(lr, cfm, voc, S, HOP, BLOCK, LB, LS, tail=GEO["tail"], max_streams=B)
    eng.attach_output(rs_out, FADE_IN, FADE_OUT)
    eng.attach_audio(w2v, rs_in, LIN, L16, CE_DIT)
    slots = [eng.open(*ref) for _ in range(B)]
    for s in slots:
        eng.set_gate(s, GATE_DB)
    eng.set_speech(slots[0], False)
    # the statement's own state: history, context ring, SOLA buffers at the output rate, the speech flags as a column
    hist = torch.zeros(B, 2 * ZC, device=dev)
    ring = torch.zeros(int(L.svc_rt_ring_floats(B, L16)), device=dev)
    state = torch.zeros(B, GOUT["Lb"], device=dev)
    speech = torch.ones(B, 1, device=dev)
    speech[0] = 0.0
    cslots = _lib.i32_host(slots)
    audio = [((torch.rand(B, LIN, generator=g) * 2 - 1) * 0.5).to(dev) for _ in range(4)]            # four blocks, in turn
    zs = [torch.randn(B, Cm, P + S, generator=g).to(dev) for _ in range(4)]
    draws = dict(phase0=((torch.rand(B, NH, 1, generator=g) * 2 - 1) * float(np.pi)).to(dev), noise=torch.randn(B, NH, S * HOP, generator=g).to(dev))

    @torch.inference_mode()
    def statement_step(x, z):
        ctx = torch.empty(B, L16, device=dev)
        _lib.check(L.svc_rt_push(rs_in._h, _lib.ptr(x), x.stride(0), LIN, B, cslots, B, ZC, Z16, _lib.ptr(hist), _lib.ptr(ring), L16,
                                 _lib.ptr(ctx), _lib.stream_ptr()))
        content = w2v.semantic_fn(ctx)[:, CE:]
        # the model: the body of RealtimeEngine._step up to the vocoder
        st = eng._stack_prompts(slots)
        Pl = st["P"]
        cond = lr(content, ylens=torch.LongTensor([S] * B), n_quantizers=3, f0=None)[0]
        mu = pipeline._assemble_cond(st["prompt_condition"], Pl, cond, [S] * B, st["Pmax"] + S)
        x_lens = [p + S for p in Pl]
        mel = cfm.inference(mu, x_lens, st["mel"], st["style"], None, STEPS, inference_cfg_rate=CFG, z=z, prompt_lens=Pl)
        vc = pipeline._strip_prompt(mel, Pl, x_lens, S)
        wave = _lib.f32c(pipeline._vocode(voc, vc, [S] * B, False, "rt_live_bench", hop=HOP, seeds=None, vocoder_kwargs=draws)[0].wave, dev)
        y = rs_out(wave[:, START:START + N_INF]) * speech
        out = torch.empty(B, GOUT["block"], device=dev)
        _lib.check(L.svc_sola_step(_lib.ptr(y), y.size(1), 0, B, _lib.ptr(state), B, cslots, _lib.ptr(FADE_IN), _lib.ptr(FADE_OUT),
                                   GOUT["block"], GOUT["Lb"], GOUT["Ls"], _lib.ptr(out), None, _lib.stream_ptr()))
        return out, ctx

    per = {p: {"event": [], "wall": [], "enqueue": []} for p in ("live", "statement")}
    last = {}
    for k in range(args.warmup + R):
        x, z = audio[k % 4], zs[k % 4]
        for path in (("live", "statement") if k % 2 == 0 else ("statement", "live")):
            if path == "live":
                fn = lambda: eng.step_audio(slots, x, STEPS, CFG, z=z, vocoder_kwargs=draws, return_parts=True)    # noqa: E731
            else:
                fn = lambda: statement_step(x, z)                                                                 # noqa: E731
            out, ev, wall, enq = measure(fn)
            last[path] = out
            if k >= args.warmup:
                per[path]["event"].append(ev)
                per[path]["wall"].append(wall)
                per[path]["enqueue"].append(enq)
    out_l, parts = last["live"]
    out_s, ctx_s = last["statement"]
    same = {"context_bit_identical": bool(torch.equal(parts["ctx"], ctx_s)), "last_block_max_abs_diff": (out_l - out_s).abs().max().item(),
            "same_sola_buffers": bool(torch.equal(eng.state, state)), "frames_muted_by_the_gate": int(parts["gate_mask"].sum()),
            "muted_stream_is_silent": bool(not out_l[0].any())}

    # ---- (b) the calls alone: fresh state, the same inputs every round
    wave = (torch.randn(B, S * HOP, generator=g) * 0.1).to(dev)
    seg = wave[:, START:START + N_INF].contiguous()
    st1, st2 = torch.zeros(B, GOUT["Lb"], device=dev), torch.zeros(B, GOUT["Lb"], device=dev)
    infer, y2 = torch.empty(B, GOUT["n_inf"], device=dev), torch.empty(B, GOUT["n_inf"], device=dev)
    o1, o2 = torch.empty(B, GOUT["block"], device=dev), torch.empty(B, GOUT["block"], device=dev)

    def out_rounds(n=50):
        for _ in range(n):
            _lib.check(L.svc_rt_out(rs_out._h, _lib.ptr(wave), wave.stride(0), START, N_INF, B, _lib.ptr(st1), B, cslots, None, _lib.ptr(FADE_IN),
                                    _lib.ptr(FADE_OUT), GOUT["block"], GOUT["Lb"], GOUT["Ls"], _lib.ptr(infer), _lib.ptr(o1), None,
                                    _lib.stream_ptr()))

    def composed_rounds(n=50):
        for _ in range(n):
            _lib.check(L.svc_resample(rs_out._h, _lib.ptr(seg), None, B, N_INF, _lib.ptr(y2), y2.size(1), _lib.stream_ptr()))
            _lib.check(L.svc_sola_step(_lib.ptr(y2), y2.size(1), 0, B, _lib.ptr(st2), B, cslots, _lib.ptr(FADE_IN), _lib.ptr(FADE_OUT),
                                       GOUT["block"], GOUT["Lb"], GOUT["Ls"], _lib.ptr(o2), None, _lib.stream_ptr()))

    hs = [torch.zeros(B, 2 * ZC, device=dev) for _ in range(3)]
    rings = [torch.zeros(int(L.svc_rt_ring_floats(B, L16)), device=dev) for _ in range(3)]
    ge = torch.zeros(B, 3, device=dev)
    ctxs = [torch.empty(B, L16, device=dev) for _ in range(3)]
    x0 = audio[0]
    pows = (C.c_float * B)(*([POWER] * B))

    def push_rounds(n=50):
        for _ in range(n):
            _lib.check(L.svc_rt_push(rs_in._h, _lib.ptr(x0), LIN, LIN, B, cslots, B, ZC, Z16, _lib.ptr(hs[0]), _lib.ptr(rings[0]), L16,
                                     _lib.ptr(ctxs[0]), _lib.stream_ptr()))

    def gated_rounds(n=50, which=1, p=None):
        for _ in range(n):
            _lib.check(L.svc_rt_push_gated(rs_in._h, _lib.ptr(x0), LIN, LIN, B, cslots, B, ZC, Z16, _lib.ptr(hs[which]), _lib.ptr(rings[which]),
                                           L16, _lib.ptr(ctxs[which]), p, _lib.ptr(ge), None, _lib.stream_ptr()))

    names = ("svc_rt_out", "svc_resample+svc_sola_step", "svc_rt_push", "svc_rt_push_gated_off", "svc_rt_push_gated_on")
    fns = (out_rounds, composed_rounds, push_rounds, lambda n: gated_rounds(n, 1, None), lambda n: gated_rounds(n, 2, pows))
    alone = {n: {"event": [], "host": []} for n in names}
    for r in range(7):
        for name, fn in zip(names, fns):
            _, ev, _, enq = measure(lambda: fn(50))
            if r >= 2:
                alone[name]["event"].append(ev / 50)
                alone[name]["host"].append(enq / 50)
    alone = {n: {"event": stats(v["event"]), "host": stats(v["host"])} for n, v in alone.items()}
    same_alone = {"rt_out_equals_composition": bool(torch.equal(o1, o2) and torch.equal(st1, st2) and torch.equal(infer, y2)),
                  "gated_pushes_equal_plain": bool(torch.equal(ctxs[0], ctxs[1]) and torch.equal(ctxs[0], ctxs[2]))}

    lv, stm = {k: stats(v) for k, v in per["live"].items()}, {k: stats(v) for k, v in per["statement"].items()}
    rec = {"workload": "live real-time block step: 48 kHz in and out, XLS-R-size wav2vec 2.0 (12 layers) + tiny DiT + HiFT at 22.05 kHz, "
                       "10 steps, cfg 0.7, block 0.18 s, gate -40 dB on every stream, stream 0 without speech",
           "B": B, "repeats": R, "warmup": args.warmup, "sampler_steps": STEPS, "prompt_frames": P, "geometry": GEO, "input_geometry": GIN,
           "output_geometry": GOUT, "hop": HOP, "block_ms_of_audio": round(LIN / SR_IO * 1e3, 2),
           "live_step_audio": lv, "statement_with_existing_calls": stm,
           "statement_minus_live": {k: compare(lv[k], stm[k]) for k in ("event", "wall", "enqueue")},
           "live_not_slower_than_statement_beyond_spreads": {k: bool(lv[k]["ms"] - stm[k]["ms"] <= lv[k]["spread_ms"] + stm[k]["spread_ms"])
                                                             for k in ("event", "wall")},
           "same_output": same,
           "calls_alone_per_call": alone,
           "calls_alone": {"composition_minus_rt_out": {k: compare(alone["svc_rt_out"][k], alone["svc_resample+svc_sola_step"][k])
                                                        for k in ("event", "host")},
                           "gated_off_minus_push": {k: compare(alone["svc_rt_push"][k], alone["svc_rt_push_gated_off"][k]) for k in ("event", "host")},
                           "gated_on_minus_push": {k: compare(alone["svc_rt_push"][k], alone["svc_rt_push_gated_on"][k]) for k in ("event", "host")},
                           "same_results": same_alone,
                           "note": "per call: HIP events around 50 back-to-back rounds / 50, host = time until the calls returned / 50; 5 "
                                   "repeats after 2 warm-ups, the five variants in turn"}}
    print(json.dumps(rec), flush=True)
    records.append(rec)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        command = f"python tools/rt_live_bench.py --batch {args.batch} --repeats {R} --warmup {args.warmup} --steps {STEPS} --prompt {P}"
        json.dump({"tool": "tools/rt_live_bench.py", "command": command, "records": records}, f, indent=1)
