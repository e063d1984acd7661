"""One block step of a v2 real-time session (the timbre branch) in the reference GUI's published geometry: 22.05 kHz,
block 0.18 s, crossfade 0.04 s, extra context 2.5 s / 0.02 s, ce_dit_difference 2.0 (`realtime_geometry` /
`realtime_input_geometry`: blocks of 3969 samples, a 16 kHz context of 44160), full-size ASTRAL (`specs.astral_config()`), the
`v2_cfm` regulator, the v2 DiT and BigVGAN 22 kHz with synthetic weights, a prompt of 258 frames, 10 sampler steps, rates (0.7, 0.7).

For every B of `--batch` (default 1,64) one JSON line with two variants that alternate step by step in one process, on the same audio
and noise:
  engine    a token-mode `RealtimeEngine.step_audio`: `svc_rt_push`, `tokens_fn` (the wide head alone), `step_tokens`
  baseline  the same step written with the calls the library had before token mode: a feature-mode engine whose content encoder is
            `astral.tokens_batch(ctx)` (both heads), the torch slice and cast, `cfm_lr(tokens, ylens)`, and whose regulator passes
            that condition through to `RealtimeEngine.step`
Per step and variant: HIP-event time and the host time until the call returned (enqueue).  `--warmup` (3) untimed steps per variant,
`--repeats` (30) timed ones; median and spread (max - min) of each figure, and whether the difference of the medians exceeds the sum of
the spreads.  `same_output`: the variants' last blocks and SOLA buffers compared bit for bit.  `tokens_alone`: `tokens_fn(ctx)` against
`tokens_batch(ctx)` on the context by themselves.  `--out FILE` writes the lines to FILE as one JSON document."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("--batch", default="1,64")
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--prompt", type=int, default=258)
ap.add_argument("--precision", type=int, default=1)
ap.add_argument("--out", default="")
args = ap.parse_args()
sizes = [int(b) for b in args.batch.split(",")]
R, STEPS, P, RATES = args.repeats, args.steps, args.prompt, (0.7, 0.7)
if not sizes or min(sizes) < 1 or max(sizes) > 64 or R < 1 or args.warmup < 0:
    ap.error("--batch takes sizes in 1 .. 64, --repeats at least 1, --warmup at least 0")

import _pkgload  # noqa: E402
_pkgload.load_package()
import torch  # noqa: E402
import astral_cases as AC  # noqa: E402
import w2v_cases as VC  # noqa: E402
from seedvc_amd import specs, weights  # noqa: E402
from seedvc_amd.astral import AstralTokenizer  # noqa: E402
from seedvc_amd.audio import Resample  # noqa: E402
from seedvc_amd.cfm import CFM  # noqa: E402
from seedvc_amd.length_regulator import InterpolateRegulator  # noqa: E402
from seedvc_amd.pipeline import RealtimeEngine, gui_fade_windows, realtime_geometry, realtime_input_geometry  # noqa: E402
from seedvc_amd.vocoder import BigVGAN  # noqa: E402

assert torch.cuda.is_available(), "rt_v2_bench.py measures on the GPU; there is no fallback"
torch.set_grad_enabled(False)
dev = "cuda:0"
SR, CE_DIT = 22050, 2.0
ac, clc, dc, vh = specs.astral_config(), specs.lr_config("v2_cfm"), specs.dit_config("v2"), specs.bigvgan_config("22k")
HOP = 1
for u in vh["upsample_rates"]:
    HOP *= u
GEO = realtime_geometry(SR, HOP, 0.18, 0.04, 2.5, 0.02, CE_DIT)
GIN = realtime_input_geometry(SR, 0.18, 0.04, 2.5, 0.02)
S, BLOCK, LB, LS = (GEO[k] for k in ("S", "block", "Lb", "Ls"))
LIN, L16 = GIN["Lin"], GIN["L16"]
CE = int(CE_DIT * 50)
sd_of = lambda spec, seed, prefix: weights.make_state_dict(spec, seed=seed, prefix=prefix)      # noqa: E731
astral = AstralTokenizer(VC.make_state_dict(ac["ssl"], seed=22), [AC.make_head_sd(ac, k, seed=60 + k) for k in range(2)], cfg=ac, device=dev,
                         precision=args.precision)
cfm_lr = InterpolateRegulator(clc, sd_of(specs.lr_state_spec(clc), 6, "lr."), dev)
cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.v2."), dev)
voc = BigVGAN(vh, sd_of(specs.bigvgan_state_spec(vh), 1234, "bigvgan."), dev)
resample = Resample(SR, 16000, device=dev)
Cm, Dc = dc["C"], dc["Dc"]
FADE_IN, FADE_OUT = (w.to(dev) for w in gui_fade_windows(LB))
assert astral.codebook_size(0) <= clc["codebook_size"] and GIN["rows"] == astral.rows(L16, 0)


class BaselineContent:
    """The content side of the baseline: both heads, the torch slice and cast, the regulator -- handed on as "features"."""

    def semantic_fn(self, ctx):
        tok, _ = astral.tokens_batch(ctx)
        wide = tok[0][:, CE:].long()
        return cfm_lr(wide, ylens=torch.LongTensor([S] * ctx.size(0)))[0]


class PassThrough:
    """A regulator that hands the condition it is given to the step."""

    def __call__(self, x, ylens=None, n_quantizers=None, f0=None):
        return x, ylens, None, None, None


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
    return out, a.elapsed_time(b), (t1 - t0) * 1e3


def compare(x, y):
    d = x["ms"] - y["ms"]
    return {"difference_ms": round(d, 4), "exceeds_spreads": bool(abs(d) > x["spread_ms"] + y["spread_ms"])}


records = []
for B in sizes:
    g = torch.Generator().manual_seed(B)
    ref = ((torch.randn(1, P, Dc, generator=g)).to(dev), (torch.randn(1, Cm, P, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev),
           torch.randn(1, dc["style_dim"], generator=g).to(dev))
    mk = lambda lr: RealtimeEngine(lr, cfm, voc, S, HOP, BLOCK, LB, LS, tail=GEO["tail"], max_streams=B, fade_in=FADE_IN, fade_out=FADE_OUT)   # noqa: E731
    eng, base = mk(cfm_lr), mk(PassThrough())
    assert eng.token_mode and not base.token_mode
    eng.attach_audio(astral, resample, LIN, L16, CE_DIT)
    base.attach_audio(BaselineContent(), resample, LIN, L16, 0.0)        # the baseline's content side drops the ce rows itself
    slots = [eng.open(*ref) for _ in range(B)]
    assert [base.open(*ref) for _ in range(B)] == slots
    audio = [((torch.rand(B, LIN, generator=g) * 2 - 1) * 0.5).to(dev) for _ in range(4)]            # four blocks, in turn
    zs = [torch.randn(B, Cm, P + S, generator=g).to(dev) for _ in range(4)]
    per = {p: {"event": [], "enqueue": []} for p in ("engine", "baseline")}
    last, same_blocks, same_state = {}, True, True
    for k in range(args.warmup + R):
        x, z = audio[k % 4], zs[k % 4]
        for path in (("engine", "baseline") if k % 2 == 0 else ("baseline", "engine")):
            e = eng if path == "engine" else base
            out, ev, enq = measure(lambda: e.step_audio(slots, x, STEPS, RATES, z=z))
            last[path] = out
            if k >= args.warmup:
                per[path]["event"].append(ev)
                per[path]["enqueue"].append(enq)
        same_blocks &= bool(torch.equal(last["engine"], last["baseline"]))
        same_state &= bool(torch.equal(eng.state, base.state))
    ctx = torch.stack([eng.audio_context(s) for s in slots])
    alone = {"tokens_fn": {"event": [], "enqueue": []}, "tokens_batch": {"event": [], "enqueue": []}}
    for k in range(args.warmup + R):
        for name in (("tokens_fn", "tokens_batch") if k % 2 == 0 else ("tokens_batch", "tokens_fn")):
            fn = (lambda: astral.tokens_fn(ctx)) if name == "tokens_fn" else (lambda: astral.tokens_batch(ctx)[0])
            out, ev, enq = measure(fn)
            last[name] = out
            if k >= args.warmup:
                alone[name]["event"].append(ev)
                alone[name]["enqueue"].append(enq)
    same_tokens = bool(torch.equal(last["tokens_fn"], last["tokens_batch"][0]))
    st = {p: {k: stats(v) for k, v in per[p].items()} for p in per}
    al = {p: {k: stats(v) for k, v in alone[p].items()} for p in alone}
    rec = {"workload": "v2 real-time block step from audio (timbre branch): full-size ASTRAL + v2_cfm regulator + v2 DiT + BigVGAN 22 kHz, "
                       f"{STEPS} steps, rates {list(RATES)}, 22.05 kHz, block 0.18 s; synthetic weights",
           "B": B, "repeats": R, "warmup": args.warmup, "sampler_steps": STEPS, "prompt_frames": P, "astral_precision": args.precision,
           "geometry": GEO, "input_geometry": GIN, "tokens_after_ce": GIN["rows"] - CE, "hop": HOP,
           "block_ms_of_audio": round(BLOCK / SR * 1e3, 2),
           "engine_step_audio": st["engine"], "baseline_previous_calls": st["baseline"],
           "baseline_minus_engine": {k: compare(st["baseline"][k], st["engine"][k]) for k in ("event", "enqueue")},
           "same_output": {"blocks_bit_identical_every_step": same_blocks, "sola_buffers_bit_identical_every_step": same_state},
           "tokens_alone": {"tokens_fn_wide_head": al["tokens_fn"], "tokens_batch_both_heads": al["tokens_batch"],
                            "batch_minus_fn": {k: compare(al["tokens_batch"][k], al["tokens_fn"][k]) for k in ("event", "enqueue")},
                            "same_wide_tokens": same_tokens}}
    print(json.dumps(rec), flush=True)
    records.append(rec)
    assert same_blocks and same_state and same_tokens, "the two variants differ: the figures above compare different work"

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        command = (f"python tools/rt_v2_bench.py --batch {args.batch} --repeats {R} --warmup {args.warmup} --steps {STEPS} --prompt {P} "
                   f"--precision {args.precision}")
        json.dump({"tool": "tools/rt_v2_bench.py", "command": command, "records": records}, f, indent=1)
