"""Whisper content encoder (csrc/whisper.hip), whisper-small size, random weights: audio at 16 kHz -> content features, on five cases:

  one 10 s clip, one 30 s clip, 8 ragged clips of 3 ... 25 s, one 600 s file (24 windows) and 64 windows (64 clips of 30 s).

For each case, alternated in the same run with a rotating order (HIP events, 2 warm-up + `--repeats` timed rounds, median and
spread = max - min):
the one call `WhisperContent.content_batch`; the loop over one-window calls of this library (`semantic_fn` on every window of
the plan); and the reference's own way, transformers' `WhisperEncoder.half()` on the same GPU with torch SDPA, one window at a
time, on the device log-mel.  The stage split (log-mel, stem, layers, assemble) comes from the library's own events and covers
the LAST window group of the call (windows run in groups of 16 by default); the layer stage's TF/s is computed from the shapes
of that group.  Nothing is gated on these numbers.  `--no-torch` skips the transformers statement.  `--out FILE` writes the JSON
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
import whisper_cases as WC
from seedvc_amd.whisper import WhisperContent, window_plan

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--precision", type=int, default=1)
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
args = ap.parse_args()
R = args.repeats
torch.set_grad_enabled(False)
dev = "cuda:0"
c = WC.CFG_F
sd = WC.make_state_dict(c, seed=12)
m = WhisperContent(sd, cfg=c, device=dev, precision=args.precision)
P, D, H, NL, FF, W = c["max_source_positions"], c["d_model"], c["n_heads"], c["n_layers"], c["ffn_dim"], m.W
GROUP = 16
hf = None
if not args.no_torch:
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    hf = WhisperEncoder(WhisperConfig(num_mel_bins=c["n_mels"], d_model=D, encoder_attention_heads=H, encoder_layers=NL, encoder_ffn_dim=FF,
                                      max_source_positions=P)).eval()
    hf.load_state_dict(sd, strict=True)
    hf = hf.half().to(dev)


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
        for k in names[r % len(names):] + names[:r % len(names)]:      # the order rotates: what ran before (its weights in the
            f = fns[k]                                                  # last-level cache) is not the same for every sample
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: stats(v) for k, v in ts.items()}


def layer_flops(windows):
    per_layer = 2.0 * P * D * 3 * D + 2.0 * P * D * D + 4.0 * P * D * FF + 4.0 * P * P * D
    return windows * NL * per_layer


def case(name, secs):
    lens = [int(s * 16000) for s in secs]
    B, L = len(lens), max(lens)
    waves = torch.zeros(B, L)
    for b, n in enumerate(lens):
        src = WC.make_wave(min(n, 30 * 16000), b)
        waves[b, :n] = src.repeat(-(-n // src.numel()))[:n]
    waves = waves.to(dev)
    wins = [(b, s, n) for b, L_b in enumerate(lens) for s, n, _, _ in window_plan(L_b, W, 250 * 320)]
    one = [waves[b:b + 1, s:s + n].contiguous() for b, s, n in wins]
    last_group = len(wins) - ((len(wins) - 1) // GROUP) * GROUP
    rec = {"case": name, "clips": B, "seconds": secs, "windows": len(wins), "rows": [m.rows(n) for n in lens]}
    fns = {"content_batch": lambda: m.content_batch(waves, lens), "loop_of_one_window_calls": lambda: [m.semantic_fn(w) for w in one]}
    if hf is not None:
        def reference():
            for w in one:
                hf(m.mel(w, [w.size(1)]).half()).last_hidden_state[:, :w.size(1) // 320 + 1].float()
        fns["transformers_fp16_sdpa_one_window_at_a_time"] = reference
    rec.update(timed_alternated(fns))
    m.set_timing(True)
    split = []
    for _ in range(R):
        m.content_batch(waves, lens)
        split.append(m.last_timing())
    m.set_timing(False)
    for k in ("mel", "stem", "layers", "assemble"):
        rec["stage_" + k + "_last_group"] = stats([s[k] for s in split])
    rec["last_group_windows"] = last_group
    rec["layers_tflops_last_group"] = round(layer_flops(last_group) / (rec["stage_layers_last_group"]["ms"] * 1e-3) / 1e12, 1)
    rec["loop_over_one_call"] = round(rec["loop_of_one_window_calls"]["ms"] / rec["content_batch"]["ms"], 3)
    d = rec["content_batch"]["ms"] - rec["loop_of_one_window_calls"]["ms"]
    rec["one_call_not_slower_than_loop_beyond_spreads"] = bool(d <= rec["content_batch"]["spread_ms"] + rec["loop_of_one_window_calls"]["spread_ms"])
    if hf is not None:
        rec["transformers_over_one_call"] = round(rec["transformers_fp16_sdpa_one_window_at_a_time"]["ms"] / rec["content_batch"]["ms"], 3)
    rec["realtime_factor"] = round(sum(secs) * 1e3 / rec["content_batch"]["ms"], 1)
    print(json.dumps(rec), flush=True)
    return rec


doc = {"tool": "tools/whisper_bench.py", "label": args.label, "precision": args.precision,
       "model": "encoder of whisper-small (88.15 M parameters, random weights)", "repeats": R, "torch": torch.__version__,
       "device": torch.cuda.get_device_name(0), "window_group": GROUP,
       "records": [case("one 10 s clip", [10.0]), case("one 30 s clip", [30.0]),
                   case("8 ragged clips, 3 ... 25 s", [3.0, 25.0, 7.5, 12.0, 18.5, 5.0, 21.0, 9.0]),
                   case("one 600 s file (24 windows)", [600.0]), case("64 windows (64 clips of 30 s)", [30.0] * 64)]}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
