"""wav2vec 2.0 base family (csrc/wav2vec2.hip through svc_w2v_create_ex) at HuBERT-base size (C 512, D 768, 12 heads,
12 layers, F 3072, positional conv k 128 in 16 groups of 48 channels, 30 s windows), random weights, precision 1: audio at 16 kHz ->
content features, on five cases:

  one real-time context of 2.94 s (the GUI's extra + block + right context, `realtime_geometry`), 64 such clips, one 30 s clip,
  8 ragged clips of 3 ... 25 s and one 600 s file (24 windows).

For each case, alternated in the same run with a rotating order (HIP events, 2 warm-up + `--repeats` timed rounds, median and
spread = max - min): the one call `Wav2Vec2Content.content_batch`; the loop over one-window calls of this library (`semantic_fn` on
every window of the plan); and the reference's own way, transformers' `HubertModel.half()` on the same GPU, one window at a time,
fed the same normalised input.  The stage split (extractor, positional conv, layers, assemble) comes from the library's own events
and covers the LAST window group of the call (windows run in groups of 16 by default).  There is no threshold: nobody has measured
this network here before, the numbers are reported as they are.  `--no-torch` skips the transformers statement.  `--out FILE` writes
the JSON document."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _pkgload
_pkgload.load_package()
import torch
import w2v_base_cases as BC
from seedvc_amd import pipeline, specs
from seedvc_amd.wav2vec2 import Wav2Vec2Content, window_plan

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
c = specs.wav2vec2_base_config()
sd = BC.make_state_dict(c, seed=42)
m = Wav2Vec2Content(sd, cfg=c, device=dev, precision=args.precision)
D, H, NL, FF, K, W = c["d_model"], c["n_heads"], c["n_layers"], c["ffn_dim"], c["pos_k"], m.W
WD = D // c["pos_groups"]
GROUP = 16
hf = None
if not args.no_torch:
    from transformers import HubertConfig, HubertModel
    hf = HubertModel(HubertConfig(hidden_size=D, num_hidden_layers=NL, num_attention_heads=H, intermediate_size=FF, conv_dim=(c["conv_dim"],) * 7,
                                  conv_kernel=c["conv_kernel"], conv_stride=c["conv_stride"], feat_extract_norm="group", do_stable_layer_norm=False,
                                  conv_bias=False, num_conv_pos_embeddings=K, num_conv_pos_embedding_groups=c["pos_groups"])).eval()
    hf.load_state_dict(sd, strict=True)
    hf = hf.half().to(dev)
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


def case(name, secs):
    lens = [int(s * 16000) for s in secs]
    B, L = len(lens), max(lens)
    waves = torch.zeros(B, L)
    for b, n in enumerate(lens):
        src = BC.make_wave(min(n, 30 * 16000), b)
        waves[b, :n] = src.repeat(-(-n // src.numel()))[:n]
    waves = waves.to(dev)
    wins = [(b, s, n, r) for b, L_b in enumerate(lens) for s, n, d, r in window_plan(c, L_b, 250) if r > d]
    one = [waves[b:b + 1, s:s + n].contiguous() for b, s, n, _ in wins]
    normed = [m.normalize(w, [w.size(1)]).half() for w in one]
    last = wins[((len(wins) - 1) // GROUP) * GROUP:]
    rec = {"case": name, "clips": B, "seconds": [round(s, 3) for s in secs], "windows": len(wins), "rows": [m.rows(n) for n in lens]}
    fns = {"content_batch": lambda: m.content_batch(waves, lens), "loop_of_one_window_calls": lambda: [m.semantic_fn(w) for w in one]}
    if hf is not None:
        def reference():
            for x in normed:
                hf(x).last_hidden_state.float()
        fns["transformers_fp16_one_window_at_a_time"] = reference
    rec.update(timed_alternated(fns))
    m.set_timing(True)
    split = []
    for _ in range(R):
        m.content_batch(waves, lens)
        split.append(m.last_timing())
    m.set_timing(False)
    for k in ("extractor", "posconv", "layers", "assemble"):
        rec["stage_" + k + "_last_group"] = stats([s[k] for s in split])
    rec["last_group_windows"] = len(last)
    pos_s = rec["stage_posconv_last_group"]["ms"] * 1e-3
    rows_last = sum(r for _, _, _, r in last)
    rec["posconv_tflops_last_group"] = round(2.0 * rows_last * D * WD * K / pos_s / 1e12, 2)     # useful FLOPs: 48 of the 64 K lanes
    layer_flops = sum(NL * (2.0 * r * D * 3 * D + 2.0 * r * D * D + 4.0 * r * D * FF + 4.0 * r * r * D) for _, _, _, r in last)
    rec["layers_tflops_last_group"] = round(layer_flops / (rec["stage_layers_last_group"]["ms"] * 1e-3) / 1e12, 1)
    rec["loop_over_one_call"] = round(rec["loop_of_one_window_calls"]["ms"] / rec["content_batch"]["ms"], 3)
    if hf is not None:
        rec["transformers_over_one_call"] = round(rec["transformers_fp16_one_window_at_a_time"]["ms"] / rec["content_batch"]["ms"], 3)
    rec["realtime_factor"] = round(sum(secs) * 1e3 / rec["content_batch"]["ms"], 1)
    print(json.dumps(rec), flush=True)
    return rec


doc = {"tool": "tools/w2v_base_bench.py", "label": args.label, "precision": args.precision,
       "model": "hubert-base-ls960 geometry, 12 layers (random weights)", "repeats": R, "torch": torch.__version__,
       "device": torch.cuda.get_device_name(0), "window_group": GROUP, "realtime_context_seconds": RT_SECONDS,
       "records": [case("one real-time context", [RT_SECONDS]), case("64 real-time contexts", [RT_SECONDS] * 64),
                   case("one 30 s clip", [30.0]), case("8 ragged clips, 3 ... 25 s", [3.0, 25.0, 7.5, 12.0, 18.5, 5.0, 21.0, 9.0]),
                   case("one 600 s file (24 windows)", [600.0])]}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
