"""The device resampler (`audio.Resample`, `svc_resample`) against the torch statement of the same operator on the same device
(`F.pad` + `F.conv1d(stride=o)` with the dense kernel: what torchaudio runs and what a caller did before), at four shapes:

  clip_30s      one 30 s clip, 22050 -> 16000
  enrol_64      64 clips of 3 ... 25 s (tools/enrol_bench.py's clips), 44100 -> 16000, one ragged call; the torch statement has no
                lengths and runs as a loop over the clips
  file_600s     one 600 s file, 44100 -> 16000
  block_0.5s    one 0.5 s block, 22050 -> 48000 (what a real-time output stage would hand over)

HIP events after 2 warm-up runs, `--repeats` (7) timed windows of `inner` back-to-back calls each (a single call of the short
shapes is a few microseconds: a window of one would time the launch), median and spread (max - min) per call.  Per shape: the
bytes the operator must move, 4 (sum lens + sum out_len), over the device time as a share of 8 TB/s (the HBM rate of the other
profiles) -- with the footprint beside it, because a footprint below the 256 MiB Infinity Cache is re-read from the cache by
repeated runs; max |device - torch| ; and whether the kernel is below the torch statement by more than the two spreads.
`--enrol` adds the 64-clip line of tools/enrol_bench.py (22050 Hz clips) with the 16 kHz copies given and with `to_16k` making
them.  `--out FILE` writes the JSON document (rewritten after every shape)."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _pkgload
_pkgload.load_package()
import torch
import torch.nn.functional as F
from seedvc_amd.audio import Resample, _sinc_resample_kernel

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="clip_30s,file_600s,block_0.5s,enrol_64")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--enrol", action="store_true")
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
args = ap.parse_args()
R = args.repeats
HBM = 8.0e12

torch.set_grad_enabled(False)
dev = "cuda:0"


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 5), "spread_ms": round(ts[-1] - ts[0], 5)}


def timed(fn, inner=1, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(R):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return stats(ts)


def torch_statement(orig, new):
    o, n, width, K = _sinc_resample_kernel(orig, new)
    K = K.to(dev)[:, None, :]

    def run(x):                                                  # x (B, L) -> (B, ceil(n L / o))
        y = F.conv1d(F.pad(x, (width, width + o))[:, None, :], K, stride=o)
        return y.transpose(1, 2).reshape(x.size(0), -1)[:, :-((-n * x.size(1)) // o)]
    return run


def enrol_clip_seconds(B=64, lo=3.0, hi=25.0):
    secs = [lo + (hi - lo) * i / max(B - 1, 1) for i in range(B)]
    random.Random(0).shuffle(secs)
    return secs


SHAPES = {                                                       # name: (orig, new, seconds per clip, inner calls per window)
    "clip_30s": (22050, 16000, [30.0], 50),
    "enrol_64": (44100, 16000, enrol_clip_seconds(), 1),
    "file_600s": (44100, 16000, [600.0], 5),
    "block_0.5s": (22050, 48000, [0.5], 200),
}

doc = {"tool": "tools/resample_bench.py", "label": args.label, "repeats": R, "hbm_bytes_per_s": HBM, "records": []}


def write():
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


for name in args.shapes.split(","):
    orig, new, secs, inner = SHAPES[name]
    rs, ref = Resample(orig, new, device=dev), torch_statement(orig, new)
    lens = [int(s * orig) for s in secs]
    B, L = len(lens), max(lens)
    x = 0.1 * torch.randn(B, L, generator=torch.Generator().manual_seed(B), dtype=torch.float32).to(dev)
    ragged = len(set(lens)) > 1
    alone = [x[b:b + 1, :v].contiguous() for b, v in enumerate(lens)] if ragged else [x]
    device_fn = (lambda: rs(x, lens=lens)) if ragged else (lambda: rs(x))                # noqa: E731
    torch_fn = lambda: [ref(w) for w in alone]                                            # noqa: E731
    out_lens = [rs.out_len(v) for v in lens]
    moved = 4 * (sum(lens) + sum(out_lens))
    rec = {"shape": name, "rates": [orig, new], "B": B, "seconds": [round(min(secs), 2), round(max(secs), 2)], "tile_outputs": rs.tile,
           "inner_calls": inner, "bytes_moved": moved, "footprint_mb": round(4 * (B * L + B * rs.out_len(L)) / 2 ** 20, 1)}
    rec["device"] = timed(device_fn, inner)
    rec["torch_statement"] = timed(torch_fn, max(1, inner // 5))
    rec["device_share_of_hbm_rate"] = round(moved / (rec["device"]["ms"] * 1e-3) / HBM, 4)
    got = device_fn()
    got = got[0] if ragged else got
    want = torch_fn()
    rec["max_abs_diff_vs_torch"] = max((got[b, :out_lens[b]] - want[b if ragged else 0][0 if ragged else b, :out_lens[b]]).abs().max().item()
                                       for b in range(B))
    rec["torch_over_device"] = round(rec["torch_statement"]["ms"] / rec["device"]["ms"], 2)
    rec["device_below_torch_by_more_than_the_spreads"] = bool(
        rec["torch_statement"]["ms"] - rec["device"]["ms"] > rec["torch_statement"]["spread_ms"] + rec["device"]["spread_ms"])
    doc["records"].append(rec)
    print(json.dumps(rec), flush=True)
    write()
    del x, alone, got, want

if args.enrol:
    from seedvc_amd import specs, weights
    from seedvc_amd.audio import MelSpectrogram
    from seedvc_amd.campplus import CAMPPlus
    from seedvc_amd.pipeline import enrol_references, enrol_references_audio, to_16k
    SR = 22050
    c = specs.campplus_config()
    cp = CAMPPlus(c, weights.make_state_dict(specs.campplus_state_spec(c), seed=1234, prefix="campplus."), dev)
    mel_fn = MelSpectrogram(1024, 80, SR, 256, 1024, 0, None, center=False, device=dev)
    rs = Resample(SR, 16000, device=dev)
    lens = [int(s * SR) for s in enrol_clip_seconds()]
    waves = (0.1 * torch.randn(64, max(lens), generator=torch.Generator().manual_seed(64))).to(dev)
    w16, l16 = to_16k(rs, waves, lens)
    rec = {"shape": "enrol_bench_64", "rates": [SR, 16000], "B": 64,
           "given_16k": timed(lambda: enrol_references(mel_fn, cp, waves, lens, w16, l16)),
           "from_to_16k": timed(lambda: enrol_references_audio(mel_fn, cp, rs, waves, lens)),
           "to_16k_alone": timed(lambda: to_16k(rs, waves, lens))}
    rec["change_ms"] = round(rec["from_to_16k"]["ms"] - rec["given_16k"]["ms"], 3)
    rec["change_above_the_spreads"] = bool(abs(rec["change_ms"]) > rec["from_to_16k"]["spread_ms"] + rec["given_16k"]["spread_ms"])
    doc["records"].append(rec)
    print(json.dumps(rec), flush=True)
    write()
