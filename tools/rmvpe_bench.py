"""RMVPE pitch extractor (csrc/rmvpe.hip), full size, random weights: audio at 16 kHz -> F0, on three cases:

  one 10 s clip, one 30 s clip, and 8 ragged clips of 3 ... 25 s in one call.

For each case: the one call `RMVPE.f0_batch` (HIP events, 2 warm-up + `--repeats` timed runs, median and spread = max - min);
the stages through the seams (`mel`, `salience`, `decode`) and, inside the network, the split the library's own events give
(U-Net, GRU input projection, GRU recurrence, output layer) with the recurrence time per step (steps = padded frames of the
longest clip; a call that exceeds the plane budget runs in groups and the events cover its LAST group only, so for such a case
the split does not add up to the stage and the per-step figure is a lower bound: DESIGN 8g); the same network stated in torch (tests/rmvpe_cases.py, float32, eval, on the same GPU) on the device mel,
one clip at a time (torch has no ragged form); and, for the ragged case, a loop over one-clip `f0_batch` calls.
Nothing is gated on these numbers.  `--no-torch` skips the torch statement (its first calls tune ~70 conv shapes).
`--out FILE` writes the JSON document."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _pkgload
_pkgload.load_package()
import torch
import torch.nn.functional as F
import rmvpe_cases as RC
from seedvc_amd.rmvpe import RMVPE

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--label", default="this commit")
ap.add_argument("--out", default="")
args = ap.parse_args()
R = args.repeats
torch.set_grad_enabled(False)
dev = "cuda:0"
c, sd, net = RC.model("full", torch.float32)
m = RMVPE(sd, mel_basis=RC.basis(), device=dev, cfg=c)
net = None if args.no_torch else net.to(dev)


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "spread_ms": round(ts[-1] - ts[0], 3)}


def timed(fn, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(R):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return stats(ts)


def torch_net(mel, frames):
    """the reference's mel2hidden on each clip alone: zero-pad to a multiple of 32 frames, run, crop"""
    out = []
    for b, n in enumerate(frames):
        x = F.pad(mel[b:b + 1, :, :n], (0, 32 * ((n + 31) // 32) - n))
        out.append(net(x)[0, :n])
    return out


def case(name, secs):
    lens = [int(s * RC.SR) for s in secs]
    B, L = len(lens), max(lens)
    waves = torch.zeros(B, L)
    for b, n in enumerate(lens):
        waves[b, :n] = RC.clip(b, n)
    waves = waves.to(dev)
    frames = [m.frames(n) for n in lens]
    steps = 32 * ((max(frames) + 31) // 32)
    rec = {"case": name, "clips": B, "seconds": secs, "frames": frames, "sum_frames": sum(frames), "gru_steps": steps}
    rec["f0_batch"] = timed(lambda: m.f0_batch(waves, lens))
    mel = m.mel(waves, lens)
    sal = m.salience(mel, frames)
    rec["stage_mel"] = timed(lambda: m.mel(waves, lens))
    rec["stage_salience"] = timed(lambda: m.salience(mel, frames))
    rec["stage_decode"] = timed(lambda: m.decode(sal, frames))
    m.set_timing(True)
    split = []
    for _ in range(R):
        m.salience(mel, frames)
        split.append(m.last_timing())
    m.set_timing(False)
    for k in ("unet", "gru_in", "gru", "head"):
        rec["net_" + k] = stats([s[k] for s in split])
    rec["gru_us_per_step"] = round(1e3 * rec["net_gru"]["ms"] / steps, 3)
    rec["realtime_factor"] = round(sum(secs) * 1e3 / rec["f0_batch"]["ms"], 1)
    if B > 1:
        one = [(waves[b:b + 1, :n].contiguous(), n) for b, n in enumerate(lens)]
        rec["loop_of_one_clip_calls"] = timed(lambda: [m.f0_batch(w, [n]) for w, n in one])
        ya, yb = m.f0_batch(waves, lens), [m.f0_batch(w, [n]) for w, n in one]
        rec["ragged_equals_loop_bit_for_bit"] = bool(all(torch.equal(ya[b, :frames[b]], yb[b][0]) for b in range(B)))
        rec["loop_over_ragged"] = round(rec["loop_of_one_clip_calls"]["ms"] / rec["f0_batch"]["ms"], 3)
    if net is not None:
        rec["torch_fp32_network"] = timed(lambda: torch_net(mel, frames), warm=3)
        rec["torch_network_over_stage_salience"] = round(rec["torch_fp32_network"]["ms"] / rec["stage_salience"]["ms"], 3)
        ts = torch_net(mel, frames)
        rec["max_abs_diff_vs_torch_fp32"] = max((ts[b] - sal[b, :frames[b]]).abs().max().item() for b in range(B))
    print(json.dumps(rec), flush=True)
    return rec


doc = {"tool": "tools/rmvpe_bench.py", "label": args.label, "model": "RMVPE (full size, 90.42 M parameters, random weights)",
       "repeats": R, "torch": torch.__version__, "device": torch.cuda.get_device_name(0),
       "miopen_find_mode": os.environ.get("MIOPEN_FIND_MODE", "default"),       # conv algorithm search of the torch statement
       "records": [case("one 10 s clip", [10.0]), case("one 30 s clip", [30.0]),
                   case("8 ragged clips, 3 ... 25 s", [3.0, 25.0, 7.5, 12.0, 18.5, 5.0, 21.0, 9.0])]}
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
