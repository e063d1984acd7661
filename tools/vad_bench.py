"""The FSMN-VAD on the device, measured.  One JSON line per part; `--out FILE` (default profiles/vad.json) writes
them as one document.  Median and spread (max - min) of `--repeats` timed runs after `--warmup`, the variants of a part
alternating run by run in one process; HIP-event time, and host time until the calls returned.  Random weights.

(a) `--live`: the live block step of tools/rt_live_bench.py (48 kHz in and out, XLS-R-size wav2vec 2.0 + tiny DiT + HiFT, gate on
    every stream) on two engines that share their models, B = 1 and 64: VAD attached and on for every stream against no VAD (the
    parent commit's step).
(b) `svc_vad_step` alone per call (50 back-to-back calls / 50), B = 1 and 64, a block of 0.18 s (n_new = 2880), against a torch
    fp32 statement of the same front-end and encoder on the same rows with carried caches.  A step is 7 launches: frames, DFT
    GEMM, power, mel GEMM, log + LFR + CMVN, the network, the detector.
(c) `svc_vad_scores` on one 30 s clip, on 64 ragged clips of 3 .. 25 s and on a 600 s file: the default run length (512 rows)
    against one run per clip (seg_rows = 2^30) and against the torch statement."""
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
import vad_cases as V
from seedvc_amd.vad import FsmnVad

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--live", action="store_true")
ap.add_argument("--batch", default="1,64")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad.json"))
args = ap.parse_args()
assert torch.cuda.is_available(), "vad_bench.py measures on the GPU; there is no fallback"
torch.set_grad_enabled(False)
dev = "cuda:0"
SD, (SHIFT, SCALE) = V.random_state_dict(0), V.cmvn(0)
vad = FsmnVad(SD, torch.from_numpy(SHIFT), torch.from_numpy(SCALE), device=dev)


class TorchVad:
    """The same front-end and encoder as plain torch fp32 ops on the GPU (batched, equal lengths)."""

    def __init__(self):
        f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(dev)      # noqa: E731
        c, s = V.dft_basis(np.float32)
        self.basis, self.mel, self.win = f(np.concatenate([c, s]).T[:400]), f(V.mel_bank(np.float32).T), f(V.hamming(np.float32))
        self.shift, self.scale = f(SHIFT), f(SCALE)
        self.sd = {k: v.float().to(dev) for k, v in SD.items()}

    def features(self, w, final):
        fr = (w * 32768.0).unfold(1, 400, 160)
        fr = fr - fr.mean(2, keepdim=True)
        fr = (fr - 0.97 * torch.cat([fr[:, :, :1], fr[:, :, :-1]], 2)) * self.win
        spec = fr @ self.basis
        e = (spec[..., :257] ** 2 + spec[..., 257:] ** 2) @ self.mel
        feat = torch.log(e.clamp_min(V.EPS32))
        F = feat.size(1)
        R = F if final else F - 2
        idx = (torch.arange(R, device=dev)[:, None] + torch.arange(-2, 3, device=dev)[None, :]).clamp(0, F - 1)
        return (feat[:, idx].reshape(w.size(0), R, 400) + self.shift) * self.scale

    def encode(self, x, caches=None):
        sd, lin = self.sd, torch.nn.functional.linear
        h = torch.relu(lin(lin(x, sd["in_linear1.linear.weight"], sd["in_linear1.linear.bias"]), sd["in_linear2.linear.weight"],
                           sd["in_linear2.linear.bias"]))
        new = []
        for l in range(4):
            p = lin(h, sd[f"fsmn.{l}.linear.linear.weight"])
            full = torch.cat([caches[l] if caches else p.new_zeros(p.size(0), 19, 128), p], 1)
            y = p + torch.nn.functional.conv1d(full.transpose(1, 2), sd[f"fsmn.{l}.fsmn_block.conv_left.weight"][:, :, :, 0], groups=128).transpose(1, 2)
            new.append(full[:, -19:])
            h = torch.relu(lin(y, sd[f"fsmn.{l}.affine.linear.weight"], sd[f"fsmn.{l}.affine.linear.bias"]))
        lg = lin(lin(h, sd["out_linear1.linear.weight"], sd["out_linear1.linear.bias"]), sd["out_linear2.linear.weight"], sd["out_linear2.linear.bias"])
        return torch.softmax(lg, -1)[..., 0], new


tv = TorchVad()


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


def alternate(variants, scale=1.0):
    """variants: name -> fn.  -> name -> {event, host} stats, the variants in turn every repeat."""
    per = {n: {"event": [], "host": []} for n in variants}
    for r in range(args.warmup + args.repeats):
        for n, fn in variants.items():
            _, ev, host = measure(fn)
            if r >= args.warmup:
                per[n]["event"].append(ev * scale)
                per[n]["host"].append(host * scale)
    return {n: {k: stats(v) for k, v in d.items()} for n, d in per.items()}


def diff(a, b):
    d = round(b["event"]["ms"] - a["event"]["ms"], 4)
    return {"event_ms": d, "exceeds_spreads": bool(abs(d) > a["event"]["spread_ms"] + b["event"]["spread_ms"])}


records = []


def emit(rec):
    print(json.dumps(rec), flush=True)
    records.append(rec)


# ---------------------------------------------------------------------------------------------------------------- (b)
N_NEW, END = 2880, 2880 + 960
for B in (int(b) for b in args.batch.split(",")):
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, END + 320, generator=g) * 0.1).to(dev)
    state, flags = vad.stream_state(B)
    slots, total = list(range(B)), [160 * 600] * B
    caches = [torch.zeros(B, 19, 128, device=dev) for _ in range(4)]

    def step_rounds(n=50):
        for _ in range(n):
            vad.step(x, END, N_NEW, total, slots, state, flags)

    def torch_rounds(n=50):
        c = caches
        for _ in range(n):
            _, c = tv.encode(tv.features(x[:, :END], False), c)

    res = alternate({"svc_vad_step": step_rounds, "torch_statement": torch_rounds}, scale=1 / 50)
    emit({"part": "b", "what": "svc_vad_step alone, per call (50 back-to-back calls / 50)", "B": B, "n_new": N_NEW, "rows_per_stream": N_NEW // 160,
          "launches_per_call": 7, **res, "torch_minus_step": diff(res["svc_vad_step"], res["torch_statement"])})

# ---------------------------------------------------------------------------------------------------------------- (c)
rng = np.random.default_rng(3)
cases_c = {"one_30s_clip": [30.0], "64_ragged_clips_3_to_25s": list(rng.uniform(3.0, 25.0, 64)), "one_600s_file": [600.0]}
for name, secs in cases_c.items():
    lens = [int(s * 16000) for s in secs]
    w = (torch.randn(len(lens), max(lens), generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    variants = {"svc_vad_scores": lambda: vad.scores_batch(w, lens, final=True),
                "svc_vad_scores_one_run_per_clip": lambda: vad.scores_batch(w, lens, final=True, seg_rows=1 << 30),
                # the statement has no lengths: every clip at the longest length (its best case per row)
                "torch_statement_padded": lambda: tv.encode(tv.features(w, True))}
    res = alternate(variants)
    p1, _ = vad.scores_batch(w, lens, final=True)
    p2, _ = vad.scores_batch(w, lens, final=True, seg_rows=1 << 30)
    emit({"part": "c", "case": name, "clips": len(lens), "seconds_of_audio": round(sum(secs), 1), "rows": sum(V.rows_of(n, True) for n in lens),
          **res, "split_bit_identical_to_one_run": bool(torch.equal(p1, p2)),
          "one_run_minus_split": diff(res["svc_vad_scores"], res["svc_vad_scores_one_run_per_clip"]),
          "torch_minus_split": diff(res["svc_vad_scores"], res["torch_statement_padded"])})
    del w

# ---------------------------------------------------------------------------------------------------------------- (a)
if args.live:
    import w2v_cases as VC
    from seedvc_amd import specs, weights
    from seedvc_amd.audio import Resample
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import RealtimeEngine, gui_fade_windows, realtime_geometry, realtime_input_geometry, realtime_output_geometry
    from seedvc_amd.vocoder import HiFT
    from seedvc_amd.wav2vec2 import Wav2Vec2Content
    SR, SR_IO, CE_DIT, P, STEPS, CFG = 22050, 48000, 2.0, 258, 10, 0.7
    dc, hc, wc = specs.dit_config("tiny"), specs.hift_config(), specs.wav2vec2_config()
    lc = specs.lr_config("tiny", in_channels=wc["d_model"])
    HOP = specs.hift_total_upsample(hc)
    GEO, GIN = realtime_geometry(SR, HOP, 0.18, 0.04, 2.5, 0.02, CE_DIT), realtime_input_geometry(SR_IO, 0.18, 0.04, 2.5, 0.02)
    GOUT = realtime_output_geometry(GEO, SR, SR_IO)
    sd_of = lambda spec, seed, prefix: weights.make_state_dict(spec, seed=seed, prefix=prefix)      # noqa: E731
    cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.tiny."), dev)
    lr = InterpolateRegulator(lc, sd_of(specs.lr_state_spec(lc), 6, "lr."), dev)
    voc = HiFT(hc, sd_of(specs.hift_state_spec(hc), 1234, "hift."), dev)
    w2v = Wav2Vec2Content(VC.make_state_dict(wc, seed=22), cfg=wc, device=dev, precision=1)
    rs_in, rs_out = Resample(SR_IO, 16000, device=dev), Resample(SR, SR_IO, device=dev)
    FADE = [w.to(dev) for w in gui_fade_windows(GOUT["Lb"])]
    NH = hc["nb_harmonics"] + 1
    for B in (int(b) for b in args.batch.split(",")):
        g = torch.Generator().manual_seed(B)
        ref = (torch.randn(1, P, dc["Dc"], generator=g).to(dev), (torch.randn(1, dc["C"], P, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev),
               torch.randn(1, dc["style_dim"], generator=g).to(dev))
        engines = {}
        for name in ("with_vad", "without_vad"):
            e = RealtimeEngine(lr, cfm, voc, GEO["S"], HOP, GEO["block"], GEO["Lb"], GEO["Ls"], tail=GEO["tail"], max_streams=B)
            e.attach_output(rs_out, *FADE)
            e.attach_audio(w2v, rs_in, GIN["Lin"], GIN["L16"], CE_DIT)
            sl = [e.open(*ref) for _ in range(B)]
            for s in sl:
                e.set_gate(s, -40.0)
            if name == "with_vad":
                e.attach_vad(vad)
                for s in sl:
                    e.set_vad(s, True)
            engines[name] = (e, sl)
        audio = [((torch.rand(B, GIN["Lin"], generator=g) * 2 - 1) * 0.5).to(dev) for _ in range(4)]
        zs = [torch.randn(B, dc["C"], P + GEO["S"], generator=g).to(dev) for _ in range(4)]
        draws = dict(phase0=((torch.rand(B, NH, 1, generator=g) * 2 - 1) * float(np.pi)).to(dev),
                     noise=torch.randn(B, NH, GEO["S"] * HOP, generator=g).to(dev))
        k = [0]

        def step(name):
            e, sl = engines[name]
            i = k[0] // 2 % 4
            k[0] += 1
            return e.step_audio(sl, audio[i], STEPS, CFG, z=zs[i], vocoder_kwargs=draws)

        res = alternate({"with_vad": lambda: step("with_vad"), "without_vad": lambda: step("without_vad")})
        emit({"part": "a", "what": "live step_audio of tools/rt_live_bench.py, VAD on every stream against no VAD", "B": B, **res,
              "with_minus_without": diff(res["without_vad"], res["with_vad"]),
              "flags_after": engines["with_vad"][0]._vad["flags"].tolist()[:8]})

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/vad_bench.py", "command": "python tools/vad_bench.py " + " ".join(sys.argv[1:]), "records": records}, f, indent=1)
