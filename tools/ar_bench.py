"""v2 AR decode-step timing (config 5 of BASELINE.json: 320-token prefill, 256 one-token steps): tokens/s and the
achieved fraction of the HBM roofline (weights streamed once per token + valid KV prefix).

`--batch 1,8,16,32,64` adds the batched generate loop (`svc_ar_generate_batch`, B copies of the same prompt, sampler
included) for every B listed, next to the B = 1 `svc_ar_generate` of the same process as the anchor: three repeats each,
median and spread (max - min), us per step from the difference between a 256-token and a 32-token run (the B prefills
cancel), aggregate tokens/s of the whole call, bytes per step (weights once + B cache prefixes) and their fraction of the
8 TB/s HBM figure.  The record is printed as a second JSON line and written to `--out`."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
import _pkgload
_pkgload.load_package()
import torch
from seedvc_amd import specs, weights
from seedvc_amd.ar import ARModel

ap = argparse.ArgumentParser()
ap.add_argument("--batch", default="", help="comma-separated batch sizes for the batched generate loop, e.g. 1,8,16,32,64")
ap.add_argument("--out", default="", help="file the --batch record is written to")
args = ap.parse_args()

torch.set_grad_enabled(False)
c = specs.ar_config()
sd = weights.make_state_dict(specs.ar_state_spec(c), seed=7, prefix="ar.")
ar = ARModel(c, sd, "cuda:0")
ar.setup_caches()
n_prefill, n_steps = 320, 256
x = torch.randn(1, n_prefill, c["dim"], device="cuda")
t0 = time.perf_counter()
ar.forward_generate(x, torch.arange(n_prefill), torch.arange(n_prefill))
torch.cuda.synchronize()
t_prefill = time.perf_counter() - t0
xs = torch.randn(n_steps, c["dim"], device="cuda")
res = {}
for mode in ("eager", "graph"):
    ar.setup_caches()
    ar.forward_generate(x, torch.arange(n_prefill), torch.arange(n_prefill))
    pos = n_prefill
    if mode == "graph":
        ar.decode_step(xs[0], pos, pos)        # capture + first step
        pos += 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(1, n_steps):
        if mode == "graph":
            ar.decode_step(xs[s])
        else:
            ar.forward_generate(xs[s].reshape(1, 1, -1), torch.tensor([pos]), torch.tensor([pos]))
            pos += 1
    torch.cuda.synchronize()
    res[mode] = (time.perf_counter() - t0) / (n_steps - 1)
n_params = sum(v.numel() for k, v in sd.items() if "layers" in k or k.endswith("output.weight"))
bytes_tok = n_params * 2 + 2 * c["n_layer"] * c["n_local_heads"] * (n_prefill + n_steps // 2) * 64 * 4
out = {"prefill_ms": round(t_prefill * 1e3, 2), "eager_us_per_token": round(res["eager"] * 1e6, 1),
       "graph_us_per_token": round(res["graph"] * 1e6, 1), "tokens_per_s_graph": round(1.0 / res["graph"], 1),
       "alg_bytes_per_token": bytes_tok, "achieved_GBps": round(bytes_tok / res["graph"] / 1e9, 1),
       "hbm_peak_GBps": 8000, "frac": round(bytes_tok / res["graph"] / 8e12, 4)}
# whole generate loop on the device (8f row 4): prefill + n_steps tokens incl. embedding lookup and sampling
text = torch.randn(1, 120, c["dim"], device="cuda")
target = torch.randint(0, c["vocab_size"] - 1, (1, 200), device="cuda")
noise = torch.empty(n_steps, c["vocab_size"], device="cuda").exponential_(1)
noise[:, c["vocab_size"] - 1] = 1e30        # the EOS token never wins the exponential race: every run generates n_steps tokens
for _ in range(2):
    toks = ar.generate(text, target, exp_noise=noise, max_new=n_steps, check_every=16)
torch.cuda.synchronize()
t0 = time.perf_counter()
toks = ar.generate(text, target, exp_noise=noise, max_new=n_steps, check_every=16)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
out["generate_tokens"] = int(toks.shape[-1])
out["generate_ms"] = round(dt * 1e3, 2)
out["generate_tokens_per_s"] = round(toks.shape[-1] / dt, 1)
print(json.dumps(out))

if args.batch:
    REPEATS, SHORT = 3, 32
    sizes = [int(b) for b in args.batch.split(",")]

    def timed(fn):
        ts = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return ts[len(ts) // 2], ts[-1] - ts[0]

    # anchor: the B = 1 loop measured above, repeated (B sequences one after the other run at this rate)
    med, spread = timed(lambda: ar.generate(text, target, exp_noise=noise, max_new=n_steps, check_every=16))
    anchor = n_steps / med
    rec = {"shape": "ar_base", "prefill_tokens": int(text.shape[1] + target.shape[1] + 2), "steps": n_steps, "repeats": REPEATS,
           "b1_step_us_graph": out["graph_us_per_token"],
           "anchor_b1_generate": {"ms": round(med * 1e3, 2), "spread_ms": round(spread * 1e3, 2), "tokens_per_s": round(anchor, 1),
                                  "tokens_per_s_spread": round(n_steps / (med - spread / 2) - n_steps / (med + spread / 2), 1)},
           "hbm_peak_GBps": 8000, "batch": []}
    ar.setup_caches(max_batch_size=max(sizes))
    n_ctx = rec["prefill_tokens"] + n_steps // 2
    for B in sizes:
        texts, targets, noises = [text] * B, [target] * B, [noise] * B
        run = lambda n: ar.generate_batch(texts, targets, exp_noise=noises, max_new=n, check_every=16)
        toks = run(n_steps)                       # capture + warm
        assert all(t.shape[-1] == n_steps for t in toks)
        run(SHORT)
        t_long, s_long = timed(lambda: run(n_steps))
        t_short, s_short = timed(lambda: run(SHORT))
        step = (t_long - t_short) / (n_steps - SHORT)
        nbytes = n_params * 2 + B * 2 * c["n_layer"] * c["n_local_heads"] * n_ctx * 64 * 4
        rec["batch"].append({"B": B, "us_per_step": round(step * 1e6, 1), "us_per_step_spread": round((s_long + s_short) / (n_steps - SHORT) * 1e6, 1),
                             "generate_ms": round(t_long * 1e3, 2), "generate_spread_ms": round(s_long * 1e3, 2),
                             "tokens_per_s": round(B * n_steps / t_long, 1), "vs_serial_b1": round(B * n_steps / t_long / anchor, 2),
                             "step_tokens_per_s": round(B / step, 1),
                             "bytes_per_step": nbytes, "frac_hbm": round(nbytes / step / 8e12, 4)})
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
