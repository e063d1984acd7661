"""BASELINE config 5 as ONE workload through `pipeline.V2HotPath`: ar_base (120 condition frames + 200 prompt tokens,
256 new tokens, seeded sampling) -> v2 length regulators -> v2 DiT, 25 steps, CFG (0.7, 0.7), 430 prompt + 430 generated
frames -> BigVGAN 22k.  Random weights: a few sequences of a large batch do draw EOS before 256 tokens, so their lengths differ
and the vocoder runs once per distinct length (the record gives the token range and the number of vocoder groups).

For every B of `--batch` (default 1,64) one JSON line: per-stage milliseconds from HIP events inside the composite call
(AR with its length regulator; CFM length regulator + assembly; CFM; strip + vocoder), the AR split into prefill
(a max_new = 1 call) and decode (the rest), composite mel frames/s and AR tokens/s, the AR share; the same stages timed
alone in the same process and the difference to the composite ("glue"); at the largest B, seeded against explicit-noise
generation, alternating.  Two warm-up runs, `--repeats` (5) timed runs, median and spread (max - min) of each figure.
`--out FILE` writes the lines to FILE as one JSON document.

`--ragged`: the same models on a batch whose output lengths ALL differ (per-utterance `frames_per_token` chosen from the
utterances' own token counts so that the lengths spread evenly over 120 ... `--frames`, fixed shuffled order).  The
record gives the composite and its stages with `V2HotPath.ragged_vocoder` on (one vocoder call) and off (one call per
distinct length), alternating run by run; the stages alone and the seeded / explicit comparison are not repeated."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import _pkgload
_pkgload.load_package()
import torch
from seedvc_amd import specs, weights
from seedvc_amd.ar import ARModel
from seedvc_amd.cfm import CFM
from seedvc_amd.length_regulator import InterpolateRegulator
from seedvc_amd.pipeline import V2HotPath, _assemble_cond, _strip_prompt
from seedvc_amd.vocoder import BigVGAN

ap = argparse.ArgumentParser()
ap.add_argument("--batch", default="1,64")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tokens", type=int, default=256)
ap.add_argument("--frames", type=int, default=430, help="prompt frames and generated frames per utterance")
ap.add_argument("--steps", type=int, default=25)
ap.add_argument("--ragged", action="store_true", help="all output lengths differ; ragged vocoder call on against off")
ap.add_argument("--out", default="")
args = ap.parse_args()
sizes = [int(b) for b in args.batch.split(",")]
R, N_TOK, P, STEPS = args.repeats, args.tokens, args.frames, args.steps

torch.set_grad_enabled(False)
torch.manual_seed(0)
dev = "cuda:0"


def sd_of(spec, seed, prefix):
    return weights.make_state_dict(spec, seed=seed, prefix=prefix)


ac = specs.ar_config()
ar = ARModel(ac, sd_of(specs.ar_state_spec(ac), 7, "ar."), dev)
ar.setup_caches(max_batch_size=max(sizes))
alc, clc = specs.lr_config("v2_ar"), specs.lr_config("v2_cfm")
dc = specs.dit_config("v2")
vh = specs.bigvgan_config("22k")
cfm = CFM(dc, sd_of(specs.dit_state_spec(dc), 1234, "dit.v2."), dev)
voc = BigVGAN(vh, sd_of(specs.bigvgan_state_spec(vh), 1234, "bigvgan."), dev)
cfm_lr = InterpolateRegulator(clc, sd_of(specs.lr_state_spec(clc), 6, "lr."), dev)
hp = V2HotPath(ar, InterpolateRegulator(alc, sd_of(specs.lr_state_spec(alc), 5, "lr."), dev), cfm_lr, cfm, voc)
Cm, Dc, V = dc["C"], dc["Dc"], ac["vocab_size"]
FPT = P / N_TOK


def stats(ts):
    ts = sorted(ts)
    return {"ms": round(ts[len(ts) // 2], 3), "spread_ms": round(ts[-1] - ts[0], 3)}


def timed(fn, repeats=R, warm=1):
    """HIP-event time of fn() on the current stream, after `warm` untimed calls."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


records = []
for B in sizes:
    g = torch.Generator().manual_seed(B)
    target = hp.prepare_target(torch.randint(0, 32, (1, 40), generator=g), torch.randint(0, 2048, (1, 200), generator=g),
                               (torch.randn(1, Cm, P, generator=g) * 2 - 4).clamp(-11.5, 2), torch.randn(1, dc["style_dim"], generator=g))
    targets = [target] * B
    src = [torch.randint(0, 32, (1, 80), generator=g).to(dev) for _ in range(B)]
    seeds = list(range(1000, 1000 + B))
    if args.ragged:
        import random
        n0 = [int(o["tokens"].shape[1]) for o in hp.convert_batch(src, targets, [FPT] * B, STEPS, max_new=N_TOK, seeds=seeds)]
        want = [120 + round((P - 120) * i / max(B - 1, 1)) for i in range(B)]
        random.Random(0).shuffle(want)
        fpt = [(w + 0.5) / k for w, k in zip(want, n0)]            # int(fpt_b * n_b) = want_b: the token counts follow the seeds alone
        zfix = torch.randn(B, Cm, 2 * P, generator=g).to(dev)     # the sampler's noise, fixed: both settings convert the same mels
        run = lambda: hp.convert_batch(src, targets, fpt, STEPS, cfg_rates=(0.7, 0.7), max_new=N_TOK, seeds=seeds, z=zfix)      # noqa: E731
        stage_names = ("ar", "lr_assembly", "cfm", "strip_vocoder")
        per = {sw: {k: [] for k in stage_names + ("composite",)} for sw in (True, False)}
        outs = {}
        for sw in (True, False):
            hp.ragged_vocoder = sw
            run()
            outs[sw] = run()
        for _ in range(R):
            for sw in (True, False):
                hp.ragged_vocoder = sw
                torch.cuda.synchronize()
                hp.marks = []
                run()
                torch.cuda.synchronize()
                ev = dict(hp.marks)
                hp.marks = None
                prev = ev["start"]
                for k in stage_names:
                    per[sw][k].append(prev.elapsed_time(ev[k]))
                    prev = ev[k]
                per[sw]["composite"].append(ev["start"].elapsed_time(ev["strip_vocoder"]))
        S = [int(o["mel"].shape[2]) for o in outs[True]]
        hop = outs[True][0]["wave"].shape[1] // S[0]
        rec = {"workload": "BASELINE config 5 as one call, all output lengths different", "B": B, "repeats": R,
               "tokens_per_utterance": [min(n0), max(n0)], "frames_per_utterance": [min(S), max(S)], "mel_frames": sum(S),
               "vocoder_groups": len(set(S)), "sampler_steps": STEPS,
               "same_tokens_and_mels": bool(all(torch.equal(a["tokens"], b["tokens"]) and torch.equal(a["mel"], b["mel"])
                                                for a, b in zip(outs[True], outs[False]))),
               "waves_bit_identical_from_192_frames": bool(all(torch.equal(a["wave"], b["wave"])
                                                               for a, b in zip(outs[True], outs[False]) if a["mel"].shape[2] >= 192)),
               "wave_samples_per_frame": hop}
        for sw, name in ((True, "ragged_vocoder_on"), (False, "ragged_vocoder_off")):
            rec[name] = {"composite": stats(per[sw]["composite"]), "stages_in_composite": {k: stats(per[sw][k]) for k in stage_names},
                         "mel_frames_per_s": round(sum(S) / stats(per[sw]["composite"])["ms"] * 1e3, 1)}
        print(json.dumps(rec), flush=True)
        records.append(rec)
        continue
    run = lambda: hp.convert_batch(src, targets, [FPT] * B, STEPS, cfg_rates=(0.7, 0.7), max_new=N_TOK, seeds=seeds)      # noqa: E731
    out = run()
    run()
    n_tok = [int(o["tokens"].shape[1]) for o in out]
    frames = sum(int(o["mel"].shape[2]) for o in out)
    stage_names = ("ar", "lr_assembly", "cfm", "strip_vocoder")
    per = {k: [] for k in stage_names + ("composite",)}
    for _ in range(R):
        torch.cuda.synchronize()
        hp.marks = []
        run()
        torch.cuda.synchronize()
        ev = dict(hp.marks)
        hp.marks = None
        prev = ev["start"]
        for k in stage_names:
            per[k].append(prev.elapsed_time(ev[k]))
            prev = ev[k]
        per["composite"].append(ev["start"].elapsed_time(ev["strip_vocoder"]))
    rec = {"workload": "BASELINE config 5 as one call", "B": B, "repeats": R, "tokens_per_utterance": [min(n_tok), max(n_tok)],
           "mel_frames": frames, "vocoder_groups": len({int(o["mel"].shape[2]) for o in out}), "sampler_steps": STEPS,
           "composite": stats(per["composite"]),
           "stages_in_composite": {k: stats(per[k]) for k in stage_names}}
    comp = rec["composite"]["ms"]
    rec["mel_frames_per_s"] = round(frames / comp * 1e3, 1)
    rec["ar_share_of_composite"] = round(rec["stages_in_composite"]["ar"]["ms"] / comp, 4)

    # ---- the same stages alone
    ar_cond = hp.ar_lr(torch.cat([target["narrow"], src[0]], 1), in_lens=[120])[0]
    texts, tgts = [ar_cond] * B, [target["tokens"]] * B
    alone = {"ar": stats(timed(lambda: ar.generate_batch_raw(texts, tgts, max_new=N_TOK, seeds=seeds))),
             "ar_prefill_first_token": stats(timed(lambda: ar.generate_batch_raw(texts, tgts, max_new=1, seeds=seeds)))}
    toks, n = ar.generate_batch_raw(texts, tgts, max_new=N_TOK, seeds=seeds)
    S = [int(FPT * k) for k in n]
    Smax, T = max(S), P + max(S)
    pc = target["prompt_condition"].repeat(B, 1, 1)
    state = {}

    def lr_assembly():
        cond = cfm_lr(toks[:, :max(n)].long().clamp_(max=2047), ylens=torch.LongTensor(S), in_lens=n)[0]
        state["mu"] = _assemble_cond(pc, [P] * B, cond, S, T)

    def sampler():
        state["mel"] = cfm.inference(state["mu"], [P + s for s in S], target["mel"].repeat(B, 1, 1), target["style"].repeat(B, 1), None,
                                     STEPS, inference_cfg_rate=[0.7, 0.7], prompt_lens=[P] * B)

    def strip_vocoder():
        state["wave"] = voc(_strip_prompt(state["mel"], [P] * B, [P + s for s in S], Smax))

    alone["lr_assembly"] = stats(timed(lr_assembly))
    alone["cfm"] = stats(timed(sampler))
    alone["strip_vocoder"] = stats(timed(strip_vocoder))
    rec["stages_alone"] = alone
    total_alone = sum(alone[k]["ms"] for k in stage_names)
    rec["sum_of_stages_alone_ms"] = round(total_alone, 3)
    rec["glue_ms"] = round(comp - total_alone, 3)
    rec["ar_prefill_ms"] = alone["ar_prefill_first_token"]["ms"]
    rec["ar_decode_ms"] = round(alone["ar"]["ms"] - alone["ar_prefill_first_token"]["ms"], 3)
    rec["ar_prefill_share_of_generate"] = round(alone["ar_prefill_first_token"]["ms"] / alone["ar"]["ms"], 4)
    rec["ar_tokens_per_s"] = round(sum(n) / alone["ar"]["ms"] * 1e3, 1)

    if B == max(sizes):
        # seeded against explicit noise, alternating; the explicit draws are the seeds' own, already in the call's layout
        q = torch.stack([ar.exp_draws(s, 0, N_TOK) for s in seeds])
        variants = {"seeded": lambda: ar.generate_batch_raw(texts, tgts, max_new=N_TOK, seeds=seeds),
                    "explicit": lambda: ar.generate_batch_raw(texts, tgts, exp_noise=q, max_new=N_TOK)}
        ts = {k: [] for k in variants}
        for f in variants.values():
            f()
        for _ in range(R):
            for k, f in variants.items():
                ts[k] += timed(f, repeats=1, warm=0)
        same = torch.equal(variants["seeded"]()[0], variants["explicit"]()[0])
        rec["seeded_vs_explicit"] = {k: stats(v) for k, v in ts.items()}
        rec["seeded_vs_explicit"]["same_tokens"] = bool(same)
        rec["seeded_vs_explicit"]["explicit_noise_bytes"] = int(q.numel() * 4)
        del q
    print(json.dumps(rec), flush=True)
    records.append(rec)

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/v2_bench.py", "records": records}, f, indent=1)
        f.write("\n")
