"""Cases, float64 reference, fp32 emulation and checks of the AR sampler (csrc/ar_sampler.h) at op level, shared by
test_host_ar_sampler.py (which checks that the checks can tell a right kernel from a subtly wrong one) and
test_gpu_ar_sampler.py (which holds the kernels to them through ops.ar_sampler and ARModel.sample).  CPU only, plain torch
ops; nothing here calls the library.

Kernels: ar_rank_kernel / ar_rank_batch_kernel (penalty, suppression, counting rank), ar_sample_kernel /
ar_sample_batch_kernel (top-p scan, temperature softmax, exponential race, the loop state of one sequence and of the slots).

THREE KINDS OF CASE
  sample  (form 0)  logits [V], prev, suppress, rep_pen, T, top_p, q [V] -> idx, probs [V]
  loop1   (form 1)  one GenState: logits [V], toks [max_new], noise [max_new][V] or a seed, emb [V][D], pos [2], cnt
                    -> toks[cnt], next_x [D], pos + 1, cnt + 1, probs
  slots   (form 2)  B GenSlots in Bp = round_up(B, 16) rows -> per slot toks[cnt], cnt, done, pos, next_x row
  A loop1 case and every slot of a slots case reduce to a sample case (`loop1_sample`, `slot_sample`): the penalty sees
  toks[0] only, EOS is suppressed while cnt < min_before_eos, the draws are noise row t or those of (seed, t), t =
  min(cnt, max_new - 1).  Seeded draws are -log(u) of v2_chain_cases.reference_uniforms in float64.

REFERENCE, float64 (`ref_sample`): penalty from the ORIGINAL logits (score < 0 ? score * rp : score / rp; duplicates do
  not compound), suppression, torch.sort(descending, stable), cum = cumsum(exp(s - s0)) divided by its own last element
  (so top_p = 1 keeps all), removed where cum > float32(top_p) but never sorted position 0, kept logits / max(T, 1e-5),
  softmax, winner argmax(p / q) with ties to the lower index.  rp, T and top_p enter as the fp32 values the kernel receives.
  NaN logits and an all -inf vector are not specified and not covered.
  The loop state (`ref_loop1`, `ref_slots`) is a plain Python restatement of the tails of ar_sample_kernel and
  ar_sample_batch_kernel; test_host_ar_sampler.py runs it as a generate loop against seedvc_oracle.ar_generate.

CASE CONDITIONS, asserted here from the reference alone (`assert_conditions`; nothing is skipped or relaxed at run time)
  cut     for top_p < 1 every cum[i], i >= 1, is at least 1e-5 from top_p (~100 fp32 ulps of a sum near 1); a planted cut
          (top_p = float32 of the midpoint of cum[k-1] and cum[k]) has p_sorted[k] >= 2e-5.
  race    the winner's p / q is at least 1 + 1e-3 times the best other ratio; exact ties (same logit, same q: the same
          arithmetic in any precision) count as one winner, the lower index.
  clamp   T below 1e-5 is used only where the top two kept logits differ by >= 1e-2: the result is exactly one-hot.

CHECKS (`check_sample`, `check_loop1`, `check_slots`)
  support  exact: p == 0 wherever the reference removed (or the reference's p < 2^-149), p > 0 wherever it kept (p_ref > 2^-119)
  winner   equals the reference's
  sum      |sum(p) - 1| <= 1e-5
  kept p   |p - p_ref| <= p_ref 2^-23 (16 + 4 max_kept|lg'| / T_eff) + 2^-120.  The argument of the second softmax is
           lg' * (1 / T) - max in fp32: lg' (a penalised logit rounds once), 1 / T, the product and the difference round once
           each, 2^-24 of |lg'| / T apiece, for the element and for the terms of the sum (4 x 2 x 2^-24); 16 x 2^-23 covers
           expf, the fp32 sum over up to 4096 terms (DPP tree) and the division; the floor covers flushed denormals.  A cut
           off by one element moves every kept p by ~1 / k relative (1e-3 at k = 1024); the bound at T = 0.7 is ~1e-5.
  state    integers exact: cnt, done, pos, the written toks[t]; canaries and untouched rows exact; next_x bit-equal to the
           expected row of emb.

MEASURED (nothing above depends on it).  Worst error / bound of the kept probabilities: the fp32 emulation below on the CPU
0.175; on an MI355X 0.129 through form 0 and through ARModel.sample (the V = 4096 tie cases), 0.077 through form 1, 0.093 over
the slots' own cases; all below 0.5.  Smallest p_sorted[k] of a planted cut: 2.92e-5.

SABOTAGES of the emulation (`SAMPLE_SABOTAGES`, `LOOP_SABOTAGES`): each names the cases in which at least one check must fail.
"""
import functools
import math

import numpy as np
import torch

import v2_chain_cases as P

NINF = float("-inf")
CANARY32 = -777.25
CANARY_TOK = -7777
GUARD = 2
VS = (1, 2, 15, 16, 17, 65, 255, 256, 257, 1023, 1025, 4093, 4096)
KS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
TEMPS = (0.0, 1e-6, 0.05, 0.7, 2.0)
SUM_TOL = 1e-5
CUT_MARGIN = 1e-5
P_AT_CUT = 2e-5
RACE_MARGIN = 1.0 + 1e-3
CLAMP_GAP = 1e-2


def f32(v):
    return float(np.float32(v))


T_CLAMP = f32(1e-5)


def _gen(*key):
    """a generator seeded by the key's text (FNV-1a: the same on every machine and run)"""
    h = 2166136261
    for ch in "|".join(str(k) for k in key):
        h = ((h ^ ord(ch)) * 16777619) & 0xFFFFFFFF
    return torch.Generator().manual_seed(h & 0x7FFFFFFF)


def base_logits(V, tied, *key):
    lg = 0.5 * torch.randn(V, generator=_gen("lg", V, tied, *key))
    return torch.round(lg * 4) / 4 if tied else lg


def exp_q(V, *key):
    u = torch.rand(V, generator=_gen("q", V, *key)).clamp_min(2.0 ** -24)
    return -torch.log(u)


def seeded_q(seed, step, V):
    """the draws of (seed, step) as the sampler defines them, from the float64 uniforms"""
    return torch.from_numpy(-np.log(P.reference_uniforms(int(seed), int(step), 1, V)[0])).float()


# ------------------------------------------------------------------------------------------------ reference, float64
def penalised64(lg, prev, suppress, rep_pen):
    x = lg.double().clone()
    if prev:
        pt = torch.tensor(list(prev), dtype=torch.long)
        sc = lg.double()[pt]
        rp = f32(rep_pen)
        x[pt] = torch.where(sc < 0, sc * rp, sc / rp)
    if suppress is not None and suppress >= 0:
        x[suppress] = NINF
    return x


def ref_sample(c):
    V = c["V"]
    x = penalised64(c["logits"], c["prev"], c["suppress"], c["rep_pen"])
    s, order = torch.sort(x, descending=True, stable=True)
    cum = torch.cumsum(torch.exp(s - s[0]), 0)
    cum = cum / cum[-1]
    rem = cum > f32(c["top_p"])
    rem[0] = False
    keep = torch.ones(V, dtype=torch.bool)
    keep[order] = ~rem
    t_eff = max(f32(c["T"]), T_CLAMP)
    z = torch.where(keep, x, torch.full_like(x, NINF))
    p = torch.softmax(z / t_eff, 0)
    r = p / c["q"].double()
    win = int((r == r.max()).nonzero()[0])
    live = keep & torch.isfinite(x)
    bound = p * 2.0 ** -23 * (16 + 4 * float(x[live].abs().max()) / t_eff) + 2.0 ** -120
    return dict(x=x, sorted=s, order=order, cum=cum, keep=keep, k=int((~rem).sum()), p=p, r=r, win=win, bound=bound, t_eff=t_eff)


def race_margin(r):
    """winner's ratio over the best ratio that is not exactly equal to it (inf when nothing else is positive)"""
    top = r["r"].max()
    rest = r["r"][r["r"] != top]
    nxt = float(rest.max()) if rest.numel() else 0.0
    return math.inf if nxt <= 0 else float(top) / nxt


def cut_margin(c, r):
    if f32(c["top_p"]) >= 1.0 or c["V"] == 1:
        return math.inf
    return float((r["cum"][1:] - f32(c["top_p"])).abs().min())


def plant_cut(c, k):
    """top_p that keeps exactly k sorted entries: the fp32 midpoint of cum[k-1] and cum[k]; k = V: top_p = 1"""
    if k >= c["V"]:
        c["top_p"] = 1.0
        return c
    cum = ref_sample(dict(c, top_p=1.0))["cum"]
    c["top_p"] = f32((float(cum[k - 1]) + float(cum[k])) / 2)
    c["planted_k"] = k
    return c


def plant_winners(c, idxs):
    """shrink q at idxs (one shared value) so that they beat every other entry by a factor >= 2"""
    r = ref_sample(c)
    others = torch.ones(c["V"], dtype=torch.bool)
    others[list(idxs)] = False
    best_other = float(r["r"][others].max()) if others.any() else 0.0
    p_min = min(float(r["p"][i]) for i in idxs)
    assert p_min > 0, c["id"]
    if best_other > 0:
        c["q"] = c["q"].clone()
        c["q"][list(idxs)] = f32(0.5 * p_min / best_other)
    return c


def settle_race(c):
    """random draws: where the reference's margin is below the condition, halve the winner's q until it holds"""
    for _ in range(4):
        r = ref_sample(c)
        if race_margin(r) >= 1.01:
            break
        c["q"] = c["q"].clone()
        c["q"][r["win"]] *= 0.5
    return c


def sample_case(cid, V, logits, q, prev=(), suppress=None, rep_pen=1.0, T=0.7, top_p=1.0, **kw):
    return dict(id=cid, V=V, logits=logits.float(), q=q.float(), prev=list(prev), suppress=suppress, rep_pen=rep_pen, T=T, top_p=top_p, **kw)


@functools.lru_cache(maxsize=None)
def sample_cases():
    out = []
    # ---- planted top-p cuts at every seam of the scan, plain and tied; top_p = 1, 0 and below the first probability
    for V in VS:
        for tied in (False, True):
            name = f"V{V}-{'tied' if tied else 'plain'}"
            lg, q = base_logits(V, tied, "cut"), exp_q(V, "cut", tied)
            for k in sorted(set(k for k in KS + (V - 1,) if 1 <= k <= V - 1)):
                out.append(plant_cut(sample_case(f"cut-{name}-k{k}", V, lg, q), k))
            out.append(sample_case(f"cut-{name}-all", V, lg, q, top_p=1.0))
            out.append(sample_case(f"cut-{name}-p0", V, lg, q, top_p=0.0))
            p0 = float(ref_sample(sample_case("", V, lg, q))["cum"][0])
            out.append(sample_case(f"cut-{name}-below", V, lg, q, top_p=f32(p0 / 2)))
    # ---- an all-equal vector: the cut falls inside the one tie group, the lower indices survive
    for V, ks in ((17, (5, 16)), (4096, (5, 1025, 4095))):
        lg, q = torch.full((V,), 0.3), exp_q(V, "equal")
        for k in ks:
            out.append(plant_cut(sample_case(f"equal-V{V}-k{k}", V, lg, q), k))
        out.append(sample_case(f"equal-V{V}-all", V, lg, q, top_p=1.0))
    # ---- -inf entries besides the suppressed one
    V = 257
    lg, q = base_logits(V, False, "ninf"), exp_q(V, "ninf")
    lg[[3, 100, 256]] = NINF
    out.append(plant_cut(sample_case("ninf-V257-k100", V, lg, q, suppress=7), 100))
    out.append(sample_case("ninf-V257-all", V, lg, q, suppress=7, top_p=1.0))
    # ---- temperature: 0 and 1e-6 hit the clamp (one-hot), 0.05 / 0.7 / 2.0 are ordinary
    for V in (65, 1025):
        lg, q = base_logits(V, False, "temp"), exp_q(V, "temp")
        lg[int(lg.argmax())] += 0.5
        for T in TEMPS:
            out.append(plant_cut(sample_case(f"temp-V{V}-T{T}", V, lg, q, T=T, onehot=T < 1e-5), V // 2))
    # ---- repetition penalty: duplicates, a positive, a negative and an exact zero logit, the suppressed token; n_prev up to V
    for V in (17, 257, 4093):
        lg, q = base_logits(V, False, "pen"), exp_q(V, "pen")
        order = torch.argsort(lg, descending=True)
        a_pos, sup, a_neg, z = int(order[0]), int(order[1]), int(order[V // 2 + V // 4]), int(order[V // 3])
        assert lg[a_pos] > 0 and lg[a_neg] < 0
        lg[z] = 0.0
        g = _gen("prev", V)
        for rp in (1.0, 1.5):
            for n_prev in (0, 1, 7, 300, V):
                prev = {0: [], 1: [a_pos], 7: [a_pos, a_neg, z, sup, a_pos, a_pos, a_neg]}.get(n_prev)
                if prev is None and n_prev == 300:
                    prev = [a_pos, sup, z, a_neg] + torch.randint(0, V, (296,), generator=g).tolist()
                elif prev is None:
                    prev = torch.randperm(V, generator=g).tolist()
                c = sample_case(f"pen-V{V}-rp{rp}-n{n_prev}", V, lg, q, prev=prev, suppress=sup, rep_pen=rp)
                out.append(plant_cut(c, max(1, V // 2)))
    # ---- the race: planted winners at the seams of both race loops, and exact ties (the lower index wins)
    for V in (1025, 4096):
        lg, q = base_logits(V, False, "race"), exp_q(V, "race")
        for i in sorted(set(i for i in (0, 3, 4, 1023, 1024, V - 1) if i < V)):
            out.append(plant_winners(sample_case(f"race-V{V}-win{i}", V, lg, q, top_p=1.0), [i]))
    for V, pairs in ((257, ((5, 6), (5, 69))), (4096, ((5, 6), (5, 69), (5, 1029), (2047, 3071)))):
        for i, j in pairs:
            lg, q = base_logits(V, False, "tie"), exp_q(V, "tie")
            lg[i] = lg[j] = float(lg.max()) + 0.5
            out.append(plant_winners(sample_case(f"tie-V{V}-{i}-{j}", V, lg, q, top_p=1.0, tie=(i, j)), [i, j]))
    for c in out:
        if "tie" not in c:
            settle_race(c)
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


def sample_case_by_id(cid):
    return next(c for c in sample_cases() if c["id"] == cid)


# ------------------------------------------------------------------------------------------------ loop state cases
def _favoured(lg, a, cl, eos, eos_favoured):
    """toks[0] = a and the last input cl share the top logit M; EOS sits above both where it is favoured"""
    lg = lg.clone()
    m = float(lg.max()) + 1.0
    lg[a] = lg[cl] = m
    lg[eos] = m + 1.0 if eos_favoured else min(float(lg[eos]), m - 2.0)
    return lg


def loop1_sample(c, sab=None):
    """the sample case a loop1 case reduces to (ar_rank_body / ar_sample_kernel with gs)"""
    t = c["cnt"]
    pen_tok = int(c["toks"][t - 1 if sab == "penalty_last_token" else 0])
    mbe = c["min_before_eos"] - (1 if sab == "suppress_skipped_at_boundary" else 0)
    q = c["noise"][t] if c["noise"] is not None else seeded_q(c["seed"], t, c["V"])
    return sample_case(c["id"], c["V"], c["logits"], q, prev=[pen_tok], suppress=c["eos"] if t < mbe else None, rep_pen=c["rep_pen"],
                       T=c["T"], top_p=c["top_p"])


def _plant_loop_q(sc, trio):
    """noise row of a loop case: the favoured tokens share one small q, so the race among them is decided by p alone"""
    r = ref_sample(sc)
    live = [i for i in trio if float(r["p"][i]) > 0]
    return plant_winners(sc, live)["q"]


@functools.lru_cache(maxsize=None)
def loop1_cases():
    out = []
    V, eos, mbe, max_new = 65, 64, 10, 16
    for cnt, D, with_noise in ((8, 8, True), (9, 8, True), (10, 8, True), (11, 1100, True), (9, 1100, False), (12, 8, False)):
        cid = f"loop1-cnt{cnt}-D{D}-{'noise' if with_noise else 'seeded'}"
        g = _gen(cid)
        toks = torch.randint(0, V - 1, (max_new,), generator=g, dtype=torch.int32)
        a, cl = 11, 40
        toks[0], toks[cnt - 1] = a, cl
        lg = _favoured(base_logits(V, False, cid), a, cl, eos, True)
        c = dict(id=cid, V=V, D=D, logits=lg, toks=toks, emb=torch.randn(V, D, generator=g), pos=[5, 9], cnt=cnt, min_before_eos=mbe,
                 eos=eos, T=0.7, top_p=1.0, rep_pen=1.5, max_new=max_new, noise=None, seed=0)
        if with_noise:
            c["noise"] = -torch.log(torch.rand(max_new, V, generator=g).clamp_min(2.0 ** -24))
            c["top_p"] = plant_cut(loop1_sample(c), 20)["top_p"]
            c["noise"][cnt] = _plant_loop_q(loop1_sample(c), (a, cl, eos))
        else:
            for seed in range(1000 + cnt, 1040 + cnt):
                c["seed"] = seed
                c["top_p"] = plant_cut(loop1_sample(c), 20)["top_p"]
                if race_margin(ref_sample(loop1_sample(c))) >= 1.01:
                    break
        out.append(c)
    return tuple(out)


SLOT_SHAPES = ((1, 257, 24), (5, 65, 1100), (17, 1023, 24), (64, 4096, 16))      # (B, V, D)
SLOT_KINDS = ("live", "eos_drawn", "eos_suppressed", "last_token", "input_pos_full", "kv_pos_full", "done", "done_at_max_new")
SLOT_MAX_NEW, SLOT_LMAX, SLOT_MBE = 8, 40, 4


def slot_sample(c, b, sab=None):
    """the sample case slot b reduces to (ar_rank_body with gs = slot b, ar_sample_batch_kernel)"""
    t = c["cnt"][b]
    row = min(t, c["max_new_s"][b] - 1)
    pen_tok = int(c["toks"][b, t - 1 if sab == "penalty_last_token" else 0])
    mbe = c["min_before_eos"][b] - (1 if sab == "suppress_skipped_at_boundary" else 0)
    q = c["noise"][b, row] if c["has_noise"][b] else seeded_q(c["seed"][b], row, c["V"])
    return sample_case(f"{c['id']}-slot{b}", c["V"], c["logits"][b], q, prev=[pen_tok], suppress=c["eos"][b] if t < mbe else None,
                       rep_pen=c["rep_pen"][b], T=c["T"][b], top_p=c["top_p"][b])


@functools.lru_cache(maxsize=None)
def slots_cases():
    out = []
    for B, V, D in SLOT_SHAPES:
        cid = f"slots-B{B}-V{V}-D{D}"
        g = _gen(cid)
        eos, MN = V - 1, SLOT_MAX_NEW
        c = dict(id=cid, B=B, V=V, D=D, Lmax=SLOT_LMAX, max_new=MN, emb=torch.randn(V, D, generator=g),
                 logits=torch.zeros(B, V), toks=torch.randint(0, V - 1, (B, MN), generator=g, dtype=torch.int32),
                 noise=torch.full((B, MN, V), float("nan")), kind=[], cnt=[], done=[], max_new_s=[], min_before_eos=[SLOT_MBE] * B,
                 eos=[eos] * B, has_noise=[], T=[], top_p=[1.0] * B, rep_pen=[], seed=[0] * B, pos=[[], []])
        for b in range(B):
            kind = SLOT_KINDS[b % 8]
            c["kind"].append(kind)
            cnt, mn, done, ip, kp = 5, MN, 0, 7 + b % 5, 20 + b % 7
            if kind == "eos_suppressed":
                cnt = SLOT_MBE - 1
            elif kind == "last_token":
                cnt, mn = 6, 7
            elif kind == "input_pos_full":
                ip = SLOT_LMAX - 1
            elif kind == "kv_pos_full":
                kp = SLOT_LMAX - 1
            elif kind == "done":
                done = 1
            elif kind == "done_at_max_new":
                done, cnt, mn = 1, 6, 6
            c["cnt"].append(cnt); c["max_new_s"].append(mn); c["done"].append(done)
            c["pos"][0].append(ip); c["pos"][1].append(kp)
            c["has_noise"].append(int(((b // 8) + (b % 8)) % 2 == 0))
            c["T"].append((0.7, 2.0, 0.05, 1.0)[b % 4])
            c["rep_pen"].append(1.0 if b % 3 == 1 else 1.5)
            a, cl, last = 3 + b % 7, 12 + b % 5, 20 + b % 9         # toks[0], the favoured token, a finished slot's last input
            c["toks"][b, 0] = a
            c["toks"][b, cnt - 1] = last if done else cl
            c["logits"][b] = _favoured(base_logits(V, False, cid, b), a, cl, eos, kind in ("eos_drawn", "eos_suppressed"))
            k = min(V - 1, (2, 9, 30, 64)[b % 4])
            if c["has_noise"][b]:
                row = min(cnt, mn - 1)
                c["noise"][b] = -torch.log(torch.rand(MN, V, generator=g).clamp_min(2.0 ** -24))
                c["top_p"][b] = plant_cut(slot_sample(c, b), k)["top_p"]
                c["noise"][b, row] = _plant_loop_q(slot_sample(c, b), (a, cl, eos))
            elif kind == "eos_drawn":
                c["top_p"][b] = 0.0                               # seeded draws cannot be planted: only EOS, the top logit, survives
                c["seed"][b] = 77 + b
            else:
                for seed in range(5000 + 50 * b, 5050 + 50 * b):
                    c["seed"][b] = seed
                    c["top_p"][b] = plant_cut(slot_sample(c, b), k)["top_p"]
                    if race_margin(ref_sample(slot_sample(c, b))) >= 1.01:
                        break
        out.append(c)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ loop state, reference
def ref_loop1(c):
    """ar_sample_kernel's gs branch: token cnt recorded, embedded as the next input, positions and counter advanced"""
    r = ref_sample(loop1_sample(c))
    toks = c["toks"].clone()
    toks[c["cnt"]] = r["win"]
    return dict(win=r["win"], sample=r, toks=toks, next_x=c["emb"][r["win"]].clone(), pos=[c["pos"][0] + 1, c["pos"][1] + 1], cnt=c["cnt"] + 1)


def ref_slot_step(win, toks, cnt, done, max_new, eos, ip, kp, Lmax):
    """ar_sample_batch_kernel's tail for one slot -> (token embedded next, toks, cnt, done, ip, kp).  A finished slot records
    nothing and keeps its last input; EOS finishes the slot and is not counted (it is written at toks[cnt]); a recorded token
    finishes the slot when it was the last of max_new or when the next position would leave the cache (positions then stay)."""
    toks = list(toks)
    if done:
        return toks[cnt - 1], toks, cnt, 1, ip, kp
    toks[cnt] = win
    if win == eos:
        return toks[cnt - 1], toks, cnt, 1, ip, kp
    if cnt + 1 >= max_new or ip + 1 >= Lmax or kp + 1 >= Lmax:
        return win, toks, cnt + 1, 1, ip, kp
    return win, toks, cnt + 1, 0, ip + 1, kp + 1


def ref_slots(c):
    B, Bp = c["B"], (c["B"] + 15) // 16 * 16
    e = dict(win=[], sample=[], cnt=[], done=[], pos=[[], []], toks=c["toks"].clone(), next_x=torch.full((Bp, c["D"]), CANARY32))
    for b in range(B):
        r = ref_sample(slot_sample(c, b))
        tk, toks, cnt, done, ip, kp = ref_slot_step(r["win"], c["toks"][b].tolist(), c["cnt"][b], c["done"][b], c["max_new_s"][b], c["eos"][b],
                                                    c["pos"][0][b], c["pos"][1][b], c["Lmax"])
        e["win"].append(r["win"]); e["sample"].append(r); e["cnt"].append(cnt); e["done"].append(done)
        e["pos"][0].append(ip); e["pos"][1].append(kp)
        e["toks"][b] = torch.tensor(toks, dtype=torch.int32)
        e["next_x"][b] = c["emb"][tk]
    return e


# ------------------------------------------------------------------------------------------------ conditions
def assert_sample_conditions(c, r=None):
    r = r or ref_sample(c)
    assert cut_margin(c, r) >= CUT_MARGIN, (c["id"], "cut margin", cut_margin(c, r))
    if "planted_k" in c:
        k = c["planted_k"]
        assert r["k"] == k, (c["id"], r["k"])
        p_sorted = torch.diff(r["cum"], prepend=torch.zeros(1, dtype=torch.float64))
        assert float(p_sorted[k]) >= P_AT_CUT, (c["id"], "p at the cut", float(p_sorted[k]))
    assert race_margin(r) >= RACE_MARGIN, (c["id"], "race margin", race_margin(r))
    assert (c["q"] > 0).all() and torch.isfinite(c["q"]).all(), c["id"]
    if "tie" in c:
        i, j = c["tie"]
        assert r["r"][i] == r["r"][j] == r["r"].max() and r["win"] == i < j, c["id"]
    if f32(c["T"]) < T_CLAMP:
        kept = r["x"][r["keep"]].sort(descending=True).values
        assert kept.numel() < 2 or float(kept[0] - kept[1]) >= CLAMP_GAP, c["id"]
        assert float(r["p"].max()) == 1.0 and int((r["p"] > 0).sum()) == 1, c["id"]


def assert_conditions():
    """every condition the docstring lists, for every case; returns the smallest p_sorted[k] of the planted cuts"""
    smallest = math.inf
    inside_tie = 0
    for c in sample_cases():
        r = ref_sample(c)
        assert_sample_conditions(c, r)
        if "planted_k" in c:
            k = c["planted_k"]
            smallest = min(smallest, float(r["cum"][k] - r["cum"][k - 1]))
            inside_tie += int("tied" in c["id"] and float(r["sorted"][k - 1]) == float(r["sorted"][k]))
    assert inside_tie >= 20, inside_tie           # cuts inside a tie group: the lower indices must survive
    for c in loop1_cases():
        assert_sample_conditions(loop1_sample(c))
        assert int(c["toks"][0]) != int(c["toks"][c["cnt"] - 1]) and 1 <= c["cnt"] < c["max_new"]
    for c in slots_cases():
        e = ref_slots(c)
        for b in range(c["B"]):
            assert_sample_conditions(slot_sample(c, b), e["sample"][b])
            kind, win = c["kind"][b], e["win"][b]
            assert int(c["toks"][b, 0]) != int(c["toks"][b, c["cnt"][b] - 1])
            assert (win == c["eos"][b]) == (kind == "eos_drawn"), (c["id"], b, kind, win)
            if c["done"][b]:
                assert win != int(c["toks"][b, c["cnt"][b] - 1]), (c["id"], b)        # a finished slot must not embed the winner
            assert 0 <= min(c["toks"][b].tolist()) and max(c["toks"][b].tolist()) < c["V"]
        if c["B"] >= 17:
            assert set(zip(c["kind"], c["has_noise"])) == set((k, n) for k in SLOT_KINDS for n in (0, 1)), c["id"]
    return smallest


# ------------------------------------------------------------------------------------------------ fp32 emulation
SAMPLE_SABOTAGES = {
    # name -> ids of the sample cases that target it
    "rank_ties_higher_index_first": ("cut-V4096-tied-k1024", "equal-V17-k5"),
    "penalty_compounded_over_duplicates": ("pen-V257-rp1.5-n7", "pen-V17-rp1.5-n300"),
    "penalty_after_suppression": ("pen-V257-rp1.5-n7", "pen-V4093-rp1.0-n4093"),
    "scan_cross_wave_base_dropped": ("cut-V4096-plain-k1024", "cut-V1025-plain-k257"),
    "cut_plus_one": ("cut-V4096-plain-k1024", "cut-V17-plain-k1", "equal-V4096-k1025"),
    "cut_minus_one": ("cut-V4096-plain-k1025", "cut-V17-plain-k2", "equal-V4096-k5"),
    "sorted_position_0_not_protected": ("cut-V65-plain-p0", "cut-V4096-tied-below"),
    "temperature_before_top_p": ("temp-V1025-T0.05", "temp-V65-T2.0"),
    "clamp_missing": ("temp-V65-T0.0", "temp-V1025-T0.0"),
    "race_ties_higher_index": ("tie-V4096-5-6", "tie-V4096-5-69", "tie-V4096-5-1029", "tie-V257-5-69"),
}
LOOP_SABOTAGES = {
    # name -> (loop1 case ids, (slots case id, slot kind that shows it) pairs)
    "suppress_skipped_at_boundary": (("loop1-cnt9-D8-noise",), (("slots-B17-V1023-D24", "eos_suppressed"),)),
    "penalty_last_token": (("loop1-cnt8-D8-noise",), (("slots-B1-V257-D24", "live"),)),
    "eos_counted": ((), (("slots-B5-V65-D1100", "eos_drawn"), ("slots-B64-V4096-D16", "eos_drawn"))),
    "max_new_off_by_one": ((), (("slots-B5-V65-D1100", "last_token"),)),
    "finished_slot_advances_positions": ((), (("slots-B17-V1023-D24", "done"), ("slots-B17-V1023-D24", "done_at_max_new"))),
    "finished_slot_embeds_winner": ((), (("slots-B17-V1023-D24", "done"),)),
    "rows_beyond_nb_written": ((), (("slots-B5-V65-D1100", None), ("slots-B17-V1023-D24", None))),
}


def emu_sample(c, sab=None):
    """fp32 emulation of ar_rank_body + ar_sample_body: fp32 penalty, stable counting rank, fp32 exp with a double running sum
    (thread t owns sorted 4t .. 4t+3, wave w the 256 from 256 w on), float compare, fp32 temperature softmax with lg * (1 / T),
    fp32 race.  Returns (idx, probs fp32 [V])."""
    V = c["V"]
    lg = c["logits"].float()
    x = lg.clone()
    rp = torch.tensor(c["rep_pen"], dtype=torch.float32)
    pen = lambda sc: torch.where(sc < 0, sc * rp, sc / rp)      # noqa: E731
    sup = c["suppress"] if c["suppress"] is not None and c["suppress"] >= 0 else None
    if sab == "penalty_after_suppression" and sup is not None:
        x[sup] = NINF
    if c["prev"]:
        pt = torch.tensor(c["prev"], dtype=torch.long)
        if sab == "penalty_compounded_over_duplicates":
            for t in c["prev"]:
                x[t] = pen(x[t])
        else:
            x[pt] = pen(lg[pt])
    if sab != "penalty_after_suppression" and sup is not None:
        x[sup] = NINF
    if sab == "rank_ties_higher_index_first":
        key, o = torch.sort(x.flip(0), descending=True, stable=True)
        order = V - 1 - o
    else:
        key, order = torch.sort(x, descending=True, stable=True)
    tinv = (torch.tensor(1.0, dtype=torch.float32) /
            (torch.tensor(c["T"], dtype=torch.float32) if sab == "clamp_missing" else torch.tensor(c["T"], dtype=torch.float32).clamp_min(1e-5)))
    d = key - key[0]
    e = torch.exp(d * tinv if sab == "temperature_before_top_p" else d)
    run = torch.cumsum(e.double(), 0)
    total = run[-1].clone()
    if sab == "scan_cross_wave_base_dropped":
        wave = torch.arange(V) // 256
        base = torch.zeros(V, dtype=torch.float64)
        for w in range(1, (V + 255) // 256):
            base[wave == w] = run[256 * w - 1]
        run = run - base
    cum = (run / total).float()
    rem = cum > torch.tensor(c["top_p"], dtype=torch.float32)
    if sab != "sorted_position_0_not_protected":
        rem[0] = False
    if sab == "cut_plus_one" and V > 1:
        rem = torch.cat([rem[:1], rem[:-1]])
    if sab == "cut_minus_one" and V > 2:
        rem = torch.cat([rem[:1], rem[2:], rem[-1:]])
    x = x.clone()
    x[order[rem]] = NINF
    arg = x * tinv
    ex = torch.exp(arg - arg.max())
    p = ex * (torch.tensor(1.0, dtype=torch.float32) / ex.sum())
    r = p / c["q"].float()
    hits = (r == r.max()).nonzero()
    if hits.numel() == 0:
        return 0, p                                  # NaN everywhere: no `r > best` ever holds, the kernel answers 0
    return int(hits[-1] if sab == "race_ties_higher_index" else hits[0]), p


def emu_loop1(c, sab=None):
    """what ops.ar_sampler returns for form 1: whole guarded buffers"""
    win, p = emu_sample(loop1_sample(c, sab), sab)
    G = GUARD
    toks = torch.full((2 * G + 1, c["max_new"]), CANARY_TOK, dtype=torch.int32)
    toks[G] = c["toks"]
    toks[G, c["cnt"]] = win
    next_x = torch.full((2 * G + 1, c["D"]), CANARY32)
    next_x[G] = c["emb"][win]
    probs = torch.full((2 * G + 1, c["V"]), CANARY32)
    probs[G] = p
    return dict(cnt=c["cnt"] + 1, pos=[c["pos"][0] + 1, c["pos"][1] + 1], toks=toks, next_x=next_x, probs=probs, guard=G)


def emu_slots(c, sab=None):
    """what ops.ar_sampler returns for form 2, from emu_sample and a restatement of the batch kernel's tail with its sabotages"""
    B, G, Lmax = c["B"], GUARD, c["Lmax"]
    Bp = (B + 15) // 16 * 16
    toks = torch.full((2 * G + B, c["max_new"]), CANARY_TOK, dtype=torch.int32)
    toks[G:G + B] = c["toks"]
    next_x = torch.full((2 * G + Bp, c["D"]), CANARY32)
    out = dict(cnt=list(c["cnt"]), done=list(c["done"]), pos=[list(c["pos"][0]), list(c["pos"][1])], toks=toks, next_x=next_x, guard=G, win=[])
    for b in range(Bp if sab == "rows_beyond_nb_written" else B):
        if b >= B:
            next_x[G + b] = c["emb"][0]
            continue
        win, _ = emu_sample(slot_sample(c, b, sab), sab)
        out["win"].append(win)
        t, was_done, mn = c["cnt"][b], c["done"][b], c["max_new_s"][b]
        record = not was_done and win != c["eos"][b]
        tk = win if record or (was_done and sab == "finished_slot_embeds_winner") else int(c["toks"][b, t - 1])
        next_x[G + b] = c["emb"][tk]
        if was_done:
            if sab == "finished_slot_advances_positions":
                out["pos"][0][b] += 1; out["pos"][1][b] += 1
            continue
        toks[G + b, t] = win
        if not record:
            out["done"][b] = 1
            if sab == "eos_counted":
                out["cnt"][b] = t + 1
            continue
        ip, kp = c["pos"][0][b] + 1, c["pos"][1][b] + 1
        out["cnt"][b] = t + 1
        if (t + 1 > mn if sab == "max_new_off_by_one" else t + 1 >= mn) or ip >= Lmax or kp >= Lmax:
            out["done"][b] = 1
        else:
            out["pos"][0][b], out["pos"][1][b] = ip, kp
    return out


# ------------------------------------------------------------------------------------------------ checks
def bits(t):
    return t.contiguous().view(torch.int32)


def check_sample(c, r, idx, probs):
    """-> (list of failed checks, worst error / bound over the kept entries or None).  probs fp32 [V] or None."""
    fails = []
    if idx != r["win"]:
        fails.append(f"winner {idx}, reference {r['win']}")
    if probs is None:
        return fails, None
    p = probs.double()
    must_zero = ~r["keep"] | (r["p"] < 2.0 ** -149)
    must_pos = r["keep"] & (r["p"] > 2.0 ** -119)
    if not bool((p[must_zero] == 0).all()):
        fails.append(f"support: {int((p[must_zero] != 0).sum())} removed entries are not zero")
    if not bool((p[must_pos] > 0).all()):
        fails.append(f"support: {int((~(p[must_pos] > 0)).sum())} kept entries are not positive")
    ratio = float(((p - r["p"]).abs() / r["bound"])[r["keep"]].max())
    if not ratio <= 1.0:
        fails.append(f"kept probabilities: error / bound = {ratio:.3g}")
    if not abs(float(p.sum()) - 1.0) <= SUM_TOL:
        fails.append(f"sum(p) = {float(p.sum())!r}")
    if c.get("onehot") and not (float(p[r["win"]]) == 1.0 and int((p != 0).sum()) == 1):
        fails.append("clamped temperature: not one-hot")
    return fails, ratio


def _guards_kept(buf, G, fill, what, fails):
    want = torch.full_like(buf[:G].cpu(), fill)
    if not (torch.equal(buf[:G].cpu(), want) and torch.equal(buf[-G:].cpu(), want)):
        fails.append(f"{what}: a canary row changed")


def check_loop1(c, e, got):
    """e = ref_loop1(c), got = what ops.ar_sampler (or emu_loop1) returned -> (fails, ratio)"""
    G = got["guard"]
    fails, ratio = check_sample(loop1_sample(c), e["sample"], int(got["toks"][G, c["cnt"]]), got["probs"][G].cpu())
    if got["cnt"] != e["cnt"] or list(got["pos"]) != e["pos"]:
        fails.append(f"cnt {got['cnt']} pos {got['pos']}, expected {e['cnt']} {e['pos']}")
    if not torch.equal(got["toks"][G].cpu(), e["toks"]):
        fails.append("toks: another entry than toks[cnt] changed, or toks[cnt] is wrong")
    if not torch.equal(bits(got["next_x"][G].cpu()), bits(e["next_x"])):
        fails.append("next_x is not the embedding row of the winner")
    _guards_kept(got["toks"], G, CANARY_TOK, "toks", fails)
    _guards_kept(got["next_x"], G, CANARY32, "next_x", fails)
    _guards_kept(got["probs"], G, CANARY32, "probs", fails)
    return fails, ratio


def check_slots(c, e, got):
    """e = ref_slots(c) -> {slot index or None: [failed checks]} (empty when all hold)"""
    G, B = got["guard"], c["B"]
    fails = {}
    toks, next_x = got["toks"].cpu(), got["next_x"].cpu()
    for b in range(B):
        f = []
        for name, g_, e_ in (("cnt", got["cnt"][b], e["cnt"][b]), ("done", got["done"][b], e["done"][b]),
                             ("input_pos", got["pos"][0][b], e["pos"][0][b]), ("kv_pos", got["pos"][1][b], e["pos"][1][b])):
            if g_ != e_:
                f.append(f"{name} {g_}, expected {e_}")
        if not torch.equal(toks[G + b], e["toks"][b]):
            f.append(f"toks {toks[G + b].tolist()}, expected {e['toks'][b].tolist()}")
        if not torch.equal(bits(next_x[G + b]), bits(e["next_x"][b])):
            f.append("next_x is not the expected embedding row")
        if f:
            fails[b] = [f"{c['kind'][b]}: " + s for s in f]
    f = []
    if not torch.equal(bits(next_x[G + B:-G]), bits(e["next_x"][B:])):
        f.append("next_x rows at and beyond nb were written")
    _guards_kept(toks, G, CANARY_TOK, "toks", f)
    _guards_kept(next_x, G, CANARY32, "next_x", f)
    if f:
        fails[None] = f
    return fails
