"""References, bounds and cases of the length regulator's op-level suite (test_host_lr.py, test_gpu_lr_ops.py): the four kernels of
csrc/lr.hip, one launch each through ops.lr_stage.

What is EXACT (no tolerance)
  index map   index_map(n_out, n_in) = F.interpolate(arange(n_in), size=n_out, mode="nearest") on the CPU.  It is the fp32 formula
              min(floor(float(t) * (float(n_in) / float(n_out))), n_in - 1), NOT t * n_in // n_out: sensitive_pairs() recomputes the
              83 pairs with n_in <= 64, n_out < 130 on which the two differ.
  zeros       rows t >= ylens[b] over all ld columns, pad channels [C, ld) of live rows, the statistics' slots without a row
  additions   gather's content + f0 row is one fp32 addition: fl(a + b), bit for bit

f0 bin.  The reference is the float64 chain of f0_to_coarse on the fp32 input (a, b as the Python doubles of the reference):
    pre = 1127 ln(1 + f0 / 700) a - b,  bin = post(round_half_even(pre)),  post: c <= 0 -> 1, c >= n_bins -> 0
fp32 may land on either neighbour where pre lies within delta(f0) of a half-integer.  delta is the sum of the roundings of the fp32
chain, u = 2^-24, each carried to pre (d pre / d mel = a, d mel / d l = 1127, d l / d s = 1 / s):
    q = fl(f0 / 700), s = fl(1 + q)      relative error of s <= 2 u, so |dl| <= 2 u
    l = logf(s)                          K_LOG = 2 ulp (HIP documents 1 for logf; 1 more for the CPU's), ulp(l) <= 2 u l
    mel = fl(1127 l)                     u mel
    a32 = fl(a), b32 = fl(b)             u mel a + u |b|
    fl(mel a32), fl(. - b32)             u mel a + u |pre|     (a fused multiply-add drops the first of the two)
    delta = u (1127 a (2 + 2 K_LOG l) + 3 mel a + |b| + |pre|)
At n_bins = 256 (a = 0.257) and f0 = 1600 Hz (l = 1.19, mel = 1341, pre = 326) this is 3342 u = 1.99e-4; at 100 Hz it is 5.0e-5.
The float64 chain's own error (1e-13) is nothing against it.  A uniform grid lies inside delta with probability 2 delta per unit
of pre: 0.04 % at most, and test_host_lr.py holds the share of set (a) to 0.1 %.

GroupNorm sums.  stats[b][i] = (sum, sum of squares) over rows [i rpb, min((i + 1) rpb, len)) x C, rpb = ceil(len / 32), in double.
The reference is the correctly rounded sum (math.fsum; v * v of an fp32 v is exact in double).  Any order of n - 1 double additions is
within (n - 1) u64 sum|v| of the exact sum (u64 = 2^-53), the reference within u64 |S|: bound n u64 sum|v|, and n u64 Q for the squares.

gn_mish.  The reference folds the 32 partials it is GIVEN exactly (Fractions), so it shares the kernel's input and only the
kernel's own arithmetic is judged:  mean = S / n, var = max(Q / n - mean^2, 0), rstd = (var + eps)^-1/2,
v = (x - mean) rstd gamma + beta, o = v tanh(softplus(v)), softplus with F.softplus's threshold 20.  Bound per element:
    dvar  = u64 (32 Q / n + 2 |mean| (31 sum|S_i| / n + |mean|) + mean^2 + var)       the double fold, divide, square, subtract
    e_r   = r + dvar / (2 (var + eps)) + 3 u64                                        rstd = (float)(1 / sqrt(var + eps))
    E_v   = rstd |gamma| (r |mean| + r |d|) + |d rstd gamma| (e_r + 2 r) + r |v|      mu = (float)mean; x - mu; two products; + beta
    E_sp  = 2 K_EXP u sigmoid(v) + 2 K_LOG1P u sp                                     expf, log1pf: 2 ulp each (HIP documents 1)
    E_o   = |f'(v)| E_v + E_v^2 + |v| ((1 - th^2) E_sp + 2 K_TANH u th) + r |o| + (3 |v| + 1) 2^-126
with f' = th + v (1 - th^2) sigmoid(v), th = tanh(sp); the last term covers e, sp or th falling below the smallest normal fp32
(flushed or denormal).  r = 2 u: every fp32 rounding is booked at ONE ulp although +, - and x are correctly rounded (u), just as the
functions are booked at twice their documented error.  With r = u the bound is the exact first-order worst case, which a sum of four
aligned roundings can approach; the factor of two is what test_host_lr.py asks the CPU emulation to leave unused (it must stay
under HALF the bound, that is, under the worst case itself).  The term r |mean| rstd |gamma| is the price of subtracting a MEAN
ROUNDED TO fp32, as the reference module does too; it dominates when the input carries an offset (1e3: 1.2e-4 per unit of
rstd gamma).
Whether softplus applies its threshold cannot be seen in o: between 20 and the overflow of exp the two forms differ by e^-v < 2.1e-9,
and 1 - tanh(20) = 8.5e-18, so tanh is 1.0 in fp32 and float64 alike.  The sabotage is therefore held where it can be seen, at
softplus64 against F.softplus in float64 (test_host_lr.py); the GPU suite feeds v = 20 +- a few ulp all the same.
"""
import functools
import math
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

import cases as G

U = 2.0 ** -24
U64 = 2.0 ** -53
R = 2 * U                                     # an fp32 rounding booked at one ulp (see gn_mish above)
TINY = 2.0 ** -126
K_LOG = K_EXP = K_LOG1P = K_TANH = 2          # ulp; an ulp of y is at most 2 u |y|
PARTS = 32                                    # lr.hip's LR_GN_PARTS
CPAD = 32                                     # cpad(c, 1): channels padded to the fp32 k-tile
GUARD = 2
FILL = -777.25
EPS = float(np.float32(1e-5))
MEL_MIN = 1127 * math.log(1 + 50.0 / 700)
MEL_MAX = 1127 * math.log(1 + 1100.0 / 700)

SABOTAGES = ("index_exact", "index_divide", "round_half_away", "overflow_to_last", "stats_len_off_by_one", "stats_fp32",
             "softplus_no_threshold", "pads_unwritten")


def ld_of(C):
    return -(-C // CPAD) * CPAD


# ------------------------------------------------------------------------------------------------ the index map
@functools.lru_cache(maxsize=None)
def index_map(n_out, n_in):
    """(n_out,) long: F.interpolate(mode='nearest') of arange(n_in) to n_out on the CPU -- the definition, exact"""
    return F.interpolate(torch.arange(n_in, dtype=torch.float32)[None, None], size=n_out, mode="nearest")[0, 0].long()


def index_formula(n_out, n_in, form="float"):
    """the map by formula (numpy): 'float' the fp32 one of the kernel and the oracle, 'exact' t n_in // n_out, 'divide'
    floor(float(t) / (float(n_out) / float(n_in)))"""
    t = np.arange(n_out)
    if form == "exact":
        idx = t * n_in // n_out
    elif form == "divide":
        idx = np.floor(t.astype(np.float32) / (np.float32(n_out) / np.float32(n_in))).astype(np.int64)
    else:
        idx = np.floor(t.astype(np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64)
    return np.minimum(idx, n_in - 1)


@functools.lru_cache(maxsize=None)
def sensitive_pairs(tin_max=64, ylen_max=129):
    """(tin, ylen) on which the fp32 formula and the exact integer map differ at one position at least"""
    return tuple((tin, ylen) for tin in range(1, tin_max + 1) for ylen in range(1, ylen_max + 1)
                 if (index_formula(ylen, tin) != index_formula(ylen, tin, "exact")).any())


@functools.lru_cache(maxsize=None)
def benign_pairs():
    """as many pairs on which the two agree: tin = 1, ylen = 1, tin == ylen, shrinking and growing ones, the committed small pairs"""
    fixed = [(1, 1), (1, 2), (1, 31), (1, 129), (5, 1), (64, 1), (2, 1), (17, 17), (32, 32), (33, 33), (64, 64), (31, 26), (45, 37),
             (64, 31), (64, 33), (50, 32), (33, 32), (23, 41), (31, 37), (19, 33), (7, 129), (64, 128), (64, 65), (32, 64), (3, 100)]
    rng = np.random.Generator(np.random.Philox(key=[83, 1]))
    bad = set(sensitive_pairs())
    out = []
    for p in fixed + [(int(a), int(b)) for a, b in zip(rng.integers(1, 65, 400), rng.integers(1, 130, 400))]:
        if p not in bad and p not in out:
            out.append(p)
        if len(out) == 83:
            break
    return tuple(out)


NO_INTERP_PAIRS = ((17, 17), (17, 9), (40, 1), (33, 32), (64, 64), (64, 31), (1, 1))       # interpolate = 0: src = t, ylen <= tin
MODEL_PAIRS = ((26, 22), (14, 46), (21, 69), (3, 123))                                   # the whole-model cases of test_gpu_lr.py


def source_index(ylen, tin, interpolate=1, sab=None):
    if not interpolate:
        return torch.arange(ylen)
    if sab in ("index_exact", "index_divide"):
        return torch.from_numpy(index_formula(ylen, tin, sab[6:]))
    return index_map(ylen, tin)


# ------------------------------------------------------------------------------------------------ the f0 bin
def f0_ab(n_bins):
    a = (n_bins - 2) / (MEL_MAX - MEL_MIN)
    return a, MEL_MIN * a - 1.0


def f0_pre64(f0, n_bins):
    """the float64 pre-round value of fp32 f0 (finite, >= 0)"""
    a, b = f0_ab(n_bins)
    mel = 1127.0 * torch.log(1.0 + f0.double() / 700.0)
    return torch.where(mel > 0, mel * a - b, mel)


def f0_post(c, n_bins, sab=None):
    """the integer tail of f0_to_coarse: c <= 0 -> 1; c >= n_bins -> 0 (the reference's quirk)"""
    c = c.long().clamp(min=1)
    return torch.where(c < n_bins, c, torch.full_like(c, n_bins - 1 if sab == "overflow_to_last" else 0))


def _round(p, sab=None):
    return torch.sign(p) * torch.floor(p.abs() + 0.5) if sab == "round_half_away" else torch.round(p)


def f0_bin64(f0, n_bins, sab=None):
    return f0_post(_round(f0_pre64(f0, n_bins), sab), n_bins, sab)


def f0_delta(f0, n_bins):
    a, b = f0_ab(n_bins)
    l = torch.log(1.0 + f0.double() / 700.0)
    mel = 1127.0 * l
    return U * (1127.0 * a * (2 + 2 * K_LOG * l) + 3 * mel * a + abs(b) + (mel * a - b).abs())


def f0_judgement(f0, n_bins):
    """(bin64, inside, lo, hi): outside `inside` the bin is bin64; inside, post(floor(pre)) or post(floor(pre) + 1)"""
    pre = f0_pre64(f0, n_bins)
    fl = torch.floor(pre)
    inside = ((pre - fl - 0.5).abs() <= f0_delta(f0, n_bins)) & (pre > 0)
    return f0_bin64(f0, n_bins), inside, f0_post(fl, n_bins), f0_post(fl + 1, n_bins)


def f0_bin32(f0, n_bins, form="two", sab=None):
    """the fp32 chain on the CPU: 'two' = torch's (product and difference rounded separately, the oracle's lr_f0_to_coarse), 'fma' =
    one rounding of mel a32 - b32 (the product of two fp32 is exact in double)"""
    a, b = f0_ab(n_bins)
    a32, b32 = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    mel = 1127.0 * torch.log(1.0 + f0 / 700.0)
    assert mel.dtype == torch.float32
    p = (mel.double() * a32.double() - b32.double()).float() if form == "fma" else mel * a32 - b32
    return f0_post(_round(torch.where(mel > 0, p, mel), sab), n_bins, sab)


def f0_pre32(f0, n_bins, form="two"):
    a, b = f0_ab(n_bins)
    a32, b32 = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    mel = 1127.0 * torch.log(1.0 + f0 / 700.0)
    p = (mel.double() * a32.double() - b32.double()).float() if form == "fma" else mel * a32 - b32
    return torch.where(mel > 0, p, mel)


def f0_grid():
    """(a) a uniform grid of 16384 values on [0, 1600] Hz"""
    return torch.linspace(0.0, 1600.0, 16384, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def f0_boundaries(n_bins, side=8):
    """(b) for each boundary pre = k + 0.5, k = 1 .. n_bins - 1 (the last one is the overflow edge): the fp32 nearest the float64
    boundary and `side` neighbours on either side -> (n_bins - 1, 2 side + 1)"""
    a, b = f0_ab(n_bins)
    k = np.arange(1, n_bins, dtype=np.float64)
    mid = (700.0 * np.expm1((k + 0.5 + b) / a / 1127.0)).astype(np.float32)
    cols = {0: mid}
    up = dn = mid
    for i in range(1, side + 1):
        up = np.nextafter(up, np.float32(np.inf))
        dn = np.nextafter(dn, np.float32(-np.inf))
        cols[i], cols[-i] = up, dn
    return torch.from_numpy(np.stack([cols[i] for i in range(-side, side + 1)], 1))


def f0_quirks(n_bins):
    """(c) 0 and everything up to 50 Hz -> bin 1; 1100 Hz; the first values that overflow to bin 0; far above; and the inputs of
    set (b) whose float64 pre-round value is k + 0.5 exactly (half to even), if there are any"""
    edge = f0_boundaries(n_bins)[-1]
    first = edge[f0_bin64(edge, n_bins) == 0][:4]
    assert first.numel() >= 1
    allb = f0_boundaries(n_bins).reshape(-1)
    pre = f0_pre64(allb, n_bins)
    ties = allb[(pre - torch.floor(pre)) == 0.5]
    return torch.cat([torch.tensor([0.0, 1e-30, 1.0, 49.9, 50.0, 1100.0, 1500.0, 1600.0, 1e4, 3e38], dtype=torch.float32), first, ties])


def f0_set(n_bins):
    """sets (a), (b), (c) for n_bins, one vector"""
    return torch.cat([f0_grid(), f0_boundaries(n_bins).reshape(-1), f0_quirks(n_bins)])


F0_UNSPECIFIED = (float("nan"), float("inf"), float("-inf"), -1.0, -700.0, -701.0)          # (e): membership only


# ------------------------------------------------------------------------------------------------ the GroupNorm sums
def slot_rows(length, i):
    rpb = -(-length // PARTS)
    return i * rpb, min((i + 1) * rpb, length)


def stats_ref(x, ylens, C, sab=None):
    """x (B, T, ld) fp32 -> (ref, E): (B, 32, 2) float64 each"""
    B = x.shape[0]
    ref, E = torch.zeros(B, PARTS, 2, dtype=torch.float64), torch.zeros(B, PARTS, 2, dtype=torch.float64)
    for b in range(B):
        length = ylens[b] - 1 if sab == "stats_len_off_by_one" else ylens[b]
        for i in range(PARTS):
            r0, r1 = slot_rows(max(length, 0), i)
            if r1 <= r0:
                continue
            v = x[b, r0:r1, :C].reshape(-1)
            if sab == "stats_fp32":
                ref[b, i, 0], ref[b, i, 1] = float(v.sum(dtype=torch.float32)), float((v * v).sum(dtype=torch.float32))
            else:
                d = v.double()
                ref[b, i, 0], ref[b, i, 1] = math.fsum(d.tolist()), math.fsum((d * d).tolist())
            n = v.numel()
            E[b, i, 0], E[b, i, 1] = n * U64 * float(v.double().abs().sum()), n * U64 * float((v.double() ** 2).sum())
    return ref, E


def stats_emulate(x, ylens, C):
    """the same sums by plain float64 accumulation, in the order the kernel's threads take (4 row phases x 64 channel lanes, then
    a tree)"""
    B = x.shape[0]
    out = torch.zeros(B, PARTS, 2, dtype=torch.float64)
    for b in range(B):
        for i in range(PARTS):
            r0, r1 = slot_rows(ylens[b], i)
            if r1 <= r0:
                continue
            d = x[b, r0:r1, :C].double()
            parts = [d[p::4, lane::64] for p in range(4) for lane in range(64)]
            s = torch.stack([torch.cumsum(p.reshape(-1), 0)[-1] if p.numel() else torch.zeros((), dtype=torch.float64) for p in parts])
            q = torch.stack([torch.cumsum((p * p).reshape(-1), 0)[-1] if p.numel() else torch.zeros((), dtype=torch.float64) for p in parts])
            while s.numel() > 1:
                h = s.numel() // 2
                s, q = s[:h] + s[h:], q[:h] + q[h:]
            out[b, i, 0], out[b, i, 1] = s[0], q[0]
    return out


# ------------------------------------------------------------------------------------------------ GroupNorm + Mish
def softplus64(v, sab=None):
    if sab == "softplus_no_threshold":
        return torch.log1p(torch.exp(v))
    return torch.where(v > 20, v, torch.log1p(torch.exp(v.clamp(max=20.0))))


def fold_exact(stats_b, n):
    """(mean, var, sum|S_i|, Q) of one utterance's (32, 2) partials, folded exactly"""
    S = sum((Fraction(float(s)) for s in stats_b[:, 0]), Fraction(0))
    Q = sum((Fraction(float(q)) for q in stats_b[:, 1]), Fraction(0))
    mean = S / n
    var = max(Q / n - mean * mean, Fraction(0))
    return float(mean), float(var), float(stats_b[:, 0].abs().sum()), float(Q)


def mish_ref(x, stats, gamma, beta, ylens, C, eps=EPS, sab=None):
    """x (B, T, ld) fp32, stats (B, 32, 2) float64 -> (ref, E) (B, T, ld) float64: zeros (E = 0) in dead rows and pad channels"""
    B, T, ld = x.shape
    ref, E = torch.zeros(B, T, ld, dtype=torch.float64), torch.zeros(B, T, ld, dtype=torch.float64)
    if sab == "pads_unwritten":
        ref[:, :, C:] = FILL
    g, be = gamma.double()[None], beta.double()[None]
    for b in range(B):
        L = ylens[b]
        if L == 0:
            continue
        n = L * C
        mean, var, sabs, Q = fold_exact(stats[b], n)
        dvar = U64 * (32 * Q / n + 2 * abs(mean) * (31 * sabs / n + abs(mean)) + mean * mean + var)
        rstd = 1.0 / math.sqrt(var + eps)
        e_r = R + dvar / (2 * (var + eps)) + 3 * U64
        d = x[b, :L, :C].double() - mean
        core = d * rstd * g
        v = core + be
        E_v = rstd * g.abs() * (R * abs(mean) + R * d.abs()) + core.abs() * (e_r + 2 * R) + R * v.abs()
        sp = softplus64(v, sab)
        th = torch.tanh(sp)
        sig = torch.sigmoid(v)
        o = v * th
        E_sp = torch.where(v > 20, torch.zeros_like(v), 2 * K_EXP * U * sig + 2 * K_LOG1P * U * sp)
        fp = th + v * (1 - th * th) * sig
        ref[b, :L, :C] = o
        E[b, :L, :C] = fp.abs() * E_v + E_v * E_v + v.abs() * ((1 - th * th) * E_sp + 2 * K_TANH * U * th) + R * o.abs() + (3 * v.abs() + 1) * TINY
    return ref, E


def mish_emulate(x, stats, gamma, beta, ylens, C, eps=EPS):
    """the kernel's arithmetic on the CPU: double fold in index order, fp32 elementwise (torch's expf / log1pf / tanhf)"""
    B, T, ld = x.shape
    out = torch.zeros(B, T, ld, dtype=torch.float32)
    for b in range(B):
        L = ylens[b]
        if L == 0:
            continue
        s = q = torch.zeros((), dtype=torch.float64)
        for i in range(PARTS):
            s, q = s + stats[b, i, 0], q + stats[b, i, 1]
        n = float(L * C)
        mean = s / n
        var = (q / n - mean * mean).clamp(min=0.0)
        rstd = (1.0 / torch.sqrt(var + eps)).float()
        v = (x[b, :L, :C] - mean.float()) * rstd * gamma[None] + beta[None]
        sp = torch.where(v > 20, v, torch.log1p(torch.exp(v)))
        out[b, :L, :C] = v * torch.tanh(sp)
    return out


def judge(ref, E, got, scale=1.0):
    """(number of elements outside scale * E, worst error / E over the elements with E > 0); E = 0 means exact"""
    err = (got.double() - ref).abs()
    bad = int((~(err <= scale * E)).sum())
    live = E > 0
    worst = float((err[live] / E[live]).max()) if bool(live.any()) else 0.0
    return bad, worst


# ------------------------------------------------------------------------------------------------ inputs
def gn_input(tag, seed, B, T, C, ylens, offset=0.0, constant=None, pad=float("nan")):
    """x (B, T, ld): N(offset, 1) in the live region (or a constant), `pad` in dead rows and pad channels"""
    ld = ld_of(C)
    x = torch.full((B, T, ld), pad, dtype=torch.float32)
    body = G.randn(tag, seed, B, T, C) + offset
    if constant is not None:
        body = torch.full((B, T, C), constant, dtype=torch.float32)
    for b in range(B):
        x[b, :ylens[b], :C] = body[b, :ylens[b]]
    return x


STATS_LENS = (1, 31, 32, 33, 64, 65, 430)
STATS_CHANNELS = (64, 80)


def stats_cases():
    """name -> (x, ylens, C): every length of STATS_LENS (plus an empty utterance) in one launch per C, NaN in everything the kernel
    may not read; and the same with an offset of 1e3"""
    out = {}
    for C in STATS_CHANNELS:
        ylens = list(STATS_LENS) + [0]
        for name, off in ((f"C{C}", 0.0), (f"C{C}-offset1e3", 1e3)):
            out[name] = (gn_input("lrops.stats." + name, 3, len(ylens), max(ylens), C, ylens, offset=off), ylens, C)
    return out


def mish_params(tag, C):
    """gamma, beta with special channels: v = 20 +- a few ulp (beta 20, gamma 2e-6 k), v > 20, large negative v"""
    gamma = 1.0 + 0.3 * G.randn(tag + ".g", 5, C)
    beta = 0.5 * G.randn(tag + ".b", 5, C)
    for c, (g, be) in enumerate(((2e-6, 20.0), (-4e-6, 20.0), (8e-6, 20.0), (1.0, 25.0), (1.0, 100.0), (1.0, -30.0), (1.0, -90.0), (1.0, -200.0),
                                 (1.0, 20.0), (0.0, 20.0))):
        gamma[c], beta[c] = g, be
    return gamma, beta


def mish_cases():
    """name -> (x, stats, gamma, beta, ylens, C); stats are the reference's partials of x (correctly rounded doubles)"""
    out = {}
    for C in STATS_CHANNELS:
        ylens = [1, 33, 65, 0, 37]
        for name, kw in ((f"C{C}", {}), (f"C{C}-offset1e3", dict(offset=1e3)), (f"C{C}-constant", dict(constant=0.75))):
            x = gn_input("lrops.mish." + name, 4, len(ylens), max(ylens), C, ylens, **kw)
            gamma, beta = mish_params("lrops.mish." + name, C)
            out[name] = (x, stats_ref(x, ylens, C)[0], gamma, beta, ylens, C)
    return out


# ------------------------------------------------------------------------------------------------ the whole model in float64
def model64(sd, cfg, x, ylen, f0=None):
    """O.lr_forward restated in float64 from the stage references above: (1, T, out)"""
    sd = {k: v.double() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    C = cfg["channels"]
    h = sd["embedding.weight"][x[0]] if cfg["is_discrete"] else x[0].double() @ sd["content_in_proj.weight"].t() + sd["content_in_proj.bias"]
    tin = h.shape[0]
    interpolate = cfg["n_convs"] > 0
    T = ylen if interpolate else tin
    h = h[source_index(T, tin, interpolate)]
    if cfg["f0_condition"]:
        if f0 is None:
            h = h + sd["f0_mask"]
        else:
            h = h + sd["f0_embedding.weight"][f0_bin64(f0[0], cfg["n_f0_bins"])][index_map(T, f0.shape[1])]
    for i in range(cfg["n_convs"]):
        h = F.conv1d(h.t()[None], sd[f"model.{3 * i}.weight"], sd[f"model.{3 * i}.bias"], padding=1)[0].t()
        n = h.numel()
        mean = math.fsum(h.reshape(-1).tolist()) / n
        var = math.fsum(((h - mean) ** 2).reshape(-1).tolist()) / n
        v = (h - mean) / math.sqrt(var + EPS) * sd[f"model.{3 * i + 1}.weight"][None] + sd[f"model.{3 * i + 1}.bias"][None]
        h = v * torch.tanh(softplus64(v))
    kt = f"model.{3 * cfg['n_convs']}.weight"
    if kt in sd:
        h = F.conv1d(h.t()[None], sd[kt], sd[f"model.{3 * cfg['n_convs']}.bias"])[0].t()
    out = h[None].clone()
    if not interpolate and cfg["version"] == 1:
        out[:, min(ylen, tin):] = 0
    return out
