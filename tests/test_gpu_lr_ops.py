"""The length regulator's four kernels (csrc/lr.hip) at op level, through ops.lr_stage: ONE launch per call with the model's grid
and block on caller buffers.

lr_cases.py states the references, derives delta and the bounds and builds the cases; test_host_lr.py pins the references to torch
and the oracle, holds the CPU emulation to half the bounds and shows that every named sabotage is caught.  Held here:
  exact      every canary row keeps its fill, and so do the columns of `out` that mask_copy does not own; rows t >= ylens[b] are
             zero over all ld columns; pad channels [C, ld) of live rows are zero; what a kernel only reads is unchanged
  gather     content row r holds r and f0 embedding row k holds 1024 k, so every element of a row is source index + 1024 bin: the
             index is F.interpolate's map on all 83 float-versus-exact pairs and as many benign ones, in the feature and the token
             form, with and without interpolation, and the f0 track's index likewise; a bin is the float64 bin outside delta and one
             of the two neighbours inside; f0 = None adds f0_mask, bit for bit; non-finite and negative f0 pick SOME row of the table
  gn_stats   every partial within the bound of the correctly rounded sum, empty slots zero
  gn_mish    every element within the bound, v at 20 +- a few ulp, far below zero, var = 0, an offset of 1e3
  relations  bit for bit: the same launch twice; an utterance alone, at row 11 of 17 and at row 40 of 64; NaN against finite values
             in every row and column the kernel may not read

A device error other than a refusal ends the whole pytest session (pytest.exit, return code 3): nothing more is launched on a
device that has faulted, so a run that stops there is a FAILED run, not a short pass."""
import numpy as np
import pytest
import torch

import cases as G
import lr_cases as L

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def run(a):
    """one launch -> the written buffer between its canary rows (which must hold their fill); inputs must come back unchanged"""
    from seedvc_amd import ops
    try:
        o = ops.lr_stage(a, guard=L.GUARD, fill32=L.FILL)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "requirement failed" in str(e):
            raise
        pytest.exit(f"lr_stage {a['stage']}: the device reported an error, nothing more is launched: {e}", returncode=3)
    for name, t in o["inputs"].items():
        assert same(t.cpu(), a[name].to(t.dtype).contiguous()), f"{a['stage']}: the kernel wrote its input {name}"
    key = {"gather": "x", "gn_mish": "x", "gn_stats": "stats", "mask_copy": "out"}[a["stage"]]
    t = o[key].cpu()
    g = L.GUARD
    assert bool((t[:g] == L.FILL).all()) and bool((t[-g:] == L.FILL).all()), f"{a['stage']}: a canary row was written"
    return t[g:-g]


def dead_and_pads_are_zero(y, ylens, C):
    """y (B, T, ld): rows t >= ylens[b] over all columns and the pad channels of every row are zero"""
    for b, n in enumerate(ylens):
        assert bool((y[b, n:] == 0).all()), f"utterance {b}: a row at or above ylens is not zero"
        assert bool((y[b, :, C:] == 0).all()), f"utterance {b}: a pad channel is not zero"


# ------------------------------------------------------------------------------------------------ gather: the index maps
def _batches(pairs, n=64):
    return [pairs[i:i + n] for i in range(0, len(pairs), n)]


def _bin_centre(k, n_bins):
    a, b = L.f0_ab(n_bins)
    return (700.0 * np.expm1((np.asarray(k, dtype=np.float64) + b) / a / 1127.0)).astype(np.float32)


@pytest.mark.parametrize("form", ["features", "tokens"])
@pytest.mark.parametrize("interpolate", [1, 0])
def test_gather_index_is_the_interpolate_map(form, interpolate):
    pairs = list(L.sensitive_pairs() + L.benign_pairs()) if interpolate else list(L.NO_INTERP_PAIRS)
    n_bins, C = 256, 80 if form == "features" else 64
    ld = L.ld_of(C)
    centres = torch.from_numpy(_bin_centre(np.arange(64) + 2, n_bins))                    # f0 track position j sits in bin j + 2
    assert torch.equal(L.f0_bin64(centres, n_bins), torch.arange(64) + 2) and not bool(L.f0_judgement(centres, n_bins)[1].any())
    for batch in _batches(pairs):
        B = len(batch)
        tins, ylens = [p[0] for p in batch], [p[1] for p in batch]
        Tin, T = max(tins), max(ylens)
        a = dict(stage="gather", tout_max=T, C=C, ld=ld, ylens=ylens, in_lens=tins, interpolate=interpolate)
        if form == "features":                 # + the f0 track, tf0 -> ylen over the same pairs
            feat = torch.full((B, Tin, ld), NAN)
            f0 = torch.full((B, Tin), NAN)
            for b, n in enumerate(tins):
                feat[b, :n, :C] = torch.arange(n, dtype=torch.float32)[:, None]
                f0[b, :n] = centres[:n]
            a.update(feat=feat, f0=f0, f0_lens=tins, f0_emb=(1024.0 * torch.arange(n_bins, dtype=torch.float32))[:, None].repeat(1, C))
            tok = None
        else:
            tok = torch.full((B, Tin), 199, dtype=torch.int64)
            for b, n in enumerate(tins):
                tok[b, :n] = (torch.arange(n) * 5 + b) % 97
            a.update(tokens=tok, emb=torch.arange(200, dtype=torch.float32)[:, None].repeat(1, C))
        y = run(a).reshape(B, T, ld)
        dead_and_pads_are_zero(y, ylens, C)
        for b, (tin, ylen) in enumerate(batch):
            row = y[b, :ylen, :C]
            assert bool((row == row[:, :1]).all()), (tin, ylen, "the columns of a row disagree")
            src = L.source_index(ylen, tin, interpolate)
            v = row[:, 0].long()
            if form == "features":
                assert torch.equal(v % 1024, src), (tin, ylen, "content index")
                assert torch.equal(v // 1024 - 2, L.index_map(ylen, tin)), (tin, ylen, "f0 index")
            else:
                assert torch.equal(v, tok[b, src]), (tin, ylen, "token index")


# ------------------------------------------------------------------------------------------------ gather: the f0 bin
@pytest.mark.parametrize("n_bins", [256, 20])
def test_gather_f0_bin(n_bins):
    f = L.f0_set(n_bins)
    T, C = 4096, 64
    B = -(-f.numel() // T)
    f0 = torch.full((B * T,), 100.0)
    f0[:f.numel()] = f
    a = dict(stage="gather", tout_max=T, C=C, ld=L.ld_of(C), ylens=[T] * B, in_lens=[1] * B, interpolate=1, feat=torch.zeros(B, 1, C),
             f0=f0.reshape(B, T), f0_lens=[T] * B, f0_emb=torch.arange(n_bins, dtype=torch.float32)[:, None].repeat(1, C))
    y = run(a).reshape(B * T, -1)
    assert bool((y == y[:, :1]).all())
    got = y[:f.numel(), 0].long()
    b64, inside, lo, hi = L.f0_judgement(f, n_bins)
    wrong_out = (got != b64) & ~inside
    wrong_in = (got != lo) & (got != hi) & inside
    nb = L.f0_boundaries(n_bins).numel()
    sb = slice(L.f0_grid().numel(), L.f0_grid().numel() + nb)                               # set (b)
    two, fma = L.f0_bin32(f, n_bins, "two"), L.f0_bin32(f, n_bins, "fma")
    print(f"n_bins {n_bins}: {f.numel()} values, {int(inside.sum())} inside delta; device bin != float64 bin on {int((got != b64).sum())} (all inside delta: "
          f"{not bool(wrong_out.any())}); on set (b) the device differs from the two-rounding form on {int((got[sb] != two[sb]).sum())} and from the "
          f"single-rounding form on {int((got[sb] != fma[sb]).sum())} of {nb} (the forms differ from each other on {int((two[sb] != fma[sb]).sum())})")
    assert not bool(wrong_out.any()), ("outside delta", f[wrong_out][:8].tolist(), got[wrong_out][:8].tolist(), b64[wrong_out][:8].tolist())
    assert not bool(wrong_in.any()), ("inside delta", f[wrong_in][:8].tolist(), got[wrong_in][:8].tolist())


def test_gather_adds_one_table_row_bit_for_bit():
    """f0 = None: content + f0_mask; unspecified f0 (non-finite, negative): content + SOME row of the table; both fl(a + b)"""
    n_bins, C, n = 20, 80, len(L.F0_UNSPECIFIED)
    ld = L.ld_of(C)
    feat = torch.full((1, n, ld), NAN)
    feat[0, :, :C] = G.randn("lrops.add.x", 1, n, C)
    emb, mask = G.randn("lrops.add.emb", 1, n_bins, C), G.randn("lrops.add.mask", 1, C)
    a = dict(stage="gather", tout_max=n, C=C, ld=ld, ylens=[n], in_lens=[n], interpolate=1, feat=feat, f0_emb=emb, f0_mask=mask)
    y = run(a).reshape(n, ld)
    assert same(y[:, :C], feat[0, :, :C] + mask[None]) and bool((y[:, C:] == 0).all())
    y = run(dict(a, f0=torch.tensor([L.F0_UNSPECIFIED], dtype=torch.float32), f0_lens=[n])).reshape(n, ld)
    for t, v in enumerate(L.F0_UNSPECIFIED):
        cand = feat[0, t, :C][None] + emb
        hit = [k for k in range(n_bins) if same(cand[k], y[t, :C])]
        print(f"f0 = {v}: table row {hit}")
        assert hit, f"f0 = {v}: the row is content + no row of the table"
    assert bool((y[:, C:] == 0).all())


# ------------------------------------------------------------------------------------------------ the GroupNorm pair, mask_copy
def test_gn_stats_within_the_bound():
    worst_all = 0.0
    for name, (x, ylens, C) in L.stats_cases().items():
        B, T, ld = x.shape
        got = run(dict(stage="gn_stats", tout_max=T, C=C, ld=ld, ylens=ylens, x=x)).reshape(B, L.PARTS, 2)
        ref, E = L.stats_ref(x, ylens, C)
        bad, worst = L.judge(ref, E, got)
        print(f"gn_stats {name}: worst error / bound {worst:.3f}")
        assert not bad, name                     # E = 0 in the slots without a row: exactly zero there
        worst_all = max(worst_all, worst)
    print(f"gn_stats: worst error / bound {worst_all:.3f}")


def test_gn_mish_within_the_bound():
    worst_all = 0.0
    for name, (x, stats, gamma, beta, ylens, C) in L.mish_cases().items():
        B, T, ld = x.shape
        got = run(dict(stage="gn_mish", tout_max=T, C=C, ld=ld, ylens=ylens, x=x, stats=stats, gamma=gamma, beta=beta, eps=L.EPS)).reshape(B, T, ld)
        dead_and_pads_are_zero(got, ylens, C)
        ref, E = L.mish_ref(x, stats, gamma, beta, ylens, C)
        bad, worst = L.judge(ref, E, got)
        print(f"gn_mish {name}: worst error / bound {worst:.3f}")
        assert not bad, name
        worst_all = max(worst_all, worst)
    print(f"gn_mish: worst error / bound {worst_all:.3f}")


@pytest.mark.parametrize("ld_out", [80, 96])
def test_mask_copy(ld_out):
    ylens, T, N, ld = [37, 0, 1, 64, 33], 64, 80, 96
    x = G.randn("lrops.copy", 2, len(ylens), T, ld)
    x[:, :, N:] = NAN
    for b, n in enumerate(ylens):
        x[b, n:] = NAN
    y = run(dict(stage="mask_copy", tout_max=T, ld=ld, ylens=ylens, x=x, N=N, ld_out=ld_out)).reshape(len(ylens), T, ld_out)
    assert bool((y[:, :, N:] == L.FILL).all()), "a column at or above N was written"
    for b, n in enumerate(ylens):
        assert same(y[b, :n, :N], x[b, :n, :N]) and bool((y[b, n:, :N] == 0).all()), b


# ------------------------------------------------------------------------------------------------ relations, bit for bit
REL_C = 80


def _utt(stage, u):
    """the data of utterance u, whatever batch it sits in"""
    rng = np.random.Generator(np.random.Philox(key=[4242, u]))
    tin, ylen, tf = int(rng.integers(1, 65)), int(rng.integers(1, 130)), int(rng.integers(1, 65))
    d = dict(ylen=ylen, tin=tin, tf=tf)
    if stage == "gather":
        d["feat"] = G.randn("lrops.rel.feat", u, tin, REL_C)
        d["f0"] = torch.where(G.rand("lrops.rel.uv", u, tf) < 0.25, torch.zeros(tf), 60.0 + 1100.0 * G.rand("lrops.rel.f0", u, tf))
    else:
        d["x"] = G.randn("lrops.rel.x", u, ylen, REL_C) + (3.0 if u % 3 == 0 else 0.0)
        if stage == "gn_mish":
            d["stats"] = L.stats_ref(d["x"][None], [ylen], REL_C)[0][0]
    return d


def _batch(stage, ids, pad, T=None):
    """the launch of utterances `ids`, `pad` in everything the kernel may not read"""
    us = [_utt(stage, u) for u in ids]
    B, C, ld = len(us), REL_C, L.ld_of(REL_C)
    ylens = [u["ylen"] for u in us]
    T = T or max(ylens)
    a = dict(stage=stage, tout_max=T, C=C, ld=ld, ylens=ylens)
    if stage == "gather":
        Tin, Tf = max(u["tin"] for u in us), max(u["tf"] for u in us)
        feat, f0 = torch.full((B, Tin, ld), pad), torch.full((B, Tf), pad)
        for b, u in enumerate(us):
            feat[b, :u["tin"], :C], f0[b, :u["tf"]] = u["feat"], u["f0"]
        a.update(feat=feat, f0=f0, in_lens=[u["tin"] for u in us], f0_lens=[u["tf"] for u in us], interpolate=1,
                 f0_emb=G.randn("lrops.rel.emb", 1, 256, C))
    else:
        x = torch.full((B, T, ld), pad)
        for b, u in enumerate(us):
            x[b, :u["ylen"], :C] = u["x"]
        a.update(x=x)
        if stage == "gn_mish":
            a.update(stats=torch.stack([u["stats"] for u in us]), gamma=1.0 + 0.3 * G.randn("lrops.rel.g", 1, C), beta=0.5 * G.randn("lrops.rel.b", 1, C),
                     eps=L.EPS)
        elif stage == "mask_copy":
            a.update(N=C, ld_out=C)
    return a


def _rows(stage, a, y, b):
    """what the launch made of utterance b: its 32 partials, or its live rows"""
    if stage == "gn_stats":
        return y.reshape(-1, L.PARTS, 2)[b]
    return y.reshape(len(a["ylens"]), a["tout_max"], -1)[b, :a["ylens"][b]]


@pytest.mark.parametrize("stage", ["gather", "gn_stats", "gn_mish", "mask_copy"])
def test_relations_bit_for_bit(stage):
    u = 5
    alone = _batch(stage, [u], NAN)
    y1 = run(alone)
    assert same(run(alone), y1), "the same launch twice"
    want = _rows(stage, alone, y1, 0)
    ids17 = [100 + i for i in range(11)] + [u] + [200 + i for i in range(5)]
    ids64 = [300 + i for i in range(40)] + [u] + [400 + i for i in range(23)]
    for ids in (ids17, ids64):
        a = _batch(stage, ids, NAN)
        y = run(a)
        assert same(run(a), y), f"B = {len(ids)}: the same launch twice"
        assert same(_rows(stage, a, y, ids.index(u)), want), f"B = {len(ids)}: the utterance differs from itself alone"
        assert same(run(_batch(stage, ids, 0.625)), y), f"B = {len(ids)}: NaN where the kernel may not read changes the result"
        if stage in ("gather", "gn_mish"):
            dead_and_pads_are_zero(y.reshape(len(ids), a["tout_max"], -1), a["ylens"], REL_C)
