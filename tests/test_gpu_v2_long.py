"""GPU tests of whole-file v2 conversion, `V2HotPath.convert_long_batch`: the style branch chunk by chunk against the
oracle chain and its splice against `pipeline.stream_wave_chunks`; a file's result whatever shares the pool; the seam rule
on short chunks; the timbre branch bit for bit against `HotPath.convert_long_batch`; prompts without target tokens; the
edges; and padding that never leaks.  Reduced models and files of v2_long_cases.py."""
import functools

import numpy as np
import pytest
import torch

import ar_batch_cases as A
import seedvc_oracle as O
import v2_long_cases as L

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
WINDOW = 64          # max_context_window where the branch under test does not read it


@functools.lru_cache(maxsize=None)
def _hotpath():
    """One chain for the module (4 AR slots): every test leaves it usable, which the edge test relies on."""
    from seedvc_amd.ar import ARModel
    from seedvc_amd.cfm import CFM
    from seedvc_amd.length_regulator import InterpolateRegulator
    from seedvc_amd.pipeline import V2HotPath
    from seedvc_amd.vocoder import BigVGAN
    M = L.models()
    ar = ARModel(*M["ar"], DEV)
    ar.setup_caches(max_batch_size=4)
    return V2HotPath(ar, InterpolateRegulator(*M["ar_lr"], DEV), InterpolateRegulator(*M["cfm_lr"], DEV), CFM(*M["dit"], DEV),
                     BigVGAN(*M["voc"], DEV))


@functools.lru_cache(maxsize=None)
def _record(f):
    hp, u = _hotpath(), L.file_inputs(f)
    target = hp.prepare_target(u["target_narrow"], u["target_tokens"], u["target_mel"], u["style"])
    return dict(target=target, src_narrow=u["src_narrow"].to(DEV), src_tokens=u["src_tokens"].to(DEV),
                frames_per_token=u["frames_per_token"], source_frames=0)


def _pinned(fs, chunks_of=None):
    """exp_noise_fn / noise_fn of the files fs (in call order) from the case module's draws."""
    chunks_of = chunks_of or (lambda f: L.file_case(f)["chunks"])
    return dict(exp_noise_fn=lambda u, k: chunks_of(fs[u])[k]["noise"].to(DEV),
                noise_fn=lambda u, k, T: chunks_of(fs[u])[k]["z"][:, :, :T].to(DEV))


def _convert(fs, **kw):
    args = dict(max_context_window=WINDOW, hop=L.HOP, max_new=A.MAX_NEW, return_parts=True)
    args.update(kw)
    out = _hotpath().convert_long_batch([_record(f) for f in fs], L.N_STEPS, L.CFG_RATES, **args)
    torch.cuda.synchronize()
    return out


def _stream(parts, overlap_frame_len, kept_only=True):
    """Host `stream_wave_chunks` over a file's own kept chunk waves."""
    return torch.from_numpy(L.stream_reference([p["wave"][0].cpu().numpy() for p in parts if p["kept"]], overlap_frame_len, L.HOP))


def _check_chunk(part, ref, what):
    """tokens equal; ylen equal; mel mean abs error < 1e-3; wave RMS < 1e-4 against the oracle vocoder on the mel under test
    (the bounds of test_gpu_v2_chain._check_against)."""
    h, vsd = L.models()["voc"]
    toks, ylen, mel = ref
    assert torch.equal(part["tokens"].cpu(), toks), f"{what}: {part['tokens'].tolist()} vs {toks.tolist()}"
    assert part["ylen"] == ylen and part["mel"].shape == (1, mel.shape[1], ylen) and part["wave"].shape == (1, ylen * L.HOP)
    e_mel = (part["mel"].cpu() - mel).abs().mean().item()
    e_wav = (part["wave"].cpu() - O.bigvgan_forward(vsd, h, part["mel"].cpu()).reshape(1, -1)).pow(2).mean().sqrt().item()
    print(f"{what}: {toks.shape[1]} tokens, {ylen} frames, mel mean abs err {e_mel:.3e} (< 1e-3), wave RMS {e_wav:.3e} (< 1e-4)")
    assert e_mel < 1e-3 and e_wav < 1e-4


def _three_chunk_files():
    return [f for f in L.qualified() if len(L.file_case(f)["chunks"]) == 3]


# --------------------------------------------------------------------------------- 1. style branch, chunk by chunk, oracle
def test_style_branch_matches_the_oracle_chunk_by_chunk():
    f = [f for f in _three_chunk_files() if len({c["ylen"] for c in L.file_case(f)["chunks"]}) == 3][0]     # three lengths
    ov = 2
    waves, parts = _convert([f], ar_chunk_tokens=L.FILES[f][3], overlap_frame_len=ov, **_pinned([f]))
    assert len(parts[0]) == 3 and all(p["kept"] for p in parts[0])
    for j, part in enumerate(parts[0]):
        _check_chunk(part, L.oracle_chunk(f, j), f"file {f}, chunk {j}")
    want = _stream(parts[0], ov)
    assert waves[0].shape == (1, sum(p["ylen"] for p in parts[0]) * L.HOP - 2 * ov * L.HOP)
    assert torch.equal(waves[0][0].cpu(), want)


# ------------------------------------------------------------------------------------------------- 2. pool invariance
def test_a_file_does_not_depend_on_the_pool():
    """Three qualified files in one call with seeds, 4 AR slots and CFM micro-batches of 3 chunks; one chunk size for the
    call (9 tokens) cuts them into 3 + 3 + 4 chunks, so slots are recycled, there are four micro-batches and a seam of the
    last file crosses one.  Against each file alone: tokens equal; mel inside 1e-3 (the DiT's kernel forms agree to fp16
    rounding only); wave bit-identical wherever the mel is."""
    fs = [0, 1, 2]
    assert all(f in L.qualified() for f in fs)
    seeds, ov = [11, 2 ** 63 + 12, 13], 2
    kw = dict(ar_chunk_tokens=9, overlap_frame_len=ov, max_chunks=3)
    waves, parts = _convert(fs, seeds=seeds, **kw)
    n_chunks = [len(p) for p in parts]
    assert n_chunks == [3, 3, 4] and sum(n_chunks) >= 8
    live = [p["ylen"] > 0 for ps in parts for p in ps]
    assert all(live)                        # micro-batches are chunks 0-2, 3-5, 6-8, 9: file 2's last seam crosses one
    for i, f in enumerate(fs):
        alone_w, alone_p = _convert([f], seeds=[seeds[i]], **kw)
        same = True
        for j, (a, b) in enumerate(zip(alone_p[0], parts[i])):
            assert torch.equal(a["tokens"], b["tokens"]), f"file {f}, chunk {j}"
            assert a["ylen"] == b["ylen"] and a["kept"] == b["kept"] and a["mel"].shape == b["mel"].shape
            e_mel = (a["mel"] - b["mel"]).abs().mean().item()
            eq = torch.equal(a["mel"], b["mel"])
            print(f"file {f}, chunk {j}: {a['tokens'].shape[1]} tokens, alone vs pool mel mean abs err {e_mel:.3e} (< 1e-3), identical {eq}")
            assert e_mel < 1e-3
            if eq:
                assert torch.equal(a["wave"], b["wave"]), f"file {f}, chunk {j}: same mel, another wave"
            same = same and eq
        assert alone_w[0].shape == waves[i].shape
        if same:
            assert torch.equal(alone_w[0], waves[i]), f"file {f}: same mels, another wave"
        assert torch.equal(waves[i][0].cpu(), _stream(parts[i], ov))


# --------------------------------------------------------------------------------------------------- 3. short chunks
def test_short_chunks_follow_the_seam_rule():
    f, ov = 4, 16
    assert f in L.qualified()
    waves, parts = _convert([f], ar_chunk_tokens=L.FILES[f][3], overlap_frame_len=ov, **_pinned([f]))
    cw = [p["wave"][0].cpu().numpy() for p in parts[0]]
    assert [len(w) for w in cw] == [c["ylen"] * L.HOP for c in L.file_case(f)["chunks"]]
    assert all(len(w) < 2 * ov * L.HOP for w in cw)
    want, plan = L.seam_model(cw, [0] * len(cw), [j == len(cw) - 1 for j in range(len(cw))], ov * L.HOP, 1)
    assert [p["kept"] for p in parts[0]] == plan["kept"] == [False] * (len(cw) - 1) + [True]
    assert np.array_equal(waves[0][0].cpu().numpy(), want[0])
    assert np.array_equal(want[0], cw[-1])


# --------------------------------------------------------------------------------------------------- 4. timbre branch
def test_timbre_branch_equals_the_v1_pool():
    from seedvc_amd.pipeline import HotPath, long_batch_plan
    hp = _hotpath()
    fa, fb = L.qualified()[:2]
    ov = 2
    recs = [dict(_record(fa), source_frames=30), dict(_record(fb), source_frames=9)]
    P = [r["target"]["P"] for r in recs]
    window = P[0] + 12
    plan = long_batch_plan([30, 9], P, window, ov, L.HOP)
    assert [c[0] for c in plan["chunks"]] == [0, 0, 0, 1]                       # three windows and one
    seeds = [21, 22]
    got = hp.convert_long_batch(recs, L.N_STEPS, L.CFG_RATES, convert_style=False, max_context_window=window, hop=L.HOP,
                                overlap_frame_len=ov, seeds=seeds)
    nw = [r["src_tokens"].size(1) for r in recs]
    tok = torch.zeros(2, max(nw), dtype=torch.int64, device=DEV)
    for i, r in enumerate(recs):
        tok[i, :nw[i]] = r["src_tokens"][0]
    cond = hp.cfm_lr(tok, ylens=torch.LongTensor([30, 9]), in_lens=nw)[0]
    utts = [(cond[i:i + 1, :n], r["target"]["prompt_condition"], r["target"]["mel"], r["target"]["style"])
            for i, (r, n) in enumerate(zip(recs, [30, 9]))]
    want = HotPath(hp.cfm, hp.vocoder).convert_long_batch(utts, L.N_STEPS, list(L.CFG_RATES), L.HOP, window, overlap_frame_len=ov,
                                                          seeds=seeds, ragged_vocoder=True)
    for g, w, n in zip(got, want, plan["out_lens"]):
        assert g.shape == w.shape == (1, n) and torch.isfinite(g).all()
        assert torch.equal(g, w)
    # pinned noise reaches the pool's chunks by (file, chunk)
    asked = []

    def noise(u, k, T):
        asked.append((u, k, T))
        return torch.zeros(1, 80, T, device=DEV)
    hp.convert_long_batch(recs, L.N_STEPS, L.CFG_RATES, convert_style=False, max_context_window=window, hop=L.HOP,
                          overlap_frame_len=ov, noise_fn=noise)
    assert asked == [(0, 0, P[0] + 12), (0, 1, P[0] + 12), (0, 2, P[0] + 10), (1, 0, P[1] + 9)]


# --------------------------------------------------------------------------------------------------- 5. anonymization
def test_anonymization_prompts_have_no_target_tokens():
    """`A.oracle_tokens` takes a prompt without target tokens (ar_batch_cases has one), so the chunk tokens are compared with
    the oracle's: condition = the range alone, empty prompt target.  The CFM still uses the target record."""
    u, chunks = L.anonymized_case()
    f, ov = u["f"], 2
    waves, parts = _convert([f], ar_chunk_tokens=u["chunk_tokens"], overlap_frame_len=ov, anonymization_only=True,
                            **_pinned([f], lambda _: chunks))
    assert len(parts[0]) == len(chunks)
    for j, (part, c) in enumerate(zip(parts[0], chunks)):
        assert torch.equal(part["tokens"].cpu(), c["ref_tokens"]), f"chunk {j}: {part['tokens'].tolist()} vs {c['ref_tokens'].tolist()}"
        assert part["ylen"] == c["ylen"] and part["mel"].shape == (1, 80, c["ylen"]) and part["wave"].shape == (1, c["ylen"] * L.HOP)
        assert torch.isfinite(part["mel"]).all() and torch.isfinite(part["wave"]).all()
        _check_chunk(part, L.oracle_chunk(f, j, True), f"anonymized file {f}, chunk {j}")
    with_target = [c["ref_tokens"] for c in L.file_case(f)["chunks"]]
    assert any(not torch.equal(a, c["ref_tokens"]) for a, c in zip(with_target, chunks))          # the target tokens do matter
    assert torch.isfinite(waves[0]).all() and torch.equal(waves[0][0].cpu(), _stream(parts[0], ov))


# ------------------------------------------------------------------------------------------------------------ 6. edges
def test_edges_and_errors():
    hp = _hotpath()
    f, g = L.qualified()[1], L.qualified()[2]
    ov = 2
    kw = dict(ar_chunk_tokens=L.FILES[f][3], overlap_frame_len=ov)
    base_w, base_p = _convert([f], **kw, **_pinned([f]))
    # a file without source tokens beside a normal neighbour
    empty = dict(_record(g), src_narrow=torch.zeros(1, 0, dtype=torch.int64, device=DEV))
    pins = _pinned([g, f])
    waves, parts = hp.convert_long_batch([empty, _record(f)], L.N_STEPS, L.CFG_RATES, max_context_window=WINDOW, hop=L.HOP,
                                         max_new=A.MAX_NEW, return_parts=True, **kw, **pins)
    assert waves[0].shape == (1, 0) and parts[0] == []
    assert torch.equal(waves[1], base_w[0]) and all(torch.equal(a["mel"], b["mel"]) for a, b in zip(parts[1], base_p[0]))
    # frames_per_token so small that every ylen is 0
    tiny = dict(_record(f), frames_per_token=0.01)
    waves, parts = hp.convert_long_batch([tiny], L.N_STEPS, L.CFG_RATES, max_context_window=WINDOW, hop=L.HOP, max_new=A.MAX_NEW,
                                         return_parts=True, **kw, **_pinned([f]))
    assert waves[0].shape == (1, 0)
    for p, b in zip(parts[0], base_p[0]):
        assert p["ylen"] == 0 and not p["kept"] and p["mel"].shape == (1, 80, 0) and p["wave"].shape == (1, 0)
        assert torch.equal(p["tokens"], b["tokens"])
    # a chunk prompt too long for the 160-position cache: refused before anything runs
    long_src = dict(_record(f), src_narrow=torch.zeros(1, 300, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="file 1, chunk 0"):
        hp.convert_long_batch([_record(g), long_src], L.N_STEPS, L.CFG_RATES, max_context_window=WINDOW, hop=L.HOP, ar_chunk_tokens=200,
                              seeds=[1, 2])
    # draws that do not cover max_new: refused at submit, nothing stays admitted
    with pytest.raises(ValueError, match="exp_noise"):
        hp.convert_long_batch([_record(f)], L.N_STEPS, L.CFG_RATES, max_context_window=WINDOW, hop=L.HOP, max_new=A.MAX_NEW,
                              exp_noise_fn=lambda u, k: torch.ones(3, 33, device=DEV), **kw)
    # the object still converts: pinned as before, and seeded (twice the same)
    again_w, again_p = _convert([f], **kw, **_pinned([f]))
    assert torch.equal(again_w[0], base_w[0]) and all(torch.equal(a["tokens"], b["tokens"]) for a, b in zip(again_p[0], base_p[0]))
    a = _convert([f, g], seeds=[5, 6], ar_chunk_tokens=9, overlap_frame_len=ov, return_parts=False)
    b = _convert([f, g], seeds=[5, 6], ar_chunk_tokens=9, overlap_frame_len=ov, return_parts=False)
    assert all(x.shape[1] > 0 and torch.isfinite(x).all() and torch.equal(x, y) for x, y in zip(a, b))
    torch.manual_seed(3)
    c = _convert([f], ar_chunk_tokens=9, overlap_frame_len=ov, return_parts=False)          # neither seeds nor pinned draws
    assert c[0].shape[1] > 0 and torch.isfinite(c[0]).all()


# ------------------------------------------------------------------------------------------------ 7. padding never leaks
def test_padding_never_leaks():
    fs = [1, 2]
    kw = dict(ar_chunk_tokens=9, overlap_frame_len=2, max_chunks=3, **_pinned_by_call(fs, 9))
    first_w, first_p = _convert(fs, **kw)
    first_w = [w.cpu() for w in first_w]
    first_p = [[{n: (t.cpu() if torch.is_tensor(t) else t) for n, t in p.items()} for p in ps] for ps in first_p]
    junk = torch.full((64 << 20,), float("nan"), device="cuda")     # 256 MB of NaN handed back to the caching allocator
    torch.cuda.synchronize()
    del junk
    second_w, second_p = _convert(fs, **kw)
    for a, b in zip(first_w, second_w):
        assert torch.isfinite(b).all() and torch.equal(a, b.cpu())
    for pa, pb in zip(first_p, second_p):
        for a, b in zip(pa, pb):
            for n in ("tokens", "mel", "wave"):
                assert torch.isfinite(b[n].float()).all() and torch.equal(a[n], b[n].cpu()), n


def _pinned_by_call(fs, chunk_tokens):
    """Pinned draws for a chunking other than the case table's: any fixed draws do (nothing is compared with the oracle)."""
    import cases
    vocab = L.models()["ar"][0]["vocab_size"]

    @functools.lru_cache(maxsize=None)
    def exp(u, k):
        return (-torch.log(cases.rand(f"v2l.pad.{fs[u]}.{k}.expn", 900, A.MAX_NEW + 1, vocab).clamp_min(1e-9))).to(DEV)

    @functools.lru_cache(maxsize=None)
    def z(u, k):
        return cases.randn(f"v2l.pad.{fs[u]}.{k}.z", 900, 1, 80, 100).to(DEV)
    return dict(exp_noise_fn=exp, noise_fn=lambda u, k, T: z(u, k)[:, :, :T])
