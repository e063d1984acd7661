"""The attention kernels (csrc/attention.hip) at op level, through the raw svc_op_attention_ex seam: ONE attention_launch on
buffers the test lays out itself, so every byte the kernels read is the test's.  All twelve launched instantiations (both
families, both query-tile forms, fp16 and fp32 output), the production V^T order included.

What is held (attention_cases.py states the reference, derives the bound and builds the exact cases):
  parity        numeric cases meet the derived per-element bound against the float64 reference; routing, uniform and unit cases
                match their exact values bit for bit (fp32 output: to the stated last-bit tolerance)
  canaries      no element outside rows [q_start, Tq) of each sequence and columns [0, 64 H) is written
  relations     launches that must agree bit for bit do: V^T orders 0 and 1, the two query-tile forms in both families (and the
                launcher's own choice is one of them), fp16 of the fp32 output, a q_start launch against the full one, a constant
                length against an array, a sequence alone against any place in a batch, ld_qk = 2 D against 3 D, larger vt_ld
                and seq_rows
  poison        NaN where the kernels may load but must not use (K rows past kv_len, Q rows outside [q_start, Tq), V^T columns
                past the last tile, the third block of a 3 D row) and 65504 where they multiply by P = 0 (V^T columns of the last
                tile past kv_len) move no bit
  producer      the row-panel kernel's QKV epilogue writes what these kernels read, in every V^T order
"""
import time

import pytest
import torch

import attention_cases as A
import panel_cases as P

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

CASES = A.parity_cases()
IDS = [A.case_id(c) for c in CASES]
WORST = {}               # kernel family -> worst |out - ref| / bound seen by test_parity_and_canaries
T0 = [None]


def run(a, **over):
    """the whole output buffer of one launch, on the CPU"""
    from seedvc_amd import ops
    if T0[0] is None:
        T0[0] = time.time()
    return ops.attention_ex(dict(a, **over), fill16=A.CANARY16, fill32=A.CANARY32).cpu()


def family(vt_perm):
    return "32x32x16" if vt_perm == 2 else "16x16x32"


def same_bits(y0, y1, what=""):
    n = int((A.bits(y0) != A.bits(y1)).sum())
    assert n == 0, f"{what}: {n} of {y0.numel()} words differ"


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_parity_and_canaries(c):
    a = A.build(c)
    out = run(a)
    assert A.canaries_intact(a, out), "written outside rows [q_start, Tq) x columns [0, 64 H)"
    ok, ratio, text = A.check(a, out)
    print("attention parity", A.case_id(c), text)
    if c["kind"] == "numeric":
        WORST[family(c["vt_perm"])] = max(WORST.get(family(c["vt_perm"]), 0.0), ratio)
    assert ok, text


def test_worst_ratios():
    """the figures DESIGN.md quotes (printed; the assertion is test_parity_and_canaries's, once more over all numeric cases)"""
    print("attention parity worst |out - ref| / bound per family:", ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    if T0[0] is not None:
        print(f"attention parity: {time.time() - T0[0]:.1f} s since the first launch of this module")
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------ bit-identity relations
def base(vt_perm, qt_form, out32=0, kind="numeric", lens=(193, 70, 257, 129), nq=200, q_start=0, seed=4000, **kw):
    """a launch with dominant keys in several tiles, so that baselines move for some queries of a 16-query tile and not for others"""
    kw = dict(dict(seq_extra=16, ld3=0, vt_extra=0), **kw)
    return A.build(A.case(kind, 2, list(lens), nq, q_start, kw["seq_extra"], kw["ld3"], kw["vt_extra"], vt_perm, qt_form, out32,
                          seed=seed, const=kw.get("const", False)))


def with_vt_mode(a, mode):
    """the same launch with V^T re-stored in column order `mode`"""
    ld = a["vt"].shape[2]
    nat = a["vt"][:, :, A.vt_cols(range(ld), a["vt_perm"])]
    vt = torch.empty_like(a["vt"])
    vt[:, :, A.vt_cols(range(ld), mode)] = nat
    return dict(a, vt=vt, vt_perm=mode)


FORMS = [(vp, qf, o32) for vp in (1, 2) for qf in (1, 2) for o32 in (0, 1)]


@pytest.mark.parametrize("qt_form,out32", [(1, 0), (2, 0), (1, 1), (2, 1)])
@pytest.mark.parametrize("kind", ["numeric", "routing"])
def test_vt_orders_0_and_1_agree(kind, qt_form, out32):
    """attn_kernel<*, false> and <*, true> feed the same MFMAs the same operands"""
    a = base(0, qt_form, out32, kind=kind)
    same_bits(run(a), run(with_vt_mode(a, 1)), "vt_perm 0 vs 1")


@pytest.mark.parametrize("vt_perm,out32", [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)])
def test_query_tile_forms_agree(vt_perm, out32):
    """64- and 128-query workgroups give a wave the same arithmetic, in both families; the launcher's own choice is one of them"""
    a = base(vt_perm, 1, out32, seed=4001)
    y1, y2, y0 = run(a), run(a, qt_form=2), run(a, qt_form=0)
    same_bits(y1, y2, "qt_form 1 vs 2")
    same_bits(y0, y1, "qt_form 0 vs 1 (a small grid)")


@pytest.mark.parametrize("vt_perm,qt_form", [(0, 1), (1, 1), (1, 2), (2, 1), (2, 2)])
def test_fp32_output_rounds_to_the_fp16_output(vt_perm, qt_form):
    a = base(vt_perm, qt_form, 0, seed=4002)
    y16, y32 = run(a), run(a, out32=1)
    rows = A.window(a)
    same_bits(y16[rows], y32[rows].half(), "fp16(out32) vs out")


@pytest.mark.parametrize("vt_perm,qt_form,out32", FORMS)
@pytest.mark.parametrize("q_start", [8, 64, 72, 136])
def test_q_start_rows_equal_the_full_launch(q_start, vt_perm, qt_form, out32):
    """the DiT's last-layer window: a query's result does not depend on which queries share its tile or its workgroup"""
    a = base(vt_perm, qt_form, out32, seed=4003)
    full, part = run(a), run(a, q_start=q_start)
    assert A.canaries_intact(dict(a, q_start=q_start), part)
    rows = A.window(dict(a, q_start=q_start))
    same_bits(full[rows], part[rows], f"q_start {q_start} vs 0")


@pytest.mark.parametrize("vt_perm,qt_form,out32", FORMS)
def test_constant_length_equals_an_array(vt_perm, qt_form, out32):
    a = base(vt_perm, qt_form, out32, lens=(131, 131, 131), seed=4004)
    same_bits(run(a), run(a, kv_len=None, kv_len_const=131), "kv_len array vs kv_len_const")


def sub_launch(a, order):
    """the sequences `order` of launch a, in that order"""
    R = a["seq_rows"]
    idx = torch.tensor(order)
    qk = a["qk"].reshape(a["n_seq"], R, -1)[idx].reshape(len(order) * R, -1)
    return dict(a, qk=qk, vt=a["vt"][idx], n_seq=len(order), kv_len=[a["kv_len"][s] for s in order], lens=[a["lens"][s] for s in order])


@pytest.mark.parametrize("vt_perm,qt_form,out32", FORMS)
def test_a_sequence_does_not_depend_on_its_batch(vt_perm, qt_form, out32):
    a = base(vt_perm, qt_form, out32, seed=4005)
    R = a["seq_rows"]
    full = run(a).reshape(a["n_seq"], R, -1)
    for order in ([2], [0], [3, 2, 1, 0], [1, 1, 3], [2, 0]):
        part = run(sub_launch(a, order)).reshape(len(order), R, -1)
        for i, s in enumerate(order):
            same_bits(full[s], part[i], f"sequence {s} at place {i} of {order}")


@pytest.mark.parametrize("vt_perm,qt_form,out32", FORMS)
def test_strides_do_not_matter(vt_perm, qt_form, out32):
    """ld_qk = 3 D (the content encoders' rows), a V^T row one tile longer, and more rows per sequence"""
    a = base(vt_perm, qt_form, out32, seed=4006)
    g = torch.Generator().manual_seed(9)
    y = run(a)
    n_seq, R, D = a["n_seq"], a["seq_rows"], 64 * a["H"]
    qk3 = torch.cat([a["qk"], torch.randn(n_seq * R, D, generator=g).half()], dim=1)
    same_bits(y, run(a, qk=qk3), "ld_qk 3 D vs 2 D")
    vt2 = torch.cat([a["vt"], torch.randn(n_seq, D, 64, generator=g).half()], dim=2)
    same_bits(y, run(a, vt=vt2), "vt_ld + 64")
    R2 = R + 24
    qk2 = torch.cat([a["qk"].reshape(n_seq, R, -1), torch.randn(n_seq, 24, 2 * D, generator=g).half()], dim=1).reshape(n_seq * R2, -1)
    y2 = run(a, qk=qk2, seq_rows=R2).reshape(n_seq, R2, -1)
    same_bits(y.reshape(n_seq, R, -1)[:, :a["Tq"]], y2[:, :a["Tq"]], "seq_rows + 24")
    assert A.canaries_intact(dict(a, seq_rows=R2), y2.reshape(n_seq * R2, -1))


# ------------------------------------------------------------------------------------------------ poison
@pytest.mark.parametrize("vt_perm,qt_form,out32", FORMS + [(0, 1, 0), (0, 2, 1)])
@pytest.mark.parametrize("kind", ["numeric", "routing"])
def test_poison_where_the_kernels_must_not_look(kind, vt_perm, qt_form, out32):
    """The contract of AttnParams (common.h).  K rows at and past kv_len are loaded and masked by a select: NaN there.  Q rows
    outside [q_start, Tq) are loaded at most into lanes whose results are dropped: NaN.  V^T columns of the last tile past kv_len
    meet P = 0 in the MFMA and must be finite: the largest fp16, 65504.  V^T columns past the last tile and the third block of a
    3 D row are never read: NaN.  Lengths: 0 (no tile at all), 1, one short of a tile, a full tile (no masked tile), and ragged."""
    a = base(vt_perm, qt_form, out32, kind=kind, lens=(0, 1, 63, 64, 193), nq=120, q_start=8, seed=4007, ld3=1, vt_extra=64)
    y = run(a)
    n_seq, R, D, nan = a["n_seq"], a["seq_rows"], 64 * a["H"], float("nan")
    qk = a["qk"].clone().reshape(n_seq, R, -1)
    vt = a["vt"].clone()
    qk[:, a["Tq"]:, :D] = nan
    qk[:, :a["q_start"], :D] = nan
    qk[:, :, 2 * D:] = nan
    for s, L in enumerate(a["lens"]):
        qk[s, L:, D:2 * D] = nan
        Lt = A.round_up(L, A.KT)
        vt[s, :, A.vt_cols(range(L, Lt), vt_perm)] = 65504.0
        vt[s, :, Lt:] = nan
    assert ok_finite(y, a)
    same_bits(y, run(a, qk=qk.reshape(n_seq * R, -1), vt=vt), "poisoned vs clean")


def ok_finite(y, a):
    return torch.isfinite(y[A.window(a), :64 * a["H"]].float()).all()


# ------------------------------------------------------------------------------------------------ producer and consumer
def test_panel_qkv_feeds_attention():
    """One launch of the row-panel kernel's QKV phase (D = 384, 3 sequences of 44 rows) per V^T order, its qk and vt buffers handed
    to the attention launch unchanged: the producer's layout is the consumer's.  Each result meets the bound against the reference
    on the panel's own q, k, v read back in natural order; orders 0 and 1 give the same bits."""
    from seedvc_amd import ops
    # the smallest D = 384 launch of panel_cases with a QKV phase alone whose sequences cross a 32-key group
    c = min((c for c in P.parity_cases() if c["D"] == 384 and c["mix"] == "qkv" and c["Lout"] > 32 and c["row_off"] == 0),
            key=lambda c: c["n_seq"] * c["Lout"])
    outs = {}
    for mode in (0, 1, 2):
        pa = P.make_args(dict(c, vt_mode=mode, vt_extra=0))
        pa["vt_ld"] = A.round_up(pa["seq_rows"], A.KT)       # the attention kernels read whole 64-key tiles
        got = ops.dit_panel(pa, fill16=P.CANARY16, fill32=P.CANARY32)
        n_seq, R, H = pa["n_seq"], pa["seq_rows"], 6
        lens = ([R, R - 3, 17] + [R] * n_seq)[:n_seq]
        for qt_form, out32 in ((1, 0), (2, 1)):
            a = dict(kind="numeric", qk=got["qk"].cpu(), q_col=0, k_col=384, vt=got["vt"].cpu(), n_seq=n_seq, H=H, seq_rows=R, Tq=R,
                     q_start=0, kv_len=lens, lens=lens, kv_len_const=0, vt_perm=mode, qt_form=qt_form, out32=out32, ld_out=384)
            assert torch.isfinite(a["vt"].float()).all()
            y = run(a)
            assert A.canaries_intact(a, y)
            ok, ratio, text = A.check(a, y)
            print(f"panel -> attention, vt order {mode}, qt_form {qt_form}, out32 {out32}:", text)
            assert ok, text
            outs[mode, qt_form] = y
    for qt_form in (1, 2):
        same_bits(outs[0, qt_form], outs[1, qt_form], "panel vt order 0 vs 1")
