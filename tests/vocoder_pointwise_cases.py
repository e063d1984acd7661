"""Cases, float64 references, fp32 emulations and checks of the vocoders' pointwise kernels at op level, shared by
test_host_vocoder_pointwise.py (which checks that the checks can tell a right kernel from a subtly wrong one) and
test_gpu_vocoder_pointwise.py (which holds the kernels to them through ops.act_cl and ops.hift_signal).  CPU only, plain torch
ops; nothing here calls the library.

Kernels: act_cl_kernel / act_cl2_kernel (csrc/aa_act.hip) and hift_phase_prefix / hift_source / hift_stft / hift_frames /
hift_ola / mel_to_cl / ew_cl (csrc/vocoder.hip).

LAYOUTS
  act_cl      x fp32 [B][L][ld], planes [B][L][ld]; channels c >= C are pad.  A launch is a case (`act_case`) in a FORM:
              "f32" (fp32 plane, ld = the case's ld32), "f16" (hi only), "f16+lo" (hi + fp16 residual), "f16+p8" (hi + fp8 byte
              pair: byte 0 = fp8(hi), byte 1 = fp8(2^11 (v - hi)), OCP e4m3); the three fp16 forms use ld = ld16.  x holds NaN in
              its pad channels and in rows at and above lens[b].  `emu_act` and the GPU run both return what ops.act_cl
              returns: whole plane buffers (guard + B L + guard rows), canaries (0x6A5A / -777.25) wherever nothing was written.
  source      f0 [B][S] (micro-batch rows), phase0 [n_utt][NH], noise [n_utt][NH][S_in up], lin_w [NH], lin_b [1] -> [B][S up];
              row j is utterance src[j] and ends after len[j] frames.  f0 and noise hold NaN past the row's end.
  STFT        s [B][Lw] -> [B][F][ld]: columns 0..8 real, 9..17 imaginary, 18..ld-1 zero; utterance b has lw[b] samples (NaN
              above) and nf[b] frames, reflected at ITS last sample; frame rows at and above nf[b] are zero.
  frames      [B F][ld] (9 log-magnitudes | 9 phase pre-activations) -> [B F][16] windowed time frames.
  overlap-add frames [B][F][16] -> out [n_utt][Lw] row src[j]; samples at and above lw[j] zero; frame rows at and above nf[j]
              hold NaN.
  mel_to_cl   mel [n_utt][C][S_in] -> [B][S][ld];  ew_cl  [rows][ld] -> [rows][ld]; both in fp32, fp16, or fp16 hi + lo.

REFERENCES, all float64
  ref_act      seedvc_oracle.anti_alias_act restated op by op on float64 tensors (the oracle casts its filter to fp32), taps from
               weights.make_tensor("x.filter", (1, 1, 12)); ragged: one call per utterance on its own rows, as
               vocoder_ragged_cases.act_ragged does (test_host_vocoder_pointwise.py holds both restatements to the originals).
  mode 1       x + inv_b sin^2(a x);  mode 2 (leaky ReLU) is one fp32 product: predicted bit for bit, no reference needed.
  ref_source   seedvc_oracle.hift_source restated in float64, keeping its documented fp32 cast of the double phase sum.
  ref_stft, ref_frames, ref_ola   seedvc_oracle.stft16 / istft16 restated in float64 (istft16 in its two halves).
  fp8          kconv_cases.q8 / act_planes_p8.

BOUNDS.  Every bound comes from the kernels' documented arithmetic, never from their results, with ONE measured constant:
  TAU32  the anti-aliased Snake's fp32 error, normalised |y - ref| / (|ref| + 1).  The kernel evaluates sin on the
         transcendental unit (v_sin_f32 behind a fract), whose error is not documented; TAU32 = 4 x the largest normalised error
         measured on an MI355X over all numeric mode-0 cases (the factor covers other seeds and inputs): 4 x 1.09e-6.  For
         scale: a plain fp32 restatement differs from float64 by 1.2e-7 .. 2.9e-7 at these shapes; the kernel's argument in
         revolutions, a u / 2 pi rounded to fp32 before the fract, costs 2^-24 |a u| inv_b more, which is what was measured
         (the emulation below, with an exact sine, reaches 1.06e-6).  Every act_cl sabotage exceeds TAU32 at least tenfold in
         the case that targets it (test_host_vocoder_pointwise.py asserts it; the smallest, a lo plane cut from the unrounded
         hi, is 83 x).
  act fp32     |y - ref| <= TAU32 (|ref| + 1) [+ 2^-23 max|a u| inv_b in the large-argument case: a' = a / 2 pi and a' u each
               round once, 2^-24 relative each, on an angle of up to max|a u|, and d/dz sin^2 z <= 1].
  act planes   |hi + lo - ref| <= fp32 bound + 2^-22 |ref| + 2^-25: v - hi is exact in fp32; its fp16 rounding is 2^-11
               relative on a term <= 2^-11 |hi| (2^-22 |ref|), or half an fp16 subnormal step (2^-25) absolute.
  act fp8 lo   |hi + byte1 / 2^11 - ref| <= the same + 2^-15 p2(hi), p2(hi) = 2^floor(log2 |hi|): e4m3 rounds to 2^-4 relative, on
               a term <= 2^-11 p2(hi).
  act hi only  at most one fp16 step from half(ref) wherever the fp32 bound is below half an fp16 step; near zero, where fp16
               steps are finer than the fp32 error, |hi - ref| <= fp32 bound + half a step.
  mode 1       2^-22 (|x| + inv_b) + 2^-23 |a x| inv_b: the product a x rounds once and the Cody-Waite reduction of sin_sq is
               exact to 2^-24 of its argument; polynomial, square, product and sum are a few 2^-24 of inv_b and of |x|.  Its fp8
               lo plane adds 2^-21: below 2^-6 the scaled residual meets e4m3's subnormal step 2^-9 (half of it, over 2^11);
               and from |hi| = 512 on, what the clamp of the scaled residual at 448 cuts off (the sweep reaches |x| = 1e3).
  source       tanh is 1-Lipschitz, so the bound is that of the pre-activation: per voiced harmonic sine_amp |w_h| (2 pi
               ulp32(cum_h) + 2^-22 (2 pi + |phase0_h|) + 2^-23): the kernel's double phase sum is a product where the
               reference's is a running sum, so the two fp32 casts may fall on different sides of a rounding (one ulp32 of cum,
               times 2 pi); theta = 2 pi frac and theta + phase0 round once each, sinf is good to 2^-23.  Plus 2^-22 per term for
               its products, (NH + 2) 2^-24 of sum |terms| for the accumulation, and 2^-22 for tanhf.
               Unvoiced cases (f0 = 0): no phase enters; 2^-22 (1 + |pre-activation|) -- "a few 2^-24" -- while a wrong noise row,
               stride or harmonic moves the output by O(0.1).
  STFT         per bin 2^-19 sum_n |x_n| w_n + 2^-24 |ref|: 16 products x_n w_n t_n; the fp32 window is good to 2^-23 and the
               windowed sample rounds once (2^-24); the twiddle (angle in fp32, cosf / sinf) to 2^-23; the product rounds once;
               15 additions each round at most 2^-24 of sum |x_n| w_n: (2 + 1 + 2 + 1 + 15) 2^-24 = 21 x 2^-24 < 2^-19; the last
               term is the store-side slack of comparing with an fp32-representable reference.
  frames       per sample 2^-19 (w_n / 16) A + 2^-24 |ref|, A = sum_k c_k (|re_k| + |im_k|), c = (1, 2, .., 2, 1): expf, sinf and
               cosf / sinf of the phase leave re and im good to 2^-21 (8 x 2^-24), the twiddle 2^-23, the product 2^-24, 16
               additions 2^-24 each: 27 x 2^-24 < 2^-19.
  overlap-add  per sample (sum of its frames' bounds + 2^-20 sum |frame samples|) / env: at most 3 additions, the fp32 envelope
               (cosf, squares, 3 additions: 2^-21) and the division.  The clamp to +-limit is monotone and 1-Lipschitz: the bound
               passes through it, no sample is left out.
  casts        mel_to_cl and ew_cl are predicted bit for bit: hi = half(v), lo = half(v - hi), leaky = one fp32 product.
"""
import math

import torch
import torch.nn.functional as F

import kconv_cases as K

CANARY16 = 0x6A5A
CANARY32 = -777.25
GUARD = 8
NAN = float("nan")
# measured on an MI355X: the largest |y - ref| / (|ref| + 1) over all numeric mode-0 cases below (fp32 form) is 1.085e-6 (C = 1,
# L = 256; per channel set 1.09e-6, 5.3e-7, 4.8e-7, 6.7e-7).  The fp32 emulation below, which takes an exact sine of the same rounded
# revolutions, reaches 1.06e-6 on the same cases: the error is the fp32 rounding of a u / 2 pi (2^-24 of up to three revolutions,
# times 2 pi inv_b), not the sine unit's.
TAU32_MEASURED = 1.09e-6
TAU32 = 4.0 * TAU32_MEASURED

FORMS = ("f32", "f16", "f16+lo", "f16+p8")
ACT_LENGTHS = (1, 2, 5, 6, 7, 12, 13, 63, 64, 65, 79, 80, 143, 144, 145, 255, 256, 257, 321)
ACT_CHANNELS = ((1, 32, 64), (24, 32, 64), (33, 64, 64), (70, 96, 128))        # (C, ld fp32, ld fp16)
RAGGED_LENS = {321: ([321, 0, 1], [144, 145, 143], [64, 65, 63], [257, 8, 320]), 65: ([65, 64, 1],)}
F8 = torch.float8_e4m3fn


def taps12():
    from seedvc_amd import weights
    return weights.make_tensor("x.filter", (1, 1, 12)).reshape(12).float()


def f32(v):
    return torch.tensor(v, dtype=torch.float32)


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.float16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def ulp16(h):
    """the fp16 step at fp16-representable values h (float64): 2^(floor(log2 |h|) - 10), 2^-24 at and below the subnormals"""
    return torch.clamp(p2(h), min=2.0 ** -14) * 2.0 ** -10


def p2(h):
    """2^floor(log2 |h|) (0 for 0)"""
    m, e = torch.frexp(h.abs().double())
    return torch.where(h == 0, torch.zeros_like(m), torch.ldexp(torch.ones_like(m), e - 1))


def ulp32(v):
    m, e = torch.frexp(v.abs().double())
    return torch.ldexp(torch.ones_like(m), e - 24)


def f8_decode(byte):
    return byte.to(torch.uint8).view(F8).double()


def f8_bytes(v):
    """the kernels' fp8 conversion (lo_pair_p8): clamp to +-448, round to e4m3; the byte as int32"""
    return v.to(torch.float32).clamp(-448.0, 448.0).to(F8).view(torch.uint8).to(torch.int32)


# ================================================================================================== act_cl
def act_case(L, ch, mode=0, lens=None, big=False, sweep=False, seed=0, B=3, poison=True):
    """One launch's operands.  data (B, L, C) = 2 randn; a = exp(0.3 randn), inv_b = 1 / (exp(0.3 randn) + 1e-9).
    big: a scaled per channel so that max |a u| = 1e3 over the up-sampled signal u (the fract in front of the hardware sine).
    sweep (mode 1): |a x| swept to 1e3.  poison False: rows past lens[b] hold other finite data instead of NaN."""
    C, ld32, ld16 = ACT_CHANNELS[ch]
    g = torch.Generator().manual_seed(7000 + 131 * L + 17 * ch + seed)
    data = 2.0 * torch.randn(B, L, C, generator=g)
    a = torch.exp(0.3 * torch.randn(C, generator=g))
    ib = 1.0 / (torch.exp(0.3 * torch.randn(C, generator=g)) + 1e-9)
    c = dict(L=L, ch=ch, C=C, ld32=ld32, ld16=ld16, mode=mode, lens=lens, big=big, B=B, slope=0.1, taps=taps12(), poison=poison)
    if sweep:
        data = (torch.linspace(-1.0, 1.0, B * L * C).reshape(B, L, C) * 1e3 / a).float()
    if big:
        u = ref_act(dict(c, data=data, a=a, ib=ib, big=False))[1]
        a = (1e3 / u.abs().amax(dim=(0, 1))).float()
    c.update(data=data, a=a, ib=ib)
    return c


def act_id(c):
    s = f"L{c['L']}-C{c['C']}-m{c['mode']}"
    if c["lens"] is not None:
        s += "-r" + "_".join(str(v) for v in c["lens"])
    return s + ("-big" if c["big"] else "")


def act_ld(c, form):
    return c["ld32"] if form == "f32" else c["ld16"]


def act_x(c, form, seqs=None):
    """x (B, L, ld) as the launch reads it: NaN pad channels, NaN rows at and above lens[b]; seqs: a subset of the sequences"""
    ld = act_ld(c, form)
    x = torch.full((c["B"], c["L"], ld), NAN)
    x[:, :, :c["C"]] = c["data"]
    if c["lens"] is not None and c["poison"]:
        for b, n in enumerate(c["lens"]):
            x[b, n:] = NAN
    return x if seqs is None else x[seqs].contiguous()


def act_lens(c):
    return c["lens"] if c["lens"] is not None else [c["L"]] * c["B"]


def _aa64(x, filt, a, ib):
    """seedvc_oracle.anti_alias_act on float64 tensors; x (B, C, L).  Returns (y, up-sampled signal u)"""
    C = x.shape[1]
    f = filt.reshape(1, 1, 12).double()
    xp = F.pad(x, (5, 5), mode="replicate")
    up = 2.0 * F.conv_transpose1d(xp, f.expand(C, 1, 12), stride=2, groups=C)
    up = up[..., 15:-15]
    s = up + ib[None, :, None] * torch.sin(up * a[None, :, None]) ** 2
    sp = F.pad(s, (5, 6), mode="replicate")
    return F.conv1d(sp, f.expand(C, 1, 12), stride=2, groups=C), up


def ref_act(c):
    """(ref (B, L, C) float64 with zero rows at and above lens[b], u (B, 2 L, C) the up-sampled signal of mode 0 or None)"""
    x = c["data"].double()
    a, ib = c["a"].double(), c["ib"].double()
    if c["mode"] == 1:
        return x + ib * torch.sin(a * x) ** 2, None
    if c["mode"] == 2:
        return torch.where(x > 0, x, x * f32(c["slope"]).double()), None
    out = torch.zeros_like(x)
    u = torch.zeros(x.shape[0], 2 * x.shape[1], x.shape[2], dtype=torch.float64)
    for b, n in enumerate(act_lens(c)):          # per utterance on its own rows, as vocoder_ragged_cases.act_ragged
        if n > 0:
            y, up = _aa64(x[b:b + 1, :n].transpose(1, 2), c["taps"], a, ib)
            out[b, :n] = y[0].T
            u[b, :2 * n] = up[0].T
    return out, u


ACT_SABOTAGES = ("clamp_L-2", "clamp_batch_L", "swap_taps01", "odd_even", "no_x2_tail", "lo_unrounded", "p8_bytes_swapped")


def _emu_seq(x, n_out, n_clamp, ft, a, ib, sab):
    """mode 0 on one sequence in fp32, as act_cl_kernel orders it: x (rows, C) fp32; outputs [0, n_out), window clamped to
    [0, n_clamp)"""
    if sab == "swap_taps01":
        ft = ft.clone()
        ft[0], ft[1] = ft[1].clone(), ft[0].clone()
    f2 = 2.0 * ft
    hi_x = n_clamp - 1 - (1 if sab == "clamp_L-2" and n_clamp > 1 else 0)
    m = torch.arange(2 * n_clamp)
    jhi, t0 = (m + 15) >> 1, (m + 15) & 1
    if sab == "odd_even":
        t0 = t0 ^ 1
    u = torch.zeros(2 * n_clamp, x.shape[1], dtype=torch.float32)
    for e in range(6):
        u = u + x[(jhi - 5 - e).clamp(0, hi_x)] * f2[t0 + 2 * e][:, None]
    if sab == "no_x2_tail":
        tail = (m % 128) >= 126
        u = torch.where(tail[:, None], 0.5 * u, u)
    rev = (a * f32(0.15915494309189535)) * u
    sn = torch.sin(2.0 * math.pi * (rev - torch.floor(rev)).double()).float()
    s = u + ib * sn * sn
    i = torch.arange(n_out)
    y = torch.zeros(n_out, x.shape[1], dtype=torch.float32)
    for t in range(12):
        y = y + ft[t] * s[(2 * i - 5 + t).clamp(0, 2 * n_clamp - 1)]
    return y


def emu_values(c, sab=None):
    """(B, L, C) fp32 values v of the launch before the planes are cut; rows at and above lens[b] zero"""
    x = act_x(c, "f32")[:, :, :c["C"]]
    a, ib = c["a"], c["ib"]
    if c["mode"] == 1:
        z = a * x
        return x + ib * (torch.sin(z.double()).float()) ** 2
    if c["mode"] == 2:
        return torch.where(x > 0, x, x * f32(c["slope"]))
    v = torch.zeros_like(x)
    for b, n in enumerate(act_lens(c)):
        if n > 0:
            v[b, :n] = _emu_seq(x[b], n, c["L"] if sab == "clamp_batch_L" else n, c["taps"], a, ib, sab)
    return v


def planes_of(v, form, sab=None):
    """fp32 values -> (hi, lo) as the kernels cut them: fp32 | int16 words"""
    if form == "f32":
        return v.clone(), None
    hi = v.half()
    if form == "f16":
        return hi.view(torch.int16), None
    r = v - hi.float()
    if sab == "lo_unrounded":
        r = v - v
    if form == "f16+lo":
        return hi.view(torch.int16), r.half().view(torch.int16)
    b0, b1 = f8_bytes(hi.float()), f8_bytes(r * 2048.0)
    if sab == "p8_bytes_swapped":
        b0, b1 = b1, b0
    return hi.view(torch.int16), (b0 | (b1 << 8)).to(torch.int16)


def emu_act(c, form, sab=None):
    """what ops.act_cl returns, from the fp32 emulation"""
    ld, n = act_ld(c, form), c["B"] * c["L"]
    v = torch.zeros(c["B"], c["L"], ld)
    v[:, :, :c["C"]] = emu_values(c, sab)
    hi, lo = planes_of(v.reshape(n, ld), form, sab)

    def guarded(p):
        if p is None:
            return None
        fill = CANARY32 if p.dtype == torch.float32 else CANARY16
        out = torch.full((GUARD + n + GUARD, ld), fill, dtype=p.dtype)
        out[GUARD:GUARD + n] = p
        return out
    return guarded(hi), guarded(lo), GUARD


def act_bound32(c, ref, u):
    """the fp32 bound per element (B, L, C): TAU32 (|ref| + 1), the derived mode-1 bound, or 0 for mode 2 (exact)"""
    if c["mode"] == 1:
        x, a, ib = c["data"].double(), c["a"].double(), c["ib"].double()
        return 2.0 ** -22 * (x.abs() + ib) + 2.0 ** -23 * (a * x).abs() * ib
    if c["mode"] == 2:
        return torch.zeros_like(ref)
    bound = TAU32 * (ref.abs() + 1.0)
    if c["big"]:
        bound = bound + 2.0 ** -23 * (c["a"].double() * u).abs().amax(dim=(0, 1)) * c["ib"].double()
    return bound


def check_act(c, form, hi, lo, guard, ref, u):
    """The exact and the numeric checks of one launch's buffers.  Returns (failures, ratio, norm): the names of the failed
    checks, the largest |error| / bound of the numeric ones, and the largest |y - ref| / (|ref| + 1) (what TAU32 is measured as)."""
    fails = []
    B, L, C, ld = c["B"], c["L"], c["C"], act_ld(c, form)
    n = B * L
    f32_out = form == "f32"
    canary = CANARY32 if f32_out else CANARY16
    planes = [("hi", hi)] + ([("lo", lo)] if lo is not None else [])
    body = {}
    for name, p in planes:
        assert p.shape == (guard + n + guard, ld), (name, p.shape)
        if not (bool((p[:guard] == canary).all()) and bool((p[guard + n:] == canary).all())):
            fails.append(f"{name}: a guard row lost its canary")
        body[name] = p[guard:guard + n].reshape(B, L, ld)
        if bool((bits(body[name][:, :, C:]) != 0).any()):
            fails.append(f"{name}: pad channels are not all-zero words")
        for b, nb in enumerate(act_lens(c)):
            if bool((bits(body[name][b, nb:]) != 0).any()):
                fails.append(f"{name}: sequence {b} has non-zero words at or above row {nb}")
    h = body["hi"][:, :, :C]
    hv = h.double() if f32_out else h.view(torch.float16).double()
    if not bool(torch.isfinite(hv).all()):
        fails.append("hi: non-finite output")
        return fails, float("inf"), float("inf")
    bound = act_bound32(c, ref, u)
    err = (hv - ref).abs()
    norm = (err / (ref.abs() + 1.0)).max().item()
    if c["mode"] == 2:       # one fp32 product: bit for bit
        ld_want = torch.zeros(B, L, ld)
        ld_want[:, :, :C] = emu_values(c)
        want_hi, want_lo = planes_of(ld_want, form)
        if not torch.equal(bits(body["hi"]), bits(want_hi)):
            fails.append("hi: leaky ReLU differs from its one fp32 product")
        if lo is not None and not torch.equal(body["lo"], want_lo):
            fails.append("lo: leaky ReLU's lo plane differs from the prediction")
        return fails, 0.0, norm
    if f32_out:
        ratio = (err / bound).max().item()
        if ratio > 1.0:
            fails.append(f"fp32: |y - ref| is {ratio:.2f} x the bound")
        return fails, ratio, norm
    # hi alone: within one fp16 step of half(ref) wherever the fp32 bound is below half a step (a smaller error moves the rounding
    # by one step at most); near zero, where fp16 steps are finer than the fp32 error, |hi - ref| <= bound + half a step instead
    step = ulp16(K.half(ref))
    coarse = bound <= step / 2
    steps = K.f16_ulp_steps(h, ref.float().half().view(torch.int16))
    if bool((steps[coarse] > 1).any()):
        fails.append(f"hi: {steps[coarse].max().item()} fp16 steps from half(ref)")
    if bool((err[~coarse] > (bound + step / 2)[~coarse]).any()):
        fails.append("hi: further from ref than the fp32 bound plus half an fp16 step")
    ratio = 0.0
    if form == "f16+lo":
        lv = body["lo"][:, :, :C].view(torch.float16).double()
        if not bool(torch.isfinite(lv).all()):
            fails.append("lo: non-finite output")
        if not bool((lv.abs() <= ulp16(hv) / 2).all()):
            fails.append("lo: |lo| exceeds half an fp16 step of hi")
        pb = bound + 2.0 ** -22 * ref.abs() + 2.0 ** -25
        ratio = ((hv + lv - ref).abs() / pb).max().item()
    elif form == "f16+p8":
        w = body["lo"][:, :, :C].to(torch.int32) & 0xFFFF
        b0, b1 = f8_decode(w & 0xFF), f8_decode(w >> 8)
        if not torch.equal(b0, K.q8(hv)):
            fails.append("p8: byte 0 is not q8(hi)")
        pb = bound + 2.0 ** -22 * ref.abs() + 2.0 ** -25 + 2.0 ** -15 * p2(hv)
        if c["mode"] == 1:      # no TAU32 term here: e4m3's own subnormal step, 2^-9 of the scaled residual, counts (half of it, / 2^11)
            pb = pb + 2.0 ** -21 + torch.clamp(ulp16(hv) / 2 - 448.0 / 2048.0, min=0.0)     # and its clamp at 448 (|hi| >= 512)
        ratio = ((hv + b1 / 2048.0 - ref).abs() / pb).max().item()
    if ratio > 1.0:
        fails.append(f"planes: |hi + lo - ref| is {ratio:.2f} x the bound")
    return fails, ratio, norm


def act_cases():
    """every numeric mode-0 case: uniform at every length and channel count, the ragged sets, the large-argument case"""
    out = [act_case(L, ch) for ch in range(len(ACT_CHANNELS)) for L in ACT_LENGTHS]
    for L, sets in RAGGED_LENS.items():
        for k, lens in enumerate(sets):
            out.append(act_case(L, (k + 1) % len(ACT_CHANNELS), lens=list(lens)))
    out.append(act_case(145, 2, big=True))
    return out


def act_pointwise_cases():
    """modes 1 and 2 (fp32 out: act_cl_kernel; fp16 out: the pair kernel), and mode 1's sweep to |a x| = 1e3"""
    out = [act_case(L, ch, mode=mode) for mode in (1, 2) for L, ch in ((1, 0), (65, 1), (79, 2), (257, 3), (64, 3))]
    out.append(act_case(257, 2, mode=1, sweep=True))
    return out


# ================================================================================================== HiFT source
SRC = dict(sr=22050.0, sine_amp=0.1, noise_std=0.003, voiced_thr=10.0)
SRC_SABOTAGES = ("r_not_r+1", "noise_stride_S", "phase0_by_row")


def source_case(NH, up, ragged, kind="numeric", seed=0, S=5, S_in=7, B=3):
    """kind: numeric (voiced / unvoiced / voiced runs), onehot_w<h> (unvoiced, lin_w = e_h), onehot_noise (unvoiced, one draw
    per utterance non-zero)"""
    g = torch.Generator().manual_seed(9100 + 7 * NH + up + seed)
    n_utt = B
    lens = [5, 3, 0] if ragged else [S] * B
    src = [2, 0, 1] if ragged else list(range(B))
    f0u = 80.0 + 320.0 * torch.rand(n_utt, S_in, generator=g)          # the caller's utterances
    f0u[:, 2] = 0.0                                                    # voiced, unvoiced, voiced
    f0u[1, 0] = 0.0
    phase0 = (torch.rand(n_utt, NH, generator=g) * 2 - 1) * math.pi
    noise = torch.randn(n_utt, NH, S_in * up, generator=g)
    lin_w = torch.randn(NH, generator=g) / NH ** 0.5
    lin_b = 0.1 * torch.randn(1, generator=g)
    if kind != "numeric":
        f0u[:] = 0.0
        if kind == "onehot_noise":
            noise[:] = 0.0
            for u in range(n_utt):
                noise[u, (2 * u + 1) % NH, (u + 1) * up + u] = 3.0
        else:
            lin_w = torch.zeros(NH)
            lin_w[int(kind[len("onehot_w"):])] = 1.0
    f0 = torch.full((B, S), NAN)
    for j in range(B):
        f0[j, :lens[j]] = f0u[src[j], :lens[j]]
        noise[src[j], :, lens[j] * up:] = NAN
    return dict(NH=NH, up=up, S=S, S_in=S_in, B=B, n_utt=n_utt, ragged=ragged, kind=kind, lens=lens, src=src, f0=f0, phase0=phase0,
                noise=noise, lin_w=lin_w, lin_b=lin_b, **SRC)


def source_id(c):
    return f"NH{c['NH']}-up{c['up']}-{'ragged' if c['ragged'] else 'plain'}-{c['kind']}"


def source_args(c):
    """the fields of ops.hift_signal for this case"""
    a = dict(stage=1, B=c["B"], n_utt=c["n_utt"], NH=c["NH"], up=c["up"], S=c["S"], S_in=c["S_in"], phase0=c["phase0"], noise=c["noise"],
             lin_w=c["lin_w"], lin_b=c["lin_b"], **{k: c[k] for k in SRC})
    a["in"] = c["f0"]
    if c["ragged"]:
        a.update(src=c["src"], len=c["lens"])
    return a


def _source_row(c, j, dt, sab=None):
    """row j of the micro-batch, its first lens[j] frames: float64 restatement of seedvc_oracle.hift_source (dt float64), or the
    kernels' fp32 arithmetic (dt float32).  Returns (samples, bound): the bound's pieces come from the float64 pass"""
    n, up, NH = c["lens"][j], c["up"], c["NH"]
    u = c["src"][j]
    f0 = c["f0"][j, :n]
    f0u = f0[:, None].expand(-1, up).reshape(1, -1)                                  # nearest upsample (1, Lw)
    mult = torch.arange(1, NH + 1, dtype=torch.float32)[:, None]
    fmat = f0u * mult / f32(c["sr"])                                                 # (NH, Lw) fp32, as the oracle
    if dt == torch.float64:
        cum = torch.cumsum(fmat.double(), dim=-1).float()
    else:       # the kernels: exclusive prefix over frames of up * v, plus (r + 1) v, in double; one cast
        v = fmat[:, ::up].double()                                                   # (NH, n)
        prefix = torch.cumsum(up * v, dim=1) - up * v
        r = torch.arange(up, dtype=torch.float64)[None, None, :] + (0.0 if sab == "r_not_r+1" else 1.0)
        cum = (prefix[:, :, None] + r * v[:, :, None]).reshape(NH, -1).float()
    row_p = j if sab == "phase0_by_row" else u
    ph = c["phase0"][row_p].clone().to(dt)
    ph[0] = 0
    stride = (c["S"] if sab == "noise_stride_S" else c["S_in"]) * up
    flat = c["noise"].reshape(-1)
    base = u * NH * stride + torch.arange(NH)[:, None] * stride + torch.arange(n * up)[None, :]
    noise = flat[base].to(dt)
    two_pi = (f32(6.283185307179586) if dt == torch.float32 else torch.tensor(2 * math.pi, dtype=dt))
    frac = torch.fmod(cum, 1.0).to(dt)
    theta = two_pi * frac
    amp, std = f32(c["sine_amp"]), f32(c["noise_std"])           # the kernels' scalars are floats; the reference takes the same values
    if dt == torch.float64:
        amp, std = amp.double(), std.double()
    arg = theta + ph[:, None]
    sine = amp * (torch.sin(arg.double()).float() if dt == torch.float32 else torch.sin(arg))
    uv = (f0u > c["voiced_thr"]).to(dt)
    namp = uv * std + (1 - uv) * amp / 3
    val = sine * uv + namp * noise
    w = c["lin_w"].to(dt)[:, None]
    pre = c["lin_b"].to(dt)
    for h in range(NH):
        pre = pre + w[h] * val[h]
    out = torch.tanh(pre.double()).to(dt) if dt == torch.float32 else torch.tanh(pre)
    if dt != torch.float64:
        return out, None
    terms = (w * val).abs()
    if c["kind"] == "numeric":
        e_h = 2 * math.pi * ulp32(cum) + 2.0 ** -22 * (2 * math.pi + ph.abs()[:, None]) + 2.0 ** -23
        bound = (w.abs() * (c["sine_amp"] * uv * e_h) + 2.0 ** -22 * terms).sum(0) + \
            (NH + 2) * 2.0 ** -24 * (c["lin_b"].abs().double() + terms.sum(0)) + 2.0 ** -22
    else:
        bound = 2.0 ** -22 * (1.0 + pre.abs())
    return out, bound


def ref_source(c):
    """(ref, bound) float64 (B, S up): each row as its utterance run alone, zeros past its end"""
    ref = torch.zeros(c["B"], c["S"] * c["up"], dtype=torch.float64)
    bound = torch.zeros_like(ref)
    for j, n in enumerate(c["lens"]):
        if n:
            ref[j, :n * c["up"]], bound[j, :n * c["up"]] = _source_row(c, j, torch.float64)
    return ref, bound


def emu_source(c, sab=None):
    out = torch.zeros(c["B"], c["S"] * c["up"])
    for j, n in enumerate(c["lens"]):
        if n:
            out[j, :n * c["up"]] = _source_row(c, j, torch.float32, sab)[0]
    return out


def check_rows(out, ref, bound, what):
    """numeric check with exact zeros where the bound is zero: (failures, largest |out - ref| / bound over bound > 0)"""
    fails = []
    out = out.double()
    if not bool(torch.isfinite(out).all()):
        return [f"{what}: non-finite output"], float("inf")
    zero = bound == 0
    if bool((out[zero] != 0).any()) or bool((ref[zero] != 0).any()):
        fails.append(f"{what}: non-zero where exact zeros are due")
    ratio = ((out - ref).abs()[~zero] / bound[~zero]).max().item() if bool((~zero).any()) else 0.0
    if ratio > 1.0:
        fails.append(f"{what}: |out - ref| is {ratio:.2f} x the bound")
    return fails, ratio


def source_cases():
    out = []
    for NH in (9, 5):
        for up in (8, 256):
            for ragged in (False, True):
                out.append(source_case(NH, up, ragged))
                for kind in ("onehot_w0", f"onehot_w{NH // 2}", f"onehot_w{NH - 1}", "onehot_noise"):
                    out.append(source_case(NH, up, ragged, kind))
    return out


# ================================================================================================== STFT
STFT_SABOTAGES = ("reflect_at_Lw", "nf+1", "nf-1", "imag_sign")


def stft_case(Lw, ragged=False, kind="randn", ld=32, seed=0):
    """plain: B = 3 rows of Lw samples.  ragged: lw = [64, 32, 12, 0] in rows of 64 samples, NaN above lw[b].
    kind: randn | impulse<k> (k = 0, 1: positions 0 / 1; -1, -2: lw - 1 / lw - 2 of every row)"""
    g = torch.Generator().manual_seed(9300 + Lw + seed)
    lw = [64, 32, 12, 0] if ragged else [Lw] * 3
    B = len(lw)
    s = torch.full((B, Lw), NAN)
    for b, n in enumerate(lw):
        s[b, :n] = torch.randn(n, generator=g)
        if kind.startswith("impulse") and n:
            k = int(kind[len("impulse"):])
            s[b, :n] = 0.0
            s[b, k % n] = 1.0 + b
    nf = [n // 4 + 1 if n else 0 for n in lw]
    return dict(Lw=Lw, B=B, F=Lw // 4 + 1, ld=ld, ragged=ragged, kind=kind, lw=lw, nf=nf, s=s)


def stft_id(c):
    return f"Lw{c['Lw']}-{'ragged' if c['ragged'] else 'plain'}-{c['kind']}"


def stft_args(c):
    a = dict(stage=2, B=c["B"], n_utt=c["B"], Lw=c["Lw"], F=c["F"], ld=c["ld"])
    a["in"] = c["s"]
    if c["ragged"]:
        a.update(lw=c["lw"], nf=c["nf"])
    return a


def _hann(dt):
    n = torch.arange(16, dtype=dt)
    return 0.5 - 0.5 * torch.cos(torch.tensor(2 * math.pi, dtype=dt) * n / 16.0)


def _twiddles(dt, K=9):
    k = torch.arange(K)[:, None]
    n = torch.arange(16)[None, :]
    ang = torch.tensor(2 * math.pi, dtype=dt) * ((k * n) & 15).to(dt) / 16.0
    return torch.cos(ang), torch.sin(ang)


def ref_stft(c):
    """(ref, bound) float64 (B, F, ld): seedvc_oracle.stft16 per utterance on its own samples, zero rows at and above nf[b]"""
    ref = torch.zeros(c["B"], c["F"], c["ld"], dtype=torch.float64)
    bound = torch.zeros_like(ref)
    w = _hann(torch.float64)
    cs, sn = _twiddles(torch.float64)
    for b, n in enumerate(c["lw"]):
        if n == 0:
            continue
        xp = F.pad(c["s"][b:b + 1, None, :n].double(), (8, 8), mode="reflect")[0, 0]
        fr = xp.unfold(-1, 16, 4)
        assert fr.shape[0] == c["nf"][b]
        ref[b, :fr.shape[0], 0:9] = (fr * w) @ cs.T
        ref[b, :fr.shape[0], 9:18] = -((fr * w) @ sn.T)
        bound[b, :fr.shape[0], :18] = 2.0 ** -19 * (fr.abs() * w).sum(1, keepdim=True)
    return ref, bound + 2.0 ** -24 * ref.abs()


def emu_stft(c, sab=None):
    out = torch.zeros(c["B"], c["F"], c["ld"])
    w = _hann(torch.float32)
    cs, sn = _twiddles(torch.float32)
    n16 = torch.arange(16)
    for b in range(c["B"]):
        lw = c["Lw"] if sab == "reflect_at_Lw" else c["lw"][b]
        nf = min(c["F"], max(0, c["nf"][b] + {"nf+1": 1, "nf-1": -1}.get(sab, 0)))
        for fr in range(nf):
            q = (4 * fr - 8 + n16).abs()
            q = torch.where(q >= lw, 2 * (lw - 1) - q, q).clamp(0, c["Lw"] - 1)
            x = c["s"][b, q] * w
            re, im = torch.zeros(9), torch.zeros(9)
            for n in range(16):
                re = re + x[n] * cs[:, n]
                im = im - x[n] * sn[:, n]
            out[b, fr, 0:9], out[b, fr, 9:18] = re, (-im if sab == "imag_sign" else im)
    return out


def stft_cases():
    out = [stft_case(Lw) for Lw in (16, 20, 36, 256)] + [stft_case(64, ragged=True)]
    for kind in ("impulse0", "impulse1", "impulse-2", "impulse-1"):
        out += [stft_case(20, kind=kind), stft_case(64, ragged=True, kind=kind)]
    return out


# ================================================================================================== frames and overlap-add
ISTFT_SABOTAGES = ("nyquist_sign", "env_minus_one", "ola_nf-1")


def istft_case(F_, kind="uniform", ragged=False, ld=32, seed=0):
    """post (B, F, ld): 18 pre-activations uniform in [-3, 3], NaN-free pad columns unused by the kernel (they hold NaN here).
    kind: uniform | clip (log-magnitudes 5: exp above the clip at 100) | limit (audio_limit low enough to be reached).
    ragged: nf per row, frame rows at and above nf[b] NaN, src = [2, 0] into a 3-row output."""
    g = torch.Generator().manual_seed(9500 + F_ + seed)
    B = 2 if ragged else 3
    post = torch.full((B, F_, ld), NAN)
    post[:, :, :18] = torch.rand(B, F_, 18, generator=g) * 6.0 - 3.0
    if kind == "clip":
        post[:, :, :9] = 5.0
    limit = 0.99
    if kind == "limit":
        limit = 0.25
    nf = [F_, max(2, F_ // 2)] if ragged else [F_] * B
    lw = [4 * (n - 1) for n in nf]
    return dict(F=F_, B=B, ld=ld, kind=kind, ragged=ragged, post=post, limit=limit, nf=nf, lw=lw, Lw=4 * (F_ - 1),
                src=[2, 0] if ragged else list(range(B)), n_utt=3)


def istft_id(c):
    return f"F{c['F']}-{c['kind']}-{'ragged' if c['ragged'] else 'plain'}"


def frames_args(c):
    a = dict(stage=3, B=c["B"], n_utt=c["B"], F=c["F"], ld=c["ld"])
    a["in"] = c["post"]
    return a


def ola_args(c, frames):
    """frames (B, F, 16) fp32; the ragged form poisons the rows at and above nf[b]"""
    fr = frames.clone().reshape(c["B"], c["F"], 16)
    a = dict(stage=4, B=c["B"], n_utt=c["n_utt"], F=c["F"], Lw=c["Lw"], limit=c["limit"])
    if c["ragged"]:
        for b, n in enumerate(c["nf"]):
            fr[b, n:] = NAN
        a.update(src=c["src"], lw=c["lw"], nf=c["nf"])
    a["in"] = fr
    return a


def ref_frames(c):
    """(frames, bound) float64 (B, F, 16): the first half of seedvc_oracle.istft16 (irfft of clip(exp) e^{i sin}, windowed)"""
    v = c["post"][:, :, :18]
    mag = torch.clip(torch.exp(v[..., :9].double()), max=1e2)
    ph = torch.sin(v[..., 9:].double())
    re, im = mag * torch.cos(ph), mag * torch.sin(ph)
    w = _hann(torch.float64)
    n = torch.arange(16, dtype=torch.float64)[:, None]
    k = torch.arange(9, dtype=torch.float64)[None, :]
    ang = 2 * math.pi * n * k / 16
    wk = torch.full((9,), 2.0, dtype=torch.float64)
    wk[0] = wk[-1] = 1.0
    cosb = torch.cos(ang) * wk / 16
    sinb = -torch.sin(ang) * wk / 16
    sinb[:, 0] = 0
    sinb[:, -1] = 0
    fr = (re @ cosb.T + im @ sinb.T) * w
    A = ((re.abs() + im.abs()) * wk).sum(-1, keepdim=True)
    return fr, 2.0 ** -19 * (w / 16) * A + 2.0 ** -24 * fr.abs()


def emu_frames(c, sab=None):
    v = c["post"][:, :, :18]
    mag = torch.clamp(torch.exp(v[..., :9].double()).float(), max=1e2)
    ph = torch.sin(v[..., 9:].double()).float()
    re, im = mag * torch.cos(ph.double()).float(), mag * torch.sin(ph.double()).float()
    cs, sn = _twiddles(torch.float32, 8)
    w = _hann(torch.float32)
    out = torch.zeros(c["B"], c["F"], 16)
    for n in range(16):
        sign = 1.0 if (n % 2 == 0 or sab == "nyquist_sign") else -1.0
        acc = re[..., 0] + sign * re[..., 8]
        for k in range(1, 8):
            acc = acc + 2.0 * (re[..., k] * cs[k, n] - im[..., k] * sn[k, n])
        out[..., n] = acc * f32(1.0 / 16.0) * w[n]
    return out


def _ola(frames, nf, lw, Lw, dt, limit, sab=None):
    """one row: frames (F, 16) -> Lw samples, the second half of istft16 (overlap-add, envelope, trim), clamped; zeros from lw"""
    w = _hann(dt)
    y = torch.zeros(Lw + 16, dtype=dt)
    env = torch.zeros(Lw + 16, dtype=dt)
    absum = torch.zeros(Lw + 16, dtype=torch.float64)
    if sab == "ola_nf-1":
        nf = nf - 1
    for f in range(nf):
        y[4 * f:4 * f + 16] += frames[f].to(dt)
        absum[4 * f:4 * f + 16] += frames[f].abs().double()
        if not (sab == "env_minus_one" and f == nf - 1):
            env[4 * f:4 * f + 16] += w * w
    out = torch.zeros(Lw, dtype=dt)
    out[:lw] = (y[8:8 + lw] / env[8:8 + lw]).clamp(-limit, limit)
    return out, absum[8:8 + Lw], env[8:8 + Lw].double()


def ref_ola(c, frames, frames_bound=None):
    """(ref, bound) float64 (n_utt, Lw) with NaN marking the rows no micro-batch row maps to (they keep their canary).
    frames (B, F, 16): the stage's input; frames_bound: the bound of the frames themselves when they come from the frames stage"""
    ref = torch.full((c["n_utt"], c["Lw"]), NAN, dtype=torch.float64)
    bound = torch.zeros_like(ref)
    fr = frames.reshape(c["B"], c["F"], 16).double()
    for b in range(c["B"]):
        r, absum, env = _ola(fr[b], c["nf"][b], c["lw"][b], c["Lw"], torch.float64, float(f32(c["limit"])))
        ref[c["src"][b]] = r
        bd = 2.0 ** -20 * absum
        if frames_bound is not None:
            bd = bd + _ola(frames_bound.reshape(c["B"], c["F"], 16)[b], c["nf"][b], c["lw"][b], c["Lw"], torch.float64, 1e30)[1]
        bound[c["src"][b], :c["lw"][b]] = (bd / env)[:c["lw"][b]]
    return ref, bound


def emu_ola(c, frames, sab=None):
    out = torch.full((c["n_utt"], c["Lw"]), CANARY32)
    fr = frames.reshape(c["B"], c["F"], 16).float()
    for b in range(c["B"]):
        out[c["src"][b]] = _ola(fr[b], c["nf"][b], c["lw"][b], c["Lw"], torch.float32, f32(c["limit"]), sab)[0]
    return out


def check_ola(c, out, ref, bound):
    """canary rows first, then check_rows on the mapped rows"""
    dead = torch.isnan(ref).all(dim=1)
    fails = []
    if not bool((out[dead] == CANARY32).all()):
        fails.append("overlap-add: a row no micro-batch row maps to was written")
    f, ratio = check_rows(out[~dead], ref[~dead], bound[~dead], "overlap-add")
    return fails + f, ratio


def istft_cases():
    out = [istft_case(F_) for F_ in (2, 3, 5, 9, 17)]
    out += [istft_case(9, "clip"), istft_case(17, "limit"), istft_case(17, ragged=True), istft_case(5, ragged=True)]
    return out


# every named sabotage of an emulation: what a subtly wrong kernel would compute
SABOTAGES = {
    "clamp_L-2": "act_cl: the window clamped at L - 2",
    "clamp_batch_L": "act_cl, ragged: the window clamped at L - 1 of the batch where lens[b] - 1 is meant",
    "swap_taps01": "act_cl: taps 0 and 1 swapped",
    "odd_even": "act_cl: the odd and the even tap sets exchanged",
    "no_x2_tail": "act_cl: the x2 dropped for the last two s values of a 64-row segment",
    "lo_unrounded": "act_cl: lo computed from the unrounded hi",
    "p8_bytes_swapped": "act_cl: the two fp8 bytes swapped",
    "r_not_r+1": "source: sample offset r where r + 1 is meant",
    "noise_stride_S": "source: a harmonic's noise row read at stride S up where S_in up is meant",
    "phase0_by_row": "source: phase0 indexed by micro-batch row where the utterance is meant",
    "reflect_at_Lw": "STFT: reflected at Lw where lw[b] is meant",
    "nf+1": "STFT: nf[b] one too many", "nf-1": "STFT: nf[b] one too few", "ola_nf-1": "overlap-add: nf[b] one too few",
    "imag_sign": "STFT: the imaginary sign flipped",
    "nyquist_sign": "frames: the Nyquist bin's sign fixed",
    "env_minus_one": "overlap-add: the envelope missing one frame",
}
assert set(SABOTAGES) == set(ACT_SABOTAGES + SRC_SABOTAGES + STFT_SABOTAGES + ISTFT_SABOTAGES)


# ================================================================================================== mel_to_cl and ew_cl
VD = {"f16": 0, "f32": 1, "f16+lo": 2}


def cast_planes(v, form):
    """bit-for-bit prediction of the casts: hi = half(v), lo = half(v - hi)"""
    if form == "f32":
        return v.clone(), None
    hi = v.half()
    return hi.view(torch.int16), ((v - hi.float()).half().view(torch.int16) if form == "f16+lo" else None)


def mel_case(ragged, C=20, S=5, S_in=7, ld=32, B=3, seed=0):
    g = torch.Generator().manual_seed(9700 + seed)
    mel = torch.randn(B, C, S_in, generator=g) * 3.0
    lens = [5, 3, 0] if ragged else [S] * B
    src = [2, 0, 1] if ragged else list(range(B))
    for j in range(B):
        mel[src[j], :, lens[j]:] = NAN
    return dict(ragged=ragged, C=C, S=S, S_in=S_in, ld=ld, B=B, mel=mel, lens=lens, src=src)


def mel_args(c, form):
    a = dict(stage=5, B=c["B"], n_utt=c["B"], C=c["C"], S=c["S"], S_in=c["S_in"], ld=c["ld"], vd=VD[form])
    a["in"] = c["mel"]
    if c["ragged"]:
        a.update(src=c["src"], len=c["lens"])
    return a


def mel_want(c, form):
    v = torch.zeros(c["B"], c["S"], c["ld"])
    for j in range(c["B"]):
        n = c["lens"][j]
        v[j, :n, :c["C"]] = c["mel"][c["src"][j], :, :n].T
    return cast_planes(v, form)


def ew_case(mode, C=20, rows=7, ld=32, B=3, seed=0):
    g = torch.Generator().manual_seed(9800 + mode + seed)
    x = torch.full((B * rows, ld), NAN)
    x[:, :C] = torch.randn(B * rows, C, generator=g) * 3.0
    return dict(mode=mode, C=C, S=rows, ld=ld, B=B, x=x, slope=0.1)


def ew_args(c, form):
    a = dict(stage=6, B=c["B"], n_utt=c["B"], C=c["C"], S=c["S"], ld=c["ld"], vd=VD[form], mode=c["mode"], slope=c["slope"])
    a["in"] = c["x"]
    return a


def ew_want(c, form):
    v = torch.zeros_like(c["x"])
    x = c["x"][:, :c["C"]]
    v[:, :c["C"]] = torch.where(x > 0, x, x * f32(c["slope"])) if c["mode"] == 2 else x
    return cast_planes(v, form)
