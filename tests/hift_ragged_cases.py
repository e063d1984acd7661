"""Inputs and references shared by the ragged-HiFT tests (test_host_hift_ragged.py, test_gpu_hift_ragged.py).

`ragged_reference` is the yardstick: the CPU oracle run alone on each utterance's own frames, f0 and draws, zero tail.
`masked_model` is a CPU model of the design the HIP path implements, on the oracle's ops: every conv (the f0 predictor's,
the transposed ones and the source branch's included) reads rows at and above an utterance's end as its zero padding, the
source stops at the utterance's last sample, the STFT reflects there and gives `F_b = Lw_b / hop + 1` frames, and the
overlap-add runs over those frames.  Everything the design leaves unmasked -- the raw output of every conv, and mel frames,
f0 values and noise samples past an utterance's end -- is overwritten with NaN, so that a read of such a value shows up as
a non-finite sample."""
import numpy as np
import torch
import torch.nn.functional as F

import cases
import seedvc_oracle as O

MODEL = "hift_r"
# longest, the two sides of each kernel-choice boundary of the model (192 rows: 192 frames at the first stage, 24 at the
# second, 8 x 24 = 192), short, shorter than a conv's reach, one frame, empty, and the longest again
LENS = [300, 193, 192, 191, 47, 24, 23, 5, 1, 0, 300]
FULL_LENS = [200, 192, 47, 1]
LOG_MEL_FLOOR = -11.512925464970229
NAN = float("nan")


def total_up(c):
    return O.hift_total_upsample(c)


def utterance(c, sd, b, n, tag="hr"):
    """mel (1, 80, n), phase0 (1, nh, 1), noise (1, nh, n * up), f0 (1, n) = the oracle's f0 of the utterance alone: a fixed
    seed per utterance, whatever its place in a batch."""
    nh = c["nb_harmonics"] + 1
    mel = cases.logmel(f"{tag}.mel", 100 + b, 1, c["in_channels"], n)
    phase0 = (cases.rand(f"{tag}.phase", 100 + b, 1, nh, 1) * 2 - 1) * float(np.pi)
    noise = cases.randn(f"{tag}.noise", 100 + b, 1, nh, n * total_up(c))
    return mel, phase0, noise, O.hift_f0_predictor(sd, mel)


def batch(c, sd, lens, fill=NAN, ids=None, tag="hr"):
    """dict(mel (B, 80, S), f0 (B, S), phase0 (B, nh, 1), noise (B, nh, S * up)), S = max(lens): utterance ids[b] (default b)
    in the leading part of row b, `fill` in every padding frame, f0 slot and noise sample."""
    ids = list(range(len(lens))) if ids is None else ids
    B, S, nh, up = len(lens), max(max(lens), 1), c["nb_harmonics"] + 1, total_up(c)
    out = dict(mel=torch.full((B, c["in_channels"], S), fill), f0=torch.full((B, S), fill), phase0=torch.zeros(B, nh, 1),
               noise=torch.full((B, nh, S * up), fill))
    for b, n in enumerate(lens):
        mel, phase0, noise, f0 = utterance(c, sd, ids[b], max(n, 1), tag)
        out["phase0"][b] = phase0[0]
        if n:
            out["mel"][b, :, :n], out["f0"][b, :n], out["noise"][b, :, :n * up] = mel[0], f0[0], noise[0]
    return out


def ragged_reference(sd, c, bt, lens, predicted_f0=False):
    """(B, S * up): the oracle alone on row b's first lens[b] frames (pinned f0 unless predicted_f0), zeros above."""
    up = total_up(c)
    out = torch.zeros(bt["mel"].shape[0], bt["mel"].shape[2] * up)
    for b, n in enumerate(lens):
        if n:
            out[b, :n * up] = O.hift_forward(sd, c, bt["mel"][b:b + 1, :, :n], bt["phase0"][b:b + 1], bt["noise"][b:b + 1, :, :n * up],
                                             f0=None if predicted_f0 else bt["f0"][b:b + 1, :n])[0]
    return out


def _keep(x, L):
    return torch.arange(x.shape[-1])[None, None, :] < torch.tensor(L)[:, None, None]


def mask_rows(x, L):            # a conv's operand load: rows past the end read as zero -- a selection (0 * NaN is NaN)
    return torch.where(_keep(x, L), x, torch.zeros_like(x))


def poison(x, L):               # what the design leaves unmasked: anything at all
    return torch.where(_keep(x, L), x, torch.full_like(x, NAN))


def _conv(x, L, sd, p, Lout=None, weight_norm=True, **kw):
    """a conv of the ragged call: bounded operand load, raw output poisoned past the utterance's output rows"""
    w = O.wn_weight(sd, p) if weight_norm else sd[p + ".weight"].float()
    return poison(F.conv1d(mask_rows(x, L), w, sd[p + ".bias"].float(), **kw), L if Lout is None else Lout)


def _resblock(x, L, sd, p, k, dils):
    for d, dil in enumerate(dils):
        xt = O.snake(x, sd[f"{p}.activations1.{d}.alpha"].float())
        xt = _conv(xt, L, sd, f"{p}.convs1.{d}", dilation=dil, padding=(k * dil - dil) // 2)
        xt = O.snake(xt, sd[f"{p}.activations2.{d}.alpha"].float())
        xt = _conv(xt, L, sd, f"{p}.convs2.{d}", padding=(k - 1) // 2)
        x = xt + x
    return x


def masked_f0(sd, mel, lens):
    """(B, S): the f0 predictor of the ragged call, NaN at and above lens[b]"""
    x = mel
    for idx in (0, 2, 4, 6, 8):
        x = poison(F.elu(_conv(x, lens, sd, f"f0_predictor.condnet.{idx}", padding=1)), lens)
    y = F.linear(x.transpose(1, 2), sd["f0_predictor.classifier.weight"].float(), sd["f0_predictor.classifier.bias"].float())
    return torch.abs(y.squeeze(-1))


def masked_model(sd, c, bt, lens, predicted_f0=False):
    """-> (wave (B, S * up), f0 (B, S)) of the design on the oracle's ops."""
    mel, phase0, noise = bt["mel"], bt["phase0"], bt["noise"]
    B, S = mel.shape[0], mel.shape[2]
    up, hop, nfft = total_up(c), c["istft_hop"], c["istft_n_fft"]
    L = list(lens)
    Lw = [n * up for n in L]
    LF = [n * up // hop + 1 if n else 0 for n in L]
    f0 = masked_f0(sd, mel, L) if predicted_f0 else bt["f0"]
    f0 = mask_rows(f0[:, None, :], L)[:, 0]                                  # the gather selects; the phase prefix is causal
    # source: stops at the utterance's last sample (the NaN noise above it never enters), tail zero by selection
    s = mask_rows(O.hift_source(sd, c, f0, phase0, noise), Lw)
    # STFT per utterance: reflected at its own last sample, F_b frames, zero rows above
    F_all = S * up // hop + 1
    s_stft = torch.zeros(B, nfft + 2, F_all)
    for b in range(B):
        if L[b]:
            re, im = O.stft16(s[b:b + 1, 0, :Lw[b]], nfft, hop)
            s_stft[b, :, :LF[b]] = torch.cat([re, im], dim=1)[0]
    x = _conv(mel, L, sd, "conv_pre", padding=3)
    nk, nup, ups = len(c["resblock_kernel_sizes"]), len(c["upsample_rates"]), c["upsample_rates"]
    cum = list(np.cumprod([1] + ups[::-1][:-1]))[::-1]
    for i, (u, k) in enumerate(zip(ups, c["upsample_kernel_sizes"])):
        x = F.leaky_relu(x, c["lrelu_slope"])
        x = F.conv_transpose1d(mask_rows(x, L), O.wn_weight(sd, f"ups.{i}"), sd[f"ups.{i}.bias"].float(), stride=u, padding=(k - u) // 2)
        L = [n * u for n in L]
        if i == nup - 1:        # ReflectionPad1d((1, 0)): row 0 = row 2 of a sequence one row longer
            x = F.pad(x, (1, 0), mode="reflect")
            L = [n + 1 if n else 0 for n in L]
        x = poison(x, L)
        r = int(cum[i])
        kw = dict(stride=r, padding=r // 2) if r != 1 else {}
        si = _conv(s_stft, LF, sd, f"source_downs.{i}", Lout=L, weight_norm=False, **kw)
        si = _resblock(si, L, sd, f"source_resblocks.{i}", c["source_resblock_kernel_sizes"][i], c["source_resblock_dilation_sizes"][i])
        x = x + si
        acc = None
        for j, (rk, dils) in enumerate(zip(c["resblock_kernel_sizes"], c["resblock_dilation_sizes"])):
            y = _resblock(x, L, sd, f"resblocks.{i * nk + j}", rk, dils)
            acc = y if acc is None else acc + y
        x = acc / nk
    assert L == LF
    x = _conv(F.leaky_relu(x), L, sd, "conv_post", padding=3)
    nb = nfft // 2 + 1
    wave = torch.zeros(B, S * up)
    for b in range(B):          # overlap-add and window envelope over the utterance's own F_b frames
        if L[b]:
            y = O.istft16(torch.exp(x[b:b + 1, :nb, :L[b]]), torch.sin(x[b:b + 1, nb:, :L[b]]), nfft, hop)
            wave[b, :Lw[b]] = torch.clamp(y, -c["audio_limit"], c["audio_limit"])[0]
    return wave, mask_rows(f0[:, None, :], list(lens))[:, 0]


def rms(a, b):
    return (a - b).pow(2).mean().sqrt().item()
