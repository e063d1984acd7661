"""Inputs and references shared by the ragged-vocoder tests (test_host_vocoder_ragged.py, test_gpu_vocoder_ragged.py).

`ragged_reference` is the yardstick: the CPU oracle run alone on each utterance's own frames, zero tail.  `masked_model` is
a CPU model of the design the HIP path implements -- every producer of a conv operand respects the lengths, the convs do
not -- with everything the design leaves unmasked (raw conv outputs and input frames past an utterance's end) overwritten
with NaN, so that a read of such a row as a value shows up as a non-finite sample."""
import torch
import torch.nn.functional as F

import cases
import seedvc_oracle as O

MODELS = ("bigvgan_r", "bigvgan_r2")
# longest, mid, the two sides of the 192-row kernel-choice boundary, short, shorter than the activation's window, one frame,
# empty, and the longest again
LENS = [430, 301, 192, 191, 47, 5, 1, 0, 430]
FULL_LENS = [301, 250, 192, 47]
PAD_FRAMES = 40                      # floor-valued frames of the "padding is not a substitute" check
LOG_MEL_FLOOR = -11.512925464970229


def utterance_mel(h, b, n, tag="ragged.mel"):
    """(num_mels, n) log-mel of utterance b: a fixed seed per utterance, whatever its place in a batch."""
    return cases.logmel(tag, 100 + b, 1, h["num_mels"], n)[0]


def batch_mel(h, lens, fill=float("nan"), ids=None, tag="ragged.mel"):
    """(B, num_mels, max(lens)) with utterance ids[b] (default b) in row b and `fill` in the padding frames."""
    ids = list(range(len(lens))) if ids is None else ids
    mel = torch.full((len(lens), h["num_mels"], max(max(lens), 1)), fill)
    for b, n in enumerate(lens):
        if n:
            mel[b, :, :n] = utterance_mel(h, ids[b], n, tag)
    return mel


def total_up(h):
    up = 1
    for u in h["upsample_rates"]:
        up *= u
    return up


def ragged_reference(sd, h, mel, lens):
    """(B, 1, S * up): the oracle alone on mel[b, :, :lens[b]], zeros above lens[b] * up."""
    up = total_up(h)
    out = torch.zeros(mel.shape[0], 1, mel.shape[2] * up)
    for b, n in enumerate(lens):
        if n:
            out[b, 0, :n * up] = O.bigvgan_forward(sd, h, mel[b:b + 1, :, :n]).reshape(-1)
    return out


def _keep(x, L):
    return torch.arange(x.shape[2])[None, None, :] < torch.tensor(L)[:, None, None]


def mask_rows(x, L):            # producer side: select, not multiply (0 * NaN is NaN)
    return torch.where(_keep(x, L), x, torch.zeros_like(x))


def poison(x, L):               # what the design leaves unmasked: anything at all
    return torch.where(_keep(x, L), x, torch.full_like(x, float("nan")))


def act_ragged(x, L, filt, a, ib):      # per-utterance replicate edge at L_b - 1, zero rows past L_b
    out = torch.zeros_like(x)
    for b, n in enumerate(L):
        if n > 0:
            out[b:b + 1, :, :n] = O.anti_alias_act(x[b:b + 1, :, :n], filt, a, ib)
    return out


def masked_model(sd, h, mel, lens):
    """(B, 1, S * up) of the producer-masking design on the oracle's ops."""
    has_beta = h["activation"] == "snakebeta"
    logs = h["snake_logscale"]
    L = list(lens)
    x = poison(F.conv1d(mask_rows(mel, L), O.wn_weight(sd, "conv_pre"), sd["conv_pre.bias"].float(), padding=3), L)
    nk = len(h["resblock_kernel_sizes"])
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(mask_rows(x, L), O.wn_weight(sd, f"ups.{i}.0"), sd[f"ups.{i}.0.bias"].float(), stride=u,
                               padding=(k - u) // 2)
        L = [n * u for n in L]
        x = poison(x, L)
        acc = None
        for j, (rk, dils) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
            p = f"resblocks.{i * nk + j}"
            y = x
            for d, dil in enumerate(dils):
                filt = sd[f"{p}.activations.{2 * d}.upsample.filter"].reshape(12)
                a, ib = O.snakebeta_params(sd, f"{p}.activations.{2 * d}.act", logs, has_beta)
                xt = act_ragged(y, L, filt, a, ib)
                xt = poison(F.conv1d(xt, O.wn_weight(sd, f"{p}.convs1.{d}"), sd[f"{p}.convs1.{d}.bias"].float(), dilation=dil,
                                     padding=(rk * dil - dil) // 2), L)
                a, ib = O.snakebeta_params(sd, f"{p}.activations.{2 * d + 1}.act", logs, has_beta)
                xt = act_ragged(xt, L, filt, a, ib)
                xt = poison(F.conv1d(xt, O.wn_weight(sd, f"{p}.convs2.{d}"), sd[f"{p}.convs2.{d}.bias"].float(),
                                     padding=(rk - 1) // 2), L)
                y = xt + y
            acc = y if acc is None else acc + y
        x = acc / nk
    filt = sd["activation_post.upsample.filter"].reshape(12)
    a, ib = O.snakebeta_params(sd, "activation_post.act", logs, has_beta)
    x = act_ragged(x, L, filt, a, ib)
    b = sd.get("conv_post.bias")
    x = F.conv1d(x, O.wn_weight(sd, "conv_post"), None if b is None else b.float(), padding=3)
    x = torch.tanh(x) if h["use_tanh_at_final"] else torch.clamp(x, -1.0, 1.0)
    return mask_rows(x, L)


def rms(a, b):
    return (a - b).pow(2).mean().sqrt().item()
