"""Inputs and the CPU statement of the design shared by the ragged reference front-end tests (test_host_frontend_ragged.py,
test_gpu_frontend_ragged.py): batches of reference clips of different lengths for the log-mel, the Kaldi fbank and CAMPPlus.

Every padding sample or frame of a batch is NaN, so a read of one as a value shows up as a non-finite output.  The yardstick
is always the oracle run alone on the clip's own samples or frames.  `masked_campplus` states in torch what csrc/campplus.hip
does for a batch with lengths: time steps at and above a clip's end are zero after every FCM conv, and from the TDNN on clip b
has its own T2_b rows, its own CAM segments and global mean, and its own pooled statistics; what the design leaves unmasked
(rows at and above T2_b of the dense blocks) is overwritten with NaN."""
import numpy as np
import torch
import torch.nn.functional as F

import cases
import seedvc_oracle as O

# ---- CAMPPlus, the reduced model: T2 = 130 (two segments, the last of 30), 102 (last segment of 2 frames), 29 (less than one
# segment), 4 (the minimum); odd and even T
CP_MODEL = "campplus_r"
CP_LENS = (260, 203, 57, 8)
# ---- CAMPPlus, the drivers' model: row 0 = the campplus_full feature clip (500 frames), row 1 an independent 301-frame clip
CP_FULL_LENS = (500, 301)
# ---- log-mel: mel_r (pad 24, hop 16; 25 samples = the shortest legal clip, one frame) and the 22 kHz preset (row 0 = the
# golden clip)
MEL_R_LENS = (400, 211, 25)
MEL_22K_LENS = (22050, 9000)
# ---- Kaldi fbank: 228, 29 and 1 frames
FB_LENS = (36800, 5000, 400)

NAN = float("nan")


def t2_of(n):
    return (n - 1) // 2 + 1


def cp_clip(c, cid, n):
    """(n, feat_dim) mean-normalised features of clip `cid`: a fixed seed per clip, whatever its place in a batch."""
    f = cases.randn("fr.feat", 300 + cid, n, c["feat_dim"]) * 2.0
    return f - f.mean(dim=0, keepdim=True)


def cp_batch(c, lens=CP_LENS, ids=None):
    """(B, max(lens), feat_dim): clip ids[b] (default b) in row b, NaN in every padding frame."""
    ids = list(range(len(lens))) if ids is None else ids
    x = torch.full((len(lens), max(lens), c["feat_dim"]), NAN)
    for b, n in enumerate(lens):
        x[b, :n] = cp_clip(c, ids[b], n)
    return x


def cp_full_batch():
    """(c, sd, feat (2, 500, 80)): the campplus_full case in row 0, an independent 301-frame clip in row 1."""
    c, sd, feat = cases.campplus_case("campplus_full")
    assert feat.shape[:2] == (1, CP_FULL_LENS[0])
    x = torch.full((2, CP_FULL_LENS[0], c["feat_dim"]), NAN)
    x[0] = feat[0]
    x[1, :CP_FULL_LENS[1]] = cp_clip(c, 50, CP_FULL_LENS[1])
    return c, sd, x


def _tone(tag, cid, n, sr, f_lo, f_span, noise):
    t = torch.arange(n, dtype=torch.float32) / sr
    f1 = f_lo + f_span * float(cases.rand(tag + ".f", 400 + cid, 1))
    y = 0.4 * torch.sin(2 * np.pi * f1 * t) + 0.2 * torch.sin(2 * np.pi * 3.1 * f1 * t) + noise * cases.randn(tag + ".n", 400 + cid, n)
    return y.clamp(-1, 1)


def mel_batch(name):
    """(cfg, y (B, L) with NaN above each clip's samples, mel basis, lens).  mel_22k: row 0 is the golden clip."""
    c, y0, basis = cases.mel_case(name)
    lens = {"mel_r": MEL_R_LENS, "mel_22k": MEL_22K_LENS}[name]
    y = torch.full((len(lens), max(lens)), NAN)
    for b, n in enumerate(lens):
        if name == "mel_22k" and b == 0:
            y[0] = y0[0]
        else:
            clip = _tone("fr.mel." + name, b, n, c["sr"], 110.0, 600.0, 0.05)
            clip[n // 2: n // 2 + n // 8] *= 0.001           # a near-silent stretch (clamp / log floor)
            y[b, :n] = clip
    return c, y, basis, lens


def fbank_batch(lens=FB_LENS):
    """(B, max(lens)) sine + noise at 16 kHz, NaN above each clip's samples."""
    y = torch.full((len(lens), max(lens)), NAN)
    for b, n in enumerate(lens):
        t = torch.arange(n, dtype=torch.float32) / 16000
        f1 = 180.0 + 60.0 * b
        y[b, :n] = 0.3 * torch.sin(2 * np.pi * f1 * t) + 0.2 * torch.sin(2 * np.pi * 6.3 * f1 * t) + 0.02 * cases.randn("fr.fb", 500 + b, n)
    return y


def fbank_frames(n):
    return 1 + (n - 400) // 160 if n >= 400 else 0


# ---------------------------------------------------------------------------------------------- the design, on the CPU
def _keep(x, L):                     # x (B, ..., T): True below each clip's length along the last axis
    shape = [len(L)] + [1] * (x.dim() - 1)
    return torch.arange(x.shape[-1]).reshape([1] * (x.dim() - 1) + [-1]) < torch.tensor(L).reshape(shape)


def _zero(x, L):                     # select, not multiply (0 * NaN is NaN)
    return torch.where(_keep(x, L), x, torch.zeros_like(x))


def _poison(x, L):
    return torch.where(_keep(x, L), x, torch.full_like(x, NAN))


def masked_campplus(sd, c, feat, lens):
    """feat (B, Tmax, feat_dim) with anything above lens[b] -> (B, embedding_size), every row as if its clip ran alone."""
    L = list(lens)
    bn = O._bn
    x = _zero(feat.permute(0, 2, 1).unsqueeze(1), L)                        # (B, 1, F, T): frames above the end are not read
    out = _zero(torch.relu(bn(F.conv2d(x, sd["head.conv1.weight"], padding=1), sd, "head.bn1")), L)
    for layer in ("layer1", "layer2"):
        for b in range(2):
            p = f"head.{layer}.{b}"
            stride = (2, 1) if b == 0 else (1, 1)
            y = _zero(torch.relu(bn(F.conv2d(out, sd[p + ".conv1.weight"], stride=stride, padding=1), sd, p + ".bn1")), L)
            y = bn(F.conv2d(y, sd[p + ".conv2.weight"], padding=1), sd, p + ".bn2")
            sc = out
            if b == 0:
                sc = _zero(bn(F.conv2d(out, sd[p + ".shortcut.0.weight"], stride=stride), sd, p + ".shortcut.1"), L)
            out = _zero(torch.relu(y + sc), L)
    out = _zero(torch.relu(bn(F.conv2d(out, sd["head.conv2.weight"], stride=(2, 1), padding=1), sd, "head.bn2")), L)
    x = out.reshape(out.shape[0], out.shape[1] * out.shape[2], out.shape[3])
    x = torch.relu(bn(F.conv1d(x, sd["xvector.tdnn.linear.weight"], stride=2, padding=2), sd, "xvector.tdnn.nonlinear.batchnorm"))
    L2 = [t2_of(n) for n in L]
    x = _poison(x, L2)                                                       # rows at and above T2_b hold anything
    seg = c["seg_len"]
    for bi, (nl, k, dil) in enumerate(zip(c["block_layers"], c["block_kernel"], c["block_dilation"])):
        for i in range(nl):
            p = f"xvector.block{bi + 1}.tdnnd{i + 1}"
            h = F.conv1d(torch.relu(bn(x, sd, p + ".nonlinear1.batchnorm")), sd[p + ".linear1.weight"])
            h = torch.relu(bn(h, sd, p + ".nonlinear2.batchnorm"))
            # the dilated taps zero-pad at the clip's own last row
            y = F.conv1d(_zero(h, L2), sd[p + ".cam_layer.linear_local.weight"], padding=(k - 1) // 2 * dil, dilation=dil)
            new = torch.full_like(y, NAN)
            for b, n in enumerate(L2):                                       # the clip's own segments and global mean
                hb = h[b:b + 1, :, :n]
                sp = F.avg_pool1d(hb, kernel_size=seg, stride=seg, ceil_mode=True)
                sp = sp.unsqueeze(-1).expand(*sp.shape, seg).reshape(*sp.shape[:-1], -1)[..., :n]
                ctx = hb.mean(-1, keepdim=True) + sp
                ctx = torch.relu(F.conv1d(ctx, sd[p + ".cam_layer.linear1.weight"], sd[p + ".cam_layer.linear1.bias"]))
                m = torch.sigmoid(F.conv1d(ctx, sd[p + ".cam_layer.linear2.weight"], sd[p + ".cam_layer.linear2.bias"]))
                new[b:b + 1, :, :n] = y[b:b + 1, :, :n] * m
            x = torch.cat([x, new], dim=1)
        p = f"xvector.transit{bi + 1}"
        x = F.conv1d(torch.relu(bn(x, sd, p + ".nonlinear.batchnorm")), sd[p + ".linear.weight"])
    x = torch.relu(bn(x, sd, "xvector.out_nonlinear.batchnorm"))
    stats = torch.cat([torch.cat([x[b:b + 1, :, :n].mean(dim=-1), x[b:b + 1, :, :n].std(dim=-1, unbiased=True)], dim=-1)
                       for b, n in enumerate(L2)])
    e = F.conv1d(stats.unsqueeze(-1), sd["dense.linear.weight"]).squeeze(-1)
    return bn(e, sd, "dense.nonlinear.batchnorm", affine=False)
