"""Inputs and the yardstick shared by the RMVPE tests (test_host_rmvpe.py, test_gpu_rmvpe.py).

The yardstick is a torch restatement of RVC's `rmvpe.py` network (`E2E`: `nn.Conv2d` / `BatchNorm2d` / `ConvTranspose2d` / `GRU`
/ `Linear`, eval mode) run in **float64**, with the module tree -- and therefore the state-dict keys -- of the real `rmvpe.pt`,
plus the reference's mel front-end (torch.stft, center=True) and its numpy decode.  Weights come from a generator that also
randomises the BatchNorm gains, shifts and running statistics (with default statistics a wrong fold passes).  Every padding
sample or frame of a batch is NaN, so a read of one as a value shows up as a non-finite output."""
import functools
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from seedvc_amd import specs
from seedvc_amd.audio import htk_mel_basis

NAN = float("nan")
SR, N_FFT, HOP, N_MELS = 16000, 1024, 160, 128
CENTS0 = 1997.3794084376191

# the ragged batch: samples per clip -> 70, 32, 160 and 33 frames (1 + L // 160); 32 frames need no time padding (the deepest
# plane is one time step by four bins), 33 pad to 64, 70 to 96, 160 to 160
CLIP_LENS = (69 * 160 + 57, 31 * 160, 159 * 160 + 159, 32 * 160 + 1)
CLIP_FRAMES = tuple(1 + n // HOP for n in CLIP_LENS)
assert CLIP_FRAMES == (70, 32, 160, 33)
SHALLOW = dict(en_de_layers=1, n_blocks=1, inter_layers=1)
# |device salience - float64| allowed: four times the largest value measured on the MI355X over these cases; the
# float32 CPU restatement sits 6.5e-7 from float64 with this generator (1.6e-7 with the issue's).  May not exceed 1e-4 (the F0 test's exclusion margin rests on it)
SALIENCE_TOL = 3.7e-6              # 4 x 9.21e-7 (the 160-frame row of the ragged batch, full-size net)
assert SALIENCE_TOL <= 1e-4
MEL_TOL = 1e-4                   # the project's log-mel bound: mean |diff| of the log-mel, and the linear error relative to the frame's
                                 # largest mel value (test_gpu_frontend_ragged.py)


# ------------------------------------------------------------------------------------------------ the network, restated
class ConvBlockRes(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(),
                                  nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())
        self.is_shortcut = cin != cout
        if self.is_shortcut:
            self.shortcut = nn.Conv2d(cin, cout, 1)

    def forward(self, x):
        return self.conv(x) + (self.shortcut(x) if self.is_shortcut else x)


class ResEncoderBlock(nn.Module):
    def __init__(self, cin, cout, pool, n_blocks):
        super().__init__()
        self.conv = nn.ModuleList([ConvBlockRes(cin if j == 0 else cout, cout) for j in range(n_blocks)])
        self.pool = nn.AvgPool2d(2, 2) if pool else None

    def forward(self, x):
        for c in self.conv:
            x = c(x)
        return (x, self.pool(x)) if self.pool is not None else x


class Encoder(nn.Module):
    def __init__(self, n_layers, n_blocks, cout):
        super().__init__()
        self.bn = nn.BatchNorm2d(1)
        self.layers = nn.ModuleList()
        cin = 1
        for _ in range(n_layers):
            self.layers.append(ResEncoderBlock(cin, cout, True, n_blocks))
            cin, cout = cout, cout * 2

    def forward(self, x):
        skips = []
        x = self.bn(x)
        for layer in self.layers:
            s, x = layer(x)
            skips.append(s)
        return x, skips


class Intermediate(nn.Module):
    def __init__(self, cin, cout, n_layers, n_blocks):
        super().__init__()
        self.layers = nn.ModuleList([ResEncoderBlock(cin if i == 0 else cout, cout, False, n_blocks) for i in range(n_layers)])

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


class ResDecoderBlock(nn.Module):
    def __init__(self, cin, cout, n_blocks):
        super().__init__()
        self.conv1 = nn.Sequential(nn.ConvTranspose2d(cin, cout, 3, 2, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU())
        self.conv2 = nn.ModuleList([ConvBlockRes(2 * cout if j == 0 else cout, cout) for j in range(n_blocks)])

    def forward(self, x, skip):
        x = torch.cat((self.conv1(x), skip), dim=1)
        for c in self.conv2:
            x = c(x)
        return x


class Decoder(nn.Module):
    def __init__(self, cin, n_layers, n_blocks):
        super().__init__()
        self.layers = nn.ModuleList()
        for _ in range(n_layers):
            self.layers.append(ResDecoderBlock(cin, cin // 2, n_blocks))
            cin //= 2

    def forward(self, x, skips):
        for i, layer in enumerate(self.layers):
            x = layer(x, skips[-1 - i])
        return x


class DeepUnet(nn.Module):
    def __init__(self, c):
        super().__init__()
        L, nb, c0 = c["en_de_layers"], c["n_blocks"], c["en_out_channels"]
        self.encoder = Encoder(L, nb, c0)
        top = c0 << L
        self.intermediate = Intermediate(top // 2, top, c["inter_layers"], nb)
        self.decoder = Decoder(top, L, nb)

    def forward(self, x):
        x, skips = self.encoder(x)
        return self.decoder(self.intermediate(x), skips)


class BiGRU(nn.Module):
    def __init__(self, n_in, hidden):
        super().__init__()
        self.gru = nn.GRU(n_in, hidden, num_layers=1, batch_first=True, bidirectional=True)

    def forward(self, x):
        return self.gru(x)[0]


class E2E(nn.Module):
    """mel (B, n_mels, T) with T a multiple of 32 -> salience (B, T, n_bins)."""

    def __init__(self, c):
        super().__init__()
        self.unet = DeepUnet(c)
        self.cnn = nn.Conv2d(c["en_out_channels"], 3, 3, padding=1)
        self.fc = nn.Sequential(BiGRU(3 * c["n_mels"], c["gru_hidden"]), nn.Linear(2 * c["gru_hidden"], c["n_bins"]), nn.Dropout(0.25),
                                nn.Sigmoid())

    def forward(self, mel):
        x = mel.transpose(-1, -2).unsqueeze(1)               # (B, 1, T, n_mels)
        x = self.cnn(self.unet(x)).transpose(1, 2).flatten(-2)
        return self.fc(x)


# ------------------------------------------------------------------------------------------------ weights
def _rng(key, seed):
    return np.random.Generator(np.random.Philox(key=[zlib.crc32(key.encode()), seed & 0xFFFFFFFF]))


def make_state_dict(c, seed=0):
    """float32 state dict for `E2E(c)`: fan-in normalised convs (the second conv of a block at half gain, so the residual stream
    stays O(1) through ~30 blocks), BatchNorm gains 1 +- 0.3, shifts +- 0.2, running means +- 0.3 and variances 0.5 .. 1.5."""
    sd = {}
    for k, shp in specs.rmvpe_state_spec(c).items():
        g, leaf = _rng("rmvpe." + k, seed), k.split(".")[-1]
        if leaf == "num_batches_tracked":
            sd[k] = torch.tensor(0, dtype=torch.long)
            continue
        if leaf == "running_var":
            v = 0.5 + g.random(shp)
        elif leaf == "running_mean":
            v = g.standard_normal(shp) * 0.3
        elif len(shp) == 1 and leaf == "weight":             # BatchNorm gain
            v = 1.0 + 0.6 * (g.random(shp) - 0.5)
        elif len(shp) == 1:                                  # BatchNorm shift, conv / linear / GRU bias
            v = g.standard_normal(shp) * 0.2
        elif ".gru." in k:
            v = g.standard_normal(shp) * (0.5 / np.sqrt(shp[1])) * (3.0 if "weight_hh" in k else 1.0)
        elif "conv1.0.weight" in k:                          # ConvTranspose2d (cin, cout, 3, 3): 9 / 4 taps per output on average
            v = g.standard_normal(shp) * (1.0 / np.sqrt(shp[0] * 9 / 4))
        else:
            gain = 0.5 if ".conv.3." in k else 1.0
            v = g.standard_normal(shp) * (gain / np.sqrt(np.prod(shp[1:])))
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd


@functools.lru_cache(maxsize=None)
def model(kind, dtype=torch.float64):
    """(cfg, state dict, E2E in eval mode at `dtype`) for kind 'full' or 'shallow'."""
    c = specs.rmvpe_config(**(SHALLOW if kind == "shallow" else {}))
    sd = make_state_dict(c, seed=7 if kind == "shallow" else 3)
    net = E2E(c)
    net.load_state_dict(sd, strict=True)
    return c, sd, net.to(dtype).eval()


# ------------------------------------------------------------------------------------------------ inputs
def clip(cid, n):
    """n samples of clip `cid` at 16 kHz: a gliding harmonic tone plus noise, fixed per clip whatever its place in a batch."""
    g = _rng("rmvpe.clip", 100 + cid)
    t = np.arange(n) / SR
    f0 = 110.0 * (1 + cid) * (1.0 + 0.2 * np.sin(2 * np.pi * 1.5 * t + cid))
    ph = 2 * np.pi * np.cumsum(f0) / SR
    x = sum(np.sin(h * ph) / h for h in range(1, 6)) * 0.2 + g.standard_normal(n) * 0.02
    return torch.from_numpy(x.astype(np.float32))


def wave_batch(lens=CLIP_LENS, ids=None):
    """(B, max(lens)): clip ids[b] (default b) in row b, NaN in every padding sample."""
    ids = list(range(len(lens))) if ids is None else ids
    w = torch.full((len(lens), max(lens)), NAN)
    for b, n in enumerate(lens):
        w[b, :n] = clip(ids[b], n)
    return w


@functools.lru_cache(maxsize=None)
def basis():
    return htk_mel_basis(SR, N_FFT, N_MELS, 30, 8000)


def ref_mel(wave):
    """RMVPE's MelSpectrogram in float64: wave (n,) -> (n_mels, 1 + n // 160)."""
    w = wave.double()
    spec = torch.stft(w, N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT, dtype=torch.float64), center=True,
                      pad_mode="reflect", return_complex=True)
    mag = torch.sqrt(spec.real.pow(2) + spec.imag.pow(2))
    return torch.log(torch.clamp(basis().double() @ mag, min=1e-5))


@functools.lru_cache(maxsize=None)
def clip_mel(cid, n):
    """float64 reference mel of clip `cid`."""
    return ref_mel(clip(cid, n))


def mel_batch(lens=CLIP_LENS, ids=None):
    """(B, n_mels, max frames) float32: the reference mel of each clip rounded to float32, NaN in every padding frame."""
    ids = list(range(len(lens))) if ids is None else ids
    fr = [1 + n // HOP for n in lens]
    m = torch.full((len(lens), N_MELS, max(fr)), NAN)
    for b, n in enumerate(lens):
        m[b, :, :fr[b]] = clip_mel(ids[b], n).float()
    return m


def ref_salience(kind, mel):
    """The reference's `mel2hidden`: mel (n_mels, T) of ONE clip -> float64 salience (T, n_bins).  The clip is zero-padded in time
    to a multiple of 32 frames (`F.pad(mel, (0, n_pad), mode="constant")`), run alone, and cropped back."""
    _, _, net = model(kind)
    T = mel.shape[-1]
    Tpad = 32 * ((T + 31) // 32)
    with torch.no_grad():
        x = F.pad(mel.double().unsqueeze(0), (0, Tpad - T))
        return net(x)[0, :T]


@functools.lru_cache(maxsize=None)
def clip_salience(kind, cid, n, from_f32_mel=True):
    """float64 salience of clip `cid` run alone: from its float32-rounded reference mel (the input the salience seam gets), or
    from the float64 mel (the all-float64 chain the end-to-end test compares with)."""
    m = clip_mel(cid, n)
    return ref_salience(kind, m.float() if from_f32_mel else m)


# ------------------------------------------------------------------------------------------------ decode
def np_decode(salience, thred=0.03):
    """The reference's `decode` in float64: salience (T, 360) -> f0 (T,)."""
    s = np.asarray(salience, dtype=np.float64)
    cents_map = np.pad(20.0 * np.arange(360) + CENTS0, (4, 4))
    center = np.argmax(s, axis=1)                            # the first maximum on ties
    sp = np.pad(s, ((0, 0), (4, 4)))
    idx = center[:, None] + np.arange(9)[None, :]            # padded bins center .. center + 8 = bins center - 4 .. center + 4
    win = np.take_along_axis(sp, idx, axis=1)
    cents = (win * cents_map[idx]).sum(1) / win.sum(1)
    cents[s.max(axis=1) <= thred] = 0.0
    f0 = 10.0 * 2.0 ** (cents / 1200.0)
    f0[f0 == 10.0] = 0.0
    return f0


def top2_margin(salience):
    """per frame: the gap between the largest and the second largest salience."""
    top = torch.topk(torch.as_tensor(salience), 2, dim=-1).values
    return (top[..., 0] - top[..., 1]).numpy()


# ------------------------------------------------------------------------------------------------ the drivers' pitch step
def ref_f0_adjust(f0_alt, f0_ori, auto_f0_adjust, semitones):
    """The drivers' lines on one (source, reference) pair of float32 tracks -> (shifted f0_alt, median_alt, median_ori)."""
    voiced_alt, voiced_ori = f0_alt[f0_alt > 1], f0_ori[f0_ori > 1]
    log_alt, log_ori = torch.log(f0_alt + 1e-5), torch.log(f0_ori + 1e-5)
    m_alt = torch.median(log_alt[f0_alt > 1]) if voiced_alt.numel() else torch.tensor(0.0)
    m_ori = torch.median(log_ori[f0_ori > 1]) if voiced_ori.numel() else torch.tensor(0.0)
    shifted = log_alt.clone()
    if auto_f0_adjust and voiced_alt.numel() and voiced_ori.numel():
        shifted[f0_alt > 1] = log_alt[f0_alt > 1] - m_alt + m_ori
    out = torch.exp(shifted)
    if semitones != 0:
        out[f0_alt > 1] = out[f0_alt > 1] * 2 ** (semitones / 12)
    return out, m_alt, m_ori


def f0_tracks():
    """(f0_alt (5, 40), alt_lens, f0_ori (5, 31), ori_lens, semitones): rows with an odd and an even voiced count, one voiced
    frame, no voiced frame on the source side and no voiced frame on the reference side; NaN above every row's length."""
    g = _rng("rmvpe.tracks", 1)
    alt_lens, ori_lens = [40, 33, 17, 25, 12], [31, 20, 9, 14, 30]
    alt_voiced, ori_voiced = [21, 16, 1, 0, 7], [14, 9, 4, 6, 0]
    alt, ori = torch.full((5, 40), NAN), torch.full((5, 31), NAN)
    for t, lens, voiced in ((alt, alt_lens, alt_voiced), (ori, ori_lens, ori_voiced)):
        for b, (n, v) in enumerate(zip(lens, voiced)):
            row = np.zeros(n, dtype=np.float32)
            row[g.permutation(n)[:v]] = (80.0 + 400.0 * g.random(v)).astype(np.float32)
            if v == 1:
                row[:] = 0.0
                row[n // 2] = 220.0
            t[b, :n] = torch.from_numpy(row)
    return alt, alt_lens, ori, ori_lens, [0.0, 3.0, -2.5, 1.0, 12.0]
