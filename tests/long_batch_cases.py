"""Models and stand-ins shared by the long-form batch tests (test_host_long_batch.py, test_gpu_long_batch.py).

`gather_model` and `assemble_model` are the numpy statements of the two formulas in include/seedvc_hip.h
(`svc_chunks_gather_cond`, `svc_chunks_assemble`); the host test pins `assemble_model` to the reference-generated fixtures of
tests/golden/chunkloop.npz, so the GPU tests' yardstick is the reference's own loop.  `BatchedFakeCFM` / `fake_vocoder_*` are
`cases.fake_sampler` / `cases.fake_vocoder` for any batch size: the same single fp32 multiplies and adds per element,
exactly rounded on every device.  `MelMixCFM` is the exact stand-in sampler of the HiFT test."""
import numpy as np
import torch

import cases


def fades(ov):
    """(fade_in, fade_out) of `crossfade` (inference.py:343-350), float64."""
    return np.cos(np.linspace(np.pi / 2, 0, ov)) ** 2, np.cos(np.linspace(0, np.pi / 2, ov)) ** 2


def gather_model(prompt_cond, prompt_lens, cond, utt, row0, rows, T):
    """mu[k][t] = t < P_u ? prompt_cond[u][t] : t < P_u + rows[k] ? cond[row0[k] + t - P_u] : 0, u = utt[k]."""
    mu = np.zeros((len(utt), T, cond.shape[1]), np.float32)
    for k, u in enumerate(utt):
        P = prompt_lens[u]
        mu[k, :P] = prompt_cond[u, :P]
        mu[k, P:P + rows[k]] = cond[row0[k]:row0[k] + rows[k]]
    return mu


def assemble_model(waves, lens, first, last, ov):
    """waves (N, stride) float32, padded with anything past lens[k] -> the utterances' samples, one after the other."""
    fi, fo = fades(ov)
    out = []
    for k in range(len(lens)):
        body = lens[k] - (0 if last[k] else ov)
        v = waves[k, :body].astype(np.float64)
        if not first[k]:
            n = min(body, ov)
            v[:n] = v[:n] * fi[:n] + waves[k - 1, lens[k - 1] - ov:lens[k - 1] - ov + n].astype(np.float64) * fo[:n]
        out.append(v.astype(np.float32))
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def padded_rows(waves, stride, fill=float("nan")):
    """list of 1-D float32 arrays -> (N, stride) with `fill` past each row's length."""
    W = np.full((len(waves), stride), fill, np.float32)
    for k, w in enumerate(waves):
        W[k, :len(w)] = w
    return W


def chunkstream_rows(name):
    """(waves, lens, first, last) of a `chunkstream` case: the chunks of one utterance."""
    waves, frames = cases.chunkstream_case(name)
    waves = [w.reshape(-1).numpy() for w in waves]
    n = len(waves)
    return waves, [f * cases.CHUNK_HOP for f in frames], [k == 0 for k in range(n)], [k == n - 1 for k in range(n)]


def chunkloop_rows(name):
    """The same for a `chunkloop` case: the fake sampler and vocoder run chunk by chunk over `chunk_plan`'s windows."""
    from seedvc_amd.pipeline import chunk_plan
    c = cases.chunkloop_case(name)
    P = cases.CHUNK_P
    plan = chunk_plan(c["cond"].size(1), cases.CHUNK_WINDOW - P, cases.CHUNK_OVERLAP)
    waves = []
    for p0, s, _ in plan:
        mel = cases.fake_sampler(torch.cat([c["prompt_condition"], c["cond"][:, p0:p0 + s]], dim=1), P)[:, :, P:]
        waves.append(cases.fake_vocoder(mel).reshape(-1).numpy())
    n = len(plan)
    return waves, [s * cases.CHUNK_HOP for _, s, _ in plan], [k == 0 for k in range(n)], [k == n - 1 for k in range(n)]


class BatchedFakeCFM:
    """`cases.fake_sampler` behind the HIP sampler's call signature, any B: row b of the result is
    fake_sampler(mu[b:b+1]) (frames at and above x_lens[b] come from the zero rows of mu)."""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.batch_sizes = []

    def inference(self, mu, x_lens, prompt, style, f0, n, inference_cfg_rate=0.7, z=None, prompt_lens=None, **kw):
        self.batch_sizes.append(mu.size(0))
        m = mu.float().transpose(1, 2)                                       # (B, Dc, T)
        rows = [m[:, c] * 0.5 + m[:, c + 1] * float(c + 1) * 0.25 for c in range(cases.CHUNK_C)]
        return torch.stack(rows, dim=1).contiguous()


def _fake_wave(mel):
    j = (torch.arange(cases.CHUNK_HOP, dtype=torch.float32, device=mel.device) + 1.0) * 0.125
    w = mel[:, 0][:, :, None] * j[None, None, :] + mel[:, 1][:, :, None]
    return w.reshape(mel.size(0), 1, -1).contiguous()


class FakeVocoder:
    """`cases.fake_vocoder` for any B.  With `ragged` the call takes `lens=` like `BigVGAN.__call__`: samples at and above
    lens[b] * hop are zero.  `calls` records (B, S, lens) of every call."""

    def __init__(self, ragged):
        self.ragged = ragged
        self.calls = []

    def __call__(self, mel, **kw):
        lens = kw.pop("lens", None)
        assert not kw, kw
        assert lens is None or self.ragged, "this vocoder has no ragged call"
        self.calls.append((mel.size(0), mel.size(2), None if lens is None else list(lens)))
        w = _fake_wave(mel)
        if lens is not None:
            keep = torch.arange(w.size(2), device=w.device)[None, None, :] < (torch.tensor(lens, device=w.device) * cases.CHUNK_HOP)[:, None, None]
            w = torch.where(keep, w, torch.zeros_like(w))
        return w


class MelMixCFM:
    """Exact stand-in sampler for a vocoder with `n_mels` input channels: channel c of frame t is
    clamp(mu[t, c % Dc] * 1.5 + mu[t, (c + 1) % Dc] * 0.5 - 4, -11.5, 2), single fp32 operations per element.  Rows and
    frames are independent, so a batched call and B = 1 calls return identical mels."""

    def __init__(self, n_mels, device="cuda:0"):
        self.n_mels, self.device = n_mels, torch.device(device)

    def inference(self, mu, x_lens, prompt, style, f0, n, inference_cfg_rate=0.7, z=None, prompt_lens=None, **kw):
        m = mu.float().transpose(1, 2)                                       # (B, Dc, T)
        c = torch.arange(self.n_mels, device=mu.device)
        a, b = m[:, c % m.size(1)], m[:, (c + 1) % m.size(1)]
        return (a * 1.5 + b * 0.5 - 4.0).clamp(-11.5, 2.0).contiguous()
