"""Models and inputs shared by the tests of the live block step (test_host_rt_live.py, test_gpu_rt_live.py): the input gate of
`svc_rt_push_gated` and the output side of `svc_rt_out`.

`gate_decisions` is the float64 statement of the gate as include/seedvc_hip.h states it: per 20 ms frame the energy of the last
four frames, the three before a block carried from the block before (zeros before a stream's start), muted where that energy
is below the threshold.  `gate_audio` makes frames of constant magnitude with random signs, 0.1 ("loud") or 1e-4 ("quiet"): at
-40 dB a window is either all quiet, 10^4 below the threshold, or holds a loud frame, 25 times above it, so no decision is near
the threshold.

`out_session` is the output side step by step on the host: the segment resampled with the device's own FMA chain
(`rt_audio_cases.resample_fp32`) and with the float64 dense kernel (`resample_cases.resample_dense`), the float64 scores of the
latter against the buffer, and the splice (`realtime_cases.sola_model`) at the float64 offset."""
import numpy as np
import torch

import realtime_cases as RT
import resample_cases as RC
import rt_audio_cases as RA

LOUD, QUIET, GATE_DB = np.float32(0.1), np.float32(1e-4), -40.0
OUT_PAIRS = [(150, 250), (22050, 48000), (44100, 48000), (250, 250)]        # zc 3 -> 5, 441 -> 960, 882 -> 960, equal rates
GATE_PAIRS = [(250, 150), (22050, 16000), (48000, 16000)]
SLOTS, MAX_SLOTS = (4, 0, 2), 5
# frames that are loud, per stream, of the 6 m frames of six pushes.  Every pattern holds a loud frame followed by at least four
# quiet ones whose fourth lies in a later block than the loud frame (`pattern_crosses_a_block`)
LOUD_FRAMES = {1: ({0, 5}, {1}, {0}), 9: ({0, 7, 30}, {16, 17, 40}, {5, 26, 50})}
GAP = 1e-3                                                                   # the least float64 score gap of a case


# ---------------------------------------------------------------------------------------------------------------- the gate
def gate_power(db, zc):
    """The threshold on the energy of 4 zc samples as the host passes it: float32(4 zc 10^(dB / 10)); 0.0 at or below -60 dB."""
    return np.float32(0.0) if db is None or db <= -60.0 else np.float32(4.0 * zc * 10.0 ** (db / 10.0))


def frame_energies(x, zc):
    """x (m zc,) float32 -> float64 (m,): sum of squares per frame."""
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, zc)
    return (x * x).sum(1)


def gate_decisions(e, power, carry=(0.0, 0.0, 0.0)):
    """e (m,) frame energies of a block, carry: the three before it, oldest first -> (muted bool (m,), E float64 (m,), the new
    carry).  E_j = ((a + b) + c) + d over the four most recent frames ending at j; muted where E_j < power."""
    seq = np.concatenate([np.asarray(carry, np.float64), np.asarray(e, np.float64)])
    E = np.array([((seq[j] + seq[j + 1]) + seq[j + 2]) + seq[j + 3] for j in range(len(e))])
    return E < float(power), E, tuple(seq[-3:])


def gate_block(x, zc, power, carry):
    """One block through the float64 gate -> (x' float32 with its muted frames +0.0, muted bool (m,), the new carry)."""
    muted, _, carry = gate_decisions(frame_energies(x, zc), power, carry)
    y = np.asarray(x, np.float32).copy().reshape(-1, zc)
    y[muted] = 0.0
    return y.reshape(-1), muted, carry


def gate_audio(loud, frames, zc, seed):
    """frames * zc samples: frame f has magnitude LOUD where f is in `loud`, else QUIET; random signs."""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.random((frames, zc)) < 0.5, np.float32(-1), np.float32(1))
    mag = np.where(np.isin(np.arange(frames), sorted(loud)), LOUD, QUIET).astype(np.float32)
    return (sign * mag[:, None]).astype(np.float32).reshape(-1)


def pattern_crosses_a_block(loud, frames, m):
    """True where some loud frame f is followed by at least four quiet ones and frame f + 4, the first muted one, lies in a
    later block than f: the carried energies decide it."""
    return any(f + 4 < frames and not (set(range(f + 1, f + 5)) & set(loud)) and (f + 4) // m > f // m for f in loud)


def gate_margin(E, power):
    """The least ratio between a window energy and the threshold, on either side (>= 1)."""
    E = np.asarray(E, np.float64)
    return float(np.min(np.where(E < power, power / np.maximum(E, 1e-300), E / power)))


# ----------------------------------------------------------------------------------------------------------- the output side
def out_units(pair, Lb_units):
    """(zc_m, zc_o, geometry at the model rate, geometry at the output rate) for block 2, Lb, Ls 1 in 20 ms units."""
    from seedvc_amd.pipeline import realtime_output_geometry
    zc_m = pair[0] // 50
    gm = dict(block=2 * zc_m, Lb=Lb_units * zc_m, Ls=zc_m)
    go = realtime_output_geometry(gm, *pair)
    return zc_m, go["zc"], gm, go


def out_waves(pair, Lb_units, start, extra, steps=3):
    """The vocoder rows of `steps` steps of 3 streams: (steps, 3, start + n_in + extra) float32, NaN outside the segment; and the
    initial SOLA state (MAX_SLOTS, Lb_out) float32, noise in the rows of SLOTS and NaN elsewhere."""
    zc_m, zc_o, gm, go = out_units(pair, Lb_units)
    n_in = gm["block"] + gm["Lb"] + gm["Ls"]
    rng = np.random.default_rng(pair[0] + 31 * pair[1] + Lb_units)
    wave = np.full((steps, 3, start + n_in + extra), np.nan, np.float32)
    wave[:, :, start:start + n_in] = rng.uniform(-1, 1, (steps, 3, n_in)).astype(np.float32)
    state = np.full((MAX_SLOTS, go["Lb"]), np.nan, np.float32)
    state[list(SLOTS)] = rng.uniform(-1, 1, (3, go["Lb"])).astype(np.float32)
    return wave, state


def resample64(pair, x):
    x = np.asarray(x, np.float32)
    return x.astype(np.float64) if pair[0] == pair[1] else RC.resample_dense(*pair, torch.from_numpy(x)[None])[0].numpy()


def resample_bound(pair, x):
    x = np.asarray(x, np.float32)
    if pair[0] == pair[1]:
        return np.zeros(len(x))
    return RC.fp32_bound(*pair, torch.from_numpy(x)[None], RA.taps_of(*pair)[4].shape[1])[0].numpy()


def splice64(y64, buf, fade_in, fade_out, block, Ls):
    """The float64 splice: (out (block,), new buffer (Lb,), o*, scores, bound of the fade's three fp32 roundings per sample of
    out ‖ buffer)."""
    y64, b = np.asarray(y64, np.float64), np.asarray(buf, np.float32).astype(np.float64)
    Lb = len(b)
    scores = RT.sola_scores(y64, b, Ls)
    o = int(np.argmax(scores))
    y = y64[o:o + block + Lb].copy()
    p, q = y[:Lb] * fade_in.astype(np.float64), b * fade_out.astype(np.float64)
    y[:Lb] = p + q
    fade = np.zeros(block + Lb)
    fade[:Lb] = (np.abs(p) + np.abs(q)) * 2.0 ** -23 * 1.5
    return y[:block], y[block:block + Lb], o, scores, fade


def out_session(pair, Lb_units, wave, state, start, muted=()):
    """The host statement of `steps` calls of svc_rt_out for the 3 streams of `wave`, from `state`: per step and stream a dict of
    y32 (the device's resampled row, bit for bit), y64, bound (fp32_bound of the row), before / after (the SOLA buffer, float32,
    spliced at the float64 offset), out, o, scores.  muted: (step, stream) pairs whose row is +0.0."""
    zc_m, zc_o, gm, go = out_units(pair, Lb_units)
    n_in = gm["block"] + gm["Lb"] + gm["Ls"]
    fi, fo = RT.gui_windows(go["Lb"])
    bufs = [state[s].copy() for s in SLOTS]
    steps = []
    for t in range(wave.shape[0]):
        row = []
        for k in range(3):
            seg = wave[t, k, start:start + n_in]
            if (t, k) in muted:
                y32, y64, bound = np.zeros(go["n_inf"], np.float32), np.zeros(go["n_inf"]), np.zeros(go["n_inf"])
            else:
                y32, y64, bound = RA.resample_fp32(*pair, seg), resample64(pair, seg), resample_bound(pair, seg)
            assert len(y32) == len(y64) == go["n_inf"]
            _, _, o, scores, _ = splice64(y64, bufs[k], fi, fo, go["block"], go["Ls"])
            out, after, _, _ = RT.sola_model(y32, bufs[k], fi, fo, go["block"], go["Ls"], offset=o)
            row.append(dict(y32=y32, y64=y64, bound=bound, before=bufs[k], after=after, out=out, o=o, scores=scores))
            bufs[k] = after
        steps.append(row)
    return steps


# ------------------------------------------------------------------------------------------ the engine at an output rate
FAKE_OUT_PAIR = (200, 250)                   # zc 4 -> 5: realtime_cases.FAKE_GEOMETRY (block 44, Lb 16, Ls 12) -> 55, 20, 15


def fake_out_session(contents, muted=(), pair=FAKE_OUT_PAIR, g=RT.FAKE_GEOMETRY):
    """`realtime_cases.session_model` with the splice at the output rate: per step the fake chain's S * hop samples, the slice SOLA
    gets resampled with the device's own FMA chain (+0.0 everywhere for the steps in `muted`), `sola_model` with the output
    geometry and the GUI's windows from a zero buffer.  -> list of (out, buffer after, offset, scores, buffer before, infer)."""
    from seedvc_amd.pipeline import realtime_output_geometry
    S, hop, tail = g["S"], g["hop"], g["tail"]
    n_inf = g["block"] + g["sola_buffer"] + g["sola_search"]
    start = S * hop - tail - n_inf
    go = realtime_output_geometry(dict(block=g["block"], Lb=g["sola_buffer"], Ls=g["sola_search"]), *pair)
    fi, fo = RT.gui_windows(go["Lb"])
    buf, steps = np.zeros(go["Lb"], np.float32), []
    for t, c in enumerate(contents):
        seg = RT.fake_wave(c, S)[start:start + n_inf]
        infer = np.zeros(go["n_inf"], np.float32) if t in muted else RA.resample_fp32(*pair, seg)
        out, new, o, scores = RT.sola_model(infer, buf, fi, fo, go["block"], go["Ls"])
        steps.append((out, new, o, scores, buf, infer))
        buf = new
    return steps
