"""Shared by the seeded-noise tests (test_host_seeded_noise.py, test_gpu_seeded_noise.py): a numpy restatement of the draw
layout DESIGN.md documents (float64 Box-Muller on the words of v2_chain_cases.philox4x32_10), an independent restatement
of `pipeline.derive_seed`, and the statistics the draws are held to.

Layout: key = (seed low word, seed high word), counter = (pos, row // 4, domain, 0), word row % 4 belongs to element
(row, pos); u = ((word >> 8) + 1) / 2^24; words (0, 1) give rows 4q, 4q + 1 = r cos(2 pi u1), r sin(2 pi u1) with
r = sqrt(-2 ln u0), words (2, 3) rows 4q + 2, 4q + 3; phase0 = (2 u - 1) pi."""
import numpy as np
import torch

import v2_chain_cases as V

DOMAIN_Z, DOMAIN_HIFT_NOISE, DOMAIN_HIFT_PHASE0 = 1, 2, 3
SEEDS = (1234, 2 ** 63 + 5)                 # the second has its high key word in use
STAT_SEEDS = (1234, 77)
MAX_ABS = float(np.sqrt(48 * np.log(2)))    # sqrt(-2 ln 2^-24)


def reference_uniforms(seed, domain, rows, n, pos0=0):
    """(rows, n) float64 uniforms in (0, 1] of positions pos0 .. pos0 + n - 1."""
    nq = (rows + 3) // 4
    ctr = np.zeros((nq, n, 4), dtype=np.uint64)
    ctr[..., 0] = (pos0 + np.arange(n))[None, :]
    ctr[..., 1] = np.arange(nq)[:, None]
    ctr[..., 2] = domain
    w = V.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))         # (nq, n, 4)
    w = np.transpose(w, (0, 2, 1)).reshape(nq * 4, n)[:rows]
    return ((w >> 8).astype(np.float64) + 1.0) / 2.0 ** 24


def reference_normals(seed, domain, rows, n):
    """(rows, n) float64 normals."""
    nq = (rows + 3) // 4
    u = reference_uniforms(seed, domain, nq * 4, n).reshape(nq, 4, n)
    out = np.empty((nq, 4, n))
    for p in (0, 1):
        r = np.sqrt(-2.0 * np.log(u[:, 2 * p]))
        out[:, 2 * p] = r * np.cos(2.0 * np.pi * u[:, 2 * p + 1])
        out[:, 2 * p + 1] = r * np.sin(2.0 * np.pi * u[:, 2 * p + 1])
    return out.reshape(nq * 4, n)[:rows]


def reference_phase0(seed, nh):
    """(nh,) float64: (2 u - 1) pi of domain 3, position 0."""
    return (2.0 * reference_uniforms(seed, DOMAIN_HIFT_PHASE0, nh, 1)[:, 0] - 1.0) * np.pi


def derive_seed_reference(seed, index):
    """splitmix64's output function on seed + (index + 1) * golden gamma, in numpy uint64 arithmetic (wraps mod 2^64)."""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + np.uint64(index + 1) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int(x ^ (x >> np.uint64(31)))


def ks_normal(x):
    """Kolmogorov-Smirnov statistic of the sample x against N(0, 1)."""
    x = np.sort(np.asarray(x, dtype=np.float64).reshape(-1))
    n = x.size
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(x / np.sqrt(2.0))).numpy())
    i = np.arange(1, n + 1)
    return float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()))


def lag1_corr(x):
    """Correlation of neighbours along pos, pooled over the rows of x (rows, n)."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.corrcoef(x[:, :-1].reshape(-1), x[:, 1:].reshape(-1))[0, 1])


def check_statistics(x, what):
    """The assertions of the issue on a (rows, n) sample: KS < the 0.1 % critical value, |lag-1 correlation| < 4.5 / sqrt(n),
    every value finite and inside the Box-Muller range."""
    n = x.size
    d, r = ks_normal(x), lag1_corr(x)
    print(f"{what}: KS {d:.4f} (critical {V.ks_critical(n):.4f}), mean {x.mean():+.4f}, var {x.var():.4f}, "
          f"lag-1 corr {r:+.4f} (bound {4.5 / np.sqrt(n):.4f}), max |x| {np.abs(x).max():.3f}")
    assert np.isfinite(x).all() and np.abs(x).max() <= MAX_ABS + 1e-5
    assert d < V.ks_critical(n)
    assert abs(r) < 4.5 / np.sqrt(n)
