"""Inputs of the spectral detector's tests, shared by the CPU and the GPU suite: crafted
path planes with the wave shapes the kernel treats apart, tables, responses, and the gains that put a
wave's means on one side of the sampler's threshold of 64, on both, or near 0."""
import numpy as np

import detector_ref
import noise_ref

F = np.float32
SIZES = [(1,), (63,), (64,), (65,), (257,), (7, 13)]
BINS = [1, 3, 4, 5, 8, 32]
MESHES = [1, 3, 16]
CHANNELS = [1, 2, 3, 8]
FIRST = [0, 1, 2 ** 32 - 3, 2 ** 40 + 5]
SEEDS = [0, 1, 2 ** 63 + 12345]
FAR = {1: 2.0, 3: 2.0, 16: 0.4}                         # planes' longest path by mesh count: the sums stay alike


def table(M, K, seed=0):
    """(weights (K,), mu (M, K)): weights that alternate between small and large along the bins, so that a
    quad holds means on both sides of 64 under one gain; coefficients from 0 to 0.6, a zero among them."""
    rng = np.random.default_rng(100 * M + K + seed)
    w = (rng.uniform(0.5, 1.5, K) * np.where(np.arange(K) % 2 == 0, 1.0, 40.0)).astype(F)
    mu = rng.uniform(0.0, 0.6, (M, K)).astype(F)
    mu[rng.integers(0, M), rng.integers(0, K)] = 0.0
    return w, mu


def response(C, K, seed=0):
    """(C, K) responses: bin energies from 10 to 120, a zero here and there, the last row all zeros when
    there are at least three."""
    rng = np.random.default_rng(7 * C + K + seed)
    r = rng.uniform(10.0, 120.0, (C, K)).astype(F)
    r[rng.random((C, K)) < 0.2] = 0.0
    if C >= 3:
        r[-1] = 0.0
    return r


def windows(C, K):
    """C disjoint 0/1 windows that cover the K bins (C <= K)."""
    r = np.zeros((C, K), F)
    r[np.arange(K) * C // K, np.arange(K)] = 1.0
    return r


def planes(shape, M, seed=0, far=2.0):
    """(paths (M, *shape) f32, open shape uint16): path lengths up to `far`, about a third of them +0.0, a
    -0.0 and a negative one among them; every 11th pixel flagged."""
    rng = np.random.default_rng(seed + 1000 * M + int(np.prod(shape)))
    n = int(np.prod(shape))
    d = (rng.uniform(0.0, far, (M, n)) * (rng.random((M, n)) < 0.67)).astype(F)
    if n > 4:
        d[0, 1] = F(-0.0)
        d[M - 1, 3] = F(-0.25)
    opn = np.zeros(n, np.uint16)
    opn[5::11] = 1 << (np.arange(len(opn[5::11])) % 16)
    return d.reshape((M,) + tuple(shape)), opn.reshape(shape)


def gains(weights, mu, far=2.0):
    """{'small', 'large', 'mixed', 'dark'}: gains under which every mean of planes(..., far) lies below 64,
    every mean from 64 up, both kinds within each quad of bins (the table's alternating weights), and every
    mean near 0.  The least transmission is exp(-sum_m mu * far * 0.1) over the worst bin."""
    w = np.asarray(weights, np.float64)
    t_min = float(np.exp(-(np.asarray(mu, np.float64) * far * 0.1).sum(0).max())) * 0.999
    out = {"small": 60.0 / w.max(), "large": 70.0 / (w.min() * t_min), "dark": 1e-3 / w.max()}
    if w.size > 1:
        lo, hi = w[0::2].max(), w[1::2].min()
        assert hi * t_min > 4 * lo
        out["mixed"] = 60.0 / lo
        assert out["mixed"] * hi * t_min >= 64.0
    return {k: float(F(v)) for k, v in out.items()}


def mean_classes(paths, opn, weights, mu, gain):
    """(any mean below 64, any mean from 64 up) over the unflagged pixels."""
    lam, _ = detector_ref.bin_means(paths, weights, mu, gain)
    lam = lam[np.asarray(opn).reshape(-1) == 0]
    return bool((lam < noise_ref.SMALL).any()), bool((lam >= noise_ref.SMALL).any())


def wave_shapes(M, K):
    """{name: (paths (M, n), open (n,) or None)} over n = 192 pixels, three waves each: the shapes the
    kernel treats apart."""
    n = 192
    zeros = np.zeros((M, n), F)
    one = zeros.copy()
    one[M - 1, 70] = F(1.5)                               # a wave of zeros but for one lane, of the last mesh
    flagged = np.zeros(n, np.uint16)
    flagged[130] = 4                                      # a flagged lane in a wave of zeros
    neg = np.full((M, n), F(-0.0))
    far = zeros.copy()
    far[0] = np.linspace(0.0, 4e4, n).astype(F)           # exponents past 512 and 1024: exp's special cases
    nan = planes((n,), M, 5)[0].copy()
    nan[0, 64] = np.nan
    inf = planes((n,), M, 6)[0].copy()
    inf[0, 3], inf[M - 1, 66], inf[0, 130], inf[M - 1, 130] = np.inf, -np.inf, np.inf, -np.inf
    return {"infinite": (inf, None), "misses": (zeros, None), "one lane": (one, None), "flagged lane": (zeros, flagged),
            "minus zero": (neg, None), "far": (far, None), "nan": (nan, np.zeros(n, np.uint16))}
