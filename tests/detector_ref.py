"""The spectral detector's reference (include/xrt.h): xrt_spectral_detector restated in
numpy, composed from the two references that are pinned already -- spectrum_ref's x_e chain with
libm's exp (oracle.exp) and noise_ref's Philox4x32-10, Poisson sampler and normal deviate.  Every f64
operation is rounded on its own (numpy cannot fuse).

    if open[i] != 0:  out[c][i] = -1 for every c
    else, in f64:
        acc[c] = 0
        for e in bins:
            x   = 0; for m in meshes: x = x + mu[m][e] * (d[m] * 0.1)
            lam = (weight[e] * exp(-x)) * gain
            N   = noisy ? poisson_from_word(lam, w_e) : lam
            for c: acc[c] = acc[c] + response[c][e] * N
        if read_noise > 0: for c: acc[c] = acc[c] + read_noise * normal_from_word(v_c)
        out[c][i] = counts ? (float)acc[c] : (float)(acc[c] / gain)

w_e is word e & 3 of Philox at the counter (lo32(g), hi32(g), e >> 2, 1), v_c word c & 3 at
(lo32(g), hi32(g), c >> 2, 2), g = first_index + i, under the key (lo32(seed), hi32(seed))."""
import numpy as np

import noise_ref
from oracle import oracle

F = np.float32
U64 = np.uint64
MASK = noise_ref.MASK


def stream_words(seed, first_index, n, count, stream):
    """(n, count) words: column k is word k & 3 of the counter (lo32(g), hi32(g), k >> 2, stream) of
    pixel g = first_index + its row."""
    seed = int(seed)
    g = np.arange(n, dtype=U64) + U64(int(first_index))
    cols = []
    for q in range((count + 3) // 4):
        cols += noise_ref.philox4x32_10(g & MASK, g >> U64(32), q, stream, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(cols[:count], axis=1)


def bin_means(paths, weights, mu, gain):
    """lam (n, K) f64 and the planes' shape: the mean count of every pixel and bin."""
    w = np.asarray(weights, F).reshape(-1)
    mu = np.asarray(mu, F).reshape(-1, w.size)
    p = np.ascontiguousarray(paths, F)
    assert p.shape[0] == mu.shape[0]
    d = p.reshape(mu.shape[0], -1)
    n = d.shape[1]
    lam = np.empty((n, w.size), np.float64)
    with np.errstate(all="ignore"):
        for e in range(w.size):
            x = np.zeros(n, np.float64)
            for m in range(mu.shape[0]):
                x = x + np.float64(mu[m, e]) * (d[m].astype(np.float64) * 0.1)
            lam[:, e] = (np.float64(w[e]) * oracle.exp(-x)) * np.float64(F(gain))
    return lam, p.shape[1:]


def spectral_detector(paths, open, weights, mu, response, gain=1.0, seed=0, noisy=True, counts=True,
                      read_noise=0.0, first_index=0):
    """xrt_spectral_detector: paths (M, ...) f32, open of a plane's shape or None, weights (K,), mu (M, K),
    response (C, K); (C, ...) f32."""
    lam, shape = bin_means(paths, weights, mu, gain)
    n, K = lam.shape
    r = np.asarray(response, F).reshape(-1, K)
    C = r.shape[0]
    acc = np.zeros((C, n), np.float64)
    with np.errstate(all="ignore"):
        if noisy:
            words = stream_words(seed, first_index, n, K, 1)
        for e in range(K):
            N = noise_ref.poisson_from_word(lam[:, e], words[:, e]) if noisy else lam[:, e]
            for c in range(C):
                acc[c] = acc[c] + np.float64(r[c, e]) * N
        if noisy and F(read_noise) > 0:
            v = stream_words(seed, first_index, n, C, 2)
            for c in range(C):
                acc[c] = acc[c] + np.float64(F(read_noise)) * noise_ref.normal_from_word(v[:, c])
        out = acc.astype(F) if counts else (acc / np.float64(F(gain))).astype(F)
    if open is not None:
        out[:, np.asarray(open).reshape(-1) != 0] = F(-1.0)
    return out.reshape((C,) + tuple(shape))


def same(got, want):
    """Bit for bit where the reference is no NaN, NaN for NaN elsewhere."""
    return got.shape == want.shape and noise_ref.same(got, want)
