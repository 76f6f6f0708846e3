"""Shared cases of the scatter model's tests (test-only): shapes, tables and inputs built
from a seed, with the hand-made special values planted, and their references, computed
once per process and handed out read-only."""
import functools

import numpy as np

import lsf_ref
import scatter_ref

F = np.float32

# (W, H, D): one pixel, odd sizes, whole tiles, a tile and a bit in both directions, the largest bin,
# a strip lower than a batch of rows, a detector smaller than one block
# -- and two more: several block rows inside one batch of 4 rows (D = 2), two block columns a tile (D = 32)
SHAPES = [(1, 1, 1), (7, 13, 4), (64, 64, 8), (67, 45, 16), (130, 70, 64), (200, 3, 2), (5, 5, 64), (70, 37, 2), (130, 70, 32)]
TABLES = [(1, 1), (3, 8), (16, 32)]                     # (M, K): each instantiation's bound and one below
STACKS = [1, 3]
KERNELS = [1, 4]
BINS = [1, 2, 4, 8, 16, 32, 64]


def tables(M, K, seed=0):
    """(weights (K,), mu (M, K), sigma (M, K)): sigma a share of mu, a zero here and there in both."""
    rng = np.random.default_rng(7000 + 100 * M + K + seed)
    w = (rng.uniform(0.5, 1.5, K) * 80.0 / K).astype(F)
    mu = rng.uniform(0.02, 0.6, (M, K)).astype(F)
    sg = (mu * rng.uniform(0.05, 0.9, (M, K))).astype(F)
    mu[rng.integers(0, M), rng.integers(0, K)] = 0.0
    sg[rng.integers(0, M), rng.integers(0, K)] = 0.0
    return w, mu, sg


def planes(M, P, H, W, seed=0, specials=True):
    """(paths (M, P, H, W) f32, open (P, H, W) u16): path lengths of 0..60 with misses (+0.0 in every mesh), a few
    flagged pixels and -- where the plane has room -- a NaN, an inf, a -0.0 and a negative length, each alone in
    its pixel and the same in every plane."""
    rng = np.random.default_rng(31 * W + 7 * H + 1000 * M + P + seed)
    p = rng.uniform(0.0, 60.0, (M, P, H, W)).astype(F)
    p[rng.random((M, P, H, W)) < 0.3] = 0.0
    p[:, rng.random((P, H, W)) < 0.2] = 0.0              # a miss
    o = np.zeros((P, H, W), np.uint16)
    o[rng.random((P, H, W)) < 0.05] = 1
    o[rng.random((P, H, W)) < 0.02] = 0x8000
    if specials:
        flat = p.reshape(M, P, H * W)
        of = o.reshape(P, H * W)
        for k, v in enumerate([np.nan, np.inf, -0.0, -7.5, -np.inf]):
            at = (5 * k + 2) % (H * W)
            if H * W > 5 * k + 2:
                flat[(k % M), :, at] = F(v)
                of[:, at] = 0
        if H * W > 40:
            flat[0, :, 33] = F(np.nan)                   # a NaN under a flag: the flag wins
            of[:, 33] = 2
    return p, o


@functools.lru_cache(maxsize=None)
def source_case(W, H, D, P, M, K):
    """(paths, open, weights, mu, sigma, reference source, reference lbuffer)."""
    w, mu, sg = tables(M, K)
    p, o = planes(M, P, H, W)
    src, lb = scatter_ref.source(p, o, w, mu, sg, D)
    for a in (p, o, src, lb):
        a.setflags(write=False)
    return p, o, w, mu, sg, src, lb


def coarse(G, P, Hc, Wc):
    """Blurred-looking coarse planes: positive values, a -0.0, a zero and a spike among them."""
    rng = np.random.default_rng(900 + 13 * Wc + Hc + G + P)
    b = rng.uniform(0.0, 30.0, (G, P, Hc, Wc)).astype(F)
    flat = b.reshape(-1)
    flat[1::17] = F(-0.0)
    flat[2::19] = F(0.0)
    flat[3::23] *= F(1e3)
    return b


def amps(G, seed=0):
    a = np.random.default_rng(50 + G + seed).uniform(0.0, 0.5, G).astype(F)
    if G > 1:
        a[1] = 0.0
    return a


@functools.lru_cache(maxsize=None)
def add_case(W, H, D, P, G):
    """(blurred, amp, primary, reference out, scatter, u8, and the same without a primary)."""
    Hc, Wc = scatter_ref.coarse_size(H, D), scatter_ref.coarse_size(W, D)
    b, a = coarse(G, P, Hc, Wc), amps(G)
    prim = lsf_ref.plane(W + 3 * H + D, W, H, P)
    with_p = scatter_ref.add(b, a, D, (P, H, W), prim)
    without = scatter_ref.add(b, a, D, (P, H, W), None)
    return b, a, prim, with_p, without


def check(got, want, what):
    ok, _ = scatter_ref.same(got, want)
    g, w = np.asarray(got).reshape(np.asarray(want).shape), np.asarray(want)
    assert ok, (what, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:8] if w.dtype == F else np.argwhere(g != w)[:8])
