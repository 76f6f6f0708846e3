"""Inputs of material decomposition's tests, shared by the CPU and the GPU suite: basis
tables that fall with energy at different rates (water-like, bone-like, a K-edge), responses of
disjoint windows, and channel planes made by the detector's own reference from crafted line
integrals, with the counts a solver must survive among them."""
import numpy as np

import detector_ref

F = np.float32
SIZES = [(1,), (63,), (64,), (65,), (257,), (7, 13)]
BASES = [1, 2, 3]
BINS = [1, 4, 5, 32]
FAR = {1: 120.0, 2: 60.0, 3: 30.0}                     # the planes' longest line integral by basis count


def channel_counts(B):
    """C in B, 4, 5, 8, from B on."""
    return sorted({c for c in (B, 4, 5, 8) if c >= B})


def table(B, K):
    """(weights (K,), mu (B, K)): a spectrum with a hump, coefficients per cm that fall with energy --
    slowly (water-like), fast (bone-like), and with an edge half way up (a contrast agent)."""
    e = (np.arange(K) + 0.5) / K                        # 0 .. 1 over the bins
    w = (40.0 * (0.3 + np.sin(np.pi * (0.1 + 0.8 * e)))).astype(F)
    rows = [0.35 - 0.17 * e, 1.9 * np.exp(-2.2 * e) + 0.25, np.where(e < 0.5, 0.9 - 0.8 * e, 2.4 - 1.6 * e)]
    return w, np.array(rows[:B], F)


def windows(C, K):
    """C disjoint 0/1 windows that cover the K bins (C <= K)."""
    assert C <= K
    r = np.zeros((C, K), F)
    r[np.arange(K) * C // K, np.arange(K)] = 1.0
    return r


def response(C, K, seed=0):
    """(C, K): disjoint windows where the bins allow them, otherwise rows of positive sensitivities."""
    if C <= K:
        return windows(C, K)
    rng = np.random.default_rng(31 * C + K + seed)
    return rng.uniform(0.2, 1.0, (C, K)).astype(F)


def paths(shape, B, seed=0, far=None):
    """(B, *shape) f32 line integrals up to FAR[B], about a quarter of them +0.0."""
    far = FAR[B] if far is None else far
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed + 1000 * B + n)
    d = (rng.uniform(0.0, far, (B, n)) * (rng.random((B, n)) < 0.75)).astype(F)
    return d.reshape((B,) + tuple(shape))


def planes(shape, B, C, K, gain=1.0, counts=True, seed=0, far=None):
    """(channels (C, *shape) f32, open uint16, the line integrals they were made from): the detector
    reference's expected channels, then -- where the plane has room -- a count of zero, a negative one, one
    twice too large, and every 11th pixel masked."""
    d = paths(shape, B, seed, far)
    w, mu = table(B, K)
    ch = detector_ref.spectral_detector(d, None, w, mu, response(C, K), gain, 0, False, counts).copy()
    flat = ch.reshape(C, -1)
    n = flat.shape[1]
    if n > 8:
        flat[0, 2] = 0.0
        flat[C - 1, 4] = -3.0
        flat[:, 7] *= 2.0
    opn = np.zeros(n, np.uint16)
    opn[5::11] = 1 << (np.arange(len(opn[5::11])) % 16)
    return ch, opn.reshape(shape), d


def thick_among_thin(B, n=192, thin=0.5, thick=250.0):
    """(B, n) line integrals of `thin`, with one pixel of `thick` in basis 0 in the second wave (pixel 70):
    from zeros that lane needs many more iterations than its 63 neighbours."""
    d = np.full((B, n), thin, F)
    d[0, 70] = thick
    return d


# ------------------------------------------------------------------------------- the round trip
ROUND_TRIP_SIZE = (67, 45)                              # (W, H)
ROUND_TRIP_K = 8
ROUND_TRIP_WINDOWS = [2, 4]


def round_trip_tables(C):
    """(weights, mu (2, 8), response): two basis materials under C disjoint windows of the K = 8 bins."""
    w, mu = table(2, ROUND_TRIP_K)
    return w, mu, windows(C, ROUND_TRIP_K)


def round_trip_ulps(got, want, keep):
    """The largest difference over the kept pixels, in f32 ulps of the largest traced path."""
    top = float(np.max(want))
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))[:, keep])) / float(np.spacing(F(top)))


# ------------------------------------------------------------------------------- the small reconstruction
RECON_P, RECON_W, RECON_H, RECON_PITCH = 24, 32, 32, 0.8
RECON_DIMS = (16, 16, 16)
RECON_SPACING = F(1.0)
RECON_ORIGIN = np.array([-8.0, -8.0, -8.0], F)
RECON_AXIS_POINT = np.zeros(3, F)
RECON_BALLS = [((2.0, -1.0, 0.5), 4.0), ((-2.5, 2.0, -1.0), 2.0)]     # basis 0 (water-like), basis 1 (bone-like)


def recon_scan():
    """(paths (2, P, H, W) f32, cameras (13 f32 each)): 24 views of two balls, one per basis material, the
    source turning about the z axis -- each ball's chord lengths are its material's paths plane."""
    import fdk_kit
    import fdk_ref
    cams = [fdk_ref.turntable_camera(2.0 * np.pi * p / RECON_P, fdk_kit.SOD, fdk_kit.SDD, RECON_PITCH) for p in range(RECON_P)]
    planes = np.stack([np.stack([fdk_ref.ball_projection(c, RECON_W, RECON_H, centre, radius) for c in cams])
                       for centre, radius in RECON_BALLS])
    return planes, cams
