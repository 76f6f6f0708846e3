"""Shared shapes and cases of the OS-MLTR tests (test-only): the
pixel stage's and the fused backprojector's cases over sirt_kit's and fdk_kit's
shapes, the small scans of the bit-for-bit solver tests and the two ball scans
that show what the solver is for, with their bounds.  References are computed
once per process and handed out read-only."""
import functools

import numpy as np

import fdk_kit
import mltr_ref
import noise_ref
import sirt_kit
import sirt_ref

F = np.float32
D = np.float64


def same(got, want, what):
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    if not fdk_kit.same_bits(got, want):
        bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError((what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------- the pixel stage
def counts(seed, P, H, W, specials=False):
    """Measured counts: whole numbers about 60, with 0, NaN and +inf among them when asked."""
    y = np.random.default_rng(seed).poisson(60.0, (P, H, W)).astype(F)
    if specials:
        flat = y.reshape(-1)
        for n, v in enumerate([0.0, np.nan, np.inf]):
            flat[(n * 3 + 1) % flat.size::7] = F(v)
    return y


def flat_field(seed, H, W, specials=False):
    f = np.random.default_rng(seed + 50).uniform(80.0, 120.0, (H, W)).astype(F)
    if specials:
        flat = f.reshape(-1)
        for n, v in enumerate([0.0, np.nan]):
            flat[(n * 2 + 2) % flat.size::11] = F(v)
    return f


def background(seed, P, H, W):
    return np.random.default_rng(seed + 70).uniform(0.5, 8.0, (P, H, W)).astype(F)


def pixel_cases():
    """name -> a function building (volume, spacing, R, counts, flat, background or None): every grid of
    sirt_kit.FP_DIMS on every detector of sirt_kit.FP_PLANES with stacks of 1, 3 and 17 planes in turn (special voxels,
    counts and flat fields on the 67 x 45 detector), the hand-built rays, and expectations that underflow."""
    cases = {}

    def general(dims, n, W, H):
        def build():
            P = sirt_kit.FP_STACKS[n % len(sirt_kit.FP_STACKS)] if (W, H) != (67, 45) else 3
            sp = (W, H) == (67, 45)
            R, spacing = sirt_kit.general_rays(P, dims, W, H, seed=P)
            return (sirt_kit.volume(W + H, dims, specials=sp), spacing, R, counts(W, P, H, W, sp), flat_field(H, H, W, sp),
                    background(W, P, H, W) if n % 2 else None)
        return build

    for dims in sirt_kit.FP_DIMS:
        for n, (W, H) in enumerate(sirt_kit.FP_PLANES):
            cases[f"grid{dims}-plane{(W, H)}"] = general(dims, n, W, H)

    def stack(P):
        def build():
            dims, (W, H) = (67, 9, 3), (7, 13)
            R, spacing = sirt_kit.general_rays(P, dims, W, H, seed=1)
            return sirt_kit.volume(3, dims), spacing, R, counts(P, P, H, W, True), flat_field(P, H, W), background(P, P, H, W)
        return build

    for P in sirt_kit.FP_STACKS:
        cases[f"stack{P}"] = stack(P)

    def hand(name, specials, with_bg):
        def build():
            R, (H, W) = sirt_kit.hand_rays()[name]
            return (sirt_kit.volume(9, sirt_kit.HAND_DIMS, specials), sirt_kit.HAND_SPACING, R.reshape(1, 12),
                    counts(4, 1, H, W, specials), flat_field(4, H, W, specials), background(4, 1, H, W) if with_bg else None)
        return build

    for name in sirt_kit.hand_rays():
        for specials in (False, True):
            cases[f"hand-{name}-{'specials' if specials else 'plain'}"] = hand(name, specials, specials)

    def dark(with_bg):
        def build():
            dims, (W, H), P = (67, 9, 3), (7, 13), 3
            R, spacing = sirt_kit.general_rays(P, dims, W, H, seed=1)
            vol = (sirt_kit.volume(3, dims) * F(1e4) + F(1e4)).astype(F)        # line integrals far beyond 745: psi = 0
            return vol, spacing, R, counts(8, P, H, W), flat_field(8, H, W), background(8, P, H, W) if with_bg else None
        return build

    cases["underflow-no-background"] = dark(False)
    cases["underflow-background"] = dark(True)
    return cases


PIXEL_CASES = pixel_cases()


@functools.lru_cache(maxsize=None)
def pixel_case(name):
    """(volume, spacing, R, counts, flat, background, the reference's pairs)."""
    vol, spacing, R, y, f, b = PIXEL_CASES[name]()
    want = mltr_ref.poisson_project(vol, spacing, R, y, f, b)
    return _frozen(vol, spacing, R, y, f, b, want)


# ------------------------------------------------------------------------------- the fused backprojector
UPDATE_DIMS = fdk_kit.BP_DIMS + [(300, 2, 2)]               # the last: wider than a wave's span of the row
UPDATE_LO, UPDATE_HI = F(0.0), F(1.5)


def pairs(seed, P, H, W, nan_plane=None):
    """(P, H, W, 2): num from fdk_kit.projections (a plane of NaN when asked), den positive with negative values,
    zeros and +inf among them."""
    num = fdk_kit.projections(seed, P, H, W, nan_plane=nan_plane)
    den = np.random.default_rng(seed + 31).uniform(0.5, 3.0, (P, H, W)).astype(F)
    flat = den.reshape(-1)
    for n, v in enumerate([-1.0, 0.0, np.inf]):
        if flat.size > 8:
            flat[(n * 3 + 2) % flat.size::19] = F(v)
    return np.ascontiguousarray(np.stack([num, den], -1))


def update_cases():
    """name -> a function building (pairs, matrices, dims, start, relax, lo, hi)."""
    cases = {}

    def general(dims, n, W, H):
        def build():
            P = fdk_kit.BP_STACKS[n % len(fdk_kit.BP_STACKS)]
            A = fdk_kit.general_matrices(P, dims, W, H, seed=n)
            return (pairs(W + n, P, H, W, nan_plane=0 if (n == 2 and P > 1) else None), A, dims,
                    sirt_kit.volume(H, dims, specials=True), 0.9 if n % 2 else 1.0,
                    UPDATE_LO if n % 2 else F(-np.inf), UPDATE_HI if n % 2 else F(np.inf))
        return build

    for dims in UPDATE_DIMS:
        for n, (W, H) in enumerate(fdk_kit.BP_PLANES):
            cases[f"grid{dims}-plane{(W, H)}"] = general(dims, n, W, H)

    def stack(P):
        def build():
            dims, (W, H) = (67, 9, 3), (7, 13)
            return (pairs(P, P, H, W, nan_plane=P // 2 if P > 1 else None), fdk_kit.general_matrices(P, dims, W, H, seed=1),
                    dims, sirt_kit.volume(2, dims, specials=True), 0.7, UPDATE_LO, UPDATE_HI)
        return build

    for P in fdk_kit.BP_STACKS:
        cases[f"stack{P}"] = stack(P)

    def edge(W, H):
        def build():
            A, dims = fdk_kit.edge_matrices(W, H)
            return pairs(W, 3, H, W), A, dims, sirt_kit.volume(W, dims, specials=True), 1.0, UPDATE_LO, UPDATE_HI
        return build

    for (W, H) in fdk_kit.BP_PLANES:
        cases[f"edge{(W, H)}"] = edge(W, H)

    def landing():
        # edge_matrices' first matrix alone: voxel (i, j, 0) lands exactly on pixel (j - 1, i - 1) with w = 1, so its
        # sums are that pixel's pair; x = 0.25, den = 1 and num = bound - 0.25 land exactly on the bound, the
        # neighbours beyond it.
        W, H = 7, 13
        A, dims = fdk_kit.edge_matrices(W, H)
        pr = np.zeros((1, H, W, 2), F)
        pr[..., 1] = 1.0
        pr[0, :, :, 0] = np.tile(np.array([UPDATE_LO - F(0.25), UPDATE_HI - F(0.25), -1.0, 2.0, 0.0, 0.5, -0.25], F), (H, 1))
        return pr, A[:1], dims, np.full(dims[::-1], 0.25, F), 1.0, UPDATE_LO, UPDATE_HI

    cases["landing"] = landing
    return cases


UPDATE_CASES = update_cases()


@functools.lru_cache(maxsize=None)
def update_case(name):
    """(pairs, matrices, dims, start, relax, lo, hi, the reference's volume)."""
    pr, A, dims, start, relax, lo, hi = UPDATE_CASES[name]()
    want = mltr_ref.backproject_update(pr, A, dims, start, relax, lo, hi)
    _frozen(pr, A, start, want)
    return pr, A, tuple(dims), start, relax, lo, hi, want


# ------------------------------------------------------------------------------- the small scans
SMALL_FLAT = 200.0
SMALL_BG = 6.0
SMALL_K, SMALL_RELAX = 3, 0.9
SMALL_TV = (2, 0.2, 0.9, 1e-8)
LARGE_P, LARGE_W, LARGE_H, LARGE_DIMS = 6, 24, 20, (12, 11, 10)


def _noisy(proj, flat, bg, seed):
    """Counts by the project's sampler over flat * exp(-proj) + bg."""
    mean = (D(flat) * np.exp(-proj.astype(D)) + D(bg)).astype(F)
    return noise_ref.photon_noise(mean, 1.0, seed, counts=True)


@functools.lru_cache(maxsize=None)
def small_scan(with_bg=False):
    """sirt_kit's small scan as counts: (counts, flat (H, W), background or None, A, spacing)."""
    proj, A, spacing = sirt_kit.small_scan()
    flat = np.full(proj.shape[1:], SMALL_FLAT, F)
    bg = np.full(proj.shape, SMALL_BG, F) if with_bg else None
    y = _noisy(proj, SMALL_FLAT, SMALL_BG if with_bg else 0.0, 11)
    return _frozen(y, flat, bg, A, spacing)


@functools.lru_cache(maxsize=None)
def large_scan():
    """A scan larger than the small one in every size, with a background: (counts, flat, background, A, spacing, dims)."""
    A = fdk_kit.general_matrices(LARGE_P, LARGE_DIMS, LARGE_W, LARGE_H, seed=3)
    spacing = fdk_kit.grid_for(LARGE_DIMS, LARGE_W, LARGE_H, 0.4)[1]
    R = np.stack([sirt_ref.ray_matrix(a).reshape(12) for a in A])
    proj = sirt_ref.forward_project(sirt_kit.volume(22, LARGE_DIMS), spacing, R, (LARGE_H, LARGE_W))
    flat = flat_field(3, LARGE_H, LARGE_W) * F(2.0)
    bg = background(3, LARGE_P, LARGE_H, LARGE_W)
    y = noise_ref.photon_noise((flat.astype(D)[None] * np.exp(-proj.astype(D)) + bg).astype(F), 1.0, 12, counts=True)
    return _frozen(y, flat, bg, A, spacing) + (LARGE_DIMS,)


@functools.lru_cache(maxsize=None)
def small_reference(subsets, with_bg=False, tv=None):
    y, flat, bg, A, spacing = small_scan(with_bg)
    out = mltr_ref.mltr(y, flat, A, sirt_kit.SMALL_DIMS, spacing, SMALL_K, subsets, SMALL_RELAX, 0.0, tv=tv, background=bg)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def large_reference():
    y, flat, bg, A, spacing, dims = large_scan()
    out = mltr_ref.mltr(y, flat, A, dims, spacing, 2, 2, 1.0, 0.0, background=bg)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------- what it is for: the ball scans
BALL_S = 8
STARVED_FLAT, STARVED_K = 100.0, 4
BG_FLAT, BG_LEVEL, BG_K = 1000.0, 20.0, 3


@functools.lru_cache(maxsize=None)
def starved_scan():
    """sirt_kit's ball under a flat field of 100 counts: (counts, A)."""
    proj, _, A = sirt_kit.ball_scan(sirt_kit.BALL_P)
    return _frozen(_noisy(proj, STARVED_FLAT, 0.0, 21)) + (A,)


@functools.lru_cache(maxsize=None)
def background_scan():
    """sirt_kit's ball under a flat field of 1000 counts over a constant background of 20: (counts, A)."""
    proj, _, A = sirt_kit.ball_scan(sirt_kit.BALL_P)
    return _frozen(_noisy(proj, BG_FLAT, BG_LEVEL, 22)) + (A,)


@functools.lru_cache(maxsize=None)
def starved_reference():
    y, A = starved_scan()
    out = mltr_ref.mltr(y, STARVED_FLAT, A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING, STARVED_K, BALL_S, 1.0, 0.0)
    out.setflags(write=False)
    return out


def starved_line_integrals():
    """What SIRT is given: xrt_log_projection of the same counts, clamped at t_min = 0.5 / flat (the host
    restatement, which the GPU entry equals bit for bit)."""
    import simpleraytracing_amd as xrt
    y, _ = starved_scan()
    return xrt.host_log_projection(y, flat_value=STARVED_FLAT, t_min=0.5 / STARVED_FLAT)


@functools.lru_cache(maxsize=None)
def background_reference(modelled):
    y, A = background_scan()
    out = mltr_ref.mltr(y, BG_FLAT, A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING, BG_K, BALL_S, 1.0, 0.0,
                        background=BG_LEVEL if modelled else None)
    out.setflags(write=False)
    return out
