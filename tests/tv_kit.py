"""Shared shapes and cases of the TV tests (test-only): the gradient's grids
-- the small ones and those about the kernel's tile --, the sum's lengths, the descent's
cases, and the noisy few-view ball scan with its figures.  References are computed once
per process and handed out read-only."""
import functools
import math
import os
import re

import numpy as np

import noise_ref
import sirt_kit
import tv_ref
from conftest import ROOT

F = np.float32
D = np.float64

# ------------------------------------------------------------------------------- the gradient
GRIDS = [(1, 1, 1), (2, 1, 1), (1, 1, 5), (5, 3, 2), (67, 9, 3), (130, 2, 2)]      # (nx, ny, nz)
EPSILONS = [1e-8, 1.0, 1e-300]


def tile_extent():
    """(own x, own y, chunk z) of k_tv_gradient, from the kernel's constants: a workgroup of kTvLanesX x kTvLanesY
    lanes owns one column and one row fewer (the rim) and marches kTvChunkZ slices."""
    with open(os.path.join(ROOT, "simpleraytracing_amd", "csrc", "kernels", "xrt_kernels.h")) as f:
        text = f.read()
    lanes = re.search(r"kTvLanesX = (\d+), kTvLanesY = (\d+);", text)
    chunk = re.search(r"kTvChunkZ = (\d+);", text)
    return int(lanes.group(1)) - 1, int(lanes.group(2)) - 1, int(chunk.group(1))


def tile_grids():
    """Grids one voxel below, at and above the tile's extent on each axis (the other axes small but more than one
    voxel, so that every neighbour exists somewhere), and one of two tiles and a chunk plus one on all axes at once."""
    ox, oy, cz = tile_extent()
    out = []
    for d in (-1, 0, 1):
        out += [(ox + d, 3, 2), (4, oy + d, 2), (3, 2, cz + d)]
    out.append((2 * ox + 1, 2 * oy + 1, cz + 1))
    return out


def volume(seed, dims, specials=False):
    return sirt_kit.volume(seed, dims, specials)


# ------------------------------------------------------------------------------- the sum of squares
SUMSQ_LENGTHS = [1, 255, 256, 257, 4095, 4096, 4097, 4096 * 3 + 5]
SUMSQ_LONG = (1 << 24) + 4097                               # three levels


@functools.lru_cache(maxsize=None)
def sumsq_vectors(n):
    rng = np.random.default_rng(n)
    a, b = rng.normal(0.0, 1.0, n).astype(F), rng.normal(0.0, 1.0, n).astype(F)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def sumsq_reference(n, with_b):
    a, b = sumsq_vectors(n)
    return float(tv_ref.sumsq(a, b if with_b else None))


def same_double(got, want):
    """Equal bit for bit, a NaN standing for any NaN."""
    got, want = np.float64(got), np.float64(want)
    return bool((np.isnan(got) and np.isnan(want)) or got.view(np.uint64) == want.view(np.uint64))


# ------------------------------------------------------------------------------- the descent
DESCEND_GRIDS = [(5, 3, 2), (67, 9, 3)]
DESCEND_STEPS, DESCEND_LENGTH, DESCEND_LO, DESCEND_HI = 3, 0.7, F(0.25), F(1.75)


def descend_volume(dims):
    """Values in [0, 2) between a slab of -1 (the lower four fifths of x on a narrow grid, the lowest eighth on a wide
    one) and, on a wide grid, a slab of 3 at the other end: the first step's clamp carries the slabs onto the bounds
    [0.25, 1.75], where a flat neighbourhood has no gradient; every step wears one layer off a slab, so after three
    steps its far side still lies on the bound, and the layers between have left it."""
    v = volume(11, dims).copy()
    nx = dims[0]
    if nx < 16:
        v[:, :, :nx - 1] = F(-1.0)
    else:
        v[:, :, :nx // 8] = F(-1.0)
        v[:, :, nx - nx // 8:] = F(3.0)
    return v


# ------------------------------------------------------------------------------- the solver's small scan
SMALL_TV = (4, 0.3, 0.9, 1e-6)


@functools.lru_cache(maxsize=None)
def small_reference(subsets):
    proj, A, spacing = sirt_kit.small_scan()
    out = tv_ref.sirt_tv(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, subsets, relax=0.9, lo=0.0, tv=SMALL_TV)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------- the noisy ball scan
NOISE_GAIN, NOISE_MU, NOISE_SEED = 500.0, 0.25, 20260
BALL_TV = (10, 0.2, 1.0, 1e-8)


@functools.lru_cache(maxsize=None)
def noisy_scan():
    """The 12-view ball scan's line integrals under photon noise: counts N = Poisson(500 exp(-0.25 p)) from the
    project's counter-based sampler (tests/noise_ref.py; libm's exp and log, one call a value, so that every machine
    gets the same planes), turned back into -ln(max(N, 1) / 500) / 0.25.  (proj (P, H, W) f32, matrices)."""
    proj, _, A = sirt_kit.ball_scan(sirt_kit.FEW_P)
    p = proj.astype(D)
    vals, inv = np.unique(p, return_inverse=True)
    image = np.array([math.exp(-NOISE_MU * float(v)) for v in vals], D)[inv].reshape(p.shape).astype(F)
    counts = noise_ref.photon_noise(image, NOISE_GAIN, NOISE_SEED, counts=True).astype(D)
    counts = np.where(counts >= 1.0, counts, 1.0)
    vals, inv = np.unique(counts, return_inverse=True)
    logs = np.array([math.log(float(v) / NOISE_GAIN) for v in vals], D)[inv].reshape(p.shape)
    noisy = (-logs / NOISE_MU).astype(F)
    noisy.setflags(write=False)
    return noisy, A


@functools.lru_cache(maxsize=None)
def noisy_reference(with_tv):
    """30 iterations of SIRT from zeros with lo = 0 over the noisy scan in the reference, plain or with BALL_TV."""
    proj, A = noisy_scan()
    out = tv_ref.sirt_tv(proj, A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING, sirt_kit.FEW_K, 1, 1.0, 0.0,
                         tv=BALL_TV if with_tv else None)
    out.setflags(write=False)
    return out


def noisy_figures(vol):
    """(the standard deviation over the voxels more than 1.5 voxels inside the ball, their mean, the RMS over the
    voxels more than 1.5 voxels outside it, the RMS against the voxelised ball)."""
    rr = np.linalg.norm(sirt_kit.ball_positions() - sirt_kit.BALL_CENTRE, axis=-1)
    margin = 1.5 * float(sirt_kit.BALL_SPACING)
    v = np.asarray(vol, D)
    inner, outer = v[rr < sirt_kit.BALL_RADIUS - margin], v[rr > sirt_kit.BALL_RADIUS + margin]
    rms = float(np.sqrt(np.mean((v - sirt_kit.ball_truth().astype(D)) ** 2)))
    return float(inner.std()), float(inner.mean()), float(np.sqrt(np.mean(outer ** 2))), rms
