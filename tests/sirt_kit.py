"""Shared shapes and cases of the SIRT tests (test-only): the
forward projector's grids, detectors and hand-built ray matrices, the update's
vectors, the small scan of the bit-for-bit solver tests and the ball scans with
their bounds.  References are computed once per process and handed out
read-only."""
import functools

import numpy as np

import camera_kit
import fdk_kit
import fdk_ref
import sirt_ref

F = np.float32
D = np.float64

# ------------------------------------------------------------------------------- the forward projector
FP_DIMS = fdk_kit.BP_DIMS                                  # (nx, ny, nz)
FP_PLANES = fdk_kit.BP_PLANES                              # (W, H)
FP_STACKS = [1, 3, 17]


def volume(seed, dims, specials=False):
    """A (nz, ny, nx) f32 volume; specials: NaN, +-inf and -0.0 among the voxels."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, 2.0, dims[::-1]).astype(F)
    if specials and v.size >= 30:                      # (a grid of a few voxels stays plain: nothing else would be left)
        flat = v.reshape(-1)
        for n, s in enumerate([np.nan, np.inf, -np.inf, -0.0]):
            flat[(n * 5 + 1) % flat.size::13] = F(s)
    return v


def general_rays(P, dims, W, H, seed=0):
    """(R (P, 12), spacing): the library's ray matrices of fdk_kit.general_matrices' cameras over its grid."""
    import simpleraytracing_amd as xrt
    A = fdk_kit.general_matrices(P, dims, W, H, seed=seed)
    return np.stack([xrt.ray_matrix(a).reshape(12) for a in A]), fdk_kit.grid_for(dims, W, H, 0.4)[1]


def measured(seed, P, H, W):
    return np.random.default_rng(seed).uniform(0.0, 40.0, (P, H, W)).astype(F)


def hand_rays():
    """Hand-built ray matrices over the grid (5, 3, 2): name -> (R (12,), (H, W)).
    faces: a source at (-3, 0.5, 0.5), on the planes between voxels, d = (1, 0.4 (row - 1), (col - 1) / 8): the
      central ray runs inside two faces at once (two zero components), its neighbours inside one; row 2 enters
      through the edge x = -0.5, y = 1.5 (a tie between the axes), row 0 only touches the corner y = -0.5 (te = tx:
      a miss).
    boundary: the source on x = -0.5 exactly with d_x = 0 (O >= plane(0): inside) for col = 1, and d_x != 0 beside it.
    far_side: the source on y = 2.5 = plane(ny) exactly with d_y = 0: outside (O < plane(n) fails), a miss.
    inside: a source inside the grid, rays in every direction.
    misses: a source outside; col = 2 looks at the grid (row 3 passes it by), col = 0 points away from it (t > 0
      only), col = 1 has d_x = 0 outside the x slab.
    tiny: directions of 1e-170: ell's squares underflow to zero, so L = 0 on rays that hit.
    still: d = (0, 0, 0) at pixel (0, 0) from a source inside: ell = 0 and an infinite span, L is NaN."""
    return {
        "faces": (np.array([0, 0, 1, -3, 0, 0.4, -0.4, 0.5, 0.125, 0, -0.125, 0.5], D), (3, 3)),
        "boundary": (np.array([1, 0, -1, -0.5, 0, 1, 0.25, 0.75, 0.5, 0, 0.125, 0.5], D), (2, 3)),
        "far_side": (np.array([1, 0, 0.5, 2.0, 0, 0, 0, 2.5, 0, 0.5, -0.25, 0.5], D), (2, 2)),
        "inside": (np.array([1, 0, -1.5, 2.2, 0, 1, -1.5, 1.1, 0, 0, 0.25, 0.3], D), (4, 4)),
        "misses": (np.array([1, 0, -1, -10, 0, 0.1, -0.1, 1, 0.05, 0, -0.1, 0.5], D), (4, 3)),
        "tiny": (np.array([0, 0, 1, -3, 0, 0.5, -0.5, 0.75, 0.5, 0, -0.5, 0.25], D) * np.array([1e-170, 1e-170, 1e-170, 1] * 3), (3, 3)),
        "still": (np.array([1, 0, 0, 2.2, 0, 1, 0, 1.1, 1, 1, 0, 0.3], D), (2, 2)),
    }


HAND_DIMS = (5, 3, 2)
HAND_SPACING = np.array([0.5, 0.25, 2.0], F)

# ------------------------------------------------------------------------------- the update
UPDATE_LENGTHS = [1, 63, 64, 65, 1025]
UPDATE_LONG = (1 << 22) + 65                            # past one pass of k_volume_update's workgroups


def update_vectors(n, seed=0):
    """(x, corr, norm, lo, hi): norms of 0, -0.0, NaN, negative and inf among positive ones; values that land on
    and beyond the bounds; NaN and inf corrections."""
    rng = np.random.default_rng(seed + n)
    x = rng.uniform(-1.0, 2.0, n).astype(F)
    corr = rng.normal(0.0, 1.0, n).astype(F)
    norm = rng.uniform(0.5, 2.0, n).astype(F)
    for k, v in enumerate([0.0, np.nan, -0.0, -1.0, np.inf]):
        norm[(3 * k) % n::17] = F(v)
    corr[5 % n::29] = F(np.nan)
    corr[7 % n::31] = F(np.inf)
    lo, hi = F(0.0), F(1.5)
    # x + 1 * corr / 1 exactly on a bound
    for k, b in ((11, lo), (13, hi)):
        if k < n:
            x[k], corr[k], norm[k] = F(0.25), F(b - F(0.25)), F(1.0)
    return x, corr, norm, lo, hi


# ------------------------------------------------------------------------------- the small scan
SMALL_P, SMALL_W, SMALL_H, SMALL_DIMS = 8, 16, 12, (9, 8, 7)


@functools.lru_cache(maxsize=None)
def small_scan():
    """8 projections of 16 x 12 of a random 9 x 8 x 7 volume under general cameras: (proj, A, spacing)."""
    A = fdk_kit.general_matrices(SMALL_P, SMALL_DIMS, SMALL_W, SMALL_H, seed=2)
    spacing = fdk_kit.grid_for(SMALL_DIMS, SMALL_W, SMALL_H, 0.4)[1]
    R = np.stack([sirt_ref.ray_matrix(a).reshape(12) for a in A])
    truth = volume(21, SMALL_DIMS)
    proj = sirt_ref.forward_project(truth, spacing, R, (SMALL_H, SMALL_W))
    for a in (proj, A, spacing):
        a.setflags(write=False)
    return proj, A, spacing


@functools.lru_cache(maxsize=None)
def small_reference(subsets):
    proj, A, spacing = small_scan()
    out = sirt_ref.sirt(proj, A, SMALL_DIMS, spacing, 3, subsets, relax=0.9, lo=0.0)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------- the ball scans
BALL_CENTRE = fdk_kit.BALL_CENTRE
BALL_RADIUS = fdk_kit.BALL_RADIUS
BALL_W = BALL_H = 48
BALL_PITCH = 0.8
BALL_DIMS = (24, 24, 24)
BALL_SPACING = F(0.75)
BALL_ORIGIN = np.array([-9.0, -9.0, -9.0], F)
BALL_P, BALL_K = 24, 20
FEW_P, FEW_K = 12, 30


@functools.lru_cache(maxsize=None)
def ball_scan(P):
    """P analytic projections of the ball over a full turn of the camera: (proj (P, H, W) f32, cameras, matrices from
    the library)."""
    import simpleraytracing_amd as xrt
    cams = [fdk_ref.turntable_camera(2.0 * np.pi * p / P, fdk_kit.SOD, fdk_kit.SDD, BALL_PITCH) for p in range(P)]
    proj = np.stack([fdk_ref.ball_projection(c, BALL_W, BALL_H, BALL_CENTRE, BALL_RADIUS) for c in cams])
    A = np.stack([xrt.backprojection_matrix(camera_kit.as_camera(c, BALL_W, BALL_H), BALL_ORIGIN, BALL_SPACING) for c in cams])
    proj.setflags(write=False)
    A.setflags(write=False)
    return proj, cams, A


def ball_positions():
    n = BALL_DIMS[0]
    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return BALL_ORIGIN.astype(D) + (np.stack([ii, jj, kk], -1) + 0.5) * D(BALL_SPACING)


def ball_truth():
    """The voxelised ball: 1 where the voxel's centre lies inside."""
    return (np.linalg.norm(ball_positions() - BALL_CENTRE, axis=-1) < BALL_RADIUS).astype(F)


def ball_figures(vol):
    """(mean over the voxels more than 1 inside the surface, the distance of the centroid of the voxels above 0.5
    from the ball's centre)."""
    X = ball_positions()
    rr = np.linalg.norm(X - BALL_CENTRE, axis=-1)
    inner = np.asarray(vol, D)[rr < BALL_RADIUS - 1.0]
    dense = np.asarray(vol) > 0.5
    off = np.linalg.norm(X[dense].mean(0) - BALL_CENTRE) if dense.any() else np.inf
    return float(inner.mean()), float(off)


def residual_norm(vol, P):
    """|| b - A x || over the whole scan, in f64 from the reference's f32 projections."""
    proj, _, A = ball_scan(P)
    R = np.stack([sirt_ref.ray_matrix(a).reshape(12) for a in A])
    return float(np.linalg.norm(proj.astype(D) - sirt_ref.forward_project(vol, BALL_SPACING, R, (BALL_H, BALL_W)).astype(D)))


@functools.lru_cache(maxsize=None)
def ball_reference(P, K, subsets=1):
    """(volume, [(residual norm, inner mean) per iteration]) of SIRT from zeros with lo = 0 in the reference."""
    proj, _, A = ball_scan(P)
    table = []
    vol = sirt_ref.sirt(proj, A, BALL_DIMS, BALL_SPACING, K, subsets, 1.0, 0.0,
                        each=lambda k, x: table.append((residual_norm(x, P), ball_figures(x)[0])))
    vol.setflags(write=False)
    return vol, table
