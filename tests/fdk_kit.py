"""Shared shapes and cases of the FDK tests (test-only): the filter's and the
backprojector's shapes, the inputs built from a seed, the analytic ball scan and
its bounds.  The references are computed once per process and
handed out read-only."""
import functools

import numpy as np

import camera_kit
import fdk_ref
import pose_ref

F = np.float32
D = np.float64

# ------------------------------------------------------------------------------- the filter
FILTER_PLANES = [(1, 1), (2, 2), (7, 13), (67, 45), (257, 3)]          # (W, H)
FILTER_STACKS = [1, 3]


def filter_tap_counts(W):
    """1, 3, 2 W - 1 and longer than 2 W - 1 (odd counts, each once)."""
    return sorted({1, 3, 2 * W - 1, 2 * W + 5})


def filter_taps(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, 1.0, n) * rng.choice([1e-3, 1.0, 30.0], n)).astype(F)


def filter_image(seed, P, H, W, specials=False):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 2.0, (P, H, W)).astype(F)
    if specials:                                       # NaN, +-inf and -0.0 among the pixels
        flat = a.reshape(-1)
        for n, v in enumerate([np.nan, np.inf, -np.inf, -0.0, 0.0]):
            flat[(n * 7 + 1) % flat.size::11] = F(v)
    return a


def filter_weight(seed, H, W):
    return np.random.default_rng(seed + 99).uniform(0.5, 1.0, (H, W)).astype(F)


# ------------------------------------------------------------------------------- the backprojector
BP_DIMS = [(1, 1, 1), (5, 3, 2), (67, 9, 3), (130, 2, 2)]              # (nx, ny, nz)
BP_PLANES = [(1, 1), (2, 2), (7, 13), (67, 45)]                        # (W, H)
BP_STACKS = [1, 3, 17]
SOD, SDD = 100.0, 150.0


def grid_for(dims, W, H, ps):
    """A grid of `dims` voxels about the origin whose shadow overfills the W x H detector a little, so that some
    voxels project outside it: (origin, spacing)."""
    side = 1.2 * ps * max(W, H) * SOD / SDD
    spacing = np.full(3, side / max(dims), F)
    origin = (-0.5 * np.asarray(dims, D) * spacing.astype(D)).astype(F)
    return origin, spacing


def general_matrices(P, dims, W, H, seed=0):
    """P matrices of general cameras (camera_kit's cases, in turn) a P-th of a turn apart, from the library."""
    import simpleraytracing_amd as xrt
    ps = 0.4
    origin, spacing = grid_for(dims, W, H, ps)
    mats = []
    for p in range(P):
        base = fdk_ref.turntable_camera(2.0 * np.pi * p / P + 0.1 * seed, SOD, SDD, ps)
        c13 = camera_kit.general_camera(base, (0.0, 0.0, 0.0), W, H, **camera_kit.CASES[camera_kit.NAMES[(p + seed) % len(camera_kit.NAMES)]])
        mats.append(xrt.backprojection_matrix(camera_kit.as_camera(c13, W, H), origin, spacing))
    return np.stack(mats)


def edge_matrices(W, H):
    """Hand-built matrices over the grid (W + 3, H + 3, 2).  With k = 0 voxel (i, j) lands exactly on (col, row) =
    (i - 1, j - 1): col = -1, 0, W - 1, W and W + 1, and the rows likewise.  The slab k = 1 has c = 0 under the
    first matrix and c = -1 under the second; the third halves every coordinate (c = 2), so voxels land on half
    pixels."""
    dims = (W + 3, H + 3, 2)
    a = np.array([[1, 0, 0, -1], [0, 1, 0, -1], [0, 0, -1, 1]], D)
    b = np.array([[1, 0, 0, -1], [0, 1, 0, -1], [0, 0, -2, 1]], D)
    c = np.array([[1, 0, 0, -1], [0, 1, 0, -1], [0, 0, 0, 2]], D)
    return np.stack([a, b, c]), dims


def projections(seed, P, H, W, nan_plane=None):
    a = np.random.default_rng(seed).normal(0.0, 1.0, (P, H, W)).astype(F)
    if nan_plane is not None:
        a[nan_plane] = np.nan
    return a


def same_bits(got, want):
    """Equal bit for bit, any NaN standing for any NaN (a NaN's sign and payload are not specified)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


# ------------------------------------------------------------------------------- the ball scan
BALL_CENTRE = np.array([3.0, -2.0, 1.0])
BALL_RADIUS = 4.0
SCAN_W = SCAN_H = 64
SCAN_PITCH = 0.4
SCAN_P = 36
SCAN_DIMS = (32, 32, 32)
SCAN_SPACING = F(0.5)
SCAN_ORIGIN = np.array([-8.0, -8.0, -8.0], F)
SCAN_AXIS_POINT = np.zeros(3, F)


@functools.lru_cache(maxsize=None)
def scan(posed):
    """The ball's full-turn scan: (projections (P, H, W) f32, cameras (13 f32 each), poses or None).  posed=False:
    the camera turns about the z axis.  posed=True: the camera stands still and xrt_pose_rotation's poses (restated
    in pose_ref) turn the object the other way round."""
    cams, poses, planes = [], [], []
    for p in range(SCAN_P):
        theta = 2.0 * np.pi * p / SCAN_P
        if posed:
            c13 = fdk_ref.turntable_camera(0.0, SOD, SDD, SCAN_PITCH)
            pose = pose_ref.rotation((0.0, 0.0, 1.0), -np.degrees(theta), (0.0, 0.0, 0.0))[1]
            q = fdk_ref.pose34(pose)
            centre = q[:, :3] @ BALL_CENTRE + q[:, 3]
            poses.append(pose)
        else:
            c13 = fdk_ref.turntable_camera(theta, SOD, SDD, SCAN_PITCH)
            centre = BALL_CENTRE
        cams.append(c13)
        planes.append(fdk_ref.ball_projection(c13, SCAN_W, SCAN_H, centre, BALL_RADIUS))
    out = np.stack(planes)
    out.setflags(write=False)
    return out, cams, (poses if posed else None)


def scan_reference(posed, matrices=None):
    proj, cams, poses = scan(posed)
    return fdk_ref.fdk(proj, cams, poses, SCAN_W, SCAN_H, SCAN_DIMS, SCAN_ORIGIN, SCAN_SPACING, SCAN_AXIS_POINT,
                       matrices=matrices)


def ball_figures(vol):
    """(mean, min, max) over the voxels more than 1 inside the ball's surface, and the distance of the centroid
    of the voxels above 0.5 from the ball's centre."""
    n = SCAN_DIMS[0]
    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    X = SCAN_ORIGIN.astype(D) + (np.stack([ii, jj, kk], -1) + 0.5) * D(SCAN_SPACING)
    rr = np.linalg.norm(X - BALL_CENTRE, axis=-1)
    inner = np.asarray(vol, D)[rr < BALL_RADIUS - 1.0]
    off = np.linalg.norm(X[np.asarray(vol) > 0.5].mean(0) - BALL_CENTRE)
    return float(inner.mean()), float(inner.min()), float(inner.max()), float(off)


def check_ball(vol):
    """The bounds of DESIGN 10.11: the mean within 0.005 of 1, every inner voxel within 0.01 of 1, the centroid within a
    quarter voxel (0.125) of the centre."""
    mean, lo, hi, off = ball_figures(vol)
    print(f"ball: mean {mean:.5f}, inner voxels {lo:.4f} .. {hi:.4f}, centroid {off:.4f} off")
    assert abs(mean - 1.0) <= 0.005, mean
    assert lo >= 0.99 and hi <= 1.01, (lo, hi)
    assert off <= 0.125, off
