"""The ray table ("Ray table") restated in numpy
(test-only): the whole padded table of a camera and strip from
camera_kit.ray_directions, and the cameras the CPU and GPU suites share."""
import numpy as np

import camera_kit as ck


def pad32(n):
    return (n + 31) // 32 * 32


def table_indices(W, r0, r1):
    """(index of dx, r, c) for every padded (r, c) of the strip [r0, r1) of a
    W-wide image: r < 32 ceil((r1 - r0) / 32), c < 32 ceil(W / 32); tile-major
    over 8 x 8 tiles of 192 floats, lane (r % 8) * 8 + c % 8."""
    tiles_x = pad32(W) // 8
    r, c = np.meshgrid(np.arange(pad32(r1 - r0)), np.arange(pad32(W)), indexing="ij")
    return ((r // 8) * tiles_x + c // 8) * 192 + (r % 8) * 8 + c % 8, r, c


def expected_table(c13, W, H, r0=0, r1=None):
    """Every float of the table: pixel (r0 + r, c) with the row clamped to
    H - 1 and the column to W - 1; dy and dz lie 64 and 128 floats after dx."""
    r1 = H if r1 is None else r1
    d = ck.ray_directions(c13, W, H)
    idx, r, c = table_indices(W, r0, r1)
    val = d[np.minimum(r0 + r, H - 1), np.minimum(c, W - 1)]          # (rows, cols, 3)
    n = 3 * pad32(r1 - r0) * pad32(W)
    out = np.zeros(n, np.float32)
    written = np.zeros(n, np.int32)
    for k in range(3):
        out[idx + 64 * k] = val[..., k]
        np.add.at(written, (idx + 64 * k).ravel(), 1)
    assert (written == 1).all()                 # the formula covers every float of the table once
    return out


def mismatches(table, want):
    """Indices where the table differs: by bits, or, where the expected value
    is NaN, by not being NaN (host and device NaNs differ in sign: DESIGN 10.3)."""
    table = np.ascontiguousarray(table, np.float32)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(table), table.view(np.uint32) != want.view(np.uint32))
    return np.nonzero(bad)[0]


def source_on_detector_camera():
    """(c13, W, H): the detector's centre is the source and W, H are odd, so the
    centre pixel's offsets are exactly 0 and its direction 0 / 0: NaN after the
    first normalisation, which the second keeps (NaN != 0: not its zero-length
    branch).  Every other pixel is finite."""
    c13 = np.array([1.0, 2.0, 3.0, 1.0, 2.0, 3.0, 0.1, 0.9, 0.2, 0.8, -0.1, 0.3, 0.5], np.float32)
    return c13, 9, 7


def underflow_camera():
    """(c13, W, H): every component of detector + up v + right u - origin is
    about 1e-30, a normal float whose square underflows to 0 (with or without
    denormals), so the first length is 0, the first normalisation gives
    +-inf (0 / 0 = NaN for a zero component), the second length is inf and
    inf / inf = NaN: every float of the table is NaN.  The second
    normalisation's zero-length branch is not reached here either."""
    s = np.float32(1e-30)
    c13 = np.array([0.0, 0.0, 0.0, 3.0, 1.0, -2.0, 0.25, 1.0, 0.125, 1.0, -0.25, 0.5, 0.0], np.float32) * s
    c13[12] = np.float32(1.0)
    return c13, 11, 5


def random_cameras(n=20, seed=20261020):
    rng = np.random.default_rng(seed)
    return [ck.random_general_camera(rng, 40) for _ in range(n)]
