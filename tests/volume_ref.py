"""Reference of the voxel trace (test-only): volume_ray restated in f64 scalars, one ray at a
time, over camera_kit.ray_directions.  Python floats are IEEE binary64 and every operation below is rounded on
its own, as the C function's; every min or max is the written select."""
import math

import numpy as np

import camera_kit

INF = float("inf")


def bbox(dims, origin, spacing):
    """xrt_volume_bbox: the minimum corner as given, the far corner narrowed from plane(a, n).  dims, origin
    and spacing are in x, y, z order."""
    lo = np.asarray(origin, np.float32)
    s = np.asarray(spacing, np.float32)
    hi = np.array([float(lo[a]) + float(int(dims[a])) * float(s[a]) for a in range(3)], np.float64)
    return lo.copy(), hi.astype(np.float32)


def _ray(O, d, lab, den, n, lo, s, acc):
    """One ray: acc[m] (a list of M floats, zero on entry) gets label m + 1's runs.  Returns (te, tx) of a
    ray that meets the volume, None of one that misses."""
    def plane(a, i):
        return lo[a] + float(i) * s[a]

    te, tx = 0.0, INF
    inv = [0.0, 0.0, 0.0]
    for a in range(3):
        if d[a] == 0.0:
            if not (O[a] >= plane(a, 0) and O[a] < plane(a, n[a])):
                return None
        else:
            inv[a] = 1.0 / d[a]
            t0 = (plane(a, 0) - O[a]) * inv[a]
            t1 = (plane(a, n[a]) - O[a]) * inv[a]
            mn = t0 if t0 < t1 else t1
            mx = t1 if t0 < t1 else t0
            te = mn if mn > te else te
            tx = mx if mx < tx else tx
    if not (te < tx):
        return None
    idx, step, up = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    for a in range(3):
        f = math.floor(((O[a] + te * d[a]) - lo[a]) / s[a])
        f = f if f >= 0 else 0
        f = f if f <= n[a] - 1 else n[a] - 1
        idx[a] = int(f)
        step[a] = 1 if d[a] > 0.0 else -1
        up[a] = 1 if d[a] > 0.0 else 0

    def tnext(a):
        return INF if d[a] == 0.0 else (plane(a, idx[a] + up[a]) - O[a]) * inv[a]

    tc, run, cur = te, 0.0, 0
    nx, ny = n[0], n[1]
    for _ in range(n[0] + n[1] + n[2] + 3):
        tn = (tnext(0), tnext(1), tnext(2))
        a = 0
        if tn[1] < tn[a]:
            a = 1
        if tn[2] < tn[a]:
            a = 2
        t = tn[a]
        tend = t if t < tx else tx
        seg = tend - tc
        v = (idx[2] * ny + idx[1]) * nx + idx[0]
        L = lab[v]
        if L != cur:
            if cur:
                acc[cur - 1] += run
            run = 0.0
            cur = L
        if L and seg > 0.0:
            run += seg * den[v] if den is not None else seg
        if seg > 0.0:
            tc = tend
        if not (t < tx):
            break
        idx[a] += step[a]
        if idx[a] < 0 or idx[a] >= n[a]:
            break
    if cur:
        acc[cur - 1] += run
    return te, tx


def volume_paths(c13, W, H, labels, spacing, origin=(0.0, 0.0, 0.0), density=None, num_labels=None, row_begin=0,
                 row_end=None, spans=None, narrow=True):
    """The planes of xrt_volume_paths: (M, rows, W) float32.  labels is (nz, ny, nx) uint8; spacing and origin
    are (x, y, z).  spans, when given a (rows, W, 2) float64 array, receives (te, tx) per ray (NaN for a miss).
    narrow=False returns the f64 sums before (float)acc[m]."""
    labels = np.ascontiguousarray(labels, np.uint8)
    nz, ny, nx = labels.shape
    M = int(labels.max()) if num_labels is None else int(num_labels)
    row_end = H if row_end is None else row_end
    c = np.asarray(c13, np.float32)
    dirs = camera_kit.ray_directions(c, W, H).astype(np.float64)
    O = [float(x) for x in c[0:3]]
    lo = [float(np.float32(x)) for x in origin]
    s = [float(np.float32(x)) for x in spacing]
    lab = labels.tobytes()
    den = None if density is None else np.ascontiguousarray(density, np.float32).astype(np.float64).ravel().tolist()
    out = np.zeros((M, row_end - row_begin, W), np.float64)
    for r in range(row_begin, row_end):
        for col in range(W):
            acc = [0.0] * M
            hit = _ray(O, dirs[r, col].tolist(), lab, den, (nx, ny, nz), lo, s, acc)
            out[:, r - row_begin, col] = acc
            if spans is not None:
                spans[r - row_begin, col] = hit if hit else (float("nan"), float("nan"))
    if not narrow:
        return out
    with np.errstate(over="ignore"):
        return out.astype(np.float32)
