"""TV-regularised SIRT restated in numpy (test-only; DESIGN 10.13, include/xrt.h):
xrt_tv_gradient over whole arrays -- every operation an elementwise f64 one, rounded on
its own, so the voxels carry the scalar contract's bits --, xrt_volume_sumsq's written
order, xrt_tv_descend and xrt_sirt_tv's loop over them and tests/sirt_ref.py's pieces."""
import math

import numpy as np

import fdk_ref
import sirt_ref

F = np.float32
D = np.float64
CHUNK, LANES, ROUNDS = 4096, 256, 16


def _quotients(x, eps):
    """(qx, qy, qz, n) of every voxel of the (nz, ny, nx) volume, f64."""
    v = np.ascontiguousarray(x, F).astype(D)
    dx, dy, dz = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    dx[:, :, :-1] = v[:, :, 1:] - v[:, :, :-1]
    dy[:, :-1, :] = v[:, 1:, :] - v[:, :-1, :]
    dz[:-1, :, :] = v[1:, :, :] - v[:-1, :, :]
    n = np.sqrt(((dx * dx + dy * dy) + dz * dz) + D(eps))
    return dx / n, dy / n, dz / n, n


def tv(x, eps):
    """TV(x) = the sum of n(p), in f64 (math.fsum: the exactly rounded sum)."""
    with np.errstate(all="ignore"):
        return math.fsum(_quotients(x, eps)[3].ravel())


def gradient(x, eps=1e-8, narrow=True):
    """xrt_tv_gradient: (nz, ny, nx) f32; narrow=False: the f64 value before the narrowing."""
    with np.errstate(all="ignore"):
        qx, qy, qz, _ = _quotients(x, eps)
        bx, by, bz = np.zeros_like(qx), np.zeros_like(qx), np.zeros_like(qx)
        bx[:, :, 1:] = qx[:, :, :-1]
        by[:, 1:, :] = qy[:, :-1, :]
        bz[1:, :, :] = qz[:-1, :, :]
        g = ((bx + by) + bz) - ((qx + qy) + qz)
        return g.astype(F) if narrow else g


def reduce(w):
    """The contract's reduce(w, m) over a flat f64 array."""
    w = np.ascontiguousarray(w, D).ravel()
    with np.errstate(all="ignore"):
        while w.size > 1:
            chunks = -(-w.size // CHUNK)
            padded = np.zeros(chunks * CHUNK, D)
            padded[:w.size] = w
            rounds = padded.reshape(chunks, ROUNDS, LANES)
            acc = np.zeros((chunks, LANES), D)
            for r in range(ROUNDS):
                acc = acc + rounds[:, r, :]
            h = LANES // 2
            while h >= 1:
                acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
                h //= 2
            w = np.ascontiguousarray(acc[:, 0])
    return D(w[0])


def sumsq(a, b=None):
    """xrt_volume_sumsq: an f64 scalar."""
    with np.errstate(all="ignore"):
        e = np.ascontiguousarray(a, F).ravel().astype(D)
        if b is not None:
            e = e - np.ascontiguousarray(b, F).ravel().astype(D)
        return reduce(e * e)


def descend(x, steps, length, eps=1e-8, lo=-np.inf, hi=np.inf, moved=None):
    """xrt_tv_descend: the descended copy of x (f32).  moved: the solver's D -- the step is length * sqrt(moved)."""
    x = np.array(x, F)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        for _ in range(int(steps)):
            g = gradient(x, eps)
            gn = np.sqrt(sumsq(g))
            if not gn > 0:
                continue
            step = D(length) if moved is None else D(length) * np.sqrt(D(moved))
            c = step / gn
            v = (x.astype(D) - c * g.astype(D)).astype(F)
            v = np.where(v < lo, lo, v)
            x = np.where(v > hi, hi, v).astype(F)
    return x


def sirt_tv(proj, matrices, dims, spacing, iterations, subsets=1, relax=1.0, lo=0.0, hi=np.inf, start=None, tv=None):
    """xrt_sirt_tv: (nz, ny, nx) f32; tv = (steps, alpha, reduction, eps) or None."""
    if tv is None or int(tv[0]) == 0:
        return sirt_ref.sirt(proj, matrices, dims, spacing, iterations, subsets, relax, lo, hi, start)
    steps, alpha, reduction, eps = int(tv[0]), D(tv[1]), D(tv[2]), D(tv[3])
    proj = np.ascontiguousarray(proj, F)
    P = proj.shape[0]
    A = np.ascontiguousarray(matrices, D).reshape(P, 12)
    R = np.stack([sirt_ref.ray_matrix(A[p]).reshape(12) for p in range(P)])
    nx, ny, nz = (int(v) for v in dims)
    x = np.zeros((nz, ny, nx), F) if start is None else np.array(start, F)
    sets = sirt_ref.subsets_of(P, subsets)
    ones = np.ones_like(proj)
    norms = [fdk_ref.backproject(ones[q], A[q], dims, 1.0) for q in sets]
    a_k = alpha
    for _ in range(iterations):
        x0 = x.copy()
        for s, q in enumerate(sets):
            r = sirt_ref.forward_project(x, spacing, R[q], mode=sirt_ref.RESIDUAL, meas=proj[q])
            c = fdk_ref.backproject(r, A[q], dims, 1.0)
            x = sirt_ref.volume_update(x, c, norms[s], relax, lo, hi)
        x = descend(x, steps, a_k, eps, lo, hi, moved=sumsq(x, x0))
        a_k = a_k * reduction
    return x
