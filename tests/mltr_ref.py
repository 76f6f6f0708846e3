"""OS-MLTR restated in numpy (test-only; DESIGN 10.17, include/xrt.h):
xrt_poisson_project's pixel stage over sirt_ref's ray walk (its f64 line
integral before the narrowing and its lengths), xrt_backproject_update as the
composition it equals by construction -- fdk_ref.backproject of the two
components and sirt_ref.volume_update --, and xrt_mltr's loop over them and
tv_ref's descent.  exp is the oracle's (glibc's, which xrt_exp restates)."""
import numpy as np

import fdk_ref
import sirt_ref
import tv_ref
from oracle import oracle

F = np.float32
D = np.float64
INF = float("inf")


def poisson_project(volume, spacing, rays, counts, flat, background=None):
    """xrt_poisson_project: (P, H, W, 2) f32, (num, den) interleaved."""
    y = np.ascontiguousarray(counts, F)
    if y.ndim == 2:
        y = y[None]
    P, H, W = y.shape
    flat = np.ascontiguousarray(flat, F).reshape(H, W)
    L = np.zeros((P, H, W), D)
    l = sirt_ref.forward_project(volume, spacing, rays, (H, W), narrow=False, lengths=L)      # acc * ell; a miss: L = 0
    out = np.zeros((P, H, W, 2), F)
    with np.errstate(all="ignore"):
        psi = flat.astype(D)[None] * oracle.exp(-l).reshape(P, H, W)
        r = np.zeros((P, H, W), D) if background is None else np.ascontiguousarray(background, F).reshape(P, H, W).astype(D)
        yh = psi + r
        ok = (L > 0.0) & (yh > 0.0)
        q = psi / np.where(ok, yh, 1.0)
        out[..., 0] = np.where(ok, (psi - y.astype(D) * q).astype(F), F(0.0))
        out[..., 1] = np.where(ok, ((L * psi) * q).astype(F), F(0.0))
    return out


def backproject_update(pairs, matrices, dims, volume, relax=1.0, lo=-INF, hi=INF):
    """xrt_backproject_update: the updated copy of the volume (f32)."""
    pairs = np.ascontiguousarray(pairs, F)
    num = fdk_ref.backproject(np.ascontiguousarray(pairs[..., 0]), matrices, dims, 1.0)
    den = fdk_ref.backproject(np.ascontiguousarray(pairs[..., 1]), matrices, dims, 1.0)
    return sirt_ref.volume_update(volume, num, den, relax, lo, hi)


def mltr(counts, flat, matrices, dims, spacing, iterations, subsets=1, relax=1.0, lo=0.0, hi=INF, start=None, tv=None,
         background=None, each=None):
    """xrt_mltr: (nz, ny, nx) f32; tv = (steps, alpha, reduction, eps) or None.  each(k, volume), when given, is
    called after every full iteration."""
    y = np.ascontiguousarray(counts, F)
    P, H, W = y.shape
    flat = np.ascontiguousarray(np.broadcast_to(np.asarray(flat, F), (H, W)))
    bg = None if background is None else np.ascontiguousarray(np.broadcast_to(np.asarray(background, F), y.shape))
    A = np.ascontiguousarray(matrices, D).reshape(P, 12)
    R = np.stack([sirt_ref.ray_matrix(A[p]).reshape(12) for p in range(P)])
    nx, ny, nz = (int(v) for v in dims)
    x = np.zeros((nz, ny, nx), F) if start is None else np.array(start, F)
    sets = sirt_ref.subsets_of(P, subsets)
    with_tv = tv is not None and int(tv[0]) > 0
    a_k = D(tv[1]) if with_tv else D(0.0)
    for k in range(iterations):
        x0 = x.copy()
        for q in sets:
            pairs = poisson_project(x, spacing, R[q], y[q], flat, None if bg is None else bg[q])
            x = backproject_update(pairs, A[q], dims, x, relax, lo, hi)
        if with_tv:
            x = tv_ref.descend(x, int(tv[0]), a_k, D(tv[3]), lo, hi, moved=tv_ref.sumsq(x, x0))
            a_k = a_k * D(tv[2])
        if each is not None:
            each(k, x)
    return x
