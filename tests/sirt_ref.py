"""SIRT / OS-SART restated in numpy (test-only; DESIGN 10.12, include/xrt.h):
xrt_ray_matrix in Python floats, xrt_forward_project's contract vectorised over
the rays of a plane -- the Python loop is over the steps; every operation is an
elementwise f64 one, rounded on its own, so the lanes carry the scalar contract's
bits --, xrt_volume_update, and xrt_sirt's loop over them and
fdk_ref.backproject."""
import numpy as np

import fdk_ref

F = np.float32
D = np.float64
PROJECT, RESIDUAL = 0, 1
INF = float("inf")


def ray_matrix(A):
    """[A3^-1 | -A3^-1 a4] by cofactors in the header's written order: (3, 4) f64."""
    A = [float(v) for v in np.asarray(A, D).reshape(12)]
    M = [[A[4 * i + j] for j in range(3)] for i in range(3)]
    C = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[i][j] = M[i1][j1] * M[i2][j2] - M[i1][j2] * M[i2][j1]
    det = (M[0][0] * C[0][0] + M[0][1] * C[0][1]) + M[0][2] * C[0][2]
    R = np.empty((3, 4), D)
    for i in range(3):
        N = [C[j][i] / det for j in range(3)]
        R[i, :3] = N
        R[i, 3] = -((N[0] * A[3] + N[1] * A[7]) + N[2] * A[11])
    return R


def _plane(i):
    return -0.5 + np.asarray(i, D) * 1.0


def _trace(vol, n, O, d):
    """forward_ray over flat arrays of rays: (hit, acc, span).  vol is the flat f64 volume, n = (nx, ny, nz), O
    three floats, d three f64 arrays."""
    shape = d[0].shape
    te, tx = np.zeros(shape, D), np.full(shape, INF, D)
    hit = np.ones(shape, bool)
    inv = []
    for a in range(3):
        p0, pn = float(_plane(0)), float(_plane(n[a]))
        zero = d[a] == 0.0
        hit &= ~zero | bool(O[a] >= p0 and O[a] < pn)
        iv = np.where(zero, 0.0, 1.0 / np.where(zero, 1.0, d[a]))
        t0, t1 = (p0 - O[a]) * iv, (pn - O[a]) * iv
        mn, mx = np.where(t0 < t1, t0, t1), np.where(t0 < t1, t1, t0)
        te = np.where(~zero & (mn > te), mn, te)
        tx = np.where(~zero & (mx < tx), mx, tx)
        inv.append(iv)
    hit &= te < tx
    idx, step, up, tn = [], [], [], []
    for a in range(3):
        f = np.floor(((O[a] + te * d[a]) - (-0.5)) / 1.0)
        f = np.where(f >= 0.0, f, 0.0)
        f = np.where(f <= float(n[a] - 1), f, float(n[a] - 1))
        idx.append(f.astype(np.int64))
        step.append(np.where(d[a] > 0.0, 1, -1).astype(np.int64))
        up.append(np.where(d[a] > 0.0, 1, 0).astype(np.int64))
        tn.append(np.where(d[a] == 0.0, INF, (_plane(idx[a] + up[a]) - O[a]) * inv[a]))
    tc, acc = te.copy(), np.zeros(shape, D)
    alive = hit.copy()
    nx, ny = n[0], n[1]
    for _ in range(n[0] + n[1] + n[2] + 3):
        if not alive.any():
            break
        t, ax = tn[0], np.zeros(shape, np.int64)
        for a in (1, 2):
            m = tn[a] < t
            t, ax = np.where(m, tn[a], t), np.where(m, a, ax)
        tend = np.where(t < tx, t, tx)
        seg = tend - tc
        vox = (idx[2] * ny + idx[1]) * nx + idx[0]
        add = alive & (seg > 0.0)
        acc = np.where(add, acc + seg * vol[vox], acc)
        tc = np.where(add, tend, tc)
        alive = alive & (t < tx)
        for a in range(3):
            sel = alive & (ax == a)
            new = idx[a] + step[a]
            out = sel & ((new < 0) | (new >= n[a]))
            alive = alive & ~out
            go = sel & ~out
            idx[a] = np.where(go, new, idx[a])
            tn[a] = np.where(go, (_plane(idx[a] + up[a]) - O[a]) * inv[a], tn[a])
    return hit, acc, tx - te


def forward_project(volume, spacing, rays, shape=None, mode=PROJECT, meas=None, narrow=True, lengths=None):
    """xrt_forward_project: (P, H, W) f32.  narrow=False, PROJECT mode: the f64 acc * ell before the narrowing.
    lengths, when given a (P, H, W) f64 array, receives L per ray (0 for a miss)."""
    v = np.ascontiguousarray(volume, F)
    nz, ny, nx = v.shape
    vol = v.astype(D).ravel()
    s = [float(x) for x in np.broadcast_to(np.asarray(spacing, F), (3,))]
    R = np.ascontiguousarray(rays, D).reshape(-1, 12)
    P = R.shape[0]
    if meas is not None:
        meas = np.ascontiguousarray(meas, F).reshape(P, *np.shape(meas)[-2:])
        shape = meas.shape[1:]
    H, W = shape
    row, col = np.meshgrid(np.arange(H, dtype=D), np.arange(W, dtype=D), indexing="ij")
    row, col = row.ravel(), col.ravel()
    out = np.zeros((P, H * W), D)
    with np.errstate(all="ignore"):
        for p in range(P):
            r = [float(x) for x in R[p]]
            d = [r[4 * a] * col + (r[4 * a + 1] * row + r[4 * a + 2]) for a in range(3)]
            hit, acc, span = _trace(vol, (nx, ny, nz), (r[3], r[7], r[11]), d)
            ell = np.sqrt(((s[0] * d[0]) * (s[0] * d[0]) + (s[1] * d[1]) * (s[1] * d[1])) + (s[2] * d[2]) * (s[2] * d[2]))
            L = span * ell
            if lengths is not None:
                lengths[p] = np.where(hit, L, 0.0).reshape(H, W)
            if mode == PROJECT:
                val = acc * ell
                out[p] = np.where(hit, val if not narrow else val.astype(F).astype(D), 0.0)
            else:
                ok = hit & (L > 0.0)
                val = (meas[p].astype(D).ravel() - acc * ell) / np.where(ok, L, 1.0)
                out[p] = np.where(ok, val.astype(F).astype(D), 0.0)
        out = out.reshape(P, H, W)
        return out.astype(F) if narrow or mode != PROJECT else out


def volume_update(x, corr, norm, relax=1.0, lo=-INF, hi=INF):
    """xrt_volume_update: the updated copy of x (f32)."""
    x, c, n = (np.ascontiguousarray(a, F) for a in (x, corr, norm))
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):
        v = (x.astype(D) + D(relax) * (c.astype(D) / n.astype(D))).astype(F)
        v = np.where(v < lo, lo, v)
        v = np.where(v > hi, hi, v)
        return np.where(n > 0, v, x).astype(F)


def subsets_of(P, S):
    return [list(range(s, P, S)) for s in range(S)]


def sirt(proj, matrices, dims, spacing, iterations, subsets=1, relax=1.0, lo=0.0, hi=INF, start=None, each=None):
    """xrt_sirt: (nz, ny, nx) f32.  each(k, volume), when given, is called after every full iteration."""
    proj = np.ascontiguousarray(proj, F)
    P = proj.shape[0]
    A = np.ascontiguousarray(matrices, D).reshape(P, 12)
    R = np.stack([ray_matrix(A[p]).reshape(12) for p in range(P)])
    nx, ny, nz = (int(v) for v in dims)
    x = np.zeros((nz, ny, nx), F) if start is None else np.array(start, F)
    sets = subsets_of(P, subsets)
    ones = np.ones_like(proj)
    norms = [fdk_ref.backproject(ones[q], A[q], dims, 1.0) for q in sets]
    for k in range(iterations):
        for s, q in enumerate(sets):
            r = forward_project(x, spacing, R[q], mode=RESIDUAL, meas=proj[q])
            c = fdk_ref.backproject(r, A[q], dims, 1.0)
            x = volume_update(x, c, norms[s], relax, lo, hi)
        if each is not None:
            each(k, x)
    return x
