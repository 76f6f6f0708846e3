"""The materials model's reference: the L-buffer fork's loop over the meshes
(src/main-pthreads-lbuffer.cxx:768-810) with its mesh filter (:788) lifted and
one coefficient per mesh, composed from oracle entry points that are pinned
already -- hit_pairs, intersect_batch, triangle_normals, exp -- and the ray of
the signed model restated in numpy f32 / f64 (main.cxx:652-660).

    L = 80.0f
    for m in meshes, in scene order:
        if L == -1: break
        distance = 0.0f; signSum = 0
        for each triangle of mesh m, in order, with intersect && t > 1e-7:
            sign = signum(direction . normal); distance += sign * t; signSum += sign
        if signSum != 0: L = -1
        else: L = (float)((double)L * exp(-((double)mu[m] * ((double)distance * 0.1))))

Anchored by tests/test_materials_cpu.py: with one mesh it is
oracle.render_signed_rows bit for bit, and so it is on a scene of several
meshes with the filter put back (mesh0_only).
"""
import numpy as np

from oracle import oracle

F = np.float32


def _rays(cam13, W, H):
    """(origin (3,), once-normalised direction (H * W, 3)), f32 as make_ray forms them."""
    cam = np.asarray(cam13, F)
    o, c, up, right, spacing = cam[0:3], cam[3:6], cam[6:9], cam[9:12], cam[12]
    v = (np.float64(spacing) * ((0.5 + np.arange(H, dtype=np.float64)) - np.float64(H) / 2.0)).astype(F)
    u = (np.float64(spacing) * ((0.5 + np.arange(W, dtype=np.float64)) - np.float64(W) / 2.0)).astype(F)
    vv = np.repeat(v, W)
    uu = np.tile(u, H)
    X = [((c[k] + up[k] * vv) + right[k] * uu) - o[k] for k in range(3)]       # :659, f32 left to right
    length = np.sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2])                # Vec3::normalise
    with np.errstate(all="ignore"):
        d = np.stack([X[k] / length for k in range(3)], 1)
    assert d.dtype == F
    return o, d


class Result:
    """lbuffer (H * W f32, -1 flags), nhits (every mesh's), mesh_hits (H * W, M) and,
    per pixel, flagged_by: the mesh that flagged the ray (-1: none)."""


def render(meshes, mu, cam13, W, H, mesh0_only=False):
    tris, counts = oracle.scene_arrays(meshes)
    M = len(counts)
    mu = np.asarray(mu, F)
    assert mu.size == M
    ends = np.cumsum(counts.astype(np.int64))
    n = W * H
    px, tr = oracle.hit_pairs(tris, cam13, W, H, np.arange(H, dtype=np.uint32))
    px, tr = px.astype(np.int64), tr.astype(np.int64)
    if mesh0_only:                                         # the fork's :788
        keep = tr < ends[0]
        px, tr = px[keep], tr[keep]
    order = np.lexsort((tr, px))
    px, tr = px[order], tr[order]
    mesh = np.searchsorted(ends, tr, side="right")

    origin, direction = _rays(cam13, W, H)
    rays = np.concatenate([np.broadcast_to(origin, (len(px), 3)), direction[px]], 1)
    hit, t = oracle.intersect_batch(rays, tris[tr])
    assert hit.all() and (t.astype(np.float64) > 0.0000001).all()
    nrm = oracle.triangle_normals(tris)[tr]
    s = direction[px]
    with np.errstate(all="ignore"):
        dp = (s[:, 0] * nrm[:, 0] + s[:, 1] * nrm[:, 1]) + s[:, 2] * nrm[:, 2]   # :791
        sign = (F(0.0) < dp).astype(np.int32) - (dp < F(0.0)).astype(np.int32)   # :729-731
        term = sign.astype(F) * t                                                # :792
    assert dp.dtype == F and term.dtype == F

    # sequential f32 sums per (pixel, mesh), in triangle order, from 0.0f
    group = px * M + mesh
    first = np.r_[True, group[1:] != group[:-1]] if len(group) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(group)), 0)) if len(group) else first
    rank = np.arange(len(group)) - start
    distance = np.zeros(n * M, F)
    sign_sum = np.zeros(n * M, np.int64)
    mesh_hits = np.zeros(n * M, np.int64)
    with np.errstate(all="ignore"):
        for k in range(int(rank.max()) + 1 if len(rank) else 0):
            sel = rank == k
            g = group[sel]                                 # distinct groups: one hit of rank k each
            distance[g] = distance[g] + term[sel]
            sign_sum[g] += sign[sel]
            mesh_hits[g] += 1
    distance = distance.reshape(n, M)
    sign_sum = sign_sum.reshape(n, M)

    L = np.full(n, 80.0, F)
    flagged_by = np.full(n, -1, np.int64)
    with np.errstate(all="ignore"):
        for m in range(M):
            live = ~(L == F(-1.0))                         # :772
            flag = live & (sign_sum[:, m] != 0)            # :805-806
            upd = live & ~flag
            e = oracle.exp(-(np.float64(mu[m]) * (distance[upd, m].astype(np.float64) * 0.1)))
            L[upd] = (L[upd].astype(np.float64) * e).astype(F)                   # :808
            L[flag] = F(-1.0)
            flagged_by[flag] = m
    r = Result()
    r.lbuffer = L
    r.mesh_hits = mesh_hits.reshape(n, M)
    r.nhits = r.mesh_hits.sum(1)
    r.flagged_by = flagged_by
    r.flagged = int(np.count_nonzero(flagged_by >= 0))
    return r
