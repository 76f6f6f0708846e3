"""The spectrum model's reference (XRT_MODEL_SPECTRUM): a
polychromatic beam of K energy bins over the materials model's scene,

    I = sum_e weight[e] * exp(-sum_m mu[m][e] * d_m),

composed as materials_ref.render is from oracle entry points that are pinned
already -- hit_pairs, intersect_batch, triangle_normals, exp -- and the signed
model's ray restated in numpy (materials_ref._rays).

    for m in meshes:                       # the materials model's per-mesh sums
        distance[m] = 0.0f; signSum[m] = 0
        for each hit of mesh m in triangle order:
            distance[m] += sign * t (f32); signSum[m] += sign
    if any signSum[m] != 0: L = -1.0f
    else:
        E = 0.0                            # f64, left to right
        for e in bins:
            x = 0.0
            for m in meshes: x = x + (double)mu[m][e] * ((double)distance[m] * 0.1)
            E = E + (double)weight[e] * exp(-x)
        L = (float)E

Anchored by tests/test_spectrum_cpu.py: with one bin of weight 80 and one mesh
it is oracle.render_signed_rows bit for bit; on the phantom its flags and hit
counts are materials_ref.render's.
"""
import numpy as np

from materials_ref import _rays
from oracle import oracle

F = np.float32


def integrate(distance, sign_sum, weights, mu):
    """The model's final loop for n rays: distance and sign_sum (n, M), weights (K,),
    mu (M, K).  x86 arithmetic through numpy, glibc's exp."""
    w = np.asarray(weights, F).reshape(-1)
    mu = np.asarray(mu, F).reshape(-1, w.size)
    d = np.asarray(distance, F).reshape(-1, mu.shape[0])
    s = np.zeros(d.shape, np.int64) if sign_sum is None else np.asarray(sign_sum).reshape(d.shape)
    E = np.zeros(len(d), np.float64)
    with np.errstate(all="ignore"):
        for e in range(w.size):
            x = np.zeros(len(d), np.float64)
            for m in range(mu.shape[0]):
                x = x + np.float64(mu[m, e]) * (d[:, m].astype(np.float64) * 0.1)
            E = E + np.float64(w[e]) * oracle.exp(-x)
        L = E.astype(F)
    L[(s != 0).any(1)] = F(-1.0)
    return L


def miss_value(weights):
    """What a ray without a hit gets: the chain E = E + weight[e] * 1.0, rounded to f32."""
    E = np.float64(0.0)
    for w in np.asarray(weights, F).reshape(-1):
        E = E + np.float64(w) * np.float64(1.0)
    return F(E)


class Sums:
    """distance (n, M) f32, sign_sum (n, M), mesh_hits (n, M): a scene's per-mesh sums
    under one camera, whatever the table."""


def sums(meshes, cam13, W, H):
    tris, counts = oracle.scene_arrays(meshes)
    M = len(counts)
    ends = np.cumsum(counts.astype(np.int64))
    n = W * H
    px, tr = oracle.hit_pairs(tris, cam13, W, H, np.arange(H, dtype=np.uint32))
    px, tr = px.astype(np.int64), tr.astype(np.int64)
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
        dp = (s[:, 0] * nrm[:, 0] + s[:, 1] * nrm[:, 1]) + s[:, 2] * nrm[:, 2]
        sign = (F(0.0) < dp).astype(np.int32) - (dp < F(0.0)).astype(np.int32)
        term = sign.astype(F) * t
    assert dp.dtype == F and term.dtype == F

    # sequential f32 sums per (pixel, mesh), in triangle order, from 0.0f
    group = px * M + mesh
    r = Sums()
    r.distance = np.zeros(n * M, F)
    r.sign_sum = np.zeros(n * M, np.int64)
    r.mesh_hits = np.zeros(n * M, np.int64)
    if len(group):
        first = np.r_[True, group[1:] != group[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(len(group)), 0))
        rank = np.arange(len(group)) - start
        with np.errstate(all="ignore"):
            for k in range(int(rank.max()) + 1):
                sel = rank == k
                g = group[sel]                             # distinct groups: one hit of rank k each
                r.distance[g] = r.distance[g] + term[sel]
                r.sign_sum[g] += sign[sel]
                r.mesh_hits[g] += 1
    r.distance = r.distance.reshape(n, M)
    r.sign_sum = r.sign_sum.reshape(n, M)
    r.mesh_hits = r.mesh_hits.reshape(n, M)
    return r


class Result:
    """lbuffer (H * W f32, -1 flags), distance, sign_sum and mesh_hits (H * W, M), nhits
    (every mesh's), flagged_by (the first mesh whose signs do not cancel, -1: none), flagged."""


def from_sums(su, weights, mu):
    r = Result()
    r.distance, r.sign_sum, r.mesh_hits = su.distance, su.sign_sum, su.mesh_hits
    r.lbuffer = integrate(su.distance, su.sign_sum, weights, mu)
    r.nhits = su.mesh_hits.sum(1)
    bad = su.sign_sum != 0
    r.flagged_by = np.where(bad.any(1), bad.argmax(1), -1)
    r.flagged = int(np.count_nonzero(r.flagged_by >= 0))
    return r


def render(meshes, weights, mu, cam13, W, H):
    mu = np.asarray(mu, F)
    assert mu.ndim == 2 and mu.shape == (len(meshes), np.asarray(weights).size)
    return from_sums(sums(meshes, cam13, W, H), weights, mu)
