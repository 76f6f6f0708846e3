"""The voxeliser's contract (include/xrt.h "voxelise the scene") restated in numpy (test-only).

Every operation is a float64 ufunc of its own, so nothing is fused.  `voxelize` is the definition: every triangle
against every column of the grid, no footprint anywhere.  `voxelize_fast` walks each triangle's box of columns
instead, vectorised over the triangles; it is the same crossing function and is checked against `voxelize`
(test_voxelize_cpu.py) before it stands in for it on the scenes the definition is too slow for (the dragon)."""
import numpy as np

F, D = np.float32, np.float64
MAX_MESHES = 16


def centres(origin, spacing, n):
    """c(i) = (double)origin + ((double)i + 0.5) * (double)spacing for i < n."""
    return D(F(origin)) + (np.arange(n, dtype=D) + D(0.5)) * D(F(spacing))


def _grid(dims, origin, spacing):
    o = np.broadcast_to(np.asarray(origin, F), (3,))
    s = np.broadcast_to(np.asarray(spacing, F), (3,))
    return [centres(o[a], s[a], int(dims[a])) for a in range(3)]


def _edge(ax, ay, bx, by, px, py):
    """Whether edges a-b count at (px, py); every argument broadcasts.  Ends ordered so that a.y < b.y."""
    swap = by < ay
    ax, bx = np.where(swap, bx, ax), np.where(swap, ax, bx)
    ay, by = np.where(swap, by, ay), np.where(swap, ay, by)
    straddle = (ay <= py) != (by <= py)
    w = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
    return (ay != by) & straddle & (w > 0.0)


def crossing(p, px, py):
    """Triangles p (..., 3, 3) float64 against points (px, py), broadcasting: (crossed, z)."""
    p0, p1, p2 = p[..., 0, :], p[..., 1, :], p[..., 2, :]
    e1, e2 = p1 - p0, p2 - p0
    nx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
    ny = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
    nz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
    odd = (_edge(p0[..., 0], p0[..., 1], p1[..., 0], p1[..., 1], px, py)
           ^ _edge(p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1], px, py)
           ^ _edge(p2[..., 0], p2[..., 1], p0[..., 0], p0[..., 1], px, py))
    with np.errstate(divide="ignore", invalid="ignore"):
        z = p0[..., 2] - (nx * (px - p0[..., 0]) + ny * (py - p0[..., 1])) / nz
    return odd & (nz != 0.0), z


def _slices(Z, z):
    """The least k in [0, nz] with Z[k] >= z (Z never decreases), nz when none is."""
    return np.searchsorted(Z, z, side="left")


def _flip(flip, k, j, i, bit):
    np.bitwise_xor.at(flip, (k, j, i), np.uint16(bit))


def scatter(meshes, dims, origin, spacing):
    """The flip volume (nz + 1, ny, nx) uint16 by the definition: every triangle against every column."""
    X, Y, Z = _grid(dims, origin, spacing)
    flip = np.zeros((len(Z) + 1, len(Y), len(X)), np.uint16)
    jj, ii = np.indices((len(Y), len(X)))
    for m, soup in enumerate(meshes):
        for tri in np.asarray(soup, F).reshape(-1, 3, 3).astype(D):
            hit, z = crossing(tri, X[None, :], Y[:, None])
            _flip(flip, _slices(Z, z[hit]), jj[hit], ii[hit], 1 << m)
    return flip


def _boxes(p, X, Y):
    """Each triangle's box of columns: (i0, j0, ni, nj)."""
    xmin, xmax = p[..., 0].min(1), p[..., 0].max(1)
    ymin, ymax = p[..., 1].min(1), p[..., 1].max(1)
    i0 = np.searchsorted(X, xmin - (xmax - xmin) * D(2.0) ** -40, side="left")
    i1 = np.searchsorted(X, xmax, side="right")
    j0 = np.searchsorted(Y, ymin, side="left")
    j1 = np.searchsorted(Y, ymax, side="left")
    return i0, j0, np.maximum(i1 - i0, 0), np.maximum(j1 - j0, 0)


def footprints(meshes, dims, origin, spacing):
    """Per triangle of the scene, the (columns, rows) of the box the kernels walk for it: 0 columns for a triangle
    with n.z == 0, which they skip.  What the scatter's schedule and its counters go by."""
    X, Y, _ = _grid(dims, origin, spacing)
    p = np.concatenate([np.asarray(m, F).reshape(-1, 3, 3) for m in meshes]).astype(D)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    _, _, ni, nj = _boxes(p, X, Y)
    nj = np.where(nz != 0.0, nj, 0)
    return ni * nj, nj


def scatter_fast(meshes, dims, origin, spacing):
    """The same flip volume from each triangle's box of columns -- rows with ymin <= c_y < ymax, columns with
    xmin - 2^-40 (xmax - xmin) <= c_x <= xmax, outside which nothing counts --, one pass over all
    triangles per offset inside the box."""
    X, Y, Z = _grid(dims, origin, spacing)
    flip = np.zeros((len(Z) + 1, len(Y), len(X)), np.uint16)
    for m, soup in enumerate(meshes):
        p = np.asarray(soup, F).reshape(-1, 3, 3).astype(D)
        if not len(p):
            continue
        i0, j0, ni, nj = _boxes(p, X, Y)
        for dj in range(int(nj.max(initial=0))):
            rows = np.nonzero((nj > dj) & (ni > 0))[0]
            for di in range(int(ni[rows].max(initial=0))):
                sel = rows[ni[rows] > di]
                i, j = i0[sel] + di, j0[sel] + dj
                hit, z = crossing(p[sel], X[i], Y[j])
                _flip(flip, _slices(Z, z[hit]), j[hit], i[hit], 1 << m)
    return flip


def scan(flip, num_meshes, value=None):
    """The outputs of a flip volume: dict(mask, labels, odd_columns[, volume])."""
    nz = flip.shape[0] - 1
    mask = np.bitwise_xor.accumulate(flip[:nz], axis=0) if nz else flip[:0].copy()
    total = (mask[-1] if nz else np.zeros_like(flip[0])) ^ flip[nz]
    labels = np.zeros(mask.shape, np.uint8)
    for m in range(MAX_MESHES):
        labels[(mask >> m & 1) != 0] = m + 1                    # the later mesh wins
    out = dict(mask=mask, labels=labels,
               odd_columns=np.array([int(np.count_nonzero(total >> m & 1)) for m in range(num_meshes)], np.uint64))
    if value is not None:
        acc = np.zeros(mask.shape, D)
        for m in range(num_meshes):
            acc = np.where((mask >> m & 1) != 0, acc + D(F(value[m])), acc)
        out["volume"] = acc.astype(F)
    return out


def voxelize(meshes, dims, origin, spacing, value=None):
    return scan(scatter(meshes, dims, origin, spacing), len(meshes), value)


def voxelize_fast(meshes, dims, origin, spacing, value=None):
    return scan(scatter_fast(meshes, dims, origin, spacing), len(meshes), value)


def mesh_volume(soup):
    """The divergence-theorem volume of a closed soup in float64: sum of p0 . (p1 x p2) / 6."""
    p = np.asarray(soup, F).reshape(-1, 3, 3).astype(D)
    return float(np.einsum("ti,ti->t", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


def dragon_grid(soup, n):
    """The cubic grid of n^3 voxels about a soup: lower corner = bbox lower - f32(0.035) * (longest extent),
    spacing = f32(longest extent * 1.07 / n).  Returns (dims, origin f32[3], spacing f32)."""
    v = np.asarray(soup, F).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    extent = F((hi - lo).max())
    return (n, n, n), (lo - F(0.035) * extent).astype(F), F(extent * F(1.07) / F(n))
