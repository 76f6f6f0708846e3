"""FDK reconstruction restated in numpy (test-only; DESIGN 10.11, include/xrt.h):
xrt_fdk_filter's and xrt_backproject's contracts with every operation rounded on
its own -- numpy does not fuse, so the restatement is exact --, the host helpers
(ramp, cosine weights, scale) in their own operation order, the backprojection
matrix by a numpy inversion (an independent route to the same geometry) and the
analytic ball scan of the accuracy tests."""
import numpy as np

F = np.float32
D = np.float64
RAMLAK, HANN = 0, 1


# --------------------------------------------------------------------------- the row filter
def fdk_filter(image, taps, weight=None):
    """out[..., y, x] = (float)(+0.0 + sum over k in order of (double)taps[k] * (double)pw[..., y, x + k - r]),
    only where the pixel lies in the row; pw = image * weight in f32."""
    a = np.ascontiguousarray(image, F)
    t = np.ascontiguousarray(taps, F).reshape(-1)
    assert t.size % 2 == 1
    r = (t.size - 1) // 2
    W = a.shape[-1]
    with np.errstate(all="ignore"):
        pw = a if weight is None else a * np.ascontiguousarray(weight, F)
        assert pw.dtype == F
        pd = pw.astype(D)
        s = np.zeros(a.shape, D)
        for k in range(t.size):
            sh = k - r
            lo, hi = max(0, -sh), min(W, W - sh)            # the outputs x with 0 <= x + sh < W
            if lo < hi:
                s[..., lo:hi] = s[..., lo:hi] + D(t[k]) * pd[..., lo + sh:hi + sh]
        return s.astype(F)


# --------------------------------------------------------------------------- the backprojector
def backproject(proj, matrices, dims, scale=1.0, slabs=None, volume=None, accumulate=False):
    """xrt_backproject: (slabs, ny, nx) f32."""
    proj = np.ascontiguousarray(proj, F)
    if proj.ndim == 2:
        proj = proj[None]
    P, H, W = proj.shape
    A = np.ascontiguousarray(matrices, D).reshape(P, 12)
    nx, ny, nz = (int(v) for v in dims)
    k0, k1 = (0, nz) if slabs is None else slabs
    k, j, i = np.meshgrid(np.arange(k0, k1, dtype=D), np.arange(ny, dtype=D), np.arange(nx, dtype=D), indexing="ij")
    acc = np.zeros(i.shape, D)
    padded = np.zeros((H + 2, W + 2), F)

    def sample(y, x):
        return padded[y + 1, x + 1]

    with np.errstate(all="ignore"):
        for p in range(P):
            m = A[p]
            a = m[0] * i + ((m[1] * j + m[2] * k) + m[3])
            b = m[4] * i + ((m[5] * j + m[6] * k) + m[7])
            c = m[8] * i + ((m[9] * j + m[10] * k) + m[11])
            w = 1.0 / c
            col, row = a * w, b * w
            ok = (c > 0) & (col > -1) & (col < W) & (row > -1) & (row < H)
            col, row = np.where(ok, col, 0.0), np.where(ok, row, 0.0)
            fc, fr = np.floor(col), np.floor(row)
            fx, fy = (col - fc).astype(F), (row - fr).astype(F)
            x0, y0 = fc.astype(np.int64), fr.astype(np.int64)
            padded[:] = 0
            padded[1:-1, 1:-1] = proj[p]
            s00, s01, s10, s11 = sample(y0, x0), sample(y0, x0 + 1), sample(y0 + 1, x0), sample(y0 + 1, x0 + 1)
            top = s00 + fx * (s01 - s00)
            bot = s10 + fx * (s11 - s10)
            v = top + fy * (bot - top)
            assert v.dtype == F
            acc = np.where(ok, acc + v.astype(D) * (w * w), acc)
        if accumulate:
            return (np.ascontiguousarray(volume, F).astype(D) + acc * D(scale)).astype(F)
        return (acc * D(scale)).astype(F)


# --------------------------------------------------------------------------- the helpers
def _ramlak(n):
    n = np.asarray(n, np.int64)
    dn = np.where(n == 0, 1, n).astype(D)
    g = -1.0 / ((np.pi * np.pi) * (dn * dn))
    return np.where(n == 0, 0.25, np.where(n % 2 == 0, 0.0, g))


def ramp_filter(num_taps, window=RAMLAK):
    r = (num_taps - 1) // 2
    n = np.arange(num_taps, dtype=np.int64) - r
    if window == RAMLAK:
        return _ramlak(n).astype(F)
    return ((0.25 * _ramlak(n - 1) + 0.5 * _ramlak(n)) + 0.25 * _ramlak(n + 1)).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _offsets(ps, n):
    """The render's pixel offsets kept in f64."""
    return D(F(ps)) * ((0.5 + np.arange(n, dtype=D)) - D(n) / 2.0)


def _parts(c13):
    c = np.asarray(c13, F).astype(D)
    return c[0:3], c[3:6], c[6:9], c[9:12], c[12]


def fdk_weights(c13, W, H):
    S, Dt, up, right, ps = _parts(c13)
    ax = Dt - S
    v = _offsets(ps, H)[:, None, None]
    u = _offsets(ps, W)[None, :, None]
    d = (ax + up * v) + right * u
    return (_dot(d, ax) / (np.sqrt(_dot(d, d)) * np.sqrt(_dot(ax, ax)))).astype(F)


def fdk_scale(c13, axis_point, P):
    S, Dt, up, right, ps = _parts(c13)
    ax = Dt - S
    q = np.asarray(axis_point, F).astype(D) - S
    sdd = np.sqrt(_dot(ax, ax))
    sod = _dot(q, ax) / sdd
    return float(((np.pi / D(P)) * (sod / sdd)) / (ps * np.sqrt(_dot(right, right))))


def pose34(pose):
    return np.hstack([np.eye(3), np.zeros((3, 1))]) if pose is None else np.asarray(pose, F).astype(D).reshape(3, 4)


def backprojection_matrix(c13, W, H, origin, spacing, pose=None):
    """The matrix by numpy's inversion: index -> rest frame -> world -> (a', b', c) -> pixel coordinates."""
    S, Dt, up, right, ps = _parts(c13)
    q = pose34(pose)
    org = np.asarray(origin, F).astype(D)
    spc = np.broadcast_to(np.asarray(spacing, F).astype(D), (3,))
    to_rest = np.hstack([np.diag(spc), (org + 0.5 * spc)[:, None]])                  # 3 x 4
    to_world = q[:, :3] @ to_rest
    to_world[:, 3] += q[:, 3]
    to_world[:, 3] -= S
    Q = np.linalg.inv(np.stack([right, up, Dt - S], axis=1)) @ to_world
    return np.stack([Q[0] / ps + (W / 2.0 - 0.5) * Q[2], Q[1] / ps + (H / 2.0 - 0.5) * Q[2], Q[2]])


def pixel_point(c13, W, H, row, col):
    """The world point of the (fractional) pixel (row, col): the render's pixel formula in f64."""
    S, Dt, up, right, ps = _parts(c13)
    v = ps * ((0.5 + np.asarray(row, D)) - D(H) / 2.0)
    u = ps * ((0.5 + np.asarray(col, D)) - D(W) / 2.0)
    return Dt + up * v[..., None] + right * u[..., None]


# --------------------------------------------------------------------------- the analytic scan
def turntable_camera(theta, sod, sdd, ps):
    """13 f32 values: the source at distance sod and the detector centre at sdd - sod from the z axis, turned by
    theta about it; right = the turned +y, up = +z."""
    cs, sn = np.cos(theta), np.sin(theta)
    Rz = np.array([[cs, -sn, 0.0], [sn, cs, 0.0], [0.0, 0.0, 1.0]])
    return np.concatenate([Rz @ [-sod, 0.0, 0.0], Rz @ [sdd - sod, 0.0, 0.0], [0.0, 0.0, 1.0], Rz @ [0.0, 1.0, 0.0],
                           [ps]]).astype(F)


def ball_projection(c13, W, H, centre, radius):
    """The chord length of every pixel's ray through a ball (mu = 1), computed in f64, as f32 (H, W)."""
    S = _parts(c13)[0]
    r, q = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = pixel_point(c13, W, H, r, q) - S
    d = d / np.sqrt(_dot(d, d))[..., None]
    oc = S - np.asarray(centre, D)
    b = _dot(d, oc)
    disc = b * b - (_dot(oc, oc) - radius * radius)
    return (2.0 * np.sqrt(np.maximum(disc, 0.0))).astype(F)


def fdk(projections, cams13, poses, W, H, dims, origin, spacing, axis_point, window=RAMLAK, matrices=None):
    """Context.fdk, all in this module (matrices: the library's own instead of the numpy inversion's, where the
    volume is compared bit for bit -- two routes to one inverse differ in their last bits)."""
    P = len(projections)
    poses = [None] * P if poses is None else poses
    taps = ramp_filter(2 * W - 1, window)
    filtered = np.stack([fdk_filter(projections[p], taps, fdk_weights(cams13[p], W, H)) for p in range(P)])
    if matrices is None:
        matrices = np.stack([backprojection_matrix(cams13[p], W, H, origin, spacing, poses[p]) for p in range(P)])
    return backproject(filtered, matrices, dims, fdk_scale(cams13[0], axis_point, P))
