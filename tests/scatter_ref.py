"""The scatter model's reference (include/xrt.h): the contract of
xrt_scatter_source and xrt_scatter_add restated in numpy -- f64, one operation at a
time in the contract's order, exp from the oracle as spectrum_ref takes it -- and the
chain source -> lsf_ref per kernel -> add that Context.scatter composes.  Also the two
studies DESIGN 10.16 reports: what binning costs against the unbinned estimate of the
same physical kernel, and whether the estimate cups a reconstruction."""
import numpy as np

import lsf_ref
from oracle import oracle

F = np.float32


def coarse_size(n, D):
    return (n + D - 1) // D


def pixel(paths, weights, mu, sigma):
    """(E, Q) f64 per pixel of mesh-major planes paths (M, ...)."""
    w = np.asarray(weights, F).reshape(-1)
    mu = np.asarray(mu, F).reshape(-1, w.size)
    sg = np.asarray(sigma, F).reshape(mu.shape)
    p = np.asarray(paths, F)
    assert p.shape[0] == mu.shape[0]
    E = np.zeros(p.shape[1:], np.float64)
    Q = np.zeros(p.shape[1:], np.float64)
    with np.errstate(all="ignore"):
        d = [p[m].astype(np.float64) * 0.1 for m in range(mu.shape[0])]
        for e in range(w.size):
            xe = np.zeros(p.shape[1:], np.float64)
            se = np.zeros(p.shape[1:], np.float64)
            for m in range(mu.shape[0]):
                xe = xe + np.float64(mu[m, e]) * d[m]
                se = se + np.float64(sg[m, e]) * d[m]
            t = np.float64(w[e]) * oracle.exp(-xe).reshape(xe.shape)
            E = E + t
            Q = Q + t * se
    return E, Q


def source(paths, open, weights, mu, sigma, D):
    """(source (P, Hc, Wc), lbuffer (P, H, W)) of paths (M, P, H, W) and open (P, H, W) or None."""
    p = np.asarray(paths, F)
    assert p.ndim == 4
    _, P, H, W = p.shape
    E, Q = pixel(p, weights, mu, sigma)
    flagged = np.zeros((P, H, W), bool) if open is None else np.asarray(open).reshape(P, H, W) != 0
    with np.errstate(all="ignore"):
        lb = E.astype(F)
    lb[flagged] = F(-1.0)
    q = np.where(flagged, np.float64(0.0), Q)
    Hc, Wc = coarse_size(H, D), coarse_size(W, D)
    acc = np.full((P, Hc, Wc), -0.0, np.float64)
    with np.errstate(all="ignore"):
        for dy in range(D):
            ys = np.arange(Hc) * D + dy
            yv = ys < H
            if not yv.any():
                break
            r = np.full((P, int(yv.sum()), Wc), -0.0, np.float64)
            for dx in range(D):
                xs = np.arange(Wc) * D + dx
                xv = xs < W
                if not xv.any():
                    break
                r[:, :, xv] = r[:, :, xv] + q[:, ys[yv]][:, :, xs[xv]]
            acc[:, yv] = acc[:, yv] + r
        rows = np.minimum(D, H - np.arange(Hc) * D)
        cols = np.minimum(D, W - np.arange(Wc) * D)
        src = (acc / (rows[:, None] * cols[None, :]).astype(np.float64)).astype(F)
    return src, lb


def axis(n, D, nc):
    """(i0, i1, f) of the n fine samples on a coarse axis of nc."""
    u = (np.arange(n, dtype=np.float64) + 0.5) / np.float64(D) - 0.5
    u = np.where(u < 0.0, 0.0, u)
    u = np.where(u > nc - 1, np.float64(nc - 1), u)
    u0 = np.floor(u)
    i0 = u0.astype(np.int64)
    return i0, np.minimum(i0 + 1, nc - 1), u - u0


def add(blurred, amp, D, shape, primary=None):
    """(out, scatter, u8) on the fine (P, H, W) `shape` from blurred (G, P, Hc, Wc)."""
    P, H, W = shape
    b = np.asarray(blurred, F)
    a = np.asarray(amp, F).reshape(-1)
    Hc, Wc = coarse_size(H, D), coarse_size(W, D)
    assert b.shape == (a.size, P, Hc, Wc)
    x0, x1, fx = axis(W, D, Wc)
    y0, y1, fy = axis(H, D, Hc)
    fx, fy = fx[None, None, :], fy[None, :, None]
    S = np.zeros((P, H, W), np.float64)
    with np.errstate(all="ignore"):
        for g in range(a.size):
            c = b[g].astype(np.float64)
            c00, c01 = c[:, y0][:, :, x0], c[:, y0][:, :, x1]
            c10, c11 = c[:, y1][:, :, x0], c[:, y1][:, :, x1]
            va = np.where(fx == 0.0, c00, c00 + fx * (c01 - c00))
            vb = np.where(fx == 0.0, c10, c10 + fx * (c11 - c10))
            v = np.where(fy == 0.0, va, va + fy * (vb - va))
            S = S + np.float64(a[g]) * v
        sc = S.astype(F)
        out = sc if primary is None else (np.asarray(primary, F).reshape(shape).astype(np.float64) + S).astype(F)
    return out, sc, oracle.lut_u8_array(out.reshape(-1)).reshape(out.shape)


def estimate(src, kernels, D, shape, primary=None):
    """The blur of the coarse source by each (amp, hx, hy) and the sum: add()'s results."""
    blurred = np.stack([lsf_ref.apply(src, hx, hy)[0] for _, hx, hy in kernels])
    return add(blurred, [k[0] for k in kernels], D, shape, primary)


def same(got, want):
    """lsf_ref.same: bit for bit where the reference is no NaN, NaN for NaN elsewhere."""
    return lsf_ref.same(np.asarray(got).reshape(np.asarray(want).shape), want)


# --------------------------------------------------------------------------- the studies
def ball_chords(W, H, R, cx=None, cy=None):
    """A ball's analytic chord lengths (mm, parallel beam, one pixel a mm) on a W x H detector."""
    cx = (W - 1) / 2.0 if cx is None else cx
    cy = (H - 1) / 2.0 if cy is None else cy
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    r2 = (xx - cx) ** 2 + (yy - cy) ** 2
    return (2.0 * np.sqrt(np.maximum(R * R - r2, 0.0))).astype(F)


BALL_TABLE = (np.array([50.0, 30.0], F), np.array([[0.05, 0.03]], F), np.array([[0.02, 0.015]], F))


def binning_deviation(D, sigma_pixels=14.0, size=192, R=60.0):
    """The largest deviation of the estimate at binning D from the D = 1 estimate of the same
    Gaussian (whose taps fit untruncated at full resolution), as a share of the D = 1 scatter
    plane's maximum."""
    w, mu, sg = BALL_TABLE
    paths = ball_chords(size, size, R)[None, None]
    planes = {}
    for d in (1, D):
        taps = 2 * int(np.ceil(4.0 * sigma_pixels / d)) + 1
        assert taps <= 129
        h = lsf_ref.gaussian(sigma_pixels / d, taps)[1]
        src, _ = source(paths, None, w, mu, sg, d)
        planes[d] = estimate(src, [(1.0, h, h)], d, (1, size, size))[1].astype(np.float64)
    return float(np.abs(planes[D] - planes[1]).max() / planes[1].max())


def cupping_study(D=4, sigma_pixels=12.0, amp=1.0):
    """DESIGN 10.11's ball scan, its line integrals taken as the path lengths of one material
    under a one-bin beam, reconstructed by fdk_ref from -ln of the primary alone and of the
    primary with the scatter estimate added: ((centre, rim) without, (centre, rim) with), the
    means of the voxels within 1.5 of the ball's centre and of those 2.5 to 3.0 from it."""
    import fdk_kit
    import fdk_ref
    proj, cams, poses = fdk_kit.scan(False)
    P, H, W = proj.shape
    w, mu, sg = np.array([80.0], F), np.array([[2.5]], F), np.array([[1.0]], F)
    src, lb = source(np.asarray(proj, F)[None], None, w, mu, sg, D)
    taps = 2 * int(np.ceil(4.0 * sigma_pixels / D)) + 1
    h = lsf_ref.gaussian(sigma_pixels / D, taps)[1]
    total, _, _ = estimate(src, [(amp, h, h)], D, (P, H, W), lb)
    n = fdk_kit.SCAN_DIMS[0]
    kk, jj, ii = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    X = fdk_kit.SCAN_ORIGIN.astype(np.float64) + (np.stack([ii, jj, kk], -1) + 0.5) * np.float64(fdk_kit.SCAN_SPACING)
    rr = np.linalg.norm(X - fdk_kit.BALL_CENTRE, axis=-1)
    figures = []
    for image in (lb, total):
        line = (-np.log(image.astype(np.float64) / 80.0) / 0.25).astype(F)      # mu * 0.1 = 0.25 a unit of length
        vol = np.asarray(fdk_ref.fdk(line, cams, poses, W, H, fdk_kit.SCAN_DIMS, fdk_kit.SCAN_ORIGIN, fdk_kit.SCAN_SPACING,
                                     fdk_kit.SCAN_AXIS_POINT), np.float64)
        figures.append((float(vol[rr < 1.5].mean()), float(vol[(rr > 2.5) & (rr < 3.0)].mean())))
    return figures[0], figures[1]
