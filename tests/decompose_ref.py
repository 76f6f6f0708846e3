"""Material decomposition's reference (include/xrt.h): xrt_decompose and
xrt_decompose_guess restated in numpy, composed from what is pinned already -- libm's exp
(oracle.exp), logf_ref.logf and the x chain of spectrum_ref / detector_ref.bin_means.  Every f64
operation is rounded on its own (numpy cannot fuse); the pixels of a plane run side by side, each
leaving the iteration where the contract's loop ends for it.

    masked:  out = +0, iters = 254
    y[c] = channels[c] (times gain under INTENSITY);  A = 0, or guess @ -logf(max((float)(y / y0), 1e-30f))
    while it < max_iter:
        lam[e] = (w[e] * exp(-sum_b mu[b][e] * (A[b] * 0.1))) * gain
        ybar[c] = sum_e r[c][e] * lam[e];  J[c][b] = sum_e mu[b][e] * (r[c][e] * lam[e])
        over the channels with ybar > 0:  g[b] += J[c][b] * (1 - y / ybar);  H[b][b'] += (J[c][b] * J[c][b']) / ybar
        H[b][b] += H[b][b] * damping;  LDL^T in the contract's order; a pivot not > 0: iters = 255, A stays
        A[b] += x[b] / 0.1;  it += 1;  every |step| <= tol: done
    out = (float)A, iters = it"""
import numpy as np

import logf_ref
from oracle import oracle

F = np.float32
D = np.float64
MASKED, FAILED = 254, 255


def solve(H, g, B):
    """The contract's LDL^T: H[b][b2] (b2 >= b) and g[b] arrays over the pixels; (x list, ok)."""
    with np.errstate(all="ignore"):
        d0 = H[0][0]
        ok = d0 > 0
        if B == 1:
            return [g[0] / d0], ok
        l10 = H[0][1] / d0
        d1 = H[1][1] - l10 * H[0][1]
        z0 = g[0]
        z1 = g[1] - l10 * z0
        ok = ok & (d1 > 0)
        if B == 2:
            x1 = z1 / d1
            return [z0 / d0 - l10 * x1, x1], ok
        l20 = H[0][2] / d0
        l21 = (H[1][2] - l20 * H[0][1]) / d1
        d2 = (H[2][2] - l20 * H[0][2]) - l21 * (l21 * d1)
        z2 = (g[2] - l20 * z0) - l21 * z1
        ok = ok & (d2 > 0)
        x2 = z2 / d2
        x1 = z1 / d1 - l21 * x2
        x0 = (z0 / d0 - l10 * x1) - l20 * x2
        return [x0, x1, x2], ok


def tables(weights, mu, response):
    w = np.asarray(weights, F).reshape(-1)
    mu = np.asarray(mu, F).reshape(-1, w.size)
    r = np.asarray(response, F).reshape(-1, w.size)
    return w, mu, r


def mean_coefficients(weights, mu, response):
    """(mbar (C, B) f64, used (C,)): each channel's mean coefficient a basis, and whether its denominator
    is > 0."""
    w, mu, r = tables(weights, mu, response)
    B, C, K = mu.shape[0], r.shape[0], w.size
    mbar = np.zeros((C, B), D)
    used = np.zeros(C, bool)
    for c in range(C):
        den, num = D(0.0), [D(0.0)] * B
        for e in range(K):
            rw = D(r[c, e]) * D(w[e])
            den = den + rw
            for b in range(B):
                num[b] = num[b] + rw * D(mu[b, e])
        used[c] = den > 0
        if used[c]:
            for b in range(B):
                mbar[c, b] = D(0.1) * (num[b] / den)
    return mbar, used


def guess(weights, mu, response):
    """xrt_decompose_guess: (B, C) f64, or None where a pivot is not > 0."""
    mbar, used = mean_coefficients(weights, mu, response)
    C, B = mbar.shape
    N = [[D(0.0)] * 3 for _ in range(3)]
    for c in range(C):
        if not used[c]:
            continue
        for b in range(B):
            for b2 in range(b, B):
                N[b][b2] = N[b][b2] + mbar[c, b] * mbar[c, b2]
    out = np.zeros((B, C), D)
    for c in range(C):
        x, ok = solve(N, [mbar[c, b] for b in range(B)], B)
        if not ok:
            return None
        if used[c]:
            out[:, c] = x
    return out


def expected_at_zero(weights, response, gain):
    """y0 (C,): the channels at A = 0."""
    w = np.asarray(weights, F).reshape(-1)
    r = np.asarray(response, F).reshape(-1, w.size)
    y0 = np.zeros(r.shape[0], D)
    for c in range(r.shape[0]):
        for e in range(w.size):
            y0[c] = y0[c] + D(r[c, e]) * ((D(w[e]) * D(1.0)) * D(F(gain)))
    return y0


def decompose(channels, open, weights, mu, response, gain=1.0, counts=True, guess=None, max_iter=32, tol=1e-6,
              damping=0.0):
    """xrt_decompose: channels (C, ...) f32, open of a plane's shape or None, weights (K,), mu (B, K), response
    (C, K), guess (B, C) f64 or None; ((B, ...) f32, iters uint8 of a plane's shape)."""
    w, mu, r = tables(weights, mu, response)
    B, C, K = mu.shape[0], r.shape[0], w.size
    ch = np.ascontiguousarray(channels, F)
    assert ch.shape[0] == C
    shape = ch.shape[1:]
    y = ch.reshape(C, -1).astype(D)
    n = y.shape[1]
    gd = D(F(gain))
    tol, damping = D(tol), D(damping)
    with np.errstate(all="ignore"):
        if not counts:
            y = y * gd
        A = np.zeros((B, n), D)
        if guess is not None:
            G = np.asarray(guess, D).reshape(B, C)
            y0 = expected_at_zero(w, r, gain)
            p = np.empty((C, n), D)
            for c in range(C):
                t = (y[c] / y0[c]).astype(F)
                t = np.where(t >= F(1e-30), t, F(1e-30)).astype(F)
                p[c] = -(logf_ref.logf(t).astype(D))
            for b in range(B):
                for c in range(C):
                    A[b] = A[b] + G[b, c] * p[c]
        iters = np.zeros(n, np.int64)
        live = np.ones(n, bool) if open is None else np.asarray(open).reshape(-1) == 0
        masked = ~live
        idx = np.flatnonzero(live)
        for it in range(int(max_iter)):
            if idx.size == 0:
                break
            a, yy = A[:, idx], y[:, idx]
            ybar = [np.zeros(idx.size, D) for _ in range(C)]
            J = [[np.zeros(idx.size, D) for _ in range(B)] for _ in range(C)]
            for e in range(K):
                x = np.zeros(idx.size, D)
                for b in range(B):
                    x = x + D(mu[b, e]) * (a[b] * D(0.1))
                lam = (D(w[e]) * oracle.exp(-x)) * gd
                for c in range(C):
                    t = D(r[c, e]) * lam
                    ybar[c] = ybar[c] + t
                    for b in range(B):
                        J[c][b] = J[c][b] + D(mu[b, e]) * t
            g = [np.zeros(idx.size, D) for _ in range(3)]
            H = [[np.zeros(idx.size, D) for _ in range(3)] for _ in range(3)]
            for c in range(C):
                use = ybar[c] > 0
                q = yy[c] / ybar[c]
                rr = D(1.0) - q
                v = D(1.0) / ybar[c]
                for b in range(B):
                    g[b] = np.where(use, g[b] + J[c][b] * rr, g[b])
                for b in range(B):
                    for b2 in range(b, B):
                        H[b][b2] = np.where(use, H[b][b2] + (J[c][b] * J[c][b2]) * v, H[b][b2])
            for b in range(B):
                H[b][b] = H[b][b] + H[b][b] * damping
            xs, ok = solve(H, g, B)
            iters[idx[~ok]] = FAILED
            done = np.ones(idx.size, bool)
            for b in range(B):
                s = xs[b] / D(0.1)
                A[b, idx[ok]] = (a[b] + s)[ok]
                done &= np.abs(s) <= tol
            iters[idx[ok]] = it + 1
            idx = idx[ok & ~done]
        out = A.astype(F)
    out[:, masked] = F(0.0)
    iters[masked] = MASKED
    return out.reshape((B,) + tuple(shape)), iters.astype(np.uint8).reshape(shape)


def same(got, want):
    """Bit for bit where the reference is no NaN, NaN for NaN elsewhere."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != F or want.dtype != F:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and np.isnan(got[nan]).all())
