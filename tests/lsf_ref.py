"""The detector response's reference (include/xrt.h): a separable line-spread
function over an image, in numpy -- f64, one tap at a time in index order, np.clip indices
(the edge pixels replicated), cast to f32 after each pass.  The product of two f32 values is
exact in f64, so adding one product at a time here rounds as the device's fused chain does."""
import numpy as np

from oracle import oracle

F = np.float32


def _pass(plane, h, axis):
    """sum_k h[k] * plane[clip(i + k - r)] along `axis`: the sum starts as the k = 0 product."""
    h = np.asarray(h, F).reshape(-1)
    n = plane.shape[axis]
    r = (h.size - 1) // 2
    at = np.arange(n)
    acc = None
    with np.errstate(all="ignore"):
        for k in range(h.size):
            v = np.take(plane, np.clip(at + k - r, 0, n - 1), axis=axis).astype(np.float64)
            term = np.float64(h[k]) * v
            acc = term if acc is None else acc + term
        return acc.astype(F)


def apply(image, hx, hy=None):
    """(out f32, u8) of an (H, W) image or a (P, H, W) stack; hy None: hx on both axes."""
    a = np.asarray(image, F)
    assert a.ndim in (2, 3)
    hy = hx if hy is None else hy
    tmp = _pass(a, hx, a.ndim - 1)
    out = _pass(tmp, hy, a.ndim - 2)
    return out, oracle.lut_u8_array(out.reshape(-1)).reshape(out.shape)


def gaussian(sigma, taps):
    """xrt_lsf_gaussian restated: f64 values (not yet rounded to f32) and their f32 rounding."""
    r = (taps - 1) // 2
    g = np.exp(-0.5 * ((np.arange(taps, dtype=np.float64) - r) / np.float64(sigma)) ** 2)
    s = np.float64(0.0)
    for v in g:
        s = s + v
    return g / s, (g / s).astype(F)


def same(got, want):
    """Bit for bit where the reference is no NaN, NaN for NaN elsewhere; the count of NaNs."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False, 0
    if got.dtype != F:
        return bool(np.array_equal(got, want)), 0
    nan = np.isnan(want)
    ok = np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and bool(np.isnan(got[nan]).all())
    return bool(ok), int(np.count_nonzero(nan))


def plane(seed, W, H, P=None):
    """Seeded finite f32 in [-10, 90] with planted 0, -0.0, 80 and isolated spikes."""
    rng = np.random.default_rng(seed)
    shape = (H, W) if P is None else (P, H, W)
    a = rng.uniform(-10.0, 90.0, shape).astype(F)
    flat = a.reshape(-1)
    k = rng.integers(0, 23, flat.size)
    flat[k == 1] = F(0.0)
    flat[k == 2] = F(-0.0)
    flat[k == 3] = F(80.0)
    flat[k == 4] *= F(1e4)                              # spikes
    flat[k == 5] = F(1e-41)                             # a denormal
    assert np.isfinite(a).all()
    return a


def taps(seed, n):
    """Asymmetric random taps (a symmetric table would hide a flipped loop), roughly normalised."""
    rng = np.random.default_rng(1000 + seed)
    h = rng.uniform(-0.3, 1.0, n)
    return (h / np.abs(h).sum()).astype(F) if n > 1 else np.array([0.75], F)
