"""The line-integral projections' reference (include/xrt.h): glibc 2.35's logf
restated in numpy -- f64 operations, each rounded on its own (numpy cannot fuse), which equals
libm on every input (tools/check_logf.c) --, xrt_log_projection's pixel function in separately
rounded f32 operations, and the sinogram reorder.  The constants are the contract's literals."""
import numpy as np

F = np.float32
U = np.uint32

LN2 = float.fromhex("0x1.62e42fefa39efp-1")
A0 = float.fromhex("-0x1.00ea348b88334p-2")
A1 = float.fromhex("0x1.5575b0be00b6ap-2")
A2 = float.fromhex("-0x1.ffffef20a4123p-2")
_TAB = [
    ("0x1.661ec79f8f3bep+0", "-0x1.57bf7808caadep-2"), ("0x1.571ed4aaf883dp+0", "-0x1.2bef0a7c06ddbp-2"),
    ("0x1.49539f0f010b0p+0", "-0x1.01eae7f513a67p-2"), ("0x1.3c995b0b80385p+0", "-0x1.b31d8a68224e9p-3"),
    ("0x1.30d190c8864a5p+0", "-0x1.6574f0ac07758p-3"), ("0x1.25e227b0b8ea0p+0", "-0x1.1aa2bc79c8100p-3"),
    ("0x1.1bb4a4a1a343fp+0", "-0x1.a4e76ce8c0e5ep-4"), ("0x1.12358f08ae5bap+0", "-0x1.1973c5a611cccp-4"),
    ("0x1.0953f419900a7p+0", "-0x1.252f438e10c1ep-5"), ("0x1p+0", "0x0p+0"),
    ("0x1.e608cfd9a47acp-1", "0x1.aa5aa5df25984p-5"), ("0x1.ca4b31f026aa0p-1", "0x1.c5e53aa362eb4p-4"),
    ("0x1.b2036576afce6p-1", "0x1.526e57720db08p-3"), ("0x1.9c2d163a1aa2dp-1", "0x1.bc2860d224770p-3"),
    ("0x1.886e6037841edp-1", "0x1.1058bc8a07ee1p-2"), ("0x1.767dcf5534862p-1", "0x1.4043057b6ee09p-2"),
]
INVC = np.array([float.fromhex(a) for a, _ in _TAB], np.float64)
LOGC = np.array([float.fromhex(b) for _, b in _TAB], np.float64)


def logf(x):
    """glibc logf of an f32 array, bit for bit (a NaN's sign and payload aside)."""
    x = np.ascontiguousarray(x, F)
    bits = x.view(U)
    with np.errstate(all="ignore"):
        odd = (bits - U(0x00800000)) >= U(0x7F800000 - 0x00800000)      # u32 arithmetic wraps
        scaled = (x * F(2.0 ** 23)).view(U) - U(23 << 23)
        ix = np.where(odd, scaled, bits)
        tmp = ix - U(0x3F330000)
        i = (tmp >> U(19)) % U(16)
        k = tmp.view(np.int32) >> 23                                    # arithmetic
        iz = ix - (tmp & U(0xFF800000))
        z = iz.view(F).astype(np.float64)
        r = z * INVC[i] - 1.0
        y0 = LOGC[i] + k.astype(np.float64) * LN2
        r2 = r * r
        y = A1 * r + A2
        y = A0 * r2 + y
        y = y * r2 + (y0 + r)
        out = y.astype(F)
    out = np.where(odd & (((bits & U(0x80000000)) != 0) | (bits * U(2) >= U(0xFF000000))), F(np.nan), out)
    out = np.where(odd & (bits == U(0x7F800000)), x, out)
    out = np.where(odd & (bits * U(2) == 0), F(-np.inf), out)
    out = np.where(bits == U(0x3F800000), F(0.0), out)
    return out.astype(F)


def pixels(image, flat=None, dark=None, flat_value=None, t_min=0.0):
    """xrt_log_projection's pixel function over an (H, W) image or a (P, H, W) stack (flat and dark: one
    (H, W) plane each, or None), in projection order; every step one f32 operation."""
    a = np.asarray(image, F)
    with np.errstate(all="ignore"):
        num = a - np.asarray(dark, F) if dark is not None else a
        if flat is not None:
            den = np.asarray(flat, F) - np.asarray(dark, F) if dark is not None else np.asarray(flat, F)
        else:
            den = F(flat_value) - np.asarray(dark, F) if dark is not None else F(flat_value)
        t = (num / den).astype(F)
        assert t.dtype == F
        if t_min > 0:
            t = np.where(t < F(t_min), F(t_min), t)                    # a NaN compares false and stays
        return (F(0.0) - logf(t).reshape(t.shape)).astype(F)


def sinograms(planes):
    """(P, H, W) -> (H, P, W): one P x W sinogram per detector row."""
    planes = np.asarray(planes)
    if planes.ndim == 2:
        planes = planes[None]
    return np.ascontiguousarray(planes.transpose(1, 0, 2))


def apply(image, flat=None, dark=None, flat_value=None, t_min=0.0, sino=False):
    out = pixels(image, flat, dark, flat_value, t_min)
    return sinograms(out) if sino else out


def same(got, want):
    """Bit for bit where the reference is no NaN, NaN for NaN elsewhere; the count of NaNs."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != F or want.dtype != F:
        return False, 0
    nan = np.isnan(want)
    ok = np.array_equal(got.view(U)[~nan], want.view(U)[~nan]) and bool(np.isnan(got[nan]).all())
    return bool(ok), int(np.count_nonzero(nan))


SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xBF800000,
                     0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000, 0x3F7FFFFF,
                     0x3F800001], U).view(F)


def sweeps():
    """The inputs the restatement is compared on, as chunks of f32: a full mantissa period -- every float in
    [0x3F330000, 0x3FB30000): all 16 intervals and 1.0 --, a stride of 4099 over all 2^32 bit patterns, every
    64th subnormal, and the specials."""
    yield "period", np.arange(0x3F330000, 0x3FB30000, dtype=np.uint64).astype(U).view(F)
    yield "stride", np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(U).view(F)
    yield "subnormals", np.arange(0, 0x00800000, 64, dtype=np.uint64).astype(U).view(F)
    yield "specials", SPECIALS.copy()


def planes(seed, W, H, P=None, flat=True, dark=True):
    """Seeded inputs with image in (dark, flat] per pixel -- every transmission in (0, 1], every output
    finite: (image, flat plane or None, dark plane or None, flat_value)."""
    rng = np.random.default_rng(seed)
    shape = (H, W) if P is None else (P, H, W)
    d = rng.uniform(0.5, 2.0, (H, W)).astype(F) if dark else None
    f = rng.uniform(60.0, 90.0, (H, W)).astype(F) if flat else None
    flat_value = F(80.0)
    lo = d if dark else F(0.0)
    hi = f if flat else flat_value
    u = rng.uniform(0.0, 1.0, shape).astype(F)
    u.reshape(-1)[rng.integers(0, u.size, max(u.size // 9, 1))] = F(1.0)       # I == flat: t = 1
    u.reshape(-1)[rng.integers(0, u.size, max(u.size // 9, 1))] = F(0.001)     # below t_min = 0.01
    image = (lo + (hi - lo) * u).astype(F)
    image = np.minimum(np.maximum(image, np.nextafter(np.broadcast_to(lo, shape).astype(F), F(np.inf))),
                       np.broadcast_to(hi, shape)).astype(F)
    return image, f, d, float(flat_value)
