"""The photon noise's reference (include/xrt.h): xrt_photon_noise restated in numpy --
Philox4x32-10, the word's uniform, the sequential search below a mean of 64 and, from there on, the
AS241 PPND7 normal deviate with the second-order Cornish-Fisher term.  Every f64 and f32 operation is
rounded on its own (numpy cannot fuse); sqrt and / are IEEE-correct.  exp is libm's, one call a
distinct mean (math.exp; numpy's own exp may differ from glibc's in the last place), which xrt_exp
restates (tests/test_abi.py), and logf is tests/logf_ref.py's.  The constants are the contract's
literals."""
import math

import numpy as np

import logf_ref

F = np.float32
U = np.uint32
U64 = np.uint64

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
A = (3.3871327179, 50.434271938, 159.29113202, 59.109374720)
B = (None, 17.895169469, 78.757757664, 67.187563600)
C = (1.4234372777, 2.7568153900, 1.3067284816, 0.17023821103)
D = (None, 0.73700164250, 0.12021132975)
SMALL = 64.0
CAP = 255
MASK = U64(0xFFFFFFFF)

# (counter, key, words): the known answers published with Random123 for philox4x32-10
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """The four output words of Philox4x32-10 for arrays (or scalars) of counter and key words."""
    c = [np.atleast_1d(np.asarray(v, U64)) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = U64(int(k0) & 0xFFFFFFFF), U64(int(k1) & 0xFFFFFFFF)
    for rnd in range(10):
        p0, p1 = U64(M0) * c[0], U64(M1) * c[2]                     # 32 x 32 -> 64 bits: no wrap
        c = [(p1 >> U64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> U64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + U64(W0)) & MASK, (k1 + U64(W1)) & MASK       # (after the last round: unused)
    return [v.astype(U) for v in c]


def words(seed, first_index, n):
    """The random word of each of n pixels from global index first_index on: word g & 3 of the counter g >> 2."""
    seed, first_index = int(seed), int(first_index)
    j0, j1 = first_index >> 2, (first_index + n - 1) >> 2
    j = np.arange(j1 - j0 + 1, dtype=U64) + U64(j0)
    w = np.stack(philox4x32_10(j & MASK, j >> U64(32), 0, 0, seed & 0xFFFFFFFF, seed >> 32), axis=1).reshape(-1)
    skip = first_index & 3
    return np.ascontiguousarray(w[skip:skip + n])


def uniform_from_word(w):
    return (np.asarray(w, U).astype(np.float64) + 0.5) * 2.0 ** -32


def normal_from_word(w):
    """AS241 PPND7 at u = (w + 0.5) 2^-32, its third branch left out (unreachable: t >= 2^-33)."""
    u = uniform_from_word(w)
    q = u - 0.5
    with np.errstate(all="ignore"):
        r = 0.180625 - q * q
        num = ((A[3] * r + A[2]) * r + A[1]) * r + A[0]
        den = ((B[3] * r + B[2]) * r + B[1]) * r + 1.0
        centre = (q * num) / den
        t = np.where(q < 0, u, 1.0 - u)
        r = np.sqrt(-logf_ref.logf(t.astype(F)).astype(np.float64)) - 1.6
        num = ((C[3] * r + C[2]) * r + C[1]) * r + C[0]
        den = (D[2] * r + D[1]) * r + 1.0
        tail = num / den
        tail = np.where(q < 0, -tail, tail)
    return np.where(np.abs(q) <= 0.425, centre, tail)


def _exp_neg(lam):
    """libm's exp(-lam), one call a distinct value."""
    vals, inv = np.unique(lam, return_inverse=True)
    return np.array([math.exp(-float(v)) for v in vals], np.float64)[inv].reshape(lam.shape)


def poisson_from_word(lam, w):
    """N as f64 for f64 means lam and words w: NaN for a NaN or negative mean, +inf for +inf."""
    lam = np.atleast_1d(np.asarray(lam, np.float64))
    w = np.atleast_1d(np.asarray(w, U))
    lam, w = np.broadcast_arrays(lam, w)
    out = np.full(lam.shape, np.nan, np.float64)
    u = uniform_from_word(w)
    with np.errstate(all="ignore"):
        small = (lam < SMALL) & ~(lam < 0)                          # (-0.0 is not below 0: it counts as 0)
        if small.any():
            l, us = lam[small], u[small]
            p = _exp_neg(l)
            s = p.copy()
            N = np.zeros(l.shape, np.float64)
            live = np.flatnonzero(us > s)
            step = 0
            while live.size and step < CAP:
                step += 1
                p[live] = (p[live] * l[live]) / float(step)
                s[live] = s[live] + p[live]
                N[live] = float(step)
                live = live[us[live] > s[live]]
            out[small] = N
        large = (lam >= SMALL) & np.isfinite(lam)
        if large.any():
            l = lam[large]
            z = normal_from_word(w[large])
            x = l + np.sqrt(l) * z + (z * z - 1.0) / 6.0
            v = np.floor(x + 0.5)
            out[large] = np.where(v > 0.0, v, 0.0)
        out[lam == np.inf] = np.inf
    return out


def photon_noise(image, gain, seed, counts=False, first_index=0):
    """xrt_photon_noise over an array of any shape, flat: pixel i has the global index first_index + i."""
    a = np.ascontiguousarray(image, F)
    with np.errstate(all="ignore"):
        lam_f = (a.reshape(-1) * F(gain)).astype(F)
        assert lam_f.dtype == F
        N = poisson_from_word(lam_f.astype(np.float64), words(seed, first_index, a.size)).astype(F)
        out = N if counts else (N / F(gain)).astype(F)
    return out.reshape(a.shape)


def same(got, want):
    """Bit for bit where the reference is no NaN, NaN for NaN elsewhere."""
    return logf_ref.same(got, want)[0]


# every class of mean the contract names (as f32 image values under a gain of 1)
LAMBDAS = np.array([-1.0, -0.0, 0.0, 1e-45, 0.5, 63.999996, 64.0, 100.0, 1e4, 2.0 ** 24 + 1, 3e38, np.inf, np.nan], F)


def _crossings():
    """The words around both |q| = 0.425 crossings: u = 0.075 and u = 0.925."""
    out = []
    for u in (0.075, 0.925):
        w = int(u * 2.0 ** 32)
        out += list(range(w - 4, w + 5))
    return out


def word_set():
    """The words the hooks and the device probe are compared on."""
    edge = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1] + _crossings(), dtype=np.uint64)
    stride = np.arange(0, 1 << 32, 4099, dtype=np.uint64)
    return np.concatenate([edge, stride]).astype(U)
