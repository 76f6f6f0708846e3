"""Material decomposition without a GPU: the kernel's pixel function compiled for the host
(xrt_host_decompose) bit for bit against tests/decompose_ref.py, iters included; xrt_decompose_guess against
the reference and numpy's pseudo-inverse; the closed-form anchor; the round trip's and the reconstruction's
bounds measured on the reference; the argument errors that need no device, the CLI's, k_decompose's
code-object metadata and a stand-alone sanitizer build of the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import decompose_kit as kit
import decompose_ref as ref
import detector_ref
import fdk_ref
import simpleraytracing_amd as xrt
import volume_kit
from simpleraytracing_amd import _abi
from conftest import DRAGON, ROOT, bits
from test_materials_cpu import _render_kernel_metadata
from test_pose_cpu import _sanitizer_runtime

F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")

# Bounds, each four times (the pseudo-inverse: ten times) what the reference itself shows here; DESIGN 10.14
# records the measurements.
PINV_BOUND = 3.6e-12                                    # measured 3.6e-13 of the largest entry, cond(mbar) up to 402
CLOSED_FORM_BOUND = 2.4e-7                              # measured 5.9e-8 of max(|A|, 1): half an f32 ulp
ROUND_TRIP_ULPS = {2: 37.2, 4: 21.6}                    # measured 9.3 and 5.4 f32 ulps of the largest path (9.91)
RECON_BOUND = [4.8e-6, 1.24e-6]                         # measured 1.2e-6 and 3.1e-7 of the volume's largest value


def check(got, want, what):
    assert ref.same(got[0], want[0]), (what, np.argwhere(bits(got[0]) != bits(want[0]))[:8])
    assert np.array_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:8], got[1].reshape(-1)[:16],
                                             want[1].reshape(-1)[:16])


def test_symbols_are_declared_and_bound():
    """The entries and the constants in xrt.h, the hook in xrt_debug.h only; every one exported and bound;
    the ABI version stays."""
    pub = open(os.path.join(ROOT, "include", "xrt.h")).read()
    dbg = open(os.path.join(ROOT, "include", "xrt_debug.h")).read()
    for name in ("xrt_decompose(", "xrt_decompose_device(", "xrt_decompose_guess(", "XRT_MAX_BASIS 3",
                 "XRT_DECOMPOSE_MASKED 254", "XRT_DECOMPOSE_FAILED 255"):
        assert name in pub, name
    assert "xrt_host_decompose(" in dbg and "xrt_host_decompose" not in pub
    lib = _abi.load()
    for name in ("xrt_decompose", "xrt_decompose_device", "xrt_decompose_guess", "xrt_host_decompose"):
        assert name in _abi.XRT_SYMBOLS and getattr(lib, name) is not None
    assert lib.xrt_abi_version() == 5 and "#define XRT_ABI_VERSION 5" in pub
    assert (_abi.XRT_MAX_BASIS, _abi.XRT_DECOMPOSE_MASKED, _abi.XRT_DECOMPOSE_FAILED) == (3, 254, 255)
    for name in ("decompose", "host_decompose", "decompose_guess", "XRT_MAX_BASIS", "XRT_DECOMPOSE_FAILED"):
        assert name in xrt.__all__
    assert hasattr(xrt.Context, "decompose") and hasattr(xrt.Context, "decompose_device")


def _call(lib, entry, n, ch, opn, w, mu, B, K, r, C, gain, mode, guess, it, tol, damp, out, iters):
    def fp(a):
        return None if a is None else a.ctypes.data_as(_abi._fp)

    def vp(a):
        return None if a is None else ctypes.c_void_p(a.ctypes.data)
    g = None if guess is None else guess.ctypes.data_as(_abi._dp)
    if entry == "device":
        return lib.xrt_decompose_device(None, n, vp(ch), vp(opn), fp(w), fp(mu), B, K, fp(r), C, gain, mode, g, it, tol, damp,
                                        vp(out), vp(iters), None)
    u16 = None if opn is None else opn.ctypes.data_as(_abi._u16p)
    u8 = None if iters is None else iters.ctypes.data_as(_abi._u8p)
    if entry == "host":
        return lib.xrt_decompose(None, n, fp(ch), u16, fp(w), fp(mu), B, K, fp(r), C, gain, mode, g, it, tol, damp, fp(out), u8)
    return lib.xrt_host_decompose(n, fp(ch), u16, fp(w), fp(mu), B, K, fp(r), C, gain, mode, g, it, tol, damp, fp(out), u8)


@pytest.mark.parametrize("entry", ["host", "device", "hook"])
def test_argument_errors_without_a_device(entry):
    """Every check comes before the context is looked at: with a NULL context each is XRT_ERR_ARGUMENT with a
    message that names the argument (the entries), or XRT_ERR_ARGUMENT (the hook)."""
    lib = _abi.load()
    buf = np.zeros(128, F)                                  # channels: 2 planes of 12 at [0, 24); room beside them
    ch, out = buf[:24], buf[48:72]
    opn = np.zeros(12, np.uint16)
    iters = np.zeros(12, np.uint8)
    w, mu, r = np.array([1.0, 2.0], F), np.array([[0.1, 0.2], [0.0, 0.3]], F), np.array([[1.0, 0.0], [0.0, 1.0]], F)
    guess = np.array([[1.0, 0.0], [0.0, 1.0]])
    CO, IN = _abi.XRT_DETECT_COUNTS, _abi.XRT_DETECT_INTENSITY
    nan, inf = float("nan"), float("inf")
    good = dict(n=12, ch=ch, opn=opn, w=w, mu=mu, B=2, K=2, r=r, C=2, gain=1.0, mode=CO, guess=guess, it=32, tol=1e-6,
                damp=0.0, out=out, iters=iters)

    def bad(word, **change):
        args = dict(good, **change)
        assert _call(lib, entry, **args) == _abi.XRT_ERR_ARGUMENT, (word, change.keys())
        if entry != "hook":
            assert word.encode() in lib.xrt_last_error(None), (word, lib.xrt_last_error(None))

    bad("channels is NULL", ch=None)
    bad("weight is NULL", w=None)
    bad("mu is NULL", mu=None)
    bad("response is NULL", r=None)
    bad("out is NULL", out=None)
    bad("num_basis", B=0)
    bad("num_basis", B=4)
    bad("energy bins", K=0)
    bad("energy bins", K=33)
    for v in (0.0, -1.0, inf, nan):
        bad("weight", w=np.array([1.0, v], F))
        bad("gain", gain=v)
    for v in (-0.5, inf, nan):
        bad("coefficient", mu=np.array([[0.1, 0.2], [v, 0.3]], F))
        bad("response", r=np.array([[1.0, 0.0], [0.0, v]], F))
    bad("num_channels", C=0)
    bad("num_channels", C=9)
    bad("num_channels is below num_basis", C=1)
    bad("in_mode", mode=2)
    bad("in_mode", mode=-1)
    bad("max_iter", it=0)
    bad("max_iter", it=201)
    for v in (-1e-9, inf, nan):
        bad("tol", tol=v)
        bad("damping", damp=v)
    for v in (inf, -inf, nan):
        bad("guess", guess=np.array([[1.0, 0.0], [v, 1.0]]))
    bad("num_pixels", n=0)
    bad("workgroups", n=(2 ** 31 - 1) * 256 + 1)
    bad("workgroups", n=2 ** 63)
    bad("out overlaps channels", out=buf[0:24])
    bad("out overlaps channels", out=buf[23:47])            # the last count
    bad("out overlaps channels", ch=buf[71:95])             # the last line integral
    bad("out overlaps open", opn=buf[71:77].view(np.uint16))
    bad("iters overlaps channels", iters=buf[23:26].view(np.uint8))
    bad("iters overlaps channels", iters=buf[0:3].view(np.uint8))
    bad("iters overlaps open", iters=opn.view(np.uint8)[12:24])
    # arguments in order: the entries then fail on the context alone, the hook computes
    for ok in (dict(), dict(out=buf[24:48]), dict(opn=None), dict(iters=None), dict(guess=None), dict(mode=IN, gain=2.5),
               dict(it=1), dict(it=200, tol=0.0, damp=0.5), dict(iters=buf[24:27].view(np.uint8)),
               dict(r=np.array([[-0.0, 1.0], [2.0, 0.0]], F)), dict(B=1, C=1, guess=np.array([[1.0]]))):
        rc = _call(lib, entry, **dict(good, **ok))
        if entry == "hook":
            assert rc == _abi.XRT_OK, ok.keys()
        else:
            assert rc == _abi.XRT_ERR_ARGUMENT and b"context is NULL" in lib.xrt_last_error(None), ok.keys()
    with pytest.raises(ValueError):
        xrt.host_decompose(np.zeros((3, 5), F), None, w, mu, r)                   # three planes, two channels' response
    with pytest.raises(ValueError):
        xrt.host_decompose(np.zeros((2, 5), F), None, w, mu, np.ones((2, 3), F))
    with pytest.raises(ValueError):
        xrt.host_decompose(np.zeros((2, 5), F), np.zeros(4, np.uint16), w, mu, r)
    with pytest.raises(ValueError):
        xrt.host_decompose(np.zeros((2, 5), F), None, w, mu, r, guess=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        xrt.host_decompose(np.zeros((2, 5), F), None, w, mu, r, guess="zeros")
    with pytest.raises(xrt.XrtError):
        xrt.host_decompose(np.zeros((2, 5), F), None, w, mu, r, gain=0.0, guess=None)


def test_guess_argument_errors():
    """xrt_decompose_guess: XRT_ERR_ARGUMENT naming the argument; a table that cannot be separated is refused."""
    lib = _abi.load()
    w, mu, r = np.array([1.0, 2.0], F), np.array([[0.1, 0.2], [0.05, 0.3]], F), np.array([[1.0, 0.0], [0.0, 1.0]], F)
    out = np.zeros((2, 2))

    def call(w=w, mu=mu, B=2, K=2, r=r, C=2, out=out):
        def fp(a):
            return None if a is None else a.ctypes.data_as(_abi._fp)
        rc = lib.xrt_decompose_guess(fp(w), fp(mu), B, K, fp(r), C, None if out is None else out.ctypes.data_as(_abi._dp))
        return rc, lib.xrt_last_error(None)

    assert call()[0] == _abi.XRT_OK
    for word, change in [(b"guess is NULL", dict(out=None)), (b"weight is NULL", dict(w=None)), (b"mu is NULL", dict(mu=None)),
                         (b"response is NULL", dict(r=None)), (b"num_basis", dict(B=0)), (b"num_basis", dict(B=4)),
                         (b"energy bins", dict(K=0)), (b"num_channels", dict(C=9)), (b"below num_basis", dict(C=1)),
                         (b"coefficient", dict(mu=np.array([[0.1, -0.2], [0.0, 0.3]], F))),
                         (b"response", dict(r=np.array([[1.0, np.nan], [0.0, 1.0]], F))),
                         (b"not separable", dict(mu=np.array([[0.1, 0.2], [0.0, 0.0]], F))),
                         (b"not separable", dict(r=np.zeros((2, 2), F)))]:
        rc, msg = call(**change)
        assert rc == _abi.XRT_ERR_ARGUMENT and word in msg, (word, msg)
    with pytest.raises(xrt.XrtError) as e:
        xrt.decompose_guess(w, np.array([[0.1, 0.2], [0.0, 0.0]], F), r)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "separable" in str(e.value)


GRID = [(kit.SIZES[(i + j + B) % len(kit.SIZES)], B, C, K) for B in kit.BASES for i, C in enumerate(kit.channel_counts(B))
        for j, K in enumerate(kit.BINS)]


@pytest.mark.parametrize("shape,B,C,K", GRID, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_host_hook_equals_the_reference_on_crafted_planes(shape, B, C, K):
    """B in 1, 2, 3; C in B, 4, 5, 8; K in 1, 4, 5, 32 (every quad edge); both in_modes; guess NULL and given;
    a zero, a negative and a doubled count and masked pixels among the planes.  Tables that cannot be
    separated (K = 1 under two bases) fail their pivot on both sides alike."""
    w, mu = kit.table(B, K)
    r = kit.response(C, K)
    given = ref.guess(w, mu, r)
    for counts in (True, False):
        ch, opn, _ = kit.planes(shape, B, C, K, 3.0, counts)
        for guess in (None, given):
            if guess is None and given is None and not counts:
                continue
            got = xrt.host_decompose(ch, opn, w, mu, r, 3.0, counts, guess, 32, 1e-6, 0.0, True)
            want = ref.decompose(ch, opn, w, mu, r, 3.0, counts, guess, 32, 1e-6, 0.0)
            assert got[0].shape == (B,) + tuple(shape) and got[1].shape == tuple(shape)
            check(got, want, (counts, guess is not None))
            assert (got[0][:, opn != 0] == 0).all() and (got[1][opn != 0] == 254).all()
    ch, opn, _ = kit.planes(shape, B, C, K, 1.0, True)
    check(xrt.host_decompose(ch, None, w, mu, r, 1.0, True, None, 5, 0.0, 0.5, True),
          ref.decompose(ch, None, w, mu, r, 1.0, True, None, 5, 0.0, 0.5), "open NULL, tol 0, damping")
    only = xrt.host_decompose(ch, None, w, mu, r, 1.0, True, None, 5, 0.0, 0.5)             # without the iters plane
    assert ref.same(only, ref.decompose(ch, None, w, mu, r, 1.0, True, None, 5, 0.0, 0.5)[0])


def test_nan_zero_row_and_failing_pivot():
    """One NaN count from zeros: NaN outputs, and the status the contract's loop gives (max_iter when that is 1,
    FAILED otherwise).  A response row of zeros is left out.  A basis of zeros: iters 255, A as started."""
    B, C, K = 2, 4, 8
    w, mu = kit.table(B, K)
    r = kit.response(C, K)
    ch, _, _ = kit.planes((130,), B, C, K)
    ch[1, 64] = np.nan
    for max_iter in (1, 6):
        got = xrt.host_decompose(ch, None, w, mu, r, 1.0, True, None, max_iter, 1e-6, 0.0, True)
        check(got, ref.decompose(ch, None, w, mu, r, 1.0, True, None, max_iter, 1e-6, 0.0), max_iter)
        assert np.isnan(got[0][:, 64]).all() and np.isfinite(np.delete(got[0], 64, axis=1)).all()
        assert got[1][64] == (1 if max_iter == 1 else 255)
    r0 = r.copy()
    r0[2] = 0.0
    ch0 = detector_ref.spectral_detector(kit.paths((130,), B), None, w, mu, r0, 1.0, 0, False)
    got = xrt.host_decompose(ch0, None, w, mu, r0, 1.0, True, None, 32, 1e-6, 0.0, True)
    check(got, ref.decompose(ch0, None, w, mu, r0, 1.0, True, None, 32, 1e-6, 0.0), "zero row")
    assert (got[1] < 32).all() and not ch0[2].any()
    mu0 = mu.copy()
    mu0[1] = 0.0
    start = xrt.decompose_guess(w, mu, r)                   # (the separable table's: a start that is not zero)
    for guess in (None, start):
        got = xrt.host_decompose(ch, None, w, mu0, r, 1.0, True, guess, 32, 1e-6, 0.0, True)
        check(got, ref.decompose(ch, None, w, mu0, r, 1.0, True, guess, 32, 1e-6, 0.0), "zero basis")
        assert (got[1] == 255).all()
        if guess is None:
            assert not got[0].any()
            continue
        import logf_ref                                     # the start written out: guess @ -logf(max(y / y0, 1e-30))
        t = (ch.astype(np.float64) / ref.expected_at_zero(w, r, 1.0)[:, None]).astype(F)
        p = -logf_ref.logf(np.where(t >= F(1e-30), t, F(1e-30)).astype(F)).reshape(t.shape).astype(np.float64)
        A = np.zeros((B, ch.shape[1]))
        for b in range(B):
            for c in range(C):
                A[b] = A[b] + guess[b, c] * p[c]
        assert np.array_equal(bits(got[0]), bits(A.astype(F))) and got[0].any()


def test_one_thick_pixel_among_thin_ones():
    """From zeros the iteration advances about one attenuation length a step: a pixel of 250 in a wave of
    0.5 runs many more iterations than its neighbours, and tol = 0 many more than tol = 1e-6."""
    B, C, K = 2, 4, 8
    w, mu = kit.table(B, K)
    r = kit.windows(C, K)
    d = kit.thick_among_thin(B)
    ch = detector_ref.spectral_detector(d, None, w, mu, r, 1.0, 0, False)
    loose = ref.decompose(ch, None, w, mu, r, 1.0, True, None, 64, 1e-6)
    tight = ref.decompose(ch, None, w, mu, r, 1.0, True, None, 64, 0.0)
    wave = loose[1][64:128]
    print("iters of the thick lane", loose[1][70], "of its neighbours", np.unique(np.delete(wave, 6)), "tol 0", np.unique(tight[1]))
    assert loose[1][70] >= 2 * np.delete(wave, 6).max() and loose[1][70] < 64
    assert (tight[1] >= loose[1]).all() and (tight[1] > loose[1]).any()
    check(xrt.host_decompose(ch, None, w, mu, r, 1.0, True, None, 64, 1e-6, 0.0, True), loose, "tol 1e-6")
    check(xrt.host_decompose(ch, None, w, mu, r, 1.0, True, None, 64, 0.0, 0.0, True), tight, "tol 0")


def _separable():
    return [(B, C, K) for B in kit.BASES for C in kit.channel_counts(B) for K in kit.BINS if K >= max(B, 4) or B == 1]


def test_guess_equals_the_reference_and_the_pseudo_inverse():
    """xrt_decompose_guess bit for bit against the reference's restatement of the same elimination order, and
    within PINV_BOUND of numpy.linalg.pinv of the same mean coefficients, relative to its largest entry:
    that checks the order's sense, not its bits."""
    worst = 0.0
    for B, C, K in _separable():
        w, mu = kit.table(B, K)
        r = kit.response(C, K)
        got, want = xrt.decompose_guess(w, mu, r), ref.guess(w, mu, r)
        assert want is not None and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (B, C, K)
        mbar, used = ref.mean_coefficients(w, mu, r)
        assert used.all()
        pinv = np.linalg.pinv(mbar)
        worst = max(worst, float(np.max(np.abs(got - pinv)) / np.max(np.abs(pinv))))
    print("guess against pinv: worst relative difference", worst)
    assert worst <= PINV_BOUND
    r = kit.response(4, 8)
    r[1] = 0.0                                              # a channel without a denominator is left out
    w, mu = kit.table(2, 8)
    got = xrt.decompose_guess(w, mu, r)
    assert np.array_equal(got.view(np.uint64), ref.guess(w, mu, r).view(np.uint64)) and not got[:, 1].any()
    assert np.allclose(np.delete(got, 1, axis=1), np.linalg.pinv(np.delete(ref.mean_coefficients(w, mu, r)[0], 1, axis=0)),
                       rtol=1e-9)


def test_closed_form_anchor():
    """B = C = K = 1: the iteration converges to -ln(y / (r w gain)) / (0.1 mu), from zeros and from the
    guess (which is then 1 / (0.1 mu): the start is the answer in f32 precision)."""
    worst = 0.0
    for muv in (0.05, 0.2, 1.7):
        for wv, rv, gain in ((40.0, 1.0, 1.0), (3.5, 60.0, 25.0)):
            w, mu, r = np.array([wv], F), np.array([[muv]], F), np.array([[rv]], F)
            A = np.linspace(0.0, 200.0, 401).astype(F)
            ch = detector_ref.spectral_detector(A[None], None, w, mu, r, gain, 0, False, True)
            y = ch[0].astype(np.float64)
            closed = -np.log(y / (float(r[0, 0]) * float(w[0]) * float(F(gain)))) / (0.1 * float(mu[0, 0]))
            for guess in (None, xrt.decompose_guess(w, mu, r)):
                want = ref.decompose(ch, None, w, mu, r, gain, True, guess, 200, 1e-6)
                assert (want[1] < 200).all()
                dev = float(np.max(np.abs(want[0][0].astype(np.float64) - closed) / np.maximum(np.abs(closed), 1.0)))
                worst = max(worst, dev)
                got = xrt.host_decompose(ch, None, w, mu, r, gain, True, guess, 200, 1e-6, 0.0, True)
                check(got, want, (muv, wv, gain))
                assert np.max(np.abs(got[0][0].astype(np.float64) - closed) / np.maximum(np.abs(closed), 1.0)) <= CLOSED_FORM_BOUND
    print("closed form: the reference's largest deviation", worst)


@pytest.mark.parametrize("C", kit.ROUND_TRIP_WINDOWS)
def test_round_trip_bound_on_the_reference(C):
    """The two-label volume at 67 x 45 -> the detector (EXPECTED, COUNTS) -> the decomposition, all in the
    references: no pixel fails or runs 32 iterations, and the recovered planes lie within ROUND_TRIP_ULPS
    (four times what this prints) of the traced ones.  The host hook gives the reference's bits."""
    W, H = kit.ROUND_TRIP_SIZE
    paths = volume_kit.reference("shells2", "base", W, H)
    w, mu, r = kit.round_trip_tables(C)
    ch = detector_ref.spectral_detector(paths, None, w, mu, r, 1.0, 0, False, True)
    for guess in (None, ref.guess(w, mu, r)):
        want = ref.decompose(ch, None, w, mu, r, 1.0, True, guess, 32, 1e-6)
        assert (want[1] < 32).all(), np.unique(want[1])
        ulps = kit.round_trip_ulps(want[0], paths, np.ones((H, W), bool))
        print("round trip,", C, "windows:", ulps, "f32 ulps of the largest path", float(paths.max()), "iters", np.unique(want[1]))
        assert ulps <= ROUND_TRIP_ULPS[C]
        check(xrt.host_decompose(ch, None, w, mu, r, 1.0, True, guess, 32, 1e-6, 0.0, True), want, C)


def test_reconstruction_bound_on_the_reference():
    """24 views of a 32 x 32 detector into 16^3: FDK of the decomposed planes against FDK of the paths planes,
    all in the references; the largest voxel difference relative to the volume's largest value."""
    planes, cams = kit.recon_scan()
    w, mu, r = kit.round_trip_tables(4)
    ch = detector_ref.spectral_detector(planes.reshape(2, -1), None, w, mu, r, 1.0, 0, False, True)
    out, iters = ref.decompose(ch, None, w, mu, r, 1.0, True, ref.guess(w, mu, r), 32, 1e-6)
    assert (iters < 32).all()
    out = out.reshape(planes.shape)
    for b in range(2):
        args = (cams, None, kit.RECON_W, kit.RECON_H, kit.RECON_DIMS, kit.RECON_ORIGIN, kit.RECON_SPACING, kit.RECON_AXIS_POINT)
        va, vb = fdk_ref.fdk(planes[b], *args), fdk_ref.fdk(out[b], *args)
        rel = float(np.max(np.abs(va.astype(np.float64) - vb)) / np.max(np.abs(va)))
        print("reconstruction, basis", b, "relative difference", rel, "largest value", float(va.max()))
        assert va.max() > 0.5 and rel <= RECON_BOUND[b]


def test_k_decompose_metadata():
    """k_decompose in the gfx950 code object: nine instantiations (1, 2, 3 basis materials, channel bound 2, 4
    or 8), none with scratch -- which a dynamically indexed register array would need --, a spilled vector
    or scalar register or LDS; the argument segment within 4096 bytes.  (profiles/decompose/resources.txt
    has every figure.)"""
    meta = _render_kernel_metadata()
    dec = {k: v for k, v in meta.items() if "k_decompose" in k}
    assert len(dec) == 9, sorted(dec)
    for name, f in dec.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] == 0 and f["kernarg_segment_size"] <= 4096, (name, f)
        assert f["vgpr_count"] <= 256, (name, f)            # at least two waves a SIMD


def test_cli_help_lists_the_option():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--decompose BASIS[:ITER[:TOL]]" in r.stderr


def _cli_files(tmp_path):
    (tmp_path / "beam.txt").write_text("40 25.5 14.5\n0.2059 0.1037 0.08\n")
    (tmp_path / "det.txt").write_text("1 1 0\n0 0 1\n")
    (tmp_path / "one.txt").write_text("30 60 90\n")
    (tmp_path / "basis.txt").write_text("# water, then bone\n0.2059 0.1037 0.08\n0.9 0.3 0.2 # denser\n")
    (tmp_path / "two.txt").write_text("1 2\n")
    (tmp_path / "neg.txt").write_text("1 -2 3\n")
    (tmp_path / "word.txt").write_text("1 x 3\n")
    (tmp_path / "empty.txt").write_text("# nothing\n\n")
    (tmp_path / "four.txt").write_text("1 1 1\n" * 4)


DET = ["--paths", "--spectrum", "beam.txt", "--detector", "det.txt"]


@pytest.mark.parametrize("args,word", [
    (["--paths", "--spectrum", "beam.txt", "--decompose", "basis.txt"], "--detector"),
    (["--decompose", "basis.txt"], "--detector"),
    (DET + ["--decompose", "missing.txt"], "cannot read"),
    (DET + ["--decompose", "two.txt"], "bins"),
    (DET + ["--decompose", "neg.txt"], "not a coefficient"),
    (DET + ["--decompose", "word.txt"], "not a coefficient"),
    (DET + ["--decompose", "empty.txt"], "no basis material"),
    (DET + ["--decompose", "four.txt"], "basis materials"),
    (DET + ["--decompose", "basis.txt:0"], "ITER"),
    (DET + ["--decompose", "basis.txt:201"], "ITER"),
    (DET + ["--decompose", "basis.txt:8:-1"], "TOL"),
    (DET + ["--decompose", "basis.txt:8:nan"], "TOL"),
    (DET + ["--decompose", "basis.txt:8:1e-3:4"], "--decompose"),
    (["--paths", "--spectrum", "beam.txt", "--detector", "one.txt", "--decompose", "basis.txt"], "channels"),
    (DET + ["--decompose", "basis.txt", "-g", "2"], "-g"),
])
def test_cli_errors(tmp_path, args, word):
    """Each is an error before any device is opened: exit 1, stderr 'ERROR: ...' naming the option."""
    _cli_files(tmp_path)
    r = subprocess.run([EXE, "-s", "16", "16", "-i", DRAGON] + args, capture_output=True, text=True, cwd=tmp_path,
                       timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("ERROR: --decompose") and word in r.stderr and "xrt_create" not in r.stderr, r.stderr


def test_host_code_under_sanitizers(tmp_path):
    """tools/decompose_san.cpp: a stand-alone program over csrc/xrt_decompose_host.inc (the checks, the table,
    the guess, the pass over every quad edge and channel count against the contract written out pixel by
    pixel; B = 3, C = 8, K = 32; zero, negative and NaN counts, a masked pixel, a failing pivot) with
    AddressSanitizer and UBSan.  Nothing is loaded into Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "decompose_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "decompose_san.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "decompose_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
