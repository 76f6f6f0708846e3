"""TV-regularised SIRT without a GPU: the refusals of the four entry pairs (made
before the context is looked at, so a NULL context reaches them), the host restatements of the
gradient, the sum of squares, the descent and the solver against tests/tv_ref.py bit for bit, the
gradient's properties in the reference (a constant volume, the sum of the gradient, a
directional derivative), the noisy few-view ball scan with and without TV, the CLI's refusals
and the stand-alone sanitizer program over the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fdk_kit
import sirt_kit
import tv_kit
import tv_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import ROOT, bits

F = np.float32
D = np.float64
ARG = _abi.XRT_ERR_ARGUMENT
INF = float("inf")
NAN = float("nan")


def _fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _vp(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _u32p(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _pick(value, default):
    return default if isinstance(value, str) else value


def _refused(call, passing, cases):
    """Every passing call ends at "context is NULL" (XRT_ERR_ARGUMENT too: the text tells them apart), every case
    at its own text before the context is looked at."""
    for kw in passing:
        rc, why = call(**kw)
        assert rc == ARG and "context is NULL" in why, (kw, why)
    for text, kw in cases.items():
        rc, why = call(**kw)
        assert rc == ARG and text.strip() in why and "context" not in why, (text, why)


# ------------------------------------------------------------------------------- refusals
def _gradient_call(device, vol="ok", dims=(5, 3, 2), eps=1e-8, out="ok"):
    lib = _abi.load()
    v, o = _pick(vol, np.zeros(30, F)), _pick(out, np.zeros(30, F))
    d = None if dims is None else np.array(dims, np.uint32)
    if device:
        rc = lib.xrt_tv_gradient_device(None, _vp(v), _u32p(d), eps, _vp(o), None)
    else:
        rc = lib.xrt_tv_gradient(None, _fp(v), _u32p(d), eps, _fp(o))
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_tv_gradient_refusals(device):
    buf = np.zeros(64, F)
    _refused(lambda **kw: _gradient_call(device, **kw), [{}, dict(eps=1e-300), dict(eps=1e300), dict(dims=(1, 1, 1))], {
        "volume is NULL": dict(vol=None),
        "dims is NULL": dict(dims=None),
        "out is NULL": dict(out=None),
        "1 to 2048": dict(dims=(0, 3, 2)),
        "1 to 2048 ": dict(dims=(5, 3, 2049)),
        "eps": dict(eps=0.0),
        "eps ": dict(eps=-1.0),
        "eps  ": dict(eps=INF),
        "eps   ": dict(eps=NAN),
        "overlaps": dict(vol=buf[:30], out=buf[29:59]),
        "overlaps ": dict(vol=buf[10:40], out=buf[10:40]),
    })


def _sumsq_call(device, n=8, a="ok", b=None, out="ok"):
    lib = _abi.load()
    x, o = _pick(a, np.zeros(8, F)), _pick(out, np.zeros(1, D))
    if device:
        rc = lib.xrt_volume_sumsq_device(None, n, _vp(x), _vp(b), _vp(o), None)
    else:
        rc = lib.xrt_volume_sumsq(None, n, _fp(x), _fp(b), _dp(o))
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_volume_sumsq_refusals(device):
    buf = np.zeros(8, D)
    _refused(lambda **kw: _sumsq_call(device, **kw), [{}, dict(b=np.zeros(8, F)), dict(n=1)], {
        "a is NULL": dict(a=None),
        "out is NULL": dict(out=None),
        "n is 0": dict(n=0),
        "2^33": dict(n=2 ** 33 + 1),
        "overlaps": dict(a=buf.view(F)[:8], out=buf[3:4]),
        "overlaps ": dict(b=buf.view(F)[8:16], out=buf[4:5]),
    })


def _descend_call(device, vol="ok", dims=(5, 3, 2), eps=1e-8, steps=2, length=0.5, lo=0.0, hi=1.0):
    lib = _abi.load()
    v = _pick(vol, np.zeros(30, F))
    d = None if dims is None else np.array(dims, np.uint32)
    if device:
        rc = lib.xrt_tv_descend_device(None, _vp(v), _u32p(d), eps, steps, length, lo, hi, None)
    else:
        rc = lib.xrt_tv_descend(None, _fp(v), _u32p(d), eps, steps, length, lo, hi)
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_tv_descend_refusals(device):
    _refused(lambda **kw: _descend_call(device, **kw),
             [{}, dict(steps=0), dict(length=0.0), dict(lo=-INF, hi=INF), dict(lo=0.5, hi=0.5)], {
        "volume is NULL": dict(vol=None),
        "dims is NULL": dict(dims=None),
        "1 to 2048": dict(dims=(5, 0, 2)),
        "eps": dict(eps=0.0),
        "eps ": dict(eps=NAN),
        "length": dict(length=-1.0),
        "length ": dict(length=INF),
        "length  ": dict(length=NAN),
        "NaN": dict(lo=NAN),
        "NaN ": dict(hi=NAN),
        "above hi": dict(lo=1.0, hi=0.5),
    })


def _sirt_tv_call(device, tv="ok", K=2, S=2, P=4, proj="ok", mats="ok", vol="ok", relax=1.0, lo=0.0, hi=INF):
    lib = _abi.load()
    b = _pick(proj, np.zeros(max(P, 1) * 12, F))
    m = _pick(mats, np.tile(sirt_kit.small_scan()[1][0].reshape(12), (max(P, 1), 1)))
    d, s = np.array((5, 4, 3), np.uint32), np.ones(3, F)
    v = _pick(vol, np.zeros(60, F))
    params = _abi.TvParams(*_pick(tv, (3, 0.2, 1.0, 1e-8))) if tv is not None else None
    ref = ctypes.byref(params) if params is not None else None
    if device:
        rc = lib.xrt_sirt_tv_device(None, 4, 3, P, _vp(b), _dp(m), _u32p(d), _fp(s), K, S, relax, lo, hi, ref, _vp(v), None)
    else:
        rc = lib.xrt_sirt_tv(None, 4, 3, P, _fp(b), _dp(m), _u32p(d), _fp(s), K, S, relax, lo, hi, ref, _fp(v))
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_sirt_tv_refusals(device):
    """xrt_sirt's own refusals reach the new entries unchanged; the TV parameters are checked behind them, and not
    at all without steps."""
    buf = np.zeros(200, F)
    singular = np.tile(sirt_kit.small_scan()[1][0].reshape(12), (4, 1))
    singular[2, 8:11] = singular[2, 4:7]
    singular[2, 0:3] = singular[2, 4:7]
    passing = [{}, dict(tv=None), dict(tv=(0, NAN, 0.0, -1.0)), dict(tv=(1, 0.0, 1.0, 1e-300)), dict(tv=(7, 3.0, 1e-9, 5.0))]
    _refused(lambda **kw: _sirt_tv_call(device, **kw), passing, {
        "alpha": dict(tv=(3, -0.1, 1.0, 1e-8)),
        "alpha ": dict(tv=(3, INF, 1.0, 1e-8)),
        "alpha  ": dict(tv=(3, NAN, 1.0, 1e-8)),
        "reduction": dict(tv=(3, 0.2, 0.0, 1e-8)),
        "reduction ": dict(tv=(3, 0.2, 1.5, 1e-8)),
        "reduction  ": dict(tv=(3, 0.2, NAN, 1e-8)),
        "eps": dict(tv=(3, 0.2, 1.0, 0.0)),
        "eps ": dict(tv=(3, 0.2, 1.0, INF)),
        "eps  ": dict(tv=(3, 0.2, 1.0, NAN)),
        "projections are NULL": dict(proj=None),
        "matrices are NULL": dict(mats=None),
        "volume is NULL": dict(vol=None),
        "iterations is 0": dict(K=0),
        "subsets": dict(S=5),
        "relax": dict(relax=NAN),
        "above hi": dict(lo=2.0, hi=1.0),
        "overlaps": dict(proj=buf[:48], vol=buf[40:100]),
        "no ray matrix": dict(mats=singular),
    })


# ------------------------------------------------------------------------------- the gradient, bit for bit
@pytest.mark.parametrize("dims", tv_kit.GRIDS)
def test_host_gradient_equals_the_reference(dims):
    for specials in (False, True):
        vol = tv_kit.volume(sum(dims), dims, specials)
        for eps in tv_kit.EPSILONS:
            want = tv_ref.gradient(vol, eps)
            assert fdk_kit.same_bits(xrt.host_tv_gradient(vol, eps), want), (dims, specials, eps)
            if not specials and max(dims) > 1:
                assert np.abs(want).max() > 0
    assert not bits(tv_ref.gradient(np.full((1, 1, 1), 3.0, F))).any()           # one voxel: +0.0


def test_host_gradient_about_the_tile():
    """The grids of the GPU test's tile cases: the host form does not tile, the kernel is compared on these."""
    assert min(tv_kit.tile_extent()) >= 2 and len(set(tv_kit.tile_grids())) == 10
    for dims in tv_kit.tile_grids():
        vol = tv_kit.volume(sum(dims), dims, specials=True)
        assert fdk_kit.same_bits(xrt.host_tv_gradient(vol, 1e-8), tv_ref.gradient(vol, 1e-8)), dims


# ------------------------------------------------------------------------------- the gradient's properties
def test_constant_volume_has_no_gradient():
    for dims in tv_kit.GRIDS:
        for value in (0.0, 0.75, -3.0):
            for eps in tv_kit.EPSILONS:
                g = tv_ref.gradient(np.full(dims[::-1], value, F), eps, narrow=False)
                assert not g.view(np.uint64).any(), (dims, value, eps)          # +0.0 everywhere


def test_gradient_sums_to_rounding():
    """Every quotient enters the sum of g once with each sign -- qx(p) in g(p) and, as bx, in g(p + x), or, on the
    upper border, not at all since it is 0 there --, so the exact sum of the exact g is 0.  What is left is the
    rounding of g's five additions a voxel: each rounds a partial sum of at most 6 quotients of magnitude at most
    1, an error of at most 6 * 2^-53; then the f64 sum of the N values over the array, each of magnitude at most
    6, which math.fsum rounds once.  The bound: N * 5 * 6 * 2^-53 + 6 N 2^-53 = 36 N 2^-53."""
    import math
    for dims in tv_kit.GRIDS + [(9, 8, 7)]:
        for eps in (1e-8, 1e-2, 1.0):
            g = tv_ref.gradient(tv_kit.volume(5, dims), eps, narrow=False)
            total = abs(math.fsum(g.ravel()))
            bound = 36.0 * g.size * 2.0 ** -53
            assert total <= bound, (dims, eps, total, bound)


# Measured with tv_ref alone: over the 8 random directions below on the 4 x 3 x 2 grid with
# eps = 1e-2 and h = 1e-4, the central difference of TV over the f32 volumes x +- h u (h u is added in f64 and
# narrowed, so the direction actually taken is ((x + h u) - (x - h u)) / 2h) deviates from <g, u>, g in f64 before the
# narrowing, by at most 1.183e-6.  That is the difference's own h^2 term -- 1.183e-4 at h = 1e-3, 1.18e-8 at 1e-5 --,
# not rounding.  The assert is four times the measured figure.
DIRECTIONAL_DEVIATION = 1.183e-6


def test_directional_derivative():
    dims, eps, h = (4, 3, 2), 1e-2, 1e-4
    x = tv_kit.volume(2, dims)
    g = tv_ref.gradient(x, eps, narrow=False)
    rng = np.random.default_rng(8)
    worst = 0.0
    for _ in range(8):
        u = rng.normal(0.0, 1.0, x.shape)
        up, down = (x.astype(D) + h * u).astype(F), (x.astype(D) - h * u).astype(F)
        taken = (up.astype(D) - down.astype(D)) / (2.0 * h)                    # the direction after the narrowing
        slope = (tv_ref.tv(up, eps) - tv_ref.tv(down, eps)) / (2.0 * h)
        worst = max(worst, abs(slope - float((g * taken).sum())))
    print(f"directional derivative: the largest deviation is {worst:.3e}")
    assert worst <= 4.0 * DIRECTIONAL_DEVIATION, worst
    assert np.abs(g).max() > 0.1                                                 # (against a gradient of that size)


# ------------------------------------------------------------------------------- the sum, the descent, the solver
@pytest.mark.parametrize("n", tv_kit.SUMSQ_LENGTHS)
def test_host_sumsq_equals_the_reference(n):
    a, b = tv_kit.sumsq_vectors(n)
    for with_b in (False, True):
        want = tv_kit.sumsq_reference(n, with_b)
        assert tv_kit.same_double(xrt.host_volume_sumsq(a, b if with_b else None), want), (n, with_b)
        exact = float(np.sum((a.astype(D) - (b.astype(D) if with_b else 0.0)) ** 2))
        assert abs(want - exact) <= 1e-12 * exact                                 # it is the sum, in another order
    if n == 1:
        assert tv_kit.same_double(tv_ref.sumsq(a), D(a[0]) * D(a[0]))             # m == 1: w[0] itself


def test_sumsq_special_values():
    for vals in ([np.nan], [np.inf, 1.0], [-0.0], [3e38, 3e38], [1e-30, 1e-30]):
        a = np.array(vals, F)
        assert tv_kit.same_double(xrt.host_volume_sumsq(a), tv_ref.sumsq(a)), vals
    a = np.array([np.inf, 1.0, np.nan], F)
    assert np.isnan(xrt.host_volume_sumsq(a, a))


@pytest.mark.parametrize("dims", tv_kit.DESCEND_GRIDS)
def test_host_descend_equals_the_reference(dims):
    vol = tv_kit.descend_volume(dims)
    args = (tv_kit.DESCEND_STEPS, tv_kit.DESCEND_LENGTH, 1e-8, tv_kit.DESCEND_LO, tv_kit.DESCEND_HI)
    want = tv_ref.descend(vol, *args)
    assert (want == tv_kit.DESCEND_LO).any() and ((want == tv_kit.DESCEND_HI).any() or dims[0] < 16)
    assert ((want > tv_kit.DESCEND_LO) & (want < tv_kit.DESCEND_HI)).any()
    assert fdk_kit.same_bits(xrt.host_tv_descend(vol, *args), want)
    free = tv_ref.descend(vol, 3, 0.7)
    assert fdk_kit.same_bits(xrt.host_tv_descend(vol, 3, 0.7), free)
    assert tv_ref.tv(free, 1e-8) < tv_ref.tv(vol, 1e-8)                           # it descends


def test_host_descend_leaves_a_constant_volume_and_a_zero_length():
    flat = np.full((3, 9, 67), 0.75, F)
    assert np.array_equal(bits(xrt.host_tv_descend(flat, 3, 0.7)), bits(flat))    # G = 0: nothing moves
    assert np.array_equal(bits(tv_ref.descend(flat, 3, 0.7)), bits(flat))
    vol = tv_kit.volume(4, (67, 9, 3))
    assert np.array_equal(bits(xrt.host_tv_descend(vol, 3, 0.0)), bits(vol))      # c = 0
    assert np.array_equal(bits(tv_ref.descend(vol, 3, 0.0)), bits(vol))
    special = tv_kit.volume(4, (67, 9, 3), specials=True)                         # G is NaN: gn > 0 is false
    assert fdk_kit.same_bits(xrt.host_tv_descend(special, 2, 0.5), special)
    assert fdk_kit.same_bits(tv_ref.descend(special, 2, 0.5), special)


@pytest.mark.parametrize("subsets", [1, 3])
def test_host_sirt_tv_equals_the_reference(subsets):
    """K = 3 over 8 projections of 16 x 12 into 9 x 8 x 7, four descent steps an iteration, alpha falling."""
    proj, A, spacing = sirt_kit.small_scan()
    got = xrt.host_sirt(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, subsets, relax=0.9, lo=0.0, tv=tv_kit.SMALL_TV)
    want = tv_kit.small_reference(subsets)
    assert fdk_kit.same_bits(got, want) and not np.array_equal(want, sirt_kit.small_reference(subsets))


def test_host_sirt_tv_without_steps_is_sirt():
    proj, A, spacing = sirt_kit.small_scan()
    plain = xrt.host_sirt(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, 3, relax=0.9, lo=0.0)
    none = xrt.host_sirt(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, 3, relax=0.9, lo=0.0, tv=(0, 0.2, 1.0, 1e-8))
    assert np.array_equal(bits(none), bits(plain)) and np.array_equal(bits(plain), bits(sirt_kit.small_reference(3)))


# ------------------------------------------------------------------------------- does it denoise?
# Measured in the reference (tv_ref + sirt_ref): the 12-view ball scan under photon noise of gain 500
# on exp(-0.25 p), 30 iterations from zeros with lo = 0.  Plain SIRT: inner standard deviation 0.06454, outer RMS
# 0.02017, RMS against the voxelised ball 0.05617, inner mean 1.01935.  With tv = (10, 0.2, 1, 1e-8): 0.01851 (0.287
# of plain), 0.01259, 0.05303 and 1.01369.
DENOISE_SHARE = 0.5
DENOISE_MEAN_BOUND = 0.03                                   # tests/test_sirt_cpu.py's BALL_MEAN_BOUND


def check_denoised(plain, smooth):
    p, s = tv_kit.noisy_figures(plain), tv_kit.noisy_figures(smooth)
    for name, f in (("plain SIRT", p), ("with TV", s)):
        print(f"{name}: inner std {f[0]:.5f}, inner mean {f[1]:.5f}, outer RMS {f[2]:.5f}, RMS against the ball {f[3]:.5f}")
    assert s[0] <= DENOISE_SHARE * p[0], (s[0], p[0])
    assert s[3] <= p[3], (s[3], p[3])
    assert abs(s[1] - 1.0) <= DENOISE_MEAN_BOUND, s[1]


def test_tv_denoises_the_few_view_ball_scan():
    """The volumes held to the bounds are the library's (xrt_host_sirt[_tv], the kernels' arithmetic on the host),
    bit-equal to the reference's."""
    proj, A = tv_kit.noisy_scan()
    assert proj.dtype == F and np.isfinite(proj).all()
    args = (proj, A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING, sirt_kit.FEW_K)
    plain, smooth = xrt.host_sirt(*args), xrt.host_sirt(*args, tv=tv_kit.BALL_TV)
    assert np.array_equal(bits(plain), bits(tv_kit.noisy_reference(False)))
    assert np.array_equal(bits(smooth), bits(tv_kit.noisy_reference(True)))
    check_denoised(plain, smooth)
    assert smooth.min() >= 0.0


# ------------------------------------------------------------------------------- the CLI and the sanitizer program
def test_cli_refuses_tv_without_sirt(tmp_path):
    exe = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
    base = [exe, "-i", "none.obj", "--turntable", "24:z", "--log-projection", "80", "--reconstruct", "x.mhd"]
    r = subprocess.run(base + ["--tv", "5"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 1 and "--tv needs --sirt" in r.stderr and "Loading" not in r.stdout, r.stderr
    for value in ("0", "x", "5:-1", "5:nan", "5:0.2:0", "5:0.2:1.5", "5:0.2:1:0", "5:0.2:1:1e-8:3", ""):
        r = subprocess.run(base + ["--sirt", "3", "--tv", value], capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert r.returncode == 1 and "--tv STEPS[:ALPHA[:REDUCTION[:EPS]]]" in r.stderr, (value, r.stderr)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert "--tv STEPS" in r.stdout + r.stderr and "flattens" in r.stdout + r.stderr


def test_host_code_under_sanitizers(tmp_path):
    """tools/tv_san.cpp: a stand-alone program over csrc/xrt_tv_host.inc (the checks and the four restatements over
    exact-size buffers) with AddressSanitizer and UBSan.  Nothing is loaded into Python."""
    from test_pose_cpu import _sanitizer_runtime
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "tv_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "tv_san.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "tv_san: OK" in r.stdout, out[-3000:]
