"""FDK reconstruction without a GPU: the refusals of both entry pairs
(made before the context is looked at, so a NULL context reaches them), the host
helpers against tests/fdk_ref.py bit for bit, the backprojection matrix checked
geometrically, the host restatements of the two kernels against the reference,
saveVolume / loadVolume, the ball scan's accuracy in the reference, and the
stand-alone sanitizer program over the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import camera_kit
import fdk_kit
import fdk_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import ROOT, bits

F = np.float32
D = np.float64
ARG = _abi.XRT_ERR_ARGUMENT


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------------------- refusals
def _filter_call(device, W=4, H=3, P=2, image="ok", weight=None, taps="ok", T=3, out="ok"):
    """xrt_fdk_filter (device=False) or xrt_fdk_filter_device on host addresses with a NULL context: a call
    that passes its checks ends at "context is NULL", which is XRT_ERR_ARGUMENT too -- so the error text
    tells the two apart."""
    lib = _abi.load()
    img = np.zeros((P, H, W), F) if isinstance(image, str) else image
    tp = np.ones(max(T, 1), F) if isinstance(taps, str) else taps
    o = np.zeros((P, H, W), F) if isinstance(out, str) else out
    keep = [img, tp, o, weight]
    if device:
        rc = lib.xrt_fdk_filter_device(None, W, H, P, _vp(img) if img is not None else None,
                                       _vp(weight) if weight is not None else None, _vp(tp) if tp is not None else None,
                                       T, _vp(o) if o is not None else None, None)
    else:
        rc = lib.xrt_fdk_filter(None, W, H, P, _fp(img) if img is not None else None,
                                _fp(weight) if weight is not None else None, _fp(tp) if tp is not None else None, T,
                                _fp(o) if o is not None else None)
    del keep
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_filter_refusals(device):
    rc, why = _filter_call(device)
    assert rc == ARG and "context is NULL" in why                     # everything else passed
    buf = np.zeros(4 * 3 * 2 + 8, F)
    cases = {
        "image is NULL": dict(image=None),
        "taps are NULL": dict(taps=None),
        "out is NULL": dict(out=None),
        "even": dict(T=4, taps=np.ones(4, F)),
        "outside": dict(T=0),
        "outside ": dict(T=2 * xrt.XRT_MAX_RAMP_WIDTH + 1, taps=np.ones(2 * xrt.XRT_MAX_RAMP_WIDTH + 1, F)),
        "is 0": dict(W=0),
        "is 0 ": dict(H=0),
        "is 0  ": dict(P=0),
        "above XRT_MAX_RAMP_WIDTH": dict(W=xrt.XRT_MAX_RAMP_WIDTH + 1, H=1, P=1,
                                         image=np.zeros((1, 1, xrt.XRT_MAX_RAMP_WIDTH + 1), F),
                                         out=np.zeros((1, 1, xrt.XRT_MAX_RAMP_WIDTH + 1), F)),
        "overlaps": dict(image=buf[:24].reshape(2, 3, 4), out=buf[8:32].reshape(2, 3, 4)),
        "overlaps ": dict(weight=buf[:12].reshape(3, 4), out=buf[8:32].reshape(2, 3, 4)),
        "overlaps  ": dict(taps=buf[29:32], out=buf[8:32].reshape(2, 3, 4)),
    }
    for text, kw in cases.items():
        rc, why = _filter_call(device, **kw)
        assert rc == ARG and text.strip() in why and "context" not in why, (text, why)
    # the widest row and the longest table pass the checks
    n = xrt.XRT_MAX_RAMP_WIDTH
    rc, why = _filter_call(device, W=n, H=1, P=1, image=np.zeros((1, 1, n), F), out=np.zeros((1, 1, n), F), T=2 * n - 1,
                           taps=np.ones(2 * n - 1, F))
    assert "context is NULL" in why
    # a tap that is not finite: the host form reads its taps, the device form cannot
    for bad in (np.nan, np.inf, -np.inf):
        rc, why = _filter_call(device, taps=np.array([1.0, bad, 1.0], F))
        assert rc == ARG and ("context is NULL" in why if device else "not finite" in why), (bad, why)


def _bp_call(device, W=4, H=3, P=2, proj="ok", mats="ok", dims=(5, 4, 3), slabs=(0, 3), scale=1.0, vol="ok"):
    lib = _abi.load()
    pj = np.zeros((P, H, W), F) if isinstance(proj, str) else proj
    m = np.ones((max(P, 1), 12), D) if isinstance(mats, str) else mats
    d = np.array(dims, np.uint32) if dims is not None else None
    v = np.zeros(5 * 4 * 3, F) if isinstance(vol, str) else vol
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if d is not None else None
    if device:
        rc = lib.xrt_backproject_device(None, W, H, P, _vp(pj) if pj is not None else None,
                                        _vp(m) if m is not None else None, dp, slabs[0], slabs[1], scale, 0,
                                        _vp(v) if v is not None else None, None)
    else:
        rc = lib.xrt_backproject(None, W, H, P, _fp(pj) if pj is not None else None,
                                 m.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if m is not None else None, dp,
                                 slabs[0], slabs[1], scale, 0, _fp(v) if v is not None else None)
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_backproject_refusals(device):
    rc, why = _bp_call(device)
    assert rc == ARG and "context is NULL" in why
    rc, why = _bp_call(device, slabs=(2, 2))                           # (an empty slab passes the checks as well)
    assert rc == ARG and "context is NULL" in why
    buf = np.zeros(200, F)
    mats_in_volume = np.ones((2, 12), D)
    cases = {
        "projections are NULL": dict(proj=None),
        "matrices are NULL": dict(mats=None),
        "dims is NULL": dict(dims=None),
        "volume is NULL": dict(vol=None),
        "is 0": dict(W=0),
        "is 0 ": dict(H=0),
        "is 0  ": dict(P=0),
        "65535": dict(P=65536, proj=np.zeros(8, F)),
        "2^40 pixels": dict(W=2 ** 31 - 1, H=2 ** 31 - 1, proj=np.zeros(8, F)),
        "2^31 - 1": dict(W=2 ** 31, proj=np.zeros(8, F)),
        "1 to 2048": dict(dims=(0, 4, 3)),
        "1 to 2048 ": dict(dims=(5, 2049, 3)),
        "1 to 2048  ": dict(dims=(5, 4, 0), slabs=(0, 0)),
        "slab range": dict(slabs=(2, 1)),
        "slab range ": dict(slabs=(0, 4)),
        "scale": dict(scale=float("nan")),
        "scale ": dict(scale=float("inf")),
        "overlaps": dict(proj=buf[:24].reshape(2, 3, 4), vol=buf[20:80]),
        "overlaps ": dict(mats=mats_in_volume, vol=mats_in_volume.view(F)[4:64]),
    }
    for text, kw in cases.items():
        rc, why = _bp_call(device, **kw)
        assert rc == ARG and text.strip() in why and "context" not in why, (text, why)
    for bad in (np.nan, np.inf):
        m = np.ones((2, 12), D)
        m[1, 7] = bad
        rc, why = _bp_call(device, mats=m)
        assert rc == ARG and ("context is NULL" in why if device else "not finite" in why), (bad, why)


# ------------------------------------------------------------------------------- helpers
@pytest.mark.parametrize("window", [xrt.XRT_RAMP_RAMLAK, xrt.XRT_RAMP_HANN])
def test_ramp_filter_equals_the_reference(window):
    for n in (1, 3, 5, 127, 513, 2 * xrt.XRT_MAX_RAMP_WIDTH - 1):
        got, want = xrt.ramp_filter(n, window), fdk_ref.ramp_filter(n, window)
        assert np.array_equal(bits(got), bits(want)), (n, window)
    g = xrt.ramp_filter(9, xrt.XRT_RAMP_RAMLAK)
    assert g[4] == F(0.25) and g[2] == 0 and g[6] == 0 and g[3] == g[5] == F(-1.0 / np.pi ** 2)
    for n in (0, 2, 2 * xrt.XRT_MAX_RAMP_WIDTH + 1):
        with pytest.raises(xrt.XrtError):
            xrt.ramp_filter(n, window)
    with pytest.raises(xrt.XrtError):
        xrt.ramp_filter(3, 2)


def _cameras(W, H):
    base = fdk_ref.turntable_camera(0.3, fdk_kit.SOD, fdk_kit.SDD, 0.4)
    yield "plain", base
    for name in camera_kit.NAMES:
        yield name, camera_kit.general_camera(base, (0.0, 0.0, 0.0), W, H, **camera_kit.CASES[name])


@pytest.mark.parametrize("W,H", [(1, 1), (7, 13), (64, 33)])
def test_weights_and_scale_equal_the_reference(W, H):
    for name, c13 in _cameras(W, H):
        cam = camera_kit.as_camera(c13, W, H)
        assert np.array_equal(bits(xrt.fdk_weights(cam)), bits(fdk_ref.fdk_weights(c13, W, H))), name
        for axis_point, P in (((0, 0, 0), 36), ((1.5, -2.0, 0.25), 7)):
            assert xrt.fdk_scale(cam, axis_point, P) == fdk_ref.fdk_scale(c13, axis_point, P), name
    plain = fdk_ref.turntable_camera(0.0, 100.0, 150.0, 0.4)
    w = xrt.fdk_weights(camera_kit.as_camera(plain, 64, 64))
    assert w.max() <= 1.0 and w[31, 31] == w[32, 32] and w[0, 0] < w[31, 31]         # the cosine, largest at the centre
    assert xrt.fdk_scale(camera_kit.as_camera(plain, 64, 64), (0, 0, 0), 36) == pytest.approx(np.pi / 36 * (100 / 150) / 0.4, rel=1e-6)
    with pytest.raises(xrt.XrtError):
        xrt.fdk_scale(camera_kit.as_camera(plain, 64, 64), (0, 0, 0), 0)


def test_matrix_returns_the_voxel_through_the_pixel_formula():
    """The matrix's (row, col, c) of a voxel, put back through the render's pixel formula and S + c (pixel - S), is
    pose X: the inversion is not restated, only undone."""
    rng = np.random.default_rng(11)
    W, H = 48, 40
    origin, spacing = np.array([-3.0, 2.0, -1.5], F), np.array([0.25, 0.5, 0.75], F)
    pose = xrt.pose_rotation((0.3, -1.0, 0.5), 37.0, (1.0, 2.0, -0.5))
    pose[3] += F(0.75)
    for name, c13 in _cameras(W, H):
        cam = camera_kit.as_camera(c13, W, H)
        S = np.asarray(c13[:3], D)
        for q in (None, pose):
            A = xrt.backprojection_matrix(cam, origin, spacing, q)
            idx = rng.integers(0, 64, (200, 3)).astype(D)
            a, b, c = (A[:, :3] @ idx.T + A[:, 3:4])
            pix = fdk_ref.pixel_point(c13, W, H, b / c, a / c)
            back = S + c[:, None] * (pix - S)
            X = origin.astype(D) + (idx + 0.5) * spacing.astype(D)
            q34 = fdk_ref.pose34(q)
            want = X @ q34[:, :3].T + q34[:, 3]
            assert (np.linalg.norm(back - want, axis=1) <= 1e-9 * np.linalg.norm(want, axis=1)).all(), (name, q is not None)
            # the numpy inversion is the same matrix to rounding
            ref = fdk_ref.backprojection_matrix(c13, W, H, origin, spacing, q)
            assert np.allclose(A, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max()), name
    flat = camera_kit.as_camera(fdk_ref.turntable_camera(0.0, 100.0, 150.0, 0.4), W, H)
    flat.up[:] = list(flat.right)                                       # a singular M
    with pytest.raises(xrt.XrtError):
        xrt.backprojection_matrix(flat, origin, spacing)


# ------------------------------------------------------------------------------- the host restatements
@pytest.mark.parametrize("W,H", fdk_kit.FILTER_PLANES)
def test_host_filter_equals_the_reference(W, H):
    for P in fdk_kit.FILTER_STACKS:
        for T in fdk_kit.filter_tap_counts(W):
            for weighted in (False, True):
                a = fdk_kit.filter_image(W * 100 + H + T, P, H, W, specials=weighted)
                taps = fdk_kit.filter_taps(T, T)
                wt = fdk_kit.filter_weight(W, H, W) if weighted else None
                assert fdk_kit.same_bits(xrt.host_fdk_filter(a, taps, wt), fdk_ref.fdk_filter(a, taps, wt)), (P, T, weighted)


def test_filter_skips_the_pixels_outside_the_row():
    a = np.array([[1.0, 2.0, 4.0]], F)
    assert np.array_equal(xrt.host_fdk_filter(a, [1.0, 0.0, 0.0]), [[0.0, 1.0, 2.0]])      # taps[0] meets the pixel to the left
    assert np.array_equal(xrt.host_fdk_filter(a, [1.0, 1.0, 1.0]), [[3.0, 7.0, 6.0]])      # not replicated
    z = xrt.host_fdk_filter(np.array([[-0.0]], F), [1.0])
    assert bits(z)[0, 0] == 0                                                               # the sum starts at +0.0


@pytest.mark.parametrize("dims", fdk_kit.BP_DIMS)
def test_host_backprojector_equals_the_reference(dims):
    for (W, H), P in zip(fdk_kit.BP_PLANES, [1, 3, 17, 3]):
        proj = fdk_kit.projections(W + H, P, H, W)
        mats = fdk_kit.general_matrices(P, dims, W, H)
        want = fdk_ref.backproject(proj, mats, dims, 0.37)
        assert np.abs(want).max() > 0                                    # the grid is in view
        assert fdk_kit.same_bits(xrt.host_backproject(proj, mats, dims, 0.37), want), (W, H, P)


def test_host_backprojector_edges_slabs_and_accumulation():
    W, H = 7, 5
    mats, dims = fdk_kit.edge_matrices(W, H)
    proj = fdk_kit.projections(3, 3, H, W)
    whole = fdk_ref.backproject(proj, mats, dims, 2.0)
    assert fdk_kit.same_bits(xrt.host_backproject(proj, mats, dims, 2.0), whole)
    first = fdk_ref.backproject(proj[:1], mats[:1], dims, 1.0)
    assert np.array_equal(first[0, 1:H + 1, 1:W + 1], proj[0])          # on the pixel centres: the pixels
    assert not first[0, 0].any() and not first[0, :, 0].any()           # col = -1 or row = -1: outside
    assert not first[0, H + 1:].any() and not first[0, :, W + 1:].any() # col = W, W + 1: outside
    assert not first[1].any()                                           # c = 0
    nan = fdk_kit.projections(4, 3, H, W, nan_plane=1)
    assert fdk_kit.same_bits(xrt.host_backproject(nan, mats, dims, 1.0), fdk_ref.backproject(nan, mats, dims, 1.0))
    for slabs in ((0, 1), (1, 2), (2, 2)):
        got = xrt.host_backproject(proj, mats, dims, 2.0, slabs=slabs)
        assert got.shape[0] == slabs[1] - slabs[0] and fdk_kit.same_bits(got, whole[slabs[0]:slabs[1]])
    half = fdk_ref.backproject(proj[:2], mats[:2], dims, 2.0)
    both = fdk_ref.backproject(proj[2:], mats[2:], dims, 2.0, volume=half, accumulate=True)
    got = xrt.host_backproject(proj[2:], mats[2:], dims, 2.0, volume=xrt.host_backproject(proj[:2], mats[:2], dims, 2.0),
                               accumulate=True)
    assert fdk_kit.same_bits(got, both)


# ------------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("posed", [False, True], ids=["turning-camera", "posed-object"])
def test_ball_scan_reconstructs_the_ball(posed):
    """36 analytic projections of a ball of mu = 1, radius 4 at (3, -2, 1) into 32^3 voxels of 0.5, all in the
    reference.  Measured: mean 0.99970, inner voxels 0.9973 .. 1.0028, centroid 0.0061 off (both forms)."""
    fdk_kit.check_ball(fdk_kit.scan_reference(posed))


def test_ball_scan_through_the_host_restatements():
    """The same scan through the library's helpers and host restatements: bit-equal to the reference fed the
    library's matrices."""
    proj, cams, _ = fdk_kit.scan(False)
    W, H = fdk_kit.SCAN_W, fdk_kit.SCAN_H
    cs = [camera_kit.as_camera(c, W, H) for c in cams]
    mats = np.stack([xrt.backprojection_matrix(c, fdk_kit.SCAN_ORIGIN, fdk_kit.SCAN_SPACING) for c in cs])
    taps = xrt.ramp_filter(2 * W - 1)
    filtered = np.stack([xrt.host_fdk_filter(proj[p], taps, xrt.fdk_weights(cs[p])) for p in range(len(cs))])
    vol = xrt.host_backproject(filtered, mats, fdk_kit.SCAN_DIMS, xrt.fdk_scale(cs[0], fdk_kit.SCAN_AXIS_POINT, len(cs)))
    assert np.array_equal(bits(vol), bits(fdk_kit.scan_reference(False, matrices=mats)))
    fdk_kit.check_ball(vol)


# ------------------------------------------------------------------------------- volumes and the CLI
def test_save_volume_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    vol = rng.normal(0.0, 1.0, (3, 5, 7)).astype(F)
    vol[0, 0, :4] = [np.nan, np.inf, -0.0, 1e-42]
    spacing, origin = np.array([0.1, 0.25, 1.0 / 3.0], F), np.array([-1.7, 2.0 / 3.0, 1e-3], F)
    path = str(tmp_path / "v.mhd")
    xrt.save_volume(path, vol, spacing, origin)
    assert os.path.getsize(tmp_path / "v.raw") == vol.size * 4
    back, spc, org = xrt.load_volume(path)
    assert back.dtype == F and np.array_equal(bits(back), bits(vol))
    assert np.array_equal(bits(spc), bits(spacing)) and np.array_equal(bits(org), bits(origin))
    head = open(path).read()
    assert "ElementType = MET_FLOAT" in head and "CompressedData = False" in head and "ElementDataFile = v.raw" in head
    for bad_path, kw in ((str(tmp_path / "v.raw"), {}), (str(tmp_path / "none" / "v.mhd"), {}), (path, dict(spacing=0.0))):
        with pytest.raises(xrt.XrtError):
            xrt.save_volume(bad_path, vol, kw.get("spacing", spacing), origin)


def test_cli_refuses_reconstruct_without_a_scan(tmp_path):
    """--reconstruct is refused where --sinogram is: before anything is loaded."""
    exe = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
    for args in (["--turntable", "24"], ["--log-projection", "80"], [], ["--turntable", "24:y:0", "--log-projection", "80"]):
        r = subprocess.run([exe, "-i", "none.obj", *args, "--reconstruct", "x.mhd"], capture_output=True, text=True,
                           cwd=tmp_path, timeout=120)
        assert r.returncode == 1 and "--reconstruct needs" in r.stderr and "Loading" not in r.stdout, r.stderr
    for value in ("x.raw", "x.mhd:0", "x.mhd:4096", "x.mhd:8:8"):
        r = subprocess.run([exe, "-i", "none.obj", "--turntable", "24", "--log-projection", "80", "--reconstruct", value],
                           capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert r.returncode == 1 and "--reconstruct FILE.mhd[:N]" in r.stderr, (value, r.stderr)


# ------------------------------------------------------------------------------- the sanitizer program
def test_host_code_under_sanitizers(tmp_path):
    """tools/fdk_san.cpp: a stand-alone program over csrc/xrt_fdk_host.inc (the checks, the helpers, the two
    restatements over exact-size buffers) with AddressSanitizer and UBSan.  Nothing is loaded into Python."""
    from test_pose_cpu import _sanitizer_runtime
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "fdk_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "fdk_san.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "fdk_san: OK" in r.stdout, out[-3000:]
