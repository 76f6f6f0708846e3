"""OS-MLTR without a GPU: the refusals of the three entry pairs (made before
the context is looked at, so a NULL context reaches them), the host restatements of the
pixel stage, the fused backprojector and the solver against tests/mltr_ref.py bit for bit,
what the solver is for -- starved counts and a known background on sirt_kit's ball -- in
the reference, xrt_main's refusals around --mltr and the stand-alone sanitizer program
over the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mltr_kit
import mltr_ref
import sirt_kit
import sirt_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import ROOT
from mltr_kit import same

F = np.float32
D = np.float64
ARG = _abi.XRT_ERR_ARGUMENT
INF = float("inf")


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


# ------------------------------------------------------------------------------- refusals
def _pp_call(device, W=4, H=3, P=2, vol="ok", dims=(5, 4, 3), spacing="ok", rays="ok", counts="ok", flat="ok", bg=None,
             pairs="ok"):
    """xrt_poisson_project (device=False) or its _device form on host addresses with a NULL context: a call that
    passes its checks ends at "context is NULL", which is XRT_ERR_ARGUMENT too -- the error text tells them apart."""
    lib = _abi.load()
    v = _pick(vol, np.zeros(60, F))
    d = None if dims is None else np.array(dims, np.uint32)
    s = _pick(spacing, np.ones(3, F))
    r = _pick(rays, np.ones((max(P, 1), 12), D))
    n = max(P, 1) * max(H, 1) * max(W, 1)
    y, f = _pick(counts, np.zeros(min(n, 64), F)), _pick(flat, np.ones(12, F))
    o = _pick(pairs, np.zeros(min(2 * n, 64), D).view(F))
    if device:
        rc = lib.xrt_poisson_project_device(None, W, H, P, _vp(v), _u32p(d), _fp(s), _vp(r), _vp(y), _vp(f), _vp(bg), _vp(o),
                                            None)
    else:
        rc = lib.xrt_poisson_project(None, W, H, P, _fp(v), _u32p(d), _fp(s), _dp(r), _fp(y), _fp(f), _fp(bg), _fp(o))
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_poisson_project_refusals(device):
    rc, why = _pp_call(device)
    assert rc == ARG and "context is NULL" in why                     # everything else passed
    rc, why = _pp_call(device, bg=np.zeros(24, F))
    assert rc == ARG and "context is NULL" in why
    buf = np.zeros(400, D).view(F)
    rays_in_out = np.ones((2 + 12, 12), D)
    cases = {
        "volume is NULL": dict(vol=None),
        "dims is NULL": dict(dims=None),
        "spacing is NULL": dict(spacing=None),
        "ray matrices are NULL": dict(rays=None),
        "counts are NULL": dict(counts=None),
        "flat field is NULL": dict(flat=None),
        "pairs is NULL": dict(pairs=None),
        "aligned": dict(pairs=buf[1:49]),
        "is 0": dict(W=0),
        "is 0 ": dict(H=0),
        "is 0  ": dict(P=0),
        "65535": dict(P=65536),
        "2^40 pixels": dict(W=2 ** 31 - 1, H=2 ** 31 - 1),
        "2^31 - 1": dict(W=2 ** 31),
        "tiles": dict(W=2 ** 20, H=2 ** 20),
        "1 to 2048": dict(dims=(0, 4, 3)),
        "1 to 2048 ": dict(dims=(5, 2049, 3)),
        "spacing is not": dict(spacing=np.array([1, 0, 1], F)),
        "spacing is not ": dict(spacing=np.array([np.nan, 1, 1], F)),
        "overlaps": dict(vol=buf[:60], pairs=buf[50:98]),
        "overlaps ": dict(counts=buf[100:124], pairs=buf[120:168]),
        "overlaps  ": dict(flat=buf[200:212], pairs=buf[210:258]),
        "overlaps   ": dict(bg=buf[300:324], pairs=buf[320:368]),
        "overlaps    ": dict(rays=rays_in_out[:2], pairs=rays_in_out.reshape(-1).view(F)[4:52]),
    }
    for text, kw in cases.items():
        rc, why = _pp_call(device, **kw)
        assert rc == ARG and text.strip() in why and "context" not in why, (text, why)
    for bad in (np.nan, np.inf):                       # the host form reads its ray matrices, the device form cannot
        r = np.ones((2, 12), D)
        r[1, 7] = bad
        rc, why = _pp_call(device, rays=r)
        assert rc == ARG and ("context is NULL" in why if device else "not finite" in why), (bad, why)


def _bu_call(device, W=4, H=3, P=2, pairs="ok", mats="ok", dims=(5, 4, 3), relax=1.0, lo=0.0, hi=INF, vol="ok"):
    lib = _abi.load()
    n = max(P, 1) * max(H, 1) * max(W, 1)
    a = _pick(pairs, np.zeros(min(n, 64), D).view(F))
    m = _pick(mats, np.ones((max(P, 1), 12), D))
    d = None if dims is None else np.array(dims, np.uint32)
    v = _pick(vol, np.zeros(60, F))
    if device:
        rc = lib.xrt_backproject_update_device(None, W, H, P, _vp(a), _vp(m), _u32p(d), relax, lo, hi, _vp(v), None)
    else:
        rc = lib.xrt_backproject_update(None, W, H, P, _fp(a), _dp(m), _u32p(d), relax, lo, hi, _fp(v))
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_backproject_update_refusals(device):
    for kw in ({}, dict(lo=-INF, hi=INF), dict(lo=0.5, hi=0.5), dict(relax=-2.0)):
        rc, why = _bu_call(device, **kw)
        assert rc == ARG and "context is NULL" in why, (kw, why)
    buf = np.zeros(200, D).view(F)
    mats_in_vol = np.ones((2 + 4, 12), D)
    cases = {
        "pairs is NULL": dict(pairs=None),
        "matrices are NULL": dict(mats=None),
        "dims is NULL": dict(dims=None),
        "volume is NULL": dict(vol=None),
        "aligned": dict(pairs=buf[1:49]),
        "is 0": dict(W=0),
        "is 0 ": dict(H=0),
        "is 0  ": dict(P=0),
        "65535": dict(P=65536),
        "2^40 pixels": dict(W=2 ** 31 - 1, H=2 ** 31 - 1),
        "2^31 - 1": dict(H=2 ** 31),
        "1 to 2048": dict(dims=(5, 4, 0)),
        "1 to 2048 ": dict(dims=(2049, 4, 3)),
        "relax": dict(relax=float("nan")),
        "relax ": dict(relax=INF),
        "NaN": dict(lo=float("nan")),
        "NaN ": dict(hi=float("nan")),
        "above hi": dict(lo=1.0, hi=0.5),
        "overlaps": dict(pairs=buf[:48], vol=buf[40:100]),
        "overlaps ": dict(mats=mats_in_vol[:2], vol=mats_in_vol.reshape(-1).view(F)[40:100]),
    }
    for text, kw in cases.items():
        rc, why = _bu_call(device, **kw)
        assert rc == ARG and text.strip() in why and "context" not in why, (text, why)
    for bad in (np.nan, np.inf):                       # the host form reads its matrices, the device form cannot
        m = np.ones((2, 12), D)
        m[0, 3] = bad
        rc, why = _bu_call(device, mats=m)
        assert rc == ARG and ("context is NULL" in why if device else "not finite" in why), (bad, why)


def _mltr_call(device, W=4, H=3, P=4, counts="ok", flat="ok", bg=None, mats="ok", dims=(5, 4, 3), spacing="ok", K=2, S=2,
               relax=1.0, lo=0.0, hi=INF, tv=None, vol="ok"):
    lib = _abi.load()
    y = _pick(counts, np.zeros(max(P, 1) * 12, F))
    f = _pick(flat, np.ones(12, F))
    m = _pick(mats, np.tile(sirt_kit.small_scan()[1][0].reshape(12), (max(P, 1), 1)))
    d = None if dims is None else np.array(dims, np.uint32)
    s = _pick(spacing, np.ones(3, F))
    v = _pick(vol, np.zeros(60, F))
    params = None if tv is None else ctypes.byref(_abi.TvParams(*tv))
    if device:
        rc = lib.xrt_mltr_device(None, W, H, P, _vp(y), _vp(f), _vp(bg), _dp(m), _u32p(d), _fp(s), K, S, relax, lo, hi, params,
                                 _vp(v), None)
    else:
        rc = lib.xrt_mltr(None, W, H, P, _fp(y), _fp(f), _fp(bg), _dp(m), _u32p(d), _fp(s), K, S, relax, lo, hi, params, _fp(v))
    return rc, lib.xrt_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_mltr_refusals(device):
    for kw in ({}, dict(S=1), dict(S=4), dict(P=65, S=64, counts=np.zeros(65 * 12, F)), dict(lo=-INF),
               dict(bg=np.zeros(48, F)), dict(tv=(2, 0.2, 0.9, 1e-8)), dict(tv=(0, -1.0, 7.0, 0.0))):
        rc, why = _mltr_call(device, **kw)
        assert rc == ARG and "context is NULL" in why, (kw, why)
    buf = np.zeros(300, F)
    singular = np.tile(sirt_kit.small_scan()[1][0].reshape(12), (4, 1))
    singular[2, 8:11] = singular[2, 4:7]
    singular[2, 0:3] = singular[2, 4:7]
    not_finite = np.tile(sirt_kit.small_scan()[1][0].reshape(12), (4, 1))
    not_finite[3, 5] = np.nan
    mats_in_vol = np.ones((4 + 4, 12), D)
    mats_in_vol[:4] = not_finite[0]
    cases = {
        "counts are NULL": dict(counts=None),
        "flat field is NULL": dict(flat=None),
        "matrices are NULL": dict(mats=None),
        "dims is NULL": dict(dims=None),
        "spacing is NULL": dict(spacing=None),
        "volume is NULL": dict(vol=None),
        "is 0": dict(W=0),
        "is 0 ": dict(P=0),
        "65535": dict(P=65536),
        "tiles": dict(W=2 ** 20, H=2 ** 20),
        "1 to 2048": dict(dims=(5, 4, 2049)),
        "spacing is not": dict(spacing=np.array([1, 1, 0], F)),
        "iterations is 0": dict(K=0),
        "subsets": dict(S=0),
        "subsets ": dict(S=5),
        "subsets  ": dict(P=70, S=65, counts=np.zeros(70 * 12, F)),
        "relax": dict(relax=float("nan")),
        "NaN": dict(lo=float("nan")),
        "above hi": dict(lo=1.0, hi=0.5),
        "not finite": dict(mats=not_finite),
        "overlaps": dict(counts=buf[:48], vol=buf[40:100]),
        "overlaps ": dict(flat=buf[100:112], vol=buf[110:170]),
        "overlaps  ": dict(bg=buf[200:248], vol=buf[240:300]),
        "alpha": dict(tv=(1, -0.5, 0.9, 1e-8)),
        "reduction": dict(tv=(1, 0.2, 1.5, 1e-8)),
        "eps": dict(tv=(1, 0.2, 0.9, 0.0)),
        "no ray matrix": dict(mats=singular),
    }
    for text, kw in cases.items():
        rc, why = _mltr_call(device, **kw)
        assert rc == ARG and text.strip() in why and "context" not in why, (text, why)
    rc, why = _mltr_call(device, mats=mats_in_vol[:4], vol=mats_in_vol.reshape(-1).view(F)[90:150])
    assert rc == ARG and ("context is NULL" in why if device else "overlaps" in why), why   # (host buffers only)


# ------------------------------------------------------------------------------- the pixel stage
@pytest.mark.parametrize("name", list(mltr_kit.PIXEL_CASES))
def test_host_pixel_stage_equals_the_reference(name):
    vol, spacing, R, y, f, b, want = mltr_kit.pixel_case(name)
    same(xrt.host_poisson_project(vol, spacing, R, y, f, b), want, name)


def test_underflowing_expectation():
    """psi = 0 everywhere: without a background yh = 0 and every pair is zeros; with one, q = 0 and the pairs of
    finite counts are zeros too, of +0.0's bits."""
    for name in ("underflow-no-background", "underflow-background"):
        want = mltr_kit.pixel_case(name)[-1]
        assert not want.view(np.uint32).any(), name


def test_null_background_equals_a_zero_background():
    for name in ("stack3", "hand-faces-plain", "grid(67, 9, 3)-plane(67, 45)"):
        vol, spacing, R, y, f, _, _ = mltr_kit.pixel_case(name)
        none = mltr_ref.poisson_project(vol, spacing, R, y, f, None)
        for zero in (np.zeros_like(y), -np.zeros_like(y)):
            same(mltr_ref.poisson_project(vol, spacing, R, y, f, zero), none, (name, "reference"))
            same(xrt.host_poisson_project(vol, spacing, R, y, f, zero), none, (name, "host"))
        same(xrt.host_poisson_project(vol, spacing, R, y, f, None), none, (name, "host, NULL"))


def test_pixel_stage_formulas():
    """The reference against the formulas in plain f64 on one ray with a chord known by hand: the grid (5, 3, 2)
    of ones under sirt_kit's `inside` rays, where the line integral equals the length inside the grid."""
    R, (H, W) = sirt_kit.hand_rays()["inside"]
    vol = np.ones(sirt_kit.HAND_DIMS[::-1], F)
    L = np.zeros((1, H, W), D)
    l = sirt_ref.forward_project(vol, sirt_kit.HAND_SPACING, R, (H, W), narrow=False, lengths=L)
    assert np.allclose(l, L, rtol=1e-12) and (L > 0).all()
    y, f, b = np.full((1, H, W), 30.0, F), np.full((H, W), 100.0, F), np.full((1, H, W), 5.0, F)
    got = mltr_ref.poisson_project(vol, sirt_kit.HAND_SPACING, R, y, f, b).astype(D)
    psi = 100.0 * np.exp(-L)
    assert np.allclose(got[..., 0], psi - 30.0 * psi / (psi + 5.0), rtol=1e-6)
    assert np.allclose(got[..., 1], L * psi * psi / (psi + 5.0), rtol=1e-6)


# ------------------------------------------------------------------------------- the fused backprojector
@pytest.mark.parametrize("name", list(mltr_kit.UPDATE_CASES))
def test_host_backproject_update_equals_the_reference(name):
    pr, A, dims, start, relax, lo, hi, want = mltr_kit.update_case(name)
    same(xrt.host_backproject_update(pr, A, dims, start, relax, lo, hi), want, name)


def test_host_backproject_update_equals_its_composition():
    """xrt_host_backproject of each component, then xrt_host_volume_update."""
    for name in ("stack17", "edge(7, 13)", "grid(300, 2, 2)-plane(67, 45)"):
        pr, A, dims, start, relax, lo, hi, want = mltr_kit.update_case(name)
        num = xrt.host_backproject(np.ascontiguousarray(pr[..., 0]), A, dims)
        den = xrt.host_backproject(np.ascontiguousarray(pr[..., 1]), A, dims)
        same(xrt.host_volume_update(start, num, den, relax, lo, hi), want, name)


def test_unseen_voxels_keep_their_bits():
    """Under fdk_kit.edge_matrices the slab k = 1 has c <= 0 under the first two matrices; with those alone no plane
    sees it, den = 0 and the voxels stay as they are: NaN, +-inf and -0.0 included."""
    pr, A, dims, start, relax, lo, hi, _ = mltr_kit.update_case("edge(7, 13)")
    got = xrt.host_backproject_update(pr[:2], A[:2], dims, start, relax, lo, hi)
    assert np.array_equal(got[1].view(np.uint32), start[1].view(np.uint32))
    assert np.isnan(start[1]).any() and (start[1].view(np.uint32) == 0x80000000).any()
    same(got, mltr_ref.backproject_update(pr[:2], A[:2], dims, start, relax, lo, hi), "two matrices")


def test_values_land_exactly_on_the_bounds():
    pr, A, dims, start, relax, lo, hi, want = mltr_kit.update_case("landing")
    row = want[0, 3, 1:8]                               # voxels i = 1 .. 7 of a row land on pixels 0 .. 6
    assert row.tolist() == [0.0, 1.5, 0.0, 1.5, 0.25, 0.75, 0.0], row
    assert np.array_equal(want[1].view(np.uint32), start[1].view(np.uint32))         # c = 0: unseen


# ------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize("subsets", [1, 3])
@pytest.mark.parametrize("with_bg", [False, True])
def test_host_solver_equals_the_reference(subsets, with_bg):
    y, flat, bg, A, spacing = mltr_kit.small_scan(with_bg)
    got = xrt.host_mltr(y, flat, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, subsets, mltr_kit.SMALL_RELAX, 0.0,
                        background=bg)
    same(got, mltr_kit.small_reference(subsets, with_bg), (subsets, with_bg))
    assert float(got.max()) > 0.5                       # (it moved)


def test_host_solver_with_tv():
    y, flat, bg, A, spacing = mltr_kit.small_scan(True)
    args = (y, flat, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, 3, mltr_kit.SMALL_RELAX, 0.0)
    got = xrt.host_mltr(*args, tv=mltr_kit.SMALL_TV, background=bg)
    same(got, mltr_kit.small_reference(3, True, mltr_kit.SMALL_TV), "tv")
    assert not np.array_equal(got, mltr_kit.small_reference(3, True))
    same(xrt.host_mltr(*args, tv=(0, 0.2, 0.9, 1e-8), background=bg), mltr_kit.small_reference(3, True), "tv without steps")


def test_host_solver_on_the_larger_scan():
    y, flat, bg, A, spacing, dims = mltr_kit.large_scan()
    same(xrt.host_mltr(y, flat, A, dims, spacing, 2, 2, 1.0, 0.0, background=bg), mltr_kit.large_reference(), "large")


# ------------------------------------------------------------------------------- what it is for
def test_starved_counts_in_the_reference():
    """A flat field of 100 counts: many pixels count zero.  MLTR from zeros reaches the ball's level; SIRT on the
    clamped logarithm of the same counts, at the same iterations and subsets, stays far below it."""
    y, A = mltr_kit.starved_scan()
    zeros = int((y == 0).sum())
    mean = sirt_kit.ball_figures(mltr_kit.starved_reference())[0]
    sirt = sirt_ref.sirt(mltr_kit.starved_line_integrals(), A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING,
                         mltr_kit.STARVED_K, mltr_kit.BALL_S, 1.0, 0.0)
    below = sirt_kit.ball_figures(sirt)[0]
    print(f"starved counts: {zeros} of {y.size} pixels count zero; inner mean MLTR {mean:.4f}, SIRT on the logarithm {below:.4f}")
    assert zeros > 1000
    assert abs(mean - 1.0) <= 0.1, mean
    assert below < 0.75, below


def test_known_background_in_the_reference():
    """A flat field of 1000 counts over a background of 20: modelled, the ball's level is found; ignored, it is not."""
    modelled = sirt_kit.ball_figures(mltr_kit.background_reference(True))[0]
    ignored = sirt_kit.ball_figures(mltr_kit.background_reference(False))[0]
    print(f"known background: inner mean modelled {modelled:.4f}, ignored {ignored:.4f}")
    assert 0.9 <= modelled <= 1.2, modelled
    assert ignored < 0.7, ignored


# ------------------------------------------------------------------------------- the CLI's refusals, the sanitizers
def test_cli_refusals(tmp_path):
    """--mltr's refusals come before anything is loaded or a device is opened."""
    exe = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
    scan = [exe, "-i", "none.obj", "--turntable", "24:z", "--log-projection", "80"]
    base = scan + ["--reconstruct", "x.mhd"]

    def refused(args, text):
        r = subprocess.run(args, capture_output=True, text=True, cwd=tmp_path, timeout=120)
        assert r.returncode == 1 and text in r.stderr and "Loading" not in r.stdout, (args, r.stderr)

    refused(base + ["--mltr", "3", "--sirt", "3"], "--mltr and --sirt are two solvers")
    refused(scan + ["--mltr", "3"], "--mltr needs --reconstruct")
    refused(base + ["--mltr", "3:25"], "more subsets than projections")
    refused([exe, "-i", "none.obj", "--reconstruct", "x.mhd", "--mltr", "3"], "--reconstruct needs --turntable")
    refused(base + ["--tv", "5"], "--tv needs --sirt K or --mltr K")
    for value in ("0", "x", "3:0", "3:65", "3:2:nan", "3:2:1:1", ""):
        refused(base + ["--mltr", value], "--mltr K[:S[:RELAX]]")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert "--mltr K" in r.stdout + r.stderr


def test_host_code_under_sanitizers(tmp_path):
    """tools/mltr_san.cpp: a stand-alone program over csrc/xrt_mltr_host.inc (the checks and the three restatements
    over exact-size buffers) with AddressSanitizer and UBSan.  Nothing is loaded into Python."""
    from test_pose_cpu import _sanitizer_runtime
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "mltr_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "mltr_san.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "mltr_san: OK" in r.stdout, out[-3000:]
