"""Line-integral projections without a GPU: the logf restatement against libm on
every input (tools/check_logf.c) and, host-compiled (xrt_host_logf_batch), against
tests/logf_ref.py; the pixel function over planes (xrt_host_log_projection) against the reference;
the argument errors that need no device, the CLI's, k_log_projection's code-object metadata and
a stand-alone sanitizer build of the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import logf_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import DRAGON, ROOT, bits
from test_materials_cpu import _render_kernel_metadata
from test_pose_cpu import _sanitizer_runtime

F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
PLANES = [(1, 1), (7, 13), (13, 7), (63, 5), (64, 64), (65, 33), (257, 131), (509, 3), (510, 3), (1031, 2)]


def test_logf_restatement_equals_libm_exhaustive(tmp_path):
    """tools/check_logf.c: its own copy of the algorithm and constants, every f64 operation rounded
    on its own (-ffp-contract=off), against libm's logf on all 2^32 inputs."""
    src = os.path.join(ROOT, "tools", "check_logf.c")
    exe = str(tmp_path / "check_logf")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, src, "-lm", "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "logf mismatches 0 of 4294967296" in r.stdout, r.stdout


@pytest.mark.parametrize("name", ["period", "stride", "subnormals", "specials"])
def test_host_logf_equals_the_reference(name):
    x = dict(logf_ref.sweeps())[name]
    got, want = xrt.host_logf(x), logf_ref.logf(x)
    ok, nans = logf_ref.same(got, want)
    assert ok, np.argwhere(bits(got) != bits(want))[:8]
    if name in ("period", "subnormals"):
        assert nans == 0
    if name == "period":                                # 1.0 and every table interval
        assert got[0x3F800000 - 0x3F330000] == 0 and bits(got)[0x3F800000 - 0x3F330000] == 0
        assert len(np.unique((x.view(np.uint32) - np.uint32(0x3F330000)) >> np.uint32(19))) == 16


def test_reference_logf_special_values():
    """The reference itself on the contract's special cases and against libm (numpy's log is not the
    reference: it may differ from glibc's logf in the last place)."""
    x = logf_ref.SPECIALS
    y = logf_ref.logf(x)
    assert y[0] == -np.inf and y[1] == -np.inf and y[2] == np.inf            # +-0, +inf
    assert np.isnan(y[3:8]).all()                                            # -inf, NaNs, -1
    assert np.isnan(y[9]) and np.isnan(y[13])                                # negative subnormal, -max
    assert bits(y)[14] == 0                                                  # log(1) = +0.0
    libm = ctypes.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    rng = np.random.default_rng(5)
    sample = np.concatenate([x, rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32).view(F)])
    want = np.array([libm.logf(ctypes.c_float(float(v))) for v in sample], F)
    assert logf_ref.same(logf_ref.logf(sample), want)[0]


@pytest.mark.parametrize("W,H", PLANES)
def test_host_pixel_function_equals_the_reference(W, H):
    for P in (None, 3):
        for flat in (False, True):
            for dark in (False, True):
                image, f, d, fv = logf_ref.planes(1000 * W + H, W, H, P, flat, dark)
                for t_min in (0.0, 0.01):
                    for sino in (False, True):
                        want = logf_ref.apply(image, f, d, fv, t_min, sino)
                        got = xrt.host_log_projection(image, f, d, None if flat else fv, t_min, sino)
                        assert np.isfinite(want).all()                      # no pixel is left out
                        ok, _ = logf_ref.same(got, want)
                        assert ok, (W, H, P, flat, dark, t_min, sino)
                    assert (logf_ref.pixels(image, f, d, fv, 0.01) <= -np.log(0.01) + 1e-5).all()


def test_orders_and_in_place():
    image, f, d, fv = logf_ref.planes(2, 9, 4, 3, True, True)
    proj = xrt.host_log_projection(image, f, d)
    sino = xrt.host_log_projection(image, f, d, sinograms=True)
    assert sino.shape == (4, 3, 9)
    for p in range(3):
        for y in range(4):
            assert np.array_equal(bits(sino[y, p]), bits(proj[p, y]))
    lib = _abi.load()
    a = image.copy()
    rc = lib.xrt_host_log_projection(9, 4, 3, a.ctypes.data_as(_abi._fp), f.ctypes.data_as(_abi._fp),
                                     d.ctypes.data_as(_abi._fp), 0.0, 0.0, _abi.XRT_ORDER_PROJECTIONS,
                                     a.ctypes.data_as(_abi._fp))
    assert rc == _abi.XRT_OK and np.array_equal(bits(a), bits(proj))


def test_unit_and_zero_transmission():
    image = np.array([[80.0, 0.0, -1.0, np.inf, np.nan, 40.0]], F)
    got = xrt.host_log_projection(image, flat_value=80.0)
    assert bits(got)[0, 0] == 0 and got[0, 1] == np.inf and np.isnan(got[0, 2]) and got[0, 3] == -np.inf
    assert np.isnan(got[0, 4]) and got[0, 5] == logf_ref.pixels(image, flat_value=80.0)[0, 5]
    got = xrt.host_log_projection(image, flat_value=80.0, t_min=0.25)      # clamped; the NaN stays
    assert got[0, 1] == got[0, 2] == F(0.0) - logf_ref.logf(np.array([0.25], F))[0] and np.isnan(got[0, 4])


def _call(lib, entry, w, h, p, image, flat, dark, flat_value, t_min, order, out):
    fp = _abi._fp

    def ptr(a):
        return None if a is None else a.ctypes.data_as(fp)
    if entry == "device":
        cast = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        return lib.xrt_log_projection_device(None, w, h, p, cast(image), cast(flat), cast(dark), flat_value, t_min, order,
                                             cast(out), None)
    if entry == "host":
        return lib.xrt_log_projection(None, w, h, p, ptr(image), ptr(flat), ptr(dark), flat_value, t_min, order, ptr(out))
    return lib.xrt_host_log_projection(w, h, p, ptr(image), ptr(flat), ptr(dark), flat_value, t_min, order, ptr(out))


@pytest.mark.parametrize("entry", ["host", "device", "hook"])
def test_argument_errors_without_a_device(entry):
    """Every check comes before the context is looked at: with a NULL context each is
    XRT_ERR_ARGUMENT with its own message (the entries), or XRT_ERR_ARGUMENT (the hook)."""
    lib = _abi.load()
    img, out = np.zeros(24, F), np.zeros(24, F)
    fl, dk = np.ones(12, F), np.zeros(12, F)
    PR, SI = _abi.XRT_ORDER_PROJECTIONS, _abi.XRT_ORDER_SINOGRAMS
    nan, inf = float("nan"), float("inf")
    cases = [
        ((4, 3, 2, None, fl, dk, 80.0, 0.0, PR, out), "image is NULL"),
        ((4, 3, 2, img, fl, dk, 80.0, 0.0, PR, None), "out is NULL"),
        ((0, 3, 2, img, fl, dk, 80.0, 0.0, PR, out), "is 0"),
        ((4, 0, 2, img, fl, dk, 80.0, 0.0, PR, out), "is 0"),
        ((4, 3, 0, img, fl, dk, 80.0, 0.0, PR, out), "is 0"),
        ((4, 3, 2, img, fl, dk, 80.0, 0.0, 2, out), "order"),
        ((4, 3, 2, img, fl, dk, 80.0, 0.0, -1, out), "order"),
        ((4, 3, 2, img, fl, dk, 80.0, nan, PR, out), "t_min"),
        ((4, 3, 2, img, fl, dk, 80.0, inf, PR, out), "t_min"),
        ((4, 3, 2, img, fl, dk, 80.0, -0.25, PR, out), "t_min"),
        ((4, 3, 2, img, None, dk, 0.0, 0.0, PR, out), "flat_value"),
        ((4, 3, 2, img, None, dk, -80.0, 0.0, PR, out), "flat_value"),
        ((4, 3, 2, img, None, None, nan, 0.0, PR, out), "flat_value"),
        ((4, 3, 2, img, None, None, inf, 0.0, PR, out), "flat_value"),
        ((4, 3, 2, img, fl, dk, 80.0, 0.0, SI, img), "overlaps"),                  # in place moves rows in this order
        ((4, 3, 1, img, fl, dk, 80.0, 0.0, PR, img[1:]), "overlaps"),              # a partial overlap
        ((4, 3, 1, img, fl, dk, 80.0, 0.0, PR, img[11:]), "overlaps"),             # the last pixel
        ((4, 3, 1, img, fl, dk, 80.0, 0.0, PR, fl), "overlaps"),
        ((4, 3, 1, img, fl, dk, 80.0, 0.0, SI, dk), "overlaps"),
        ((1, 0xFFFFFFFF, 2, img, fl, dk, 80.0, 0.0, PR, out), "2^32"),
    ]
    for args, word in cases:
        assert _call(lib, entry, *args) == _abi.XRT_ERR_ARGUMENT, (word, args[:3])
        if entry != "hook":
            assert word.encode() in lib.xrt_last_error(None), (word, lib.xrt_last_error(None))
    # arguments in order: the entries then fail on the context alone, the hook computes
    for ok in ((4, 3, 1, img, fl, dk, nan, 0.0, PR, img[12:]),                     # side by side; flat_value unread
               (4, 3, 2, img, fl, dk, 80.0, 0.0, PR, img),                         # in place, projection order
               (4, 3, 2, img, None, None, 80.0, 0.01, SI, out)):
        rc = _call(lib, entry, *ok)
        if entry == "hook":
            assert rc == _abi.XRT_OK
        else:
            assert rc == _abi.XRT_ERR_ARGUMENT and b"context is NULL" in lib.xrt_last_error(None)
    with pytest.raises(ValueError):
        xrt.host_log_projection(np.zeros(5, F), flat_value=80.0)
    with pytest.raises(ValueError):
        xrt.host_log_projection(np.zeros((3, 5), F))                               # neither a flat plane nor a value
    with pytest.raises(ValueError):
        xrt.host_log_projection(np.zeros((3, 5), F), flat=np.ones((5, 3), F))


def test_probe_op_is_declared():
    assert _abi.XRT_PROBE_LOGF == 6
    text = open(os.path.join(ROOT, "include", "xrt_debug.h")).read()
    assert "XRT_PROBE_LOGF = 6" in text and "XRT_PROBE_LOGF" not in open(os.path.join(ROOT, "include", "xrt.h")).read()


def test_k_log_projection_metadata():
    """k_log_projection's two instantiations (a workgroup within one row, or over several) in the
    gfx950 code object, with no scratch, no spills and no LDS."""
    meta = _render_kernel_metadata()
    proj = {k: v for k, v in meta.items() if "k_log_projection" in k}
    assert len(proj) == 2, sorted(meta)
    for name, f in proj.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] == 0 and f["vgpr_count"] <= 64, f      # the table is read from global memory
    probe = [v for k, v in meta.items() if "k_probe_math" in k]
    assert len(probe) == 1 and probe[0]["private_segment_fixed_size"] == 0 and probe[0]["vgpr_spill_count"] == 0


def test_cli_help_lists_the_options():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--log-projection I0" in r.stderr and "--sinogram FILE" in r.stderr


@pytest.mark.parametrize("args,word", [
    (["--log-projection", "0"], "--log-projection"),
    (["--log-projection", "-80"], "--log-projection"),
    (["--log-projection", "inf"], "--log-projection"),
    (["--log-projection", "nan"], "--log-projection"),
    (["--log-projection", "80x"], "--log-projection"),
    (["--log-projection", "80", "-g", "2"], "--log-projection"),
    (["--log-projection", "80", "--rows", "0:4"], "--log-projection"),
    (["--log-projection", "80", "--paths"], "--spectrum"),
    (["--sinogram", "s.raw"], "--sinogram"),
    (["--sinogram", "s.raw", "--log-projection", "80"], "--turntable"),
    (["--sinogram", "s.raw", "--turntable", "3"], "--log-projection"),
])
def test_cli_errors(tmp_path, args, word):
    """Each is an error before any device is opened: exit 1, stderr 'ERROR: ...' naming the option."""
    r = subprocess.run([EXE, "-s", "16", "16", "-i", DRAGON] + args, capture_output=True, text=True, cwd=tmp_path,
                       timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("ERROR:") and word in r.stderr and "xrt_create" not in r.stderr, r.stderr


def test_host_code_under_sanitizers(tmp_path):
    """tools/projection_san.cpp: a stand-alone program over csrc/xrt_projection_host.inc (the checks,
    logf against libm, the pixel function in every combination and in place) with AddressSanitizer
    and UBSan.  Nothing is loaded into Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "projection_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "projection_san.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "projection_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
