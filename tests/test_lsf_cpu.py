"""The detector response without a GPU: the kernel's tap loop, host-compiled
(xrt_host_lsf), against tests/lsf_ref.py bit for bit, xrt_lsf_gaussian against a numpy
restatement, the argument errors that need no device, the CLI's, k_lsf's code-object
metadata and a stand-alone sanitizer build of the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lsf_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import DRAGON, ROOT, bits
from test_materials_cpu import _render_kernel_metadata
from test_pose_cpu import _sanitizer_runtime

F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
TILE = 64                                               # kLsfTile (csrc/kernels/xrt_kernels.h)
PLANES = [(1, 1), (7, 13), (13, 7), (63, 5), (64, 64), (65, 33), (257, 131), (33, TILE - 1), (33, TILE + 1)]
TAPS = [(1, 1), (3, 1), (1, 3), (5, 9), (41, 41), (129, 129)]


def check(got, want, what):
    g, gu = got
    w, wu = want
    ok, nans = lsf_ref.same(g, w)
    assert nans == 0, what                              # finite inputs and taps: no pixel is left out
    assert ok, (what, np.argwhere(bits(g) != bits(w))[:8])
    assert np.array_equal(gu, wu), (what, np.argwhere(gu != wu)[:8])


@pytest.mark.parametrize("W,H", PLANES)
def test_host_restatement_equals_the_reference(W, H):
    a = lsf_ref.plane(1000 * W + H, W, H)
    for nx, ny in TAPS:
        hx, hy = lsf_ref.taps(nx, nx), lsf_ref.taps(ny + 1, ny)
        check(xrt.host_lsf(a, hx, hy), lsf_ref.apply(a, hx, hy), (W, H, nx, ny))


def test_stacked_planes_are_single_planes():
    a = lsf_ref.plane(5, 21, 9, P=3)
    hx, hy = lsf_ref.taps(7, 7), lsf_ref.taps(8, 11)
    got, gu = xrt.host_lsf(a, hx, hy)
    check((got, gu), lsf_ref.apply(a, hx, hy), "stack")
    for p in range(3):                                  # a plane's edge does not read its neighbour
        check((got[p], gu[p]), lsf_ref.apply(a[p], hx, hy), p)


def test_identity_returns_the_inputs_bits():
    a = lsf_ref.plane(3, 37, 19)
    a.reshape(-1)[::7] = F(-0.0)
    a.reshape(-1)[3::11] = np.array([1, 0x7FFFFF, 0x80000001, 0x00400000], np.uint32).view(F)[np.arange(a.size // 11 + 1) % 4][:a.reshape(-1)[3::11].size]
    assert (a.view(np.uint32) == 0x80000000).any() and (np.abs(a[a != 0]) < 1e-38).any()   # -0.0 and denormals
    got, _ = xrt.host_lsf(a, [1.0], [1.0])
    assert np.array_equal(bits(got), bits(a))
    ref, _ = lsf_ref.apply(a, [1.0], [1.0])
    assert np.array_equal(bits(ref), bits(a))


def test_orientation_and_edge_rule():
    """hx = {1, 0, 0}: hx[0] meets the pixel one to the LEFT -- the image moves right by one
    pixel, its left column replicated; the same down the columns with hy."""
    a = lsf_ref.plane(8, 9, 6)
    got, _ = xrt.host_lsf(a, [1.0, 0.0, 0.0], [1.0])
    want = np.concatenate([a[:, :1], a[:, :-1]], axis=1)
    assert np.array_equal(got, want)                    # (values: 1 * v + 0 * w + 0 * w may turn a -0.0 into +0.0)
    got, _ = xrt.host_lsf(a, [1.0], [0.0, 0.0, 1.0])
    assert np.array_equal(got, np.concatenate([a[1:], a[-1:]], axis=0))
    check(xrt.host_lsf(a, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]), lsf_ref.apply(a, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]), "shift")


def test_axes_are_not_transposed():
    a = lsf_ref.plane(9, 31, 12)
    hx, hy = lsf_ref.taps(1, 9), lsf_ref.taps(2, 3)
    right = lsf_ref.apply(a, hx, hy)
    wrong = lsf_ref.apply(a, hy, hx)
    assert not np.array_equal(bits(right[0]), bits(wrong[0]))
    check(xrt.host_lsf(a, hx, hy), right, "hx != hy")


def _call(lib, entry, w, h, p, image, hx, nx, hy, ny, out, u8):
    fp, u8p = _abi._fp, _abi._u8p

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    if entry == "device":
        cast = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        return lib.xrt_detector_response_device(None, w, h, p, cast(image), ptr(hx, fp), nx, ptr(hy, fp), ny, cast(out),
                                                cast(u8), None)
    if entry == "host":
        return lib.xrt_detector_response(None, w, h, p, ptr(image, fp), ptr(hx, fp), nx, ptr(hy, fp), ny, ptr(out, fp),
                                         ptr(u8, u8p))
    return lib.xrt_host_lsf(w, h, p, ptr(image, fp), ptr(hx, fp), nx, ptr(hy, fp), ny, ptr(out, fp), ptr(u8, u8p))


@pytest.mark.parametrize("entry", ["host", "device", "hook"])
def test_argument_errors_without_a_device(entry):
    """Every check comes before the context is looked at: with a NULL context each is
    XRT_ERR_ARGUMENT with its own message (the entries), or XRT_ERR_ARGUMENT (the hook)."""
    lib = _abi.load()
    img = np.zeros(24, F)
    out = np.zeros(24, F)
    u8 = np.zeros(24, np.uint8)
    h3 = np.array([0.25, 0.5, 0.25], F)
    big = np.zeros(131, F)
    nan = np.array([0.25, np.nan, 0.25], F)
    inf = np.array([np.inf, 0, 0], F)
    cases = [
        ((4, 3, 2, img, None, 3, h3, 3, out, u8), "NULL"),
        ((4, 3, 2, img, h3, 3, None, 3, out, u8), "NULL"),
        ((4, 3, 2, img, h3, 2, h3, 3, out, u8), "even"),
        ((4, 3, 2, img, h3, 3, h3, 2, out, u8), "even"),
        ((4, 3, 2, img, h3, 0, h3, 3, out, u8), "outside"),
        ((4, 3, 2, img, big, 131, h3, 3, out, u8), "outside"),
        ((4, 3, 2, img, nan, 3, h3, 3, out, u8), "finite"),
        ((4, 3, 2, img, h3, 3, inf, 3, out, u8), "finite"),
        ((0, 3, 2, img, h3, 3, h3, 3, out, u8), "is 0"),
        ((4, 0, 2, img, h3, 3, h3, 3, out, u8), "is 0"),
        ((4, 3, 0, img, h3, 3, h3, 3, out, u8), "is 0"),
        ((4, 3, 2, None, h3, 3, h3, 3, out, u8), "image is NULL"),
        ((4, 3, 2, img, h3, 3, h3, 3, None, None), "both NULL"),
        ((4, 3, 2, img, h3, 3, h3, 3, img, u8), "overlaps"),                       # in place
        ((4, 3, 1, img, h3, 3, h3, 3, img[6:], None), "overlaps"),                 # a partial overlap
        ((4, 3, 2, img, h3, 3, h3, 3, None, img.view(np.uint8)[95:]), "overlaps"),  # the last byte
    ]
    for args, word in cases:
        assert _call(lib, entry, *args) == _abi.XRT_ERR_ARGUMENT, (word, args[:3])
        if entry != "hook":
            assert word.encode() in lib.xrt_last_error(None), (word, lib.xrt_last_error(None))
    # arguments in order: the entries then fail on the context alone, the hook computes
    ok = (4, 3, 1, img, h3, 3, h3, 3, img[12:], u8)                                # side by side is no overlap
    rc = _call(lib, entry, *ok)
    if entry == "hook":
        assert rc == _abi.XRT_OK
    else:
        assert rc == _abi.XRT_ERR_ARGUMENT and b"context is NULL" in lib.xrt_last_error(None)
    with pytest.raises(ValueError):
        xrt.host_lsf(np.zeros(5, F), h3)


@pytest.mark.parametrize("sigma", [0.3, 1.0, 2.5, 10.0, 40.0])
def test_lsf_gaussian(sigma):
    worst = 0.0
    for taps in (1, 3, 41, 129):
        h = xrt.lsf_gaussian(sigma, taps)
        exact, rounded = lsf_ref.gaussian(sigma, taps)
        assert h.dtype == F and h.shape == (taps,)
        # within 1 f32 ulp of the f64 restatement (half an ulp of rounding; libm's exp against numpy's the rest)
        ulp = np.spacing(np.abs(rounded)).astype(np.float64)
        err = np.abs(h.astype(np.float64) - exact) / ulp
        worst = max(worst, err.max())
        assert np.array_equal(bits(h), bits(h[::-1].copy())), taps
        total = np.float64(0.0)
        for v in h:
            total += np.float64(v)
        assert abs(total - 1.0) <= taps * 2.0 ** -24, (taps, total)
    print("xrt_lsf_gaussian against the numpy restatement, sigma", sigma, ": worst", worst, "ulp of f32")
    assert worst <= 1.0


def test_lsf_gaussian_errors():
    for sigma, taps in ((0.0, 3), (-1.0, 3), (np.nan, 3), (np.inf, 3), (1.0, 2), (1.0, 0), (1.0, 131)):
        with pytest.raises(xrt.XrtError) as e:
            xrt.lsf_gaussian(sigma, taps)
        assert e.value.code == _abi.XRT_ERR_ARGUMENT
    assert _abi.load().xrt_lsf_gaussian(1.0, 3, None) == _abi.XRT_ERR_ARGUMENT


def test_k_lsf_metadata():
    """One k_lsf in the gfx950 code object, with no scratch and no spills; its taps travel by value."""
    meta = _render_kernel_metadata()
    lsf = {k: v for k, v in meta.items() if "k_lsf" in k}
    assert len(lsf) == 1, sorted(meta)
    (name, f), = lsf.items()
    assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
    # three pointers, two words and the table: 2 x 129 taps, widened to f64, and the two counts
    assert f["kernarg_segment_size"] >= 3 * 8 + 2 * 4 + 2 * 129 * 8 + 2 * 4, f


def test_cli_help_lists_the_options():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--lsf FILE" in r.stderr and "--lsf-gaussian SIGMA[:TAPS]" in r.stderr


@pytest.mark.parametrize("text,args,word", [
    ("0.25 0.5 x\n", [], "--lsf"),                                       # malformed
    ("0.25 nan 0.25\n", [], "--lsf"),
    ("0.5 0.5\n", [], "--lsf"),                                          # an even count
    ("1\n0.5 0.5\n", [], "--lsf"),
    ("# nothing\n\n", [], "--lsf"),
    ("1\n1\n1\n", [], "--lsf"),
    (" ".join(["0"] * 131) + "\n", [], "--lsf"),
    ("0.25 0.5 0.25\n", ["-g", "2"], "--lsf"),
    ("0.25 0.5 0.25\n", ["--rows", "0:4"], "--lsf"),
    ("0.25 0.5 0.25\n", ["--lsf-gaussian", "1.5"], "--lsf-gaussian"),    # both responses
    ("0.25 0.5 0.25\n", ["--paths"], "--spectrum"),
    (None, ["--lsf-gaussian", "0"], "--lsf-gaussian"),
    (None, ["--lsf-gaussian", "abc"], "--lsf-gaussian"),
    (None, ["--lsf-gaussian", "2:4"], "--lsf-gaussian"),
    (None, ["--lsf-gaussian", "2:131"], "--lsf-gaussian"),
    (None, ["--lsf-gaussian", "2:5:1"], "--lsf-gaussian"),
    (None, ["--lsf-gaussian", "2", "-g", "2"], "--lsf-gaussian"),
    (None, ["--lsf", "no-such-file.txt"], "--lsf"),
])
def test_cli_errors(tmp_path, text, args, word):
    """Each is an error before any device is opened: exit 1, stderr 'ERROR: ...' naming the option."""
    if text is not None:
        (tmp_path / "lsf.txt").write_text(text)
        args = ["--lsf", str(tmp_path / "lsf.txt")] + args
    r = subprocess.run([EXE, "-s", "16", "16", "-i", DRAGON] + args, capture_output=True, text=True, cwd=tmp_path,
                       timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("ERROR:") and word in r.stderr and "xrt_create" not in r.stderr, r.stderr


def test_host_code_under_sanitizers(tmp_path):
    """tools/lsf_san.cpp: a stand-alone program over csrc/xrt_lsf_host.inc (the checks, the Gaussian
    and the host restatement, 7 x 13 under 129 taps among its planes) with AddressSanitizer and
    UBSan.  Nothing is loaded into Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "lsf_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "lsf_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "lsf_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
