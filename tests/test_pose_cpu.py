"""Mesh poses without a GPU: the host arithmetic against
tests/pose_ref.py and against the fork's own expression, xrt_pose_rotation
against an f64 restatement, the argument errors that need no device, the CLI's,
k_pose's code-object metadata and a stand-alone sanitizer build of the host code."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pose_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import DRAGON, ROOT, bits
from scene_kit import synthetic_soup
from test_materials_cpu import _render_kernel_metadata

F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
NEG0 = np.uint32(0x80000000)


def hard_soup(seed, n):
    """A random soup with -0.0, denormal and huge coordinates in it."""
    rng = np.random.default_rng(seed)
    s = synthetic_soup(seed=seed, n=max(n, 30))[:n].copy().reshape(-1)
    k = rng.integers(0, 6, s.size)
    s[k == 1] = -0.0
    s[k == 2] = (rng.integers(1, 1 << 22, np.count_nonzero(k == 2)).astype(np.uint32)).view(F)      # denormals
    s[k == 3] *= F(1e36)                                                                              # huge: products overflow
    s[k == 4] = 0.0
    return s.reshape(-1, 9)


def poses_under_test():
    rng = np.random.default_rng(77)
    out = {"random": rng.normal(0, 1, 12).astype(F), "huge": (rng.normal(0, 1, 12) * 1e30).astype(F),
           "tiny": (rng.normal(0, 1, 12) * 1e-30).astype(F)}
    q = rng.normal(0, 1, 12).astype(F)
    q[[3, 7, 11]] = 0.0
    out["t = +0"] = q.copy()
    q[[3, 11]] = -0.0
    out["t = mixed +-0"] = q.copy()
    q[7] = 1e-45
    out["t = one denormal"] = q.copy()
    d = pose_ref.IDENTITY.copy()
    d[5] = -1.0
    out["mirror"] = d.copy()                           # a negative determinant is nothing special
    d[[3, 7]] = -0.0
    out["mirror, t = -0"] = d.copy()
    z = pose_ref.IDENTITY.copy()
    z[3] = -0.0
    out["identity but for a -0"] = z                   # not bitwise the identity: computed (and adds nothing)
    return out


@pytest.mark.parametrize("n", [0, 1, 2, 63, 1000])
def test_pose_triangles_equals_the_reference(n):
    soup = hard_soup(3 + n, n)
    for name, q in poses_under_test().items():
        got = xrt.pose_triangles(soup, q)
        want = pose_ref.apply_pose(soup, q)
        nan = np.isnan(want)
        assert got.shape == want.shape == (n, 9), name
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]) and np.isnan(got[nan]).all(), name
    # the identity: the input's bits, whatever they are (NaN payloads included)
    odd = soup.copy()
    if n:
        odd.reshape(-1).view(np.uint32)[::5] = 0x7FC12345
    assert np.array_equal(bits(xrt.pose_triangles(odd, pose_ref.IDENTITY)), bits(odd))
    assert np.array_equal(bits(xrt.pose_triangles(odd, None)), bits(odd))
    # in place
    q = poses_under_test()["random"]
    buf = np.ascontiguousarray(soup.copy())
    rc = _abi.load().xrt_pose_triangles(buf.ctypes.data_as(_abi._fp), n, q.ctypes.data_as(_abi._fp),
                                        buf.ctypes.data_as(_abi._fp))
    assert rc == _abi.XRT_OK
    want = pose_ref.apply_pose(soup, q)
    nan = np.isnan(want)
    assert np.array_equal(bits(buf)[~nan], bits(want)[~nan])


def test_reference_rules():
    """pose_ref itself: the identity rule and the t = +-0 rule do what DESIGN 10.4 says."""
    v = np.array([[-0.0, 5.0, -0.0, -0.0, 0.0, -0.0, 1.0, 2.0, 3.0]], F)
    assert np.array_equal(bits(pose_ref.apply_pose(v, pose_ref.IDENTITY)), bits(v))
    z = pose_ref.IDENTITY.copy()
    z[3] = -0.0                                          # computed, nothing added: 1 * -0 + 0 * 5 + 0 * -0 = -0 + 0 = +0
    assert bits(pose_ref.apply_pose(v, z))[0, 0] == 0
    m = pose_ref.IDENTITY.copy()
    m[5] = -1.0                                          # y -> -y: (0 * -0 + -1 * 0) + 0 * -0 = (-0 + -0) + -0 = -0
    got = pose_ref.apply_pose(v, m)
    assert bits(got)[0, 4] == NEG0
    m[11] = 2.0                                          # one t_j not 0: every t_i is added, and -0 + 0 = +0
    got = pose_ref.apply_pose(v, m)
    assert bits(got)[0, 4] == 0 and got[0, 8] == 5.0


def test_the_forks_own_expression():
    """src/main-pthreads-lbuffer.cxx:561-564 typed in: transformMatrix[i][0] * x + [i][1] * y + [i][2] * z,
    three f32 products summed left to right -- xrt_pose_triangles with t = 0, bit for bit."""
    rng = np.random.default_rng(9)
    a = np.deg2rad(45.0)
    rotate_mat = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F)   # :279's rotateMat
    mirror = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1]], F)
    for tm in (rotate_mat, mirror, rng.normal(0, 1, (3, 3)).astype(F)):
        soup = hard_soup(21, 500)
        soup[0, :3] = [-3.0, 0.0, -2.0]                  # under `mirror`: y = (0 * -3 + -1 * 0) + 0 * -2 = -0.0
        v = soup.reshape(-1, 3)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        want = np.empty_like(v)
        with np.errstate(all="ignore"):
            for i in range(3):
                want[:, i] = tm[i][0] * x + tm[i][1] * y + tm[i][2] * z
        pose = np.zeros((3, 4), F)
        pose[:, :3] = tm
        got = xrt.pose_triangles(soup, pose).reshape(-1, 3)
        nan = np.isnan(want)
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]) and np.isnan(got[nan]).all()
        if tm is mirror:
            assert bits(got)[0, 1] == NEG0 and bits(want)[0, 1] == NEG0
            moved = pose.copy()
            moved[:, 3] = 0.0
            moved[2, 3] = 1.0                            # an added +0.0 loses it
            assert bits(xrt.pose_triangles(soup, moved).reshape(-1, 3))[0, 1] == 0


def ulps(a, b):
    """|a - b| in units of b's f32 ulp (b the f64 value, a the f32 result)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ulp = np.spacing(np.abs(b).astype(F)).astype(np.float64)
    return np.abs(a - b) / ulp


def test_pose_rotation():
    worst = 0.0
    centre = np.array([60.0, -3.5, 12.25], F)
    for axis in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, -2, 3), (0.3, 0.2, -5.0)):
        for deg in (0.0, 30.0, 45.0, 90.0, 180.0, 270.0, 360.0, -17.25, 1.5, 725.0):
            for c in (centre, np.zeros(3, F)):
                got = xrt.pose_rotation(axis, deg, c)
                exact, rounded = pose_ref.rotation(axis, deg, c)
                assert got.dtype == F and got.shape == (12,)
                worst = max(worst, ulps(got, exact.reshape(12)).max())
                if deg == 0.0:
                    assert np.all(ulps(got[[0, 5, 10]], 1.0) <= 1.0) and np.all(got[[3, 7, 11]] == 0.0)
    print("xrt_pose_rotation against the f64 restatement: worst", worst, "ulp of f32")
    # within 1 ulp of the exact f64 value: half an ulp of rounding, the rest sin / cos and the order of sums
    assert worst <= 1.0
    # the three coordinate axes, a quarter turn: the permutation matrices to that ulp
    qy = xrt.pose_rotation((0, 1, 0), 90.0).reshape(3, 4)
    assert np.allclose(qy[:, :3], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-7) and np.all(qy[:, 3] == 0)
    # an axis is normalised: its length does not matter
    assert np.array_equal(bits(xrt.pose_rotation((0, 2, 0), 30.0, centre)), bits(xrt.pose_rotation((0, 1, 0), 30.0, centre)))
    for bad in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0)):
        with pytest.raises(xrt.XrtError) as e:
            xrt.pose_rotation(bad, 10.0)
        assert e.value.code == _abi.XRT_ERR_ARGUMENT


def test_argument_errors_without_a_device():
    lib = _abi.load()
    q = pose_ref.IDENTITY.copy()
    fp = _abi._fp
    assert lib.xrt_set_pose(None, 0, q.ctypes.data_as(fp)) == _abi.XRT_ERR_ARGUMENT
    assert b"NULL" in lib.xrt_last_error(None)
    assert lib.xrt_reset_poses(None) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_multi_set_pose(None, 0, q.ctypes.data_as(fp)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_multi_reset_poses(None) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_debug_posed_triangles(None, None, 0, None) == _abi.XRT_ERR_ARGUMENT
    tri = np.arange(9, dtype=F)
    assert lib.xrt_pose_triangles(None, 1, q.ctypes.data_as(fp), tri.ctypes.data_as(fp)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_pose_triangles(tri.ctypes.data_as(fp), 1, None, tri.ctypes.data_as(fp)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_pose_triangles(tri.ctypes.data_as(fp), 1, q.ctypes.data_as(fp), None) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_pose_triangles(None, 0, q.ctypes.data_as(fp), None) == _abi.XRT_OK                # n = 0
    a = np.array([0, 1, 0], F)
    assert lib.xrt_pose_rotation(None, 1.0, a.ctypes.data_as(fp), q.ctypes.data_as(fp)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_pose_rotation(a.ctypes.data_as(fp), 1.0, None, q.ctypes.data_as(fp)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_pose_rotation(a.ctypes.data_as(fp), 1.0, a.ctypes.data_as(fp), None) == _abi.XRT_ERR_ARGUMENT
    with pytest.raises(ValueError):
        xrt.pose_triangles(tri, np.zeros(11, F))


TWELVE = ",".join(["1", "0", "0", "0", "0", "1", "0", "0", "0", "0", "1", "0"])


@pytest.mark.parametrize("args,word", [
    (["--pose", "x=" + TWELVE], "mesh"),
    (["--pose", TWELVE], "mesh"),
    (["--pose", "-1=" + TWELVE], "mesh"),
    (["--pose", "0=1,0,0,0,0,1,0,0,0,0,1"], "12"),
    (["--pose", "0=" + TWELVE + ",0"], "12"),
    (["--pose", "0=" + TWELVE.replace("1,0", "nan,0", 1)], "finite"),
    (["--pose", "0=" + TWELVE.replace("1,0", "inf,0", 1)], "finite"),
    (["--pose", "0=" + TWELVE.replace("1,0", "1x,0", 1)], "finite"),
    (["--pose", "0=" + TWELVE, "--pose", "0=" + TWELVE], "twice"),
    (["--pose", "1=" + TWELVE], "mesh"),                               # after loading: the dragon is one mesh
    (["--turntable", "0"], "turntable"),
    (["--turntable", "three"], "turntable"),
    (["--turntable", "3:w"], "turntable"),
    (["--turntable", "3:y:a"], "mesh"),
    (["--turntable", "3:y:1"], "mesh"),                                # after loading
    (["--turntable", "3", "--paths"], "turntable"),
    (["--turntable", "3", "--batch", "2"], "turntable"),
    (["--turntable", "3", "-g", "2"], "turntable"),
])
def test_cli_errors(tmp_path, args, word):
    """Each is an error before any device is opened: exit 1, stderr 'ERROR: ...' (no 'xrt_create' in it)."""
    r = subprocess.run([EXE, "-s", "16", "16", "-i", DRAGON] + args, capture_output=True, text=True, cwd=tmp_path,
                       timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("ERROR:") and word in r.stderr and "xrt_create" not in r.stderr, r.stderr


def test_cli_help_lists_the_options():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--pose" in r.stderr and "--turntable" in r.stderr


def test_k_pose_metadata():
    """One k_pose in the gfx950 code object, with no scratch, no spills and no LDS."""
    meta = _render_kernel_metadata()
    pose = {k: v for k, v in meta.items() if "k_pose" in k}
    assert len(pose) == 1, sorted(meta)
    (name, f), = pose.items()
    assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
    assert f["group_segment_fixed_size"] == 0, f
    # the poses and range ends travel by value: two pointers, two words and the table
    assert f["kernarg_segment_size"] >= 8 + 8 + 4 + 4 + 16 * 12 * 4 + 16 * 4 + 4, f


def test_k_pose_isa_has_no_fused_multiply_add(tmp_path):
    """Every product and sum of pose_vertex is rounded on its own: k_pose's ISA holds the nine
    v_mul_f32 and nine v_add_f32 of a vertex and no v_fma / v_mac / v_mad, and it moves a vertex
    with one 12-byte load and one 12-byte store."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "gfx950.co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _abi.lib_path(), fat], check=True)
    blob = open(fat, "rb").read()
    pos = 32
    for _ in range(struct.unpack_from("<Q", blob, 24)[0]):
        off, size, tl = struct.unpack_from("<QQQ", blob, pos)
        triple = blob[pos + 24:pos + 24 + tl].decode()
        pos += 24 + tl
        if "gfx950" in triple:
            open(co, "wb").write(blob[off:off + size])
    text = subprocess.run([os.path.join(rocm, "llvm", "bin", "llvm-objdump"), "-d", "--no-show-raw-insn", co],
                          check=True, capture_output=True, text=True).stdout
    body = re.search(r"<_ZN\w*k_pose\w*>:\n(.*?)(?:\n\n|\Z)", text, re.S).group(1)
    ops = re.findall(r"^\s*(\w+)", body, re.M)
    fused = [o for o in ops if re.match(r"v_(pk_)?(fma|mac|mad|fmac)", o) and "u32" not in o and "u64" not in o]
    assert not fused, fused
    assert sum(o.startswith("v_mul_f32") for o in ops) == 9 and sum(o.startswith("v_add_f32") for o in ops) == 9, ops
    assert ops.count("global_load_dwordx3") == 1 and ops.count("global_store_dwordx3") == 1
    assert not any(o.startswith(("scratch_", "ds_")) for o in ops)


def _sanitizer_runtime(hipcc):
    r = subprocess.run([hipcc, "--cuda-host-only", "-print-file-name=libclang_rt.asan-x86_64.a"],
                       capture_output=True, text=True)
    path = r.stdout.strip()
    return r.returncode == 0 and os.path.isabs(path) and os.path.exists(path)


def test_host_arithmetic_under_sanitizers(tmp_path):
    """tools/pose_san.cpp: a stand-alone program over xrt_pose_triangles and xrt_pose_rotation
    (csrc/xrt_pose_host.inc, host-compiled) with AddressSanitizer and UBSan.  Nothing is loaded
    into Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "pose_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "pose_san.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "pose_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
