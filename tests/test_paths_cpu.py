"""The paths model and the spectrum integrator without a GPU: the kernels'
resources, the argument checks that need no device, the CLI's option errors
and the consistency of the references the GPU tests compare against."""
import os
import subprocess

import numpy as np

import materials_kit as kit
import spectrum_kit as skit
import spectrum_ref
from simpleraytracing_amd import _abi
from conftest import ROOT, bits
from test_materials_cpu import _render_kernel_metadata
from test_spectrum_cpu import _write_obj

F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


# ---------------------------------------------------------------- the kernels' resources
def test_paths_kernels_use_no_scratch_and_no_more_lds():
    """Model 4's instantiations of k_render_brute / k_render_binned spill nothing; the binned
    one parks its overflowed rays' distances in the wave's record stage (the signed model's
    8192 bytes of LDS) and keeps 5 waves per SIMD (<= 96 VGPRs).  k_apply_spectrum holds its
    distances in registers and LDS: no scratch.  (profiles/paths/resources.txt has every
    figure beside the parent commit's.)"""
    meta = _render_kernel_metadata()
    brute = [f for k, f in meta.items() if "k_render_bruteILj4E" in k]
    binned = [f for k, f in meta.items() if "k_render_binnedILj4E" in k]
    assert len(brute) == 1 and len(binned) == 1, sorted(meta)
    for f in brute + binned:
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, f
    assert binned[0]["group_segment_fixed_size"] == 8192 and binned[0]["vgpr_count"] <= 96, binned[0]
    apply = [f for k, f in meta.items() if "k_apply_spectrum" in k]
    assert len(apply) >= 1, sorted(meta)
    for f in apply:
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, f


# ---------------------------------------------------------------- arguments
def test_apply_spectrum_checks_the_table_before_the_context():
    lib = _abi.load()
    n, M = 4, 3
    paths = np.zeros((M, n), F)
    opn = np.zeros(n, np.uint16)
    out = np.zeros(n, F)

    def call(w, mu, M, K):
        w = np.ascontiguousarray(w, F)
        mu = np.ascontiguousarray(mu, F)
        rc = lib.xrt_apply_spectrum(None, n, M, paths.ctypes.data_as(_abi._fp), opn.ctypes.data_as(_abi._u16p),
                                    w.ctypes.data_as(_abi._fp), mu.ctypes.data_as(_abi._fp), K,
                                    out.ctypes.data_as(_abi._fp))
        return rc, lib.xrt_last_error(None).decode()

    good_w, good_mu = [1.0, 2.0], [[0.1, 0.2], [0.0, 0.3], [0.5, 0.5]]
    cases = [
        ([1.0, 0.0], good_mu, 3, 2, "weight"),
        (good_w, [[0.1, 0.2], [0.0, -0.3], [0.5, 0.5]], 3, 2, "coefficient"),
        (good_w, [[0.1, 0.2], [0.0, 0.3], [0.5, np.nan]], 3, 2, "coefficient"),
        ([1.0] * 33, np.full((3, 33), 0.1, F), 3, 33, "bins"),
        ([1.0], np.full((17, 1), 0.1, F), 17, 1, "meshes"),
        (good_w, good_mu, 0, 2, "meshes"),
    ]
    for w, mu, m, K, word in cases:
        rc, msg = call(w, mu, m, K)
        assert rc == _abi.XRT_ERR_ARGUMENT and word in msg, (w, m, K, msg)
    rc, msg = call(good_w, good_mu, 3, 2)              # a good table: only the context is missing
    assert rc == _abi.XRT_ERR_ARGUMENT and "context is NULL" in msg
    assert not out.any()


def test_paths_entries_refuse_a_null_context():
    lib = _abi.load()
    assert lib.xrt_set_paths(None) == _abi.XRT_ERR_ARGUMENT
    cam = _abi.Camera()
    buf = np.zeros(16, F)
    assert lib.xrt_render_paths(None, cam, 0, 1, 1, buf.ctypes.data_as(_abi._fp), None, None) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_render_paths_device(None, cam, 0, 1, 1, None, None, None) == _abi.XRT_ERR_ARGUMENT
    assert _abi.XRT_MODEL_PATHS == 4


# ---------------------------------------------------------------- xrt_main --paths
def test_cli_paths_option_errors(tmp_path):
    """Each fails before a device is opened: exit 1 and ERROR: ... on stderr."""
    meshes = kit.phantom()
    _write_obj(tmp_path / "a.obj", meshes[0])
    _write_obj(tmp_path / "b.obj", meshes[1])
    inputs = ["-i", str(tmp_path / "a.obj"), "-i", str(tmp_path / "b.obj")]

    def run(*more):
        r = subprocess.run([EXE, "-s", "16", "16", "--paths", *inputs, *more], capture_output=True, text=True,
                           cwd=tmp_path, timeout=120)
        assert r.returncode == 1 and r.stderr.startswith("ERROR: "), (more, r.returncode, r.stderr)
        return r.stderr

    assert "give one" in run("--signed")
    assert "give one" in run("--materials", "0.1,0.2")
    run("--rows", "0:4")
    run("--batch", "3")
    run("-g", "2")
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert "--paths" in r.stdout + r.stderr


# ---------------------------------------------------------------- the references
def test_integrating_the_sums_is_the_spectrum_reference():
    """The GPU tests compare the planes with spectrum_ref.sums and the applied planes with
    spectrum_ref.integrate: together they are the spectrum model's reference of the phantom."""
    W, H = 96, 80
    su = skit.phantom_sums(W, H)
    w, mu = skit.phantom_table(4)
    got = spectrum_ref.integrate(su.distance, su.sign_sum, w, mu)
    assert np.array_equal(bits(got), bits(skit.phantom_ref(W, H, 4).lbuffer))
    assert su.distance.shape == (W * H, 5) and su.distance.dtype == F
    assert not np.isnan(su.distance).any()
