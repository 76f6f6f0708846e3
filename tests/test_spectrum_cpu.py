"""The spectrum model without a GPU: the anchors that tie the tests' reference
(spectrum_ref.py) to the oracle's pinned signed model and to the materials
reference, the host build of the shared per-ray function against numpy with
glibc's exp, the table's argument checks and the --spectrum file parser."""
import os
import subprocess

import numpy as np
import pytest

import materials_kit as kit
import spectrum_kit as skit
import spectrum_ref
from simpleraytracing_amd import _abi
from oracle import oracle
from conftest import ROOT, bits
from scene_kit import corner_soup, plane_stack, striped_sheets, synthetic_soup
from test_materials_cpu import _render_kernel_metadata

F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


def host_batch(distance, sign_sum, weights, mu):
    w = np.ascontiguousarray(weights, F).reshape(-1)
    mu = np.ascontiguousarray(mu, F).reshape(-1, w.size)
    d = np.ascontiguousarray(distance, F).reshape(-1, mu.shape[0])
    s = None if sign_sum is None else np.ascontiguousarray(sign_sum, np.int32).reshape(d.shape)
    out = np.empty(len(d), F)
    _abi.load().xrt_host_spectrum_lbuffer_batch(
        d.ctypes.data_as(_abi._fp), s.ctypes.data_as(_abi._i32p) if s is not None else None,
        w.ctypes.data_as(_abi._fp), mu.ctypes.data_as(_abi._fp), mu.shape[0], w.size,
        out.ctypes.data_as(_abi._fp), len(d))
    return out


# ---------------------------------------------------------------- the reference's anchors
@pytest.mark.parametrize("name,W,H", [("sheets", 96, 80), ("corner", 33, 31), ("soup", 80, 72), ("stack", 24, 24)])
def test_reference_with_one_bin_and_one_mesh_is_the_oracles_signed_model(name, W, H):
    soup = {"sheets": striped_sheets, "corner": corner_soup, "soup": lambda: synthetic_soup(seed=9, n=2000),
            "stack": lambda: plane_stack(40, alternate=True)}[name]()
    cam = oracle.camera_for_scene([soup], W, H)
    r = spectrum_ref.render([soup], [80.0], [[0.1037]], cam, W, H)
    rlb, rnh, flagged = oracle.render_signed_rows([soup], cam, W, H)
    assert np.array_equal(bits(r.lbuffer), bits(rlb))
    assert np.array_equal(r.nhits, rnh) and r.flagged == flagged


def test_reference_flags_and_hits_are_the_materials_references():
    W, H = 96, 80
    r = skit.phantom_ref(W, H, 4)
    m = kit.phantom_ref(W, H)
    assert np.array_equal(r.lbuffer == F(-1.0), m.lbuffer == F(-1.0))
    assert np.array_equal(r.flagged_by, m.flagged_by) and r.flagged == m.flagged
    assert np.array_equal(r.mesh_hits, m.mesh_hits) and np.array_equal(r.nhits, m.nhits)
    skit.check_exercised(r, m, 20)


# ---------------------------------------------------------------- the shared function, host build
@pytest.mark.parametrize("K", [1, 4, 32])
def test_host_batch_on_the_phantoms_sums(K):
    su = skit.phantom_sums(96, 80)
    w, mu = skit.ONE_BIN if K == 1 else skit.phantom_table(K)
    want = spectrum_ref.integrate(su.distance, su.sign_sum, w, mu)
    got = host_batch(su.distance, su.sign_sum, w, mu)
    assert np.array_equal(bits(got), bits(want))
    assert np.count_nonzero(got == F(-1.0)) >= 20 and np.unique(bits(got)).size > 100


def test_host_batch_crafted_rows():
    d, s, w, mu = skit.crafted_rows()
    got = host_batch(d, s, w, mu)
    want = spectrum_ref.integrate(d, s, w, mu)
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert got[0] == F(80.0) and got[2] > F(80.0)
    assert got[3] == -1.0 and got[4] == -1.0 and got[5] == -1.0 and got[14] == -1.0
    assert got[6] == 0.0 and got[7] == np.inf
    for k in (8, 9, 10, 11, 12):
        assert bits(got)[k] == 0x7FC00000, k
    assert np.isfinite(got[1]) and np.isfinite(got[13]) and got[13] > F(1e6)


def test_host_batch_one_bin_one_mesh_is_the_signed_update():
    d = np.arange(0, 1 << 32, 8191, dtype=np.uint64).astype(np.uint32).view(F)
    d = d[~np.isnan(d)]
    s = (np.arange(d.size) % 7 == 0).astype(np.int32)
    want = np.empty_like(d)
    _abi.load().xrt_host_signed_lbuffer_batch(d.ctypes.data_as(_abi._fp), s.ctypes.data_as(_abi._i32p), F(0.1037),
                                              want.ctypes.data_as(_abi._fp), d.size)
    assert np.array_equal(bits(host_batch(d, s, [80.0], [[0.1037]])), bits(want))


def test_skipping_a_mesh_the_ray_did_not_hit_is_exact():
    """The kernels leave out the meshes no lane hit: the same rows with those columns removed."""
    rng = np.random.default_rng(5)
    w, mu = skit.table(5, 8)
    d = rng.uniform(-40, 120, (4000, 5)).astype(F)
    d[:, 1] = 0.0
    d[:, 3] = 0.0
    keep = [0, 2, 4]
    assert np.array_equal(bits(host_batch(d, None, w, mu)), bits(host_batch(d[:, keep], None, w, mu[keep])))


@pytest.mark.parametrize("K", [1, 2, 7, 32])
def test_miss_value_is_the_weight_chain(K):
    w, mu = skit.table(3, K, seed=K)
    want = spectrum_ref.miss_value(w)
    got = _abi.load().xrt_host_spectrum_miss(w.ctypes.data_as(_abi._fp), K)
    assert bits(np.array([got], F))[0] == bits(np.array([want], F))[0]
    # ... and what the shared function gives a ray of zero distances
    assert bits(host_batch(np.zeros((1, 3), F), None, w, mu))[0] == bits(np.array([want], F))[0]
    assert bits(spectrum_ref.integrate(np.zeros((1, 3), F), None, w, mu))[0] == bits(np.array([want], F))[0]


# ---------------------------------------------------------------- arguments
def test_set_spectrum_argument_errors_need_no_device():
    """The table is checked before the context: without one, xrt_last_error(NULL) says what is wrong."""
    lib = _abi.load()

    def call(w, mu, M, K):
        w = None if w is None else np.ascontiguousarray(w, F)
        mu = None if mu is None else np.ascontiguousarray(mu, F)
        rc = lib.xrt_set_spectrum(None, None if w is None else w.ctypes.data_as(_abi._fp),
                                  None if mu is None else mu.ctypes.data_as(_abi._fp), M, K)
        return rc, lib.xrt_last_error(None).decode()

    good_w, good_mu = [1.0, 2.0], [[0.1, 0.2], [0.0, 0.3], [0.5, 0.5]]
    cases = [
        (None, good_mu, 3, 2, "weight is NULL"), (good_w, None, 3, 2, "mu is NULL"),
        (good_w, good_mu, 0, 2, "meshes"), (good_w, good_mu, _abi.XRT_MAX_MESHES + 1, 2, "meshes"),
        (good_w, good_mu, 3, 0, "bins"), (good_w, good_mu, 3, _abi.XRT_MAX_BINS + 1, "bins"),
        ([1.0, 0.0], good_mu, 3, 2, "weight"), ([1.0, -1.0], good_mu, 3, 2, "weight"),
        ([np.nan, 1.0], good_mu, 3, 2, "weight"), ([1.0, np.inf], good_mu, 3, 2, "weight"),
        (good_w, [[0.1, 0.2], [0.0, -0.3], [0.5, 0.5]], 3, 2, "coefficient"),
        (good_w, [[0.1, 0.2], [0.0, 0.3], [0.5, np.nan]], 3, 2, "coefficient"),
        (good_w, [[np.inf, 0.2], [0.0, 0.3], [0.5, 0.5]], 3, 2, "coefficient"),
    ]
    for w, mu, M, K, word in cases:
        rc, msg = call(w, mu, M, K)
        assert rc == _abi.XRT_ERR_ARGUMENT and word in msg, (w, mu, M, K, msg)
    rc, msg = call(good_w, good_mu, 3, 2)              # a good table: only the context is missing
    assert rc == _abi.XRT_ERR_ARGUMENT and "context is NULL" in msg


# ---------------------------------------------------------------- xrt_main --spectrum FILE
def _write_obj(path, soup):
    with open(path, "w") as f:
        for t in soup:
            for k in range(3):
                f.write("v %r %r %r\n" % tuple(float(x) for x in t[3 * k:3 * k + 3]))
        for i in range(len(soup)):
            f.write(f"f {3 * i + 1} {3 * i + 2} {3 * i + 3}\n")


def _main(tmp_path, *args):
    return subprocess.run([EXE, "-s", "16", "16", *args], capture_output=True, text=True, cwd=tmp_path, timeout=120)


def test_cli_spectrum_file_errors(tmp_path):
    """Each fails before a device is opened: exit 1 and ERROR: ... on stderr."""
    meshes = kit.phantom()
    _write_obj(tmp_path / "a.obj", meshes[0])
    _write_obj(tmp_path / "b.obj", meshes[1])
    inputs = ["-i", str(tmp_path / "a.obj"), "-i", str(tmp_path / "b.obj")]

    def run(text, *more):
        (tmp_path / "s.txt").write_text(text)
        r = _main(tmp_path, "--spectrum", str(tmp_path / "s.txt"), *inputs, *more)
        assert r.returncode == 1 and r.stderr.startswith("ERROR: "), (r.returncode, r.stderr)
        return r.stderr

    good = "# weights\n40 30 10\n0.2 0.1 0.05  # tissue\n\n0.5 0.3 0.2\n"
    assert "coefficients in a row" in run("40 30 10\n0.2 0.1 0.05\n0.5 0.3\n")            # a ragged row
    assert "coefficients in a row" in run("40 30 10\n0.2 0.1 0.05 0.01\n0.5 0.3 0.2\n")
    assert "one row of coefficients per mesh" in run("40 30 10\n0.2 0.1 0.05\n")            # 1 row, 2 meshes
    assert "one row of coefficients per mesh" in run(good + "0.1 0.1 0.1\n")                # 3 rows, 2 meshes
    assert "not a number" in run("40 30 x\n0.2 0.1 0.05\n0.5 0.3 0.2\n")
    assert "not a number" in run("40 30 10\n0.2 0.1 0.05mm\n0.5 0.3 0.2\n")
    assert "no weights" in run("# nothing\n\n")
    assert "no mesh's coefficients" in run("40 30 10\n")
    assert "at most 32" in run(" ".join(["1"] * 33) + "\n" + " ".join(["0.1"] * 33) + "\n" * 2)
    assert "give one" in run(good, "--signed")
    assert "give one" in run(good, "--materials", "0.1,0.2")
    r = _main(tmp_path, "--spectrum", str(tmp_path / "missing.txt"), *inputs)
    assert r.returncode == 1 and "cannot read" in r.stderr


# ---------------------------------------------------------------- the kernels' resources
def test_spectrum_kernels_use_no_scratch_and_no_more_lds():
    """The model's instantiations of k_render_brute / k_render_binned (model 3) spill nothing;
    the binned one parks its distances in the wave's record stage -- the signed model's 8192
    bytes of LDS, no more -- and keeps the 5 waves per SIMD its attribute asks for (<= 96
    VGPRs).  (profiles/spectrum/resources.txt has every figure beside the parent commit's.)"""
    meta = _render_kernel_metadata()
    inst = {k: v for k, v in meta.items() if "k_render_bruteILj3E" in k or "k_render_binnedILj3E" in k}
    assert len(inst) == 2, sorted(meta)
    for name, f in inst.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
    binned = [f for k, f in inst.items() if "k_render_binned" in k][0]
    assert binned["vgpr_count"] <= 96 and binned["group_segment_fixed_size"] == 8192, binned
