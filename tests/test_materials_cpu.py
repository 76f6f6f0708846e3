"""The materials model without a GPU: the host build of the chained L update
against numpy with glibc's exp, and the two anchors that tie the tests'
reference (materials_ref.py) to the oracle's pinned signed model."""
import numpy as np
import pytest

import materials_kit as kit
import materials_ref
from simpleraytracing_amd import _abi
from oracle import oracle
from conftest import bits
from scene_kit import corner_soup, plane_stack, striped_sheets, synthetic_soup

F = np.float32
NAN_POS = np.array([0x7FC00000], np.uint32).view(F)[0]
NAN_NEG = np.array([0xFFC00000], np.uint32).view(F)[0]


def host_chain(distance, sign_sum, mu):
    d = np.ascontiguousarray(distance, F)
    mu = np.ascontiguousarray(mu, F)
    d = d.reshape(-1, mu.size)
    s = None if sign_sum is None else np.ascontiguousarray(sign_sum, np.int32).reshape(d.shape)
    out = np.empty(len(d), F)
    _abi.load().xrt_host_materials_lbuffer_batch(
        d.ctypes.data_as(_abi._fp), s.ctypes.data_as(_abi._i32p) if s is not None else None,
        mu.ctypes.data_as(_abi._fp), mu.size, out.ctypes.data_as(_abi._fp), len(d))
    return out


def numpy_chain(distance, sign_sum, mu):
    """The issue's loop, every mesh applied: x86 arithmetic through numpy, glibc exp."""
    mu = np.asarray(mu, F)
    d = np.asarray(distance, F).reshape(-1, mu.size)
    s = np.zeros(d.shape, np.int32) if sign_sum is None else np.asarray(sign_sum, np.int32).reshape(d.shape)
    L = np.full(len(d), 80.0, F)
    with np.errstate(all="ignore"):
        for m in range(mu.size):
            live = ~(L == F(-1.0))
            flag = live & (s[:, m] != 0)
            upd = live & ~flag
            e = oracle.exp(-(np.float64(mu[m]) * (d[upd, m].astype(np.float64) * 0.1)))
            L[upd] = (L[upd].astype(np.float64) * e).astype(F)
            L[flag] = F(-1.0)
    return L


def crafted_chains():
    """(distance (n, 3), sign_sum (n, 3), mu): the non-finite cases of the model, M = 3.
    (Both factors NaN with different signs is left out: C leaves the operand order,
    and with it the result's sign, to the compiler.)"""
    inf = F(np.inf)
    d = np.array([
        [NAN_NEG, 3.0, -2.5],        # 0: a NaN distance, then finite ones: 0x7FC00000, carried
        [-inf, inf, 1.0],            # 1: exp(+inf) = inf, then inf * 0: x86's default NaN 0xFFC00000, carried
        [NAN_NEG, 1.0, 2.0],         # 2
        [NAN_NEG, 5.0, 1.0],         # 3: NaN followed by a flag
        [1.0, 2.0, 3.0],             # 4: a flag in the last mesh
        [0.0, 0.0, 0.0],
        [inf, 1.0, 1.0],             # exp(-inf) = 0 stays 0
        [-800.0, -800.0, 900.0],     # the f32 L overflows to inf, then inf * 0
        [1e4, -1e4, 0.0],
    ], F)
    s = np.zeros(d.shape, np.int32)
    s[3, 1] = 2
    s[4, 2] = -1
    return d, s, np.array([0.1037, 0.3971, 0.2], F)


def test_host_chain_crafted():
    d, s, mu = crafted_chains()
    got = host_chain(d, s, mu)
    assert np.array_equal(bits(got), bits(numpy_chain(d, s, mu)))
    assert bits(got)[0] == 0x7FC00000 and bits(got)[1] == 0xFFC00000 and got[3] == -1.0 and got[4] == -1.0


def test_host_chain_zero_mu_and_infinite_distance():
    """mu == 0 with an infinite distance: 0 * inf, a NaN exponent like a NaN distance's."""
    d = np.array([[np.inf, 1.0], [1.0, -np.inf], [2.0, 3.0]], F)
    mu = np.array([0.0, 0.0], F)
    got = host_chain(d, None, mu)
    assert np.array_equal(bits(got), bits(numpy_chain(d, None, mu)))
    assert bits(got)[0] == 0x7FC00000 and got[2] == 80.0


def test_host_chain_stride_over_f32_distances():
    """A stride over all f32 distances in mesh 0, finite distances after it."""
    d0 = np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32).view(F)
    rng = np.random.default_rng(17)
    d = np.stack([d0, rng.uniform(-30, 30, d0.size).astype(F), rng.uniform(-5, 200, d0.size).astype(F)], 1)
    mu = np.array([0.1037, 0.3971, 0.05], F)
    # NaN distances of either sign in mesh 0 are not the model's (its NaN is x86's default): keep finite and inf
    ok = ~np.isnan(d0)
    got = host_chain(d[ok], None, mu)
    assert np.array_equal(bits(got), bits(numpy_chain(d[ok], None, mu)))


def test_host_chain_one_mesh_is_the_signed_update():
    d = np.arange(0, 1 << 32, 8191, dtype=np.uint64).astype(np.uint32).view(F)
    d = d[~np.isnan(d)]
    s = (np.arange(d.size) % 7 == 0).astype(np.int32)
    want = np.empty_like(d)
    _abi.load().xrt_host_signed_lbuffer_batch(d.ctypes.data_as(_abi._fp), s.ctypes.data_as(_abi._i32p), F(0.1037),
                                              want.ctypes.data_as(_abi._fp), d.size)
    assert np.array_equal(bits(host_chain(d, s, [0.1037])), bits(want))


@pytest.mark.parametrize("name,W,H", [("sheets", 96, 80), ("corner", 33, 31), ("soup", 80, 72), ("stack", 24, 24)])
def test_reference_with_one_mesh_is_the_oracles_signed_model(name, W, H):
    soup = {"sheets": striped_sheets, "corner": corner_soup, "soup": lambda: synthetic_soup(seed=9, n=2000),
            "stack": lambda: plane_stack(40, alternate=True)}[name]()
    cam = oracle.camera_for_scene([soup], W, H)
    r = materials_ref.render([soup], [0.1037], cam, W, H)
    rlb, rnh, flagged = oracle.render_signed_rows([soup], cam, W, H)
    assert np.array_equal(bits(r.lbuffer), bits(rlb))
    assert np.array_equal(r.nhits, rnh) and r.flagged == flagged


def test_reference_with_the_mesh_filter_is_the_oracles_signed_model():
    meshes = kit.phantom()
    W, H = 96, 80
    cam = oracle.camera_for_scene(meshes, W, H)
    r = materials_ref.render(meshes, [0.1037, 0.3971, 0.3971, 0.3971, 0.3971], cam, W, H, mesh0_only=True)
    rlb, rnh, flagged = oracle.render_signed_rows(meshes, cam, W, H)
    assert np.array_equal(bits(r.lbuffer), bits(rlb))
    assert np.array_equal(r.nhits, rnh) and r.flagged == flagged


def test_phantom_exercises_the_model():
    """The scene's reference: overflowing rays, flags by several meshes, rays through
    several meshes (floors of 20 at 96 x 80, > 0 at 67 x 45)."""
    for (W, H), floor in (((96, 80), 20), ((67, 45), 1)):
        kit.check_exercised(kit.phantom_ref(W, H), kit.mesh0_only_ref(W, H), floor)


def _render_kernel_metadata():
    """{kernel name: {field: int}} of libxrt.so's gfx950 code object (its .hip_fatbin
    section is a clang offload bundle; the notes are read with ROCm's llvm-readelf)."""
    import os
    import re
    import struct
    import subprocess
    import tempfile
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", _abi.lib_path(), fat], check=True)
        blob = open(fat, "rb").read()
        assert blob[:24] == b"__CLANG_OFFLOAD_BUNDLE__"
        pos = 32
        for _ in range(struct.unpack_from("<Q", blob, 24)[0]):
            off, size, tl = struct.unpack_from("<QQQ", blob, pos)
            triple = blob[pos + 24:pos + 24 + tl].decode()
            pos += 24 + tl
            if "gfx950" in triple:
                open(co, "wb").write(blob[off:off + size])
        notes = subprocess.run([os.path.join(rocm, "llvm", "bin", "llvm-readelf"), "--notes", co], check=True,
                               capture_output=True, text=True).stdout
    out = {}
    for block in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def test_materials_kernels_use_no_scratch():
    """The new instantiations of k_render_brute / k_render_binned (model 2) spill nothing
    and the binned one keeps at least 5 waves per SIMD (<= 96 VGPRs of 512), the floor its
    amdgpu_waves_per_eu attribute asks for; the other models' instantiations still use no
    scratch either.  (profiles/materials/resources.txt has every figure beside the
    parent commit's.)"""
    meta = _render_kernel_metadata()
    inst = {m: {k: v for k, v in meta.items()
                if f"k_render_bruteILj{m}E" in k or f"k_render_binnedILj{m}E" in k} for m in (0, 1, 2)}
    for m in (0, 1, 2):
        assert len(inst[m]) == 2, sorted(meta)
        for name, f in inst[m].items():
            assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
    binned = [f for k, f in inst[2].items() if "k_render_binned" in k][0]
    assert binned["vgpr_count"] <= 96 and binned["group_segment_fixed_size"] == 8192, binned
