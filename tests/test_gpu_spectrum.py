"""The spectrum model on the GPU (XRT_MODEL_SPECTRUM): energy bins with a
coefficient per mesh and bin.  References: tests/spectrum_ref.py (anchored to
the oracle and to the materials reference in tests/test_spectrum_cpu.py), bit
for bit, on the BRUTE and the BINNED kernel."""
import os
import subprocess

import numpy as np
import pytest

import materials_kit as kit
import simpleraytracing_amd as xrt
import spectrum_kit as skit
import spectrum_ref
from simpleraytracing_amd import _abi
from oracle import oracle
from conftest import ROOT, bits
from scene_kit import corner_soup, striped_sheets, synthetic_soup
from test_spectrum_cpu import _write_obj, host_batch

pytestmark = pytest.mark.gpu
F = np.float32
KERNELS = [xrt.XRT_KERNEL_BRUTE, xrt.XRT_KERNEL_BINNED]
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


def cam13(cam):
    return np.array(list(cam.origin) + list(cam.detector) + list(cam.up) + list(cam.right) +
                    [cam.pixel_spacing], F)


@pytest.fixture(scope="module")
def sctx():
    """A context of this module's own: the models and scenes set here never reach other tests."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


@pytest.fixture
def spc(sctx):
    try:
        yield sctx
    finally:
        sctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
        sctx.set_hit_capacity(0)
        sctx.set_kernel(xrt.XRT_KERNEL_AUTO)


def check_frame(got, ref, W, H):
    """(image, lbuffer, u8, stats) of render_spectrum against the reference."""
    img, lb, u8, st = got
    bad = np.nonzero(bits(lb) != bits(ref.lbuffer))[0]
    assert bad.size == 0, (bad.size, bad[:8], lb[bad[:8]], ref.lbuffer[bad[:8]])
    rimg = oracle.hole_fill(ref.lbuffer, W, H)
    assert np.array_equal(bits(img), bits(rimg))
    assert np.array_equal(u8, skit.lut(rimg))
    assert st.odd_rays == ref.flagged
    assert st.hits == int(ref.nhits.sum()) and st.hit_rays == int(np.count_nonzero(ref.nhits))


# --------------------------------------------------------------------------- 1
def _one_mesh_case(name, dragon):
    if name == "dragon":
        return dragon, 128, 112
    if name == "sheets":
        return striped_sheets(), 96, 80
    if name == "corner":
        return corner_soup(), 33, 31
    return synthetic_soup(seed=9, n=2000), 80, 72


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["sheets", "soup", "corner", "dragon"])
def test_one_bin_one_mesh_equals_signed(spc, dragon, kernel, name):
    soup, W, H = _one_mesh_case(name, dragon)
    cam = xrt.camera_for_scene([soup], W, H)
    spc.set_kernel(kernel)
    spc.upload_scene([soup])
    spc.set_spectrum([80.0], [[0.1037]])
    img, lb, u8, st = spc.render_spectrum(cam)
    rlb, rnh, flagged = oracle.render_signed_rows([soup], cam13(cam), W, H)
    assert np.array_equal(bits(lb), bits(rlb)), np.nonzero(bits(lb) != bits(rlb))[0][:8]
    assert np.array_equal(bits(img), bits(oracle.hole_fill(rlb, W, H)))
    assert st.odd_rays == flagged and st.hits == int(rnh.sum()) and st.hit_rays == int(np.count_nonzero(rnh))


# --------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("K", [4, 32])
@pytest.mark.parametrize("W,H,floor", [(96, 80, 20), (67, 45, 1)])
def test_phantom(spc, kernel, K, W, H, floor):
    meshes = kit.phantom()
    ref = skit.phantom_ref(W, H, K)
    mref = kit.phantom_ref(W, H)
    kit.check_exercised(mref, kit.mesh0_only_ref(W, H), floor)
    skit.check_exercised(ref, mref, floor)
    w, mu = skit.phantom_table(K)
    assert np.array_equal(mu[:, 0], np.asarray(kit.PHANTOM_MU, F))
    cam = xrt.camera_for_scene(meshes, W, H)
    spc.set_kernel(kernel)
    spc.upload_scene(meshes)
    spc.set_spectrum(w, mu)
    got = spc.render_spectrum(cam)
    check_frame(got, ref, W, H)
    assert got[3].overflow_rays == int(np.count_nonzero(ref.nhits > 12))
    # the rays that miss hold the weight chain
    miss = ref.nhits == 0
    assert miss.any() and np.all(bits(got[1][miss]) == bits(np.array([spectrum_ref.miss_value(w)], F))[0])


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cap", [1, 2, 5])
def test_phantom_hit_capacity(spc, kernel, cap):
    """Every hit ray has more hits than the list holds (capacity 1) or many have: per-mesh
    distances and flags from SpectrumChain on the fix-up walks -- the survivor walk on the
    BINNED kernel's culled tiles, the full walk on the BRUTE kernel."""
    W, H = 67, 45
    meshes = kit.phantom()
    ref = skit.phantom_ref(W, H, 4)
    w, mu = skit.phantom_table(4)
    cam = xrt.camera_for_scene(meshes, W, H)
    spc.set_kernel(kernel)
    spc.set_hit_capacity(cap)
    spc.upload_scene(meshes)
    spc.set_spectrum(w, mu)
    got = spc.render_spectrum(cam)
    assert got[3].overflow_rays == int(np.count_nonzero(ref.nhits > cap)) > 0
    check_frame(got, ref, W, H)


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_bin_five_meshes_is_not_the_materials_model(spc, kernel):
    """One f32 rounding at the end, not one per mesh: the spectrum reference, and at least one
    pixel that is not the materials model's."""
    W, H = 96, 80
    meshes = kit.phantom()
    ref = skit.phantom_ref(W, H, 1)
    mref = kit.phantom_ref(W, H)
    differ = np.count_nonzero(bits(ref.lbuffer) != bits(mref.lbuffer))
    assert differ >= 1
    cam = xrt.camera_for_scene(meshes, W, H)
    spc.set_kernel(kernel)
    spc.upload_scene(meshes)
    spc.set_spectrum(*skit.ONE_BIN)
    got = spc.render_spectrum(cam)
    check_frame(got, ref, W, H)
    assert np.count_nonzero(bits(got[1]) != bits(mref.lbuffer)) == differ


# --------------------------------------------------------------------------- 5
@pytest.mark.parametrize("kernel", KERNELS)
def test_dragon_scene(spc, dragon, kernel):
    W, H = 128, 112
    meshes = kit.dragon_scene(dragon)
    w, mu = skit.table(3, 8)
    ref = spectrum_ref.from_sums(skit.dragon_sums(dragon, W, H), w, mu)
    in_meshes = (ref.mesh_hits > 0).sum(1)
    assert np.count_nonzero(in_meshes >= 2) > 1000 and np.count_nonzero(in_meshes == 3) > 100
    cam = xrt.camera_for_scene(meshes, W, H)
    spc.set_kernel(kernel)
    spc.upload_scene(meshes)
    spc.set_spectrum(w, mu)
    check_frame(spc.render_spectrum(cam), ref, W, H)


# --------------------------------------------------------------------------- 6
@pytest.mark.parametrize("kernel", KERNELS)
def test_sixteen_meshes_thirty_two_bins(spc, kernel):
    """The largest table and the largest parked-distance footprint."""
    W, H = 67, 45
    meshes = skit.sixteen_boxes()
    assert len(meshes) == xrt.XRT_MAX_MESHES
    w, mu = skit.table(16, 32)
    ref = spectrum_ref.from_sums(skit.boxes_sums(W, H), w, mu)
    in_meshes = (ref.mesh_hits > 0).sum(1)
    assert in_meshes.max() == 16 and np.count_nonzero(in_meshes >= 9) > 100 and np.count_nonzero(in_meshes == 0) > 20
    cam = xrt.camera_for_scene(meshes, W, H)
    spc.set_kernel(kernel)
    spc.upload_scene(meshes)
    spc.set_spectrum(w, mu)
    check_frame(spc.render_spectrum(cam), ref, W, H)
    spc.set_hit_capacity(3)                            # ... and through the walks, every mesh parked
    check_frame(spc.render_spectrum(cam), ref, W, H)


# --------------------------------------------------------------------------- 7
def test_strips_assemble(spc):
    W, H = 96, 80
    meshes = kit.phantom()
    cam = xrt.camera_for_scene(meshes, W, H)
    spc.set_kernel(xrt.XRT_KERNEL_BINNED)
    spc.upload_scene(meshes)
    spc.set_spectrum(*skit.phantom_table(4))
    parts = [spc.render_rows(cam, r0, r1, image=False, u8=False)[1] for r0, r1 in [(0, 37), (37, 40), (40, H)]]
    assert np.array_equal(bits(np.concatenate(parts)), bits(skit.phantom_ref(W, H, 4).lbuffer))
    with pytest.raises(xrt.XrtError):          # the image is the hole fill's
        spc.render_rows(cam, 0, H)


# --------------------------------------------------------------------------- 8
@pytest.mark.parametrize("order", [(0, 1, 0, 1, 0, 1), (0, 0, 0, 0, 1, 0)], ids=["alternating", "repeating"])
def test_table_change_mid_sequence(spc, order):
    """Six device-entry frames over two cameras -- alternating, and one camera repeated so
    that its next frames are prepared ahead --, the table changed halfway (other values,
    another bin count) without a re-upload: every frame equals the reference of its camera
    and its table."""
    import torch
    W, H = 67, 45
    meshes = kit.phantom()
    wider = meshes + [kit.box((30, -40, -30), (95, 40, 30))]          # another bounding box: another camera
    cams = [xrt.camera_for_scene(meshes, W, H), xrt.camera_for_scene(wider, W, H)]
    tables = [skit.phantom_table(4), skit.table(5, 7, seed=3)]
    sums = [spectrum_ref.sums(meshes, cam13(c), W, H) for c in cams]
    refs = {(c, t): spectrum_ref.from_sums(sums[c], *tables[t]).lbuffer for c in range(2) for t in range(2)}
    assert not np.array_equal(bits(refs[(0, 0)]), bits(refs[(0, 1)]))
    assert not np.array_equal(bits(refs[(0, 0)]), bits(refs[(1, 0)]))
    spc.set_kernel(xrt.XRT_KERNEL_BINNED)
    spc.upload_scene(meshes)
    spc.set_spectrum(*tables[0])
    planes = [torch.zeros(W * H, dtype=torch.float32, device="cuda") for _ in range(6)]
    for k in range(6):
        if k == 3:
            spc.set_spectrum(*tables[1])
        spc.render_rows_device(cams[order[k]], 0, H, 0, planes[k].data_ptr(), 0)
    torch.cuda.synchronize()
    spc.read_stats()
    for k in range(6):
        want = refs[(order[k], 0 if k < 3 else 1)]
        assert np.array_equal(bits(planes[k].cpu().numpy()), bits(want)), k


# --------------------------------------------------------------------------- 9
@pytest.mark.parametrize("kernel", KERNELS)
def test_switching_models(spc, kernel):
    """spectrum -> materials -> signed -> spectrum on one context: each model's own frame."""
    W, H = 67, 45
    meshes = kit.phantom()
    cam = xrt.camera_for_scene(meshes, W, H)
    w, mu = skit.phantom_table(4)
    spc.set_kernel(kernel)
    spc.upload_scene(meshes)
    spc.set_spectrum(w, mu)
    check_frame(spc.render_spectrum(cam), skit.phantom_ref(W, H, 4), W, H)
    spc.set_materials(kit.PHANTOM_MU)
    with pytest.raises(xrt.XrtError):                  # render_spectrum needs set_spectrum
        spc.render_spectrum(cam)
    _, lb, _, st = spc.render_materials(cam)
    assert np.array_equal(bits(lb), bits(kit.phantom_ref(W, H).lbuffer)) and st.odd_rays == kit.phantom_ref(W, H).flagged
    spc.set_model(xrt.XRT_MODEL_SIGNED, 0.1037)
    _, slb, _, sst = spc.render_signed(cam)
    rs, rsn, flagged = oracle.render_signed_rows(meshes, cam13(cam), W, H)
    assert np.array_equal(bits(slb), bits(rs)) and sst.odd_rays == flagged and sst.hits == int(rsn.sum())
    with pytest.raises(xrt.XrtError):
        spc.render_materials(cam)
    spc.set_spectrum(w, mu)
    check_frame(spc.render_spectrum(cam), skit.phantom_ref(W, H, 4), W, H)


# --------------------------------------------------------------------------- 10
def test_probe(sctx):
    d, s, w, mu = skit.crafted_rows()
    got = sctx.probe_spectrum(d, s, w, mu)
    assert np.array_equal(bits(got), bits(host_batch(d, s, w, mu))), got
    assert np.array_equal(bits(got), bits(spectrum_ref.integrate(d, s, w, mu)))
    for k in (8, 9, 10, 11, 12):
        assert bits(got)[k] == 0x7FC00000, k
    assert got[6] == 0.0 and got[7] == np.inf and got[3] == -1.0 and got[14] == -1.0
    # the phantom's sums under the largest table, and a stride over the finite and infinite
    # f32 distances in mesh 0 (its NaNs are not the model's), finite ones after it
    su = skit.phantom_sums(96, 80)
    w, mu = skit.phantom_table(32)
    assert np.array_equal(bits(sctx.probe_spectrum(su.distance, su.sign_sum, w, mu)),
                          bits(host_batch(su.distance, su.sign_sum, w, mu)))
    d0 = np.arange(0, 1 << 32, 4099, dtype=np.uint64).astype(np.uint32).view(F)
    d0 = d0[~np.isnan(d0)]
    rng = np.random.default_rng(23)
    dd = np.stack([d0, rng.uniform(-30, 30, d0.size).astype(F), rng.uniform(-5, 200, d0.size).astype(F)], 1)
    w, mu = skit.table(3, 4)
    assert np.array_equal(bits(sctx.probe_spectrum(dd, None, w, mu)), bits(host_batch(dd, None, w, mu)))


# --------------------------------------------------------------------------- 11
def test_errors(spc):
    meshes = kit.phantom()
    W, H = 24, 24
    cam = xrt.camera_for_scene(meshes, W, H)
    spc.upload_scene(meshes)
    w, mu = skit.phantom_table(4)
    bad_tables = [
        ([1.0, 0.0, 1.0, 1.0], mu), ([1.0, -2.0, 1.0, 1.0], mu), ([1.0, np.nan, 1.0, 1.0], mu),
        ([np.inf, 1.0, 1.0, 1.0], mu), (w, -mu), (w, np.where(mu == mu[2, 1], np.nan, mu)),
        (w, np.where(mu == mu[0, 0], np.inf, mu)), ([1.0] * 33, np.full((5, 33), 0.1, F)),
        ([1.0], np.full((17, 1), 0.1, F)), ([], np.zeros((5, 0), F)),
    ]
    for bw, bmu in bad_tables:
        with pytest.raises(xrt.XrtError) as e:
            spc.set_spectrum(bw, bmu)
        assert e.value.code == _abi.XRT_ERR_ARGUMENT
    with pytest.raises(ValueError):                     # mu is (M, K)
        spc.set_spectrum(w, mu.T)
    spc.set_spectrum(w, mu[:3])                         # three meshes' rows, five meshes
    with pytest.raises(xrt.XrtError) as e:
        spc.render_spectrum(cam)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT
    spc.set_spectrum(w, mu)
    with pytest.raises(xrt.XrtError):                  # the L-buffer plane only
        spc.render_rows(cam, 0, H)
    spc.set_kernel(xrt.XRT_KERNEL_TILED)
    with pytest.raises(xrt.XrtError):                  # BRUTE or BINNED
        spc.render_spectrum(cam)
    spc.set_kernel(xrt.XRT_KERNEL_AUTO)
    spc.set_model(xrt.XRT_MODEL_SIGNED, 0.1037)
    with pytest.raises(xrt.XrtError):                  # render_spectrum needs set_spectrum
        spc.render_spectrum(cam)
    spc.set_spectrum(w, mu)                             # and the context still renders
    _, lb, _, _ = spc.render_spectrum(cam)
    assert np.array_equal(bits(lb), bits(spectrum_ref.render(meshes, w, mu, cam13(cam), W, H).lbuffer))


# --------------------------------------------------------------------------- 12
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_multi_strips(spc, devices):
    W, H = 96, 80
    meshes = kit.phantom()
    cam = xrt.camera_for_scene(meshes, W, H)
    w, mu = skit.phantom_table(4)
    spc.set_kernel(xrt.XRT_KERNEL_BINNED)
    spc.upload_scene(meshes)
    spc.set_spectrum(w, mu)
    one = spc.render_spectrum(cam)
    check_frame(one, skit.phantom_ref(W, H, 4), W, H)
    with xrt.MultiContext(devices) as m:
        m.set_kernel(xrt.XRT_KERNEL_BINNED)
        m.upload_scene(meshes)
        m.set_spectrum(w, mu)
        for _ in range(3):                              # the strip buffers rotate
            img, lb, u8, st = m.render_spectrum(cam)
            assert np.array_equal(bits(lb), bits(one[1])) and np.array_equal(bits(img), bits(one[0]))
            assert np.array_equal(u8, one[2]) and st.odd_rays == one[3].odd_rays and st.hits == one[3].hits


# --------------------------------------------------------------------------- 13
@pytest.mark.parametrize("gpus", [1, 2])
def test_cli_spectrum(tmp_path, gpus):
    meshes = kit.phantom()
    _write_obj(tmp_path / "tissue.obj", meshes[0])
    _write_obj(tmp_path / "sheets.obj", meshes[4])
    (tmp_path / "out").mkdir()
    (tmp_path / "beam.txt").write_text("# three bins\n40 25.5 14.5   # weights\n\n0.2059 0.1037 0.08  # tissue\n"
                                       "0.05 0 0.025\n")
    w, mu = [40.0, 25.5, 14.5], [[0.2059, 0.1037, 0.08], [0.05, 0.0, 0.025]]
    env = dict(os.environ, XRT_MULTI_DEVICES="0,0") if gpus > 1 else dict(os.environ)
    r = subprocess.run([EXE, "--spectrum", str(tmp_path / "beam.txt"), "-s", "67", "45", "-i",
                        str(tmp_path / "tissue.obj"), "-i", str(tmp_path / "sheets.obj"), "-f", "s.txt",
                        "--lbuffer", str(tmp_path / "s.f32")] + (["-g", "2"] if gpus > 1 else []),
                       capture_output=True, text=True, cwd=tmp_path, timeout=300, env=env)
    assert r.returncode == 0, r.stderr
    scene = [xrt.load_meshes(str(tmp_path / "tissue.obj"))[0], xrt.load_meshes(str(tmp_path / "sheets.obj"))[0]]
    assert np.array_equal(scene[0], meshes[0]) and np.array_equal(scene[1], meshes[4])
    ref = spectrum_ref.render(scene, w, mu, oracle.camera_for_scene(scene, 67, 45), 67, 45)
    assert ref.flagged > 20
    assert np.array_equal(bits(np.fromfile(tmp_path / "s.f32", F)), bits(ref.lbuffer))
    assert (tmp_path / "out" / "s.txt").read_bytes() == oracle.text_bytes(oracle.hole_fill(ref.lbuffer, 67, 45), 67, 45)
