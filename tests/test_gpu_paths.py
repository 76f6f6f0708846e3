"""The paths model (XRT_MODEL_PATHS) and the device spectrum integrator
(xrt_apply_spectrum) on the GPU.  The planes are compared bit for bit with
tests/spectrum_ref.py's per-mesh sums, the integrated planes with
xrt_render_spectrum's L-buffer of the same context and with the reference, on
the BRUTE and the BINNED kernel."""
import functools
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
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
KERNELS = [xrt.XRT_KERNEL_BRUTE, xrt.XRT_KERNEL_BINNED]
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


def cam13(cam):
    return np.array(list(cam.origin) + list(cam.detector) + list(cam.up) + list(cam.right) +
                    [cam.pixel_spacing], F)


@pytest.fixture(scope="module")
def pctx():
    """A context of this module's own: the models and scenes set here never reach other tests."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


@pytest.fixture
def pth(pctx):
    try:
        yield pctx
    finally:
        pctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
        pctx.set_hit_capacity(0)
        pctx.set_kernel(xrt.XRT_KERNEL_AUTO)


def planes_of(su, W, H):
    """The reference's planes (M, H, W) and mask (H, W) of per-mesh sums (n, M)."""
    M = su.distance.shape[1]
    assert not np.isnan(su.distance).any()             # (the scenes of this module hold no NaN)
    mask = ((su.sign_sum != 0).astype(np.uint32) << np.arange(M, dtype=np.uint32)).sum(1).astype(np.uint16)
    return np.ascontiguousarray(su.distance.T).reshape(M, H, W), mask.reshape(H, W)


def same_planes(got, want):
    """Bit for bit where the reference is no NaN, NaN for NaN elsewhere."""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(bits(got)[~nan], bits(want)[~nan]) and np.isnan(got[nan]).all()


def check_paths(got, su, W, H, cap=12):
    paths, opn, st = got
    want, mask = planes_of(su, W, H)
    assert paths.dtype == F and opn.dtype == np.uint16
    bad = np.argwhere(bits(paths) != bits(want))
    assert same_planes(paths, want), (len(bad), bad[:8])
    assert np.array_equal(opn, mask), np.argwhere(opn != mask)[:8]
    for m in range(want.shape[0]):                      # the mask, bit by bit
        assert np.array_equal((opn >> m) & 1, (su.sign_sum[:, m] != 0).reshape(H, W)), m
    nhits = su.mesh_hits.sum(1)
    assert st.odd_rays == int(np.count_nonzero(mask))
    assert st.hits == int(nhits.sum()) and st.hit_rays == int(np.count_nonzero(nhits))
    assert st.overflow_rays == int(np.count_nonzero(nhits > cap))


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("W,H,floor", [(96, 80, 20), (67, 45, 1)])
def test_phantom(pth, kernel, W, H, floor):
    meshes = kit.phantom()
    su = skit.phantom_sums(W, H)
    mref = kit.phantom_ref(W, H)
    kit.check_exercised(mref, kit.mesh0_only_ref(W, H), floor)
    skit.check_exercised(skit.phantom_ref(W, H, 4), mref, floor)
    _, mask = planes_of(su, W, H)
    assert np.count_nonzero((mask >> 3) & 1) > 0 and np.count_nonzero((mask >> 4) & 1) > 0   # no disguised 0 / 1
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.set_kernel(kernel)
    pth.upload_scene(meshes)
    pth.set_paths()
    check_paths(pth.render_paths(cam), su, W, H)


# --------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cap", [1, 2, 5])
def test_phantom_hit_capacity(pth, kernel, cap):
    """Rays with more hits than the list holds take the walks (PathsChain) whether their signs
    cancel or not: the other models never compute a flagged overflowed ray's distances."""
    W, H = 67, 45
    meshes = kit.phantom()
    su = skit.phantom_sums(W, H)
    over = su.mesh_hits.sum(1) > cap
    assert np.count_nonzero(over & (su.sign_sum != 0).any(1)) >= 1
    assert np.count_nonzero(over & (su.sign_sum.sum(1) != 0)) >= 1      # ... with a non-zero global sum, too
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.set_kernel(kernel)
    pth.set_hit_capacity(cap)
    pth.upload_scene(meshes)
    pth.set_paths()
    check_paths(pth.render_paths(cam), su, W, H, cap)


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("kernel", KERNELS)
def test_dragon_scene(pth, dragon, kernel):
    W, H = 128, 112
    meshes = kit.dragon_scene(dragon)
    su = skit.dragon_sums(dragon, W, H)
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.set_kernel(kernel)
    pth.upload_scene(meshes)
    pth.set_paths()
    check_paths(pth.render_paths(cam), su, W, H)


@pytest.mark.parametrize("kernel", KERNELS)
def test_sixteen_boxes(pth, kernel):
    W, H = 67, 45
    meshes = skit.sixteen_boxes()
    su = skit.boxes_sums(W, H)
    assert (su.mesh_hits > 0).sum(1).max() == 16
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.set_kernel(kernel)
    pth.upload_scene(meshes)
    pth.set_paths()
    check_paths(pth.render_paths(cam), su, W, H)
    pth.set_hit_capacity(3)                             # ... and through the walks, every mesh parked
    check_paths(pth.render_paths(cam), su, W, H, 3)


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kernel", KERNELS)
def test_strips_assemble(pth, kernel):
    W, H = 96, 80
    meshes = kit.phantom()
    want, mask = planes_of(skit.phantom_sums(W, H), W, H)
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.set_kernel(kernel)
    pth.upload_scene(meshes)
    pth.set_paths()
    parts = [pth.render_paths(cam, r0, r1) for r0, r1 in [(0, 37), (37, 40), (40, H)]]
    assert [p[0].shape for p in parts] == [(5, 37, W), (5, 3, W), (5, 40, W)]
    assert same_planes(np.concatenate([p[0] for p in parts], 1), want)
    assert np.array_equal(np.concatenate([p[1] for p in parts], 0), mask)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("W,H", [(1, 1), (7, 13)])
def test_small_frames(pth, kernel, W, H):
    meshes = kit.phantom()
    cam = xrt.camera_for_scene(meshes, W, H)
    su = spectrum_ref.sums(meshes, cam13(cam), W, H)
    pth.set_kernel(kernel)
    pth.upload_scene(meshes)
    pth.set_paths()
    check_paths(pth.render_paths(cam), su, W, H)


# --------------------------------------------------------------------------- 5
def _apply_case(name, dragon):
    if name == "dragon":
        meshes = kit.dragon_scene(dragon)
        return meshes, 128, 112, skit.dragon_sums(dragon, 128, 112), skit.table(3, 8)
    if name == "boxes":
        return skit.sixteen_boxes(), 67, 45, skit.boxes_sums(67, 45), skit.table(16, 32)
    W, H, K = {"phantom-96-4": (96, 80, 4), "phantom-96-32": (96, 80, 32), "phantom-67-4": (67, 45, 4),
               "phantom-67-32": (67, 45, 32)}[name]
    return kit.phantom(), W, H, skit.phantom_sums(W, H), skit.phantom_table(K)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("name", ["phantom-96-4", "phantom-96-32", "phantom-67-4", "phantom-67-32", "dragon", "boxes"])
def test_apply_equals_the_spectrum_render(pth, dragon, kernel, name):
    meshes, W, H, su, (w, mu) = _apply_case(name, dragon)
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.set_kernel(kernel)
    pth.upload_scene(meshes)
    pth.set_paths()
    paths, opn, _ = pth.render_paths(cam)
    got = pth.apply_spectrum(paths, opn, w, mu)
    assert got.shape == (H, W) and got.dtype == F
    ref = spectrum_ref.from_sums(su, w, mu)
    assert np.array_equal(bits(got.reshape(-1)), bits(ref.lbuffer)), np.nonzero(bits(got.reshape(-1)) != bits(ref.lbuffer))[0][:8]
    miss = ref.nhits == 0
    assert miss.any() and np.all(bits(got.reshape(-1)[miss]) == bits(np.array([spectrum_ref.miss_value(w)], F))[0])
    pth.set_spectrum(w, mu)                             # the model that traces and integrates in one kernel
    _, lb, _, _ = pth.render_spectrum(cam)
    assert np.array_equal(bits(got.reshape(-1)), bits(lb))


# --------------------------------------------------------------------------- 6
def _crafted(n):
    d, s, w, mu = skit.crafted_rows()
    rep = -(-n // len(d))
    return np.tile(d, (rep, 1))[:n], np.tile(s, (rep, 1))[:n], w, mu


def _apply_rows(ctx, d, s, w, mu, shape=None):
    """apply_spectrum over rows (n, M) laid out plane-major, masks from the sign sums."""
    M = d.shape[1]
    planes = np.ascontiguousarray(d.T)
    mask = ((s != 0).astype(np.uint32) << np.arange(M, dtype=np.uint32)).sum(1).astype(np.uint16)
    if shape is not None:
        planes, mask = planes.reshape((M,) + shape), mask.reshape(shape)
    return ctx.apply_spectrum(planes, mask, w, mu).reshape(-1)


@pytest.mark.parametrize("n,shape", [(1, None), (63, None), (64, None), (65, None), (257, None), (91, (7, 13))])
def test_apply_crafted_planes(pctx, n, shape):
    """The model's edge cases (infinities, NaN, flags by every mesh) at the tails of a wave and of a block."""
    d, s, w, mu = _crafted(n)
    got = _apply_rows(pctx, d, s, w, mu, shape)
    assert np.array_equal(bits(got), bits(spectrum_ref.integrate(d, s, w, mu))), got
    assert np.array_equal(bits(got), bits(pctx.probe_spectrum(d, s, w, mu)))


def test_apply_skips_on_bits_not_on_value(pctx):
    """A mesh whose plane holds -0.0 on every lane of a wave is no mesh of zeros; a wave of zeros
    but for one lane integrates that lane and gives the others the miss value."""
    rng = np.random.default_rng(11)
    w, mu = skit.table(3, 4)
    n = 192
    d = rng.uniform(-20, 60, (n, 3)).astype(F)
    d[:64, 1] = F(-0.0)                                 # wave 0: mesh 1 is -0.0 on every lane
    d[:64, 0] = F(0.0)                                  # ... and mesh 0 +0.0: left out
    d[64:128] = F(0.0)                                  # wave 1: zeros ...
    d[64 + 17] = [3.5, 0.0, -1.25]                      # ... but for one lane
    d[128:, 2] = F(-0.0)
    s = np.zeros(d.shape, np.int32)
    got = _apply_rows(pctx, d, s, w, mu)
    want = spectrum_ref.integrate(d, s, w, mu)
    assert np.array_equal(bits(got), bits(want))
    miss = bits(np.array([spectrum_ref.miss_value(w)], F))[0]
    assert np.all(bits(got[64:128][np.arange(64) != 17]) == miss) and bits(got)[64 + 17] != miss
    # a flagged lane in a wave of zeros: -1 there, the miss value beside it
    d[:] = F(0.0)
    s[70, 2] = 1
    got = _apply_rows(pctx, d, s, w, mu)
    assert got[70] == F(-1.0) and np.all(bits(np.delete(got, 70)) == miss)
    # no mask at all: nothing is flagged
    assert np.all(bits(pctx.apply_spectrum(np.ascontiguousarray(d.T), None, w, mu)) == miss)


# --------------------------------------------------------------------------- 7
def test_one_trace_many_tables(pth):
    """One device render, three applications back to back on one stream without a host wait
    between them: each launch carries its own table."""
    import torch
    W, H = 96, 80
    n = W * H
    meshes = kit.phantom()
    su = skit.phantom_sums(W, H)
    tables = [skit.phantom_table(4), skit.table(5, 7, seed=3), skit.phantom_table(32)]
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.set_kernel(xrt.XRT_KERNEL_BINNED)
    pth.upload_scene(meshes)
    pth.set_paths()
    d_paths = torch.full((5 * n,), 7.0, dtype=torch.float32, device="cuda")
    d_open = torch.full((n,), 3, dtype=torch.int16, device="cuda")
    outs = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in tables]
    pth.render_paths_device(cam, 0, H, 5, d_paths.data_ptr(), d_open.data_ptr())
    for (w, mu), out in zip(tables, outs):
        pth.apply_spectrum_device(n, d_paths.data_ptr(), d_open.data_ptr(), w, mu, out.data_ptr())
    torch.cuda.synchronize()
    pth.read_stats()
    want, mask = planes_of(su, W, H)
    assert same_planes(d_paths.cpu().numpy().reshape(5, H, W), want)
    assert np.array_equal(d_open.cpu().numpy().view(np.uint16).reshape(H, W), mask)
    refs = [spectrum_ref.from_sums(su, w, mu).lbuffer for w, mu in tables]
    assert not np.array_equal(bits(refs[0]), bits(refs[1])) and not np.array_equal(bits(refs[0]), bits(refs[2]))
    for k, out in enumerate(outs):
        assert np.array_equal(bits(out.cpu().numpy()), bits(refs[k])), k


# --------------------------------------------------------------------------- 8
@functools.lru_cache(maxsize=None)
def _two_cameras(W, H):
    meshes = kit.phantom()
    wider = meshes + [kit.box((30, -40, -30), (95, 40, 30))]          # another bounding box: another camera
    cams = [xrt.camera_for_scene(meshes, W, H), xrt.camera_for_scene(wider, W, H)]
    return cams, [spectrum_ref.sums(meshes, cam13(c), W, H) for c in cams]


@pytest.mark.parametrize("order", [(0, 1, 0, 1, 0, 1), (0, 0, 0, 0, 1, 0)], ids=["alternating", "repeating"])
def test_prepared_ahead_frames(pth, order):
    """Six device-entry frames over two cameras, one of them repeated so that its next frames
    are prepared ahead: each frame's planes are its camera's."""
    import torch
    W, H = 67, 45
    n = W * H
    cams, sums = _two_cameras(W, H)
    want = [planes_of(su, W, H) for su in sums]
    assert not np.array_equal(bits(want[0][0]), bits(want[1][0]))
    pth.set_kernel(xrt.XRT_KERNEL_BINNED)
    pth.upload_scene(kit.phantom())
    pth.set_paths()
    planes = [torch.full((5 * n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(6)]
    masks = [torch.full((n,), 3, dtype=torch.int16, device="cuda") for _ in range(6)]
    for k in range(6):
        pth.render_paths_device(cams[order[k]], 0, H, 5, planes[k].data_ptr(), masks[k].data_ptr())
    torch.cuda.synchronize()
    pth.read_stats()
    for k in range(6):
        assert same_planes(planes[k].cpu().numpy().reshape(5, H, W), want[order[k]][0]), k
        assert np.array_equal(masks[k].cpu().numpy().view(np.uint16).reshape(H, W), want[order[k]][1]), k


# --------------------------------------------------------------------------- 9
@pytest.mark.parametrize("kernel", KERNELS)
def test_switching_models(pth, kernel):
    """paths -> spectrum -> paths -> signed on one context: each model's own frame."""
    W, H = 67, 45
    meshes = kit.phantom()
    su = skit.phantom_sums(W, H)
    cam = xrt.camera_for_scene(meshes, W, H)
    w, mu = skit.phantom_table(4)
    pth.set_kernel(kernel)
    pth.upload_scene(meshes)
    pth.set_paths()
    check_paths(pth.render_paths(cam), su, W, H)
    pth.set_spectrum(w, mu)
    with pytest.raises(xrt.XrtError):                  # render_paths needs set_paths
        pth.render_paths(cam)
    _, lb, _, _ = pth.render_spectrum(cam)
    assert np.array_equal(bits(lb), bits(skit.phantom_ref(W, H, 4).lbuffer))
    pth.set_paths()
    check_paths(pth.render_paths(cam), su, W, H)
    pth.set_model(xrt.XRT_MODEL_SIGNED, 0.1037)
    _, slb, _, sst = pth.render_signed(cam)
    rs, rsn, flagged = oracle.render_signed_rows(meshes, cam13(cam), W, H)
    assert np.array_equal(bits(slb), bits(rs)) and sst.odd_rays == flagged and sst.hits == int(rsn.sum())


def test_errors(pth):
    meshes = kit.phantom()
    W, H = 24, 24
    cam = xrt.camera_for_scene(meshes, W, H)
    pth.upload_scene(meshes)
    pth.set_paths()

    def refused(call):
        with pytest.raises(xrt.XrtError) as e:
            call()
        assert e.value.code == _abi.XRT_ERR_ARGUMENT

    def renders(scene):
        su = spectrum_ref.sums(scene, cam13(cam), W, H)
        check_paths(pth.render_paths(cam), su, W, H)

    # the other entries' planes mean something else under this model
    refused(lambda: pth.render_rows(cam, 0, H, image=False, u8=False))
    refused(lambda: pth.render_rows(cam, 0, H))
    refused(lambda: pth.render_spectrum(cam))
    refused(lambda: pth.render_materials(cam))
    refused(lambda: pth.render_signed(cam))
    refused(lambda: pth.render_frames(cam, 2))
    renders(meshes)
    refused(lambda: pth.render_paths(cam, num_meshes=4))            # the caller's buffers are of another size
    refused(lambda: pth.render_paths(cam, num_meshes=6))
    renders(meshes)
    pth.set_kernel(xrt.XRT_KERNEL_TILED)
    refused(lambda: pth.render_paths(cam))                          # BRUTE or BINNED
    pth.set_kernel(xrt.XRT_KERNEL_AUTO)
    renders(meshes)
    for other in (lambda: pth.set_model(xrt.XRT_MODEL_SIGNED, 0.1037), lambda: pth.set_materials(kit.PHANTOM_MU),
                  lambda: pth.set_spectrum(*skit.phantom_table(4)),
                  lambda: pth.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)):
        other()                                                     # each leaves the model
        refused(lambda: pth.render_paths(cam))
        pth.set_paths()
    renders(meshes)
    # a scene of another mesh count, no new set_paths: the id ranges follow the upload
    three = [meshes[0], meshes[1], meshes[4]]
    pth.upload_scene(three)
    refused(lambda: pth.render_paths(cam, num_meshes=5))
    renders(three)
    paths, opn, _ = pth.render_paths(cam)
    refused(lambda: pth.apply_spectrum(paths, opn, [1.0, 0.0], np.full((3, 2), 0.1, F)))
    with pytest.raises(ValueError):                                 # five meshes' table, three planes
        pth.apply_spectrum(paths, opn, *skit.phantom_table(4))
    renders(three)


# --------------------------------------------------------------------------- 10
def test_cli_paths(tmp_path):
    meshes = kit.phantom()
    _write_obj(tmp_path / "a.obj", meshes[0])
    _write_obj(tmp_path / "b.obj", meshes[4])
    (tmp_path / "out").mkdir()
    (tmp_path / "beam.txt").write_text("40 25.5 14.5\n0.2059 0.1037 0.08\n0.05 0 0.025\n")
    common = ["--spectrum", str(tmp_path / "beam.txt"), "-i", str(tmp_path / "a.obj"), "-i", str(tmp_path / "b.obj"),
              "-s", "24", "24"]

    def run(*args):
        r = subprocess.run([EXE, *args], capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert r.returncode == 0, r.stderr

    run(*common, "-f", "plain.txt")
    run("--paths", *common, "-f", "o.txt")
    assert (tmp_path / "out" / "o.txt").read_bytes() == (tmp_path / "out" / "plain.txt").read_bytes()
    scene = [xrt.load_meshes(str(tmp_path / "a.obj"))[0], xrt.load_meshes(str(tmp_path / "b.obj"))[0]]
    su = spectrum_ref.sums(scene, oracle.camera_for_scene(scene, 24, 24), 24, 24)
    want, mask = planes_of(su, 24, 24)
    assert np.count_nonzero(mask) > 0 and np.count_nonzero(want[1]) > 0
    for m in range(2):                                  # the text writer's six significant digits
        assert (tmp_path / "out" / f"o.m{m}.txt").read_bytes() == oracle.text_bytes(want[m].reshape(-1), 24, 24)
    assert (tmp_path / "out" / "o.open.txt").read_bytes() == oracle.text_bytes(mask.astype(F).reshape(-1), 24, 24)
    # without a table the planes are the output
    run("--paths", "-i", str(tmp_path / "a.obj"), "-i", str(tmp_path / "b.obj"), "-s", "24", "24", "-f", "p.txt")
    assert (tmp_path / "out" / "p.m1.txt").read_bytes() == (tmp_path / "out" / "o.m1.txt").read_bytes()
    assert not (tmp_path / "out" / "p.txt").exists()
