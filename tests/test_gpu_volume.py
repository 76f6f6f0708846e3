"""The voxel trace on the GPU: k_volume_paths' planes bit for bit against tests/volume_ref.py
over the kit's volumes, cameras and detector sizes; strips, both entry forms, volumes uploaded in turn, a
trace between mesh renders, mesh and volume planes stacked under one spectrum table, a box mesh against the
same box in voxels, the refusals and the CLI."""
import os
import subprocess

import numpy as np
import pytest

import camera_kit
import detector_ref
import simpleraytracing_amd as xrt
import spectrum_ref
import volume_kit as vk
import volume_ref
from scene_kit import box
from simpleraytracing_amd import _abi
from oracle import oracle
from conftest import ROOT, bits

pytestmark = pytest.mark.gpu
F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


@pytest.fixture(scope="module")
def vctx():
    """A context of this module's own: the volumes and scenes set here never reach other tests."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def upload(ctx, vol):
    ctx.upload_volume(vol["labels"], vol["spacing"], vol["origin"], vol["density"], vol["num_labels"])


def check(got, want, what):
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (what, len(bad), bad[:8])


# Every volume under the base camera at a size with a ragged tile; then the cases that differ in kind: every
# camera over the sixteen-label volume with densities at a size that crosses tile edges both ways, the random
# volumes at the largest size, the frames of one pixel and of less than a tile, the rays in voxel faces and with
# zero direction components (odd sizes over "faces"), the source inside, and the frame that misses.
CASES = [(v, "base", 15, 11) for v in vk.VOLUMES] + [("shells16d", c, 67, 45) for c in vk.CAMERAS] + [
    ("randomd", "yaw33_pitch20_roll17", 96, 80), ("random", "mirror", 96, 80), ("shells3", "base", 96, 80),
    ("shells1d", "inside", 96, 80), ("shells1", "roll30", 67, 45), ("aniso", "mirror", 67, 45),
    ("faces", "base", 67, 45), ("faces", "pitch90", 7, 13), ("faces", "roll30", 1, 1), ("one", "inside", 1, 1),
    ("one", "pitch90", 7, 13), ("aniso", "inside", 7, 13), ("shells3d", "miss", 67, 45), ("shells16", "miss", 15, 11)]


def test_the_cases_cover_the_kit():
    assert {c[0] for c in CASES} == set(vk.VOLUMES)
    assert {c[1] for c in CASES} == set(vk.CAMERAS) | {"miss"}
    assert {c[2:] for c in CASES} == set(vk.SIZES) | {(96, 80)}
    assert {vk.volume(c[0])["num_labels"] for c in CASES} >= {1, 3, 16}


@pytest.mark.parametrize("vname,cname,W,H", CASES)
def test_kit_volumes(vctx, vname, cname, W, H):
    vol = vk.volume(vname)
    want = vk.reference(vname, cname, W, H)
    if cname == "miss":
        assert not bits(want).any()                       # +0.0f everywhere
    else:
        assert np.count_nonzero(want) > 0
    upload(vctx, vol)
    check(vctx.volume_paths(vk.camera(vol, cname, W, H)), want, (vname, cname, W, H))


@pytest.mark.parametrize("vname", ["shells3d", "shells16", "shells1"])
def test_strips_in_both_forms(vctx, vname):
    """The strips (0, 5), (5, 6) and (6, H) of a frame, through the host-buffer entry and through the device
    entry into one buffer, are the frame's rows."""
    import torch
    W, H = 15, 11
    vol = vk.volume(vname)
    M = vol["num_labels"]
    want = vk.reference(vname, "yaw33_pitch20_roll17", W, H)
    cam = vk.camera(vol, "yaw33_pitch20_roll17", W, H)
    upload(vctx, vol)
    for r0, r1 in vk.STRIPS:
        r1 = H if r1 is None else r1
        check(vctx.volume_paths(cam, r0, r1), want[:, r0:r1], (vname, r0, r1))
        d = torch.full((M * (r1 - r0) * W,), 7.0, dtype=torch.float32, device="cuda")
        vctx.volume_paths_device(cam, r0, r1, M, d.data_ptr())
        torch.cuda.synchronize()
        check(d.cpu().numpy().reshape(M, r1 - r0, W), want[:, r0:r1], (vname, "device", r0, r1))
    assert vctx.volume_paths(cam, 4, 4).shape == (M, 0, W)          # an empty strip: nothing to do


def test_volumes_in_turn(vctx):
    """The second upload replaces the first: other dims, labels, densities and label count."""
    W, H = 67, 45
    for vname in ("shells16d", "aniso", "shells16d", "shells1"):
        vol = vk.volume(vname)
        upload(vctx, vol)
        check(vctx.volume_paths(vk.camera(vol, "roll30", W, H)), vk.reference(vname, "roll30", W, H), vname)


BOX = ((40, -30, -25), (90, 30, 25))


def _box_scene(W, H):
    mesh = box(*BOX)
    c13 = oracle.camera_for_scene([mesh], W, H)
    su = spectrum_ref.sums([mesh], c13, W, H)
    return mesh, c13, su


def _inner_volume():
    """Three shells of 16^3 voxels inside BOX."""
    return dict(labels=vk.volume("shells3")["labels"], spacing=np.full(3, 3.0, F), origin=np.array([41, -24, -24], F),
                density=vk.volume("shells3d")["density"], num_labels=3)


def test_stacked_planes(vctx):
    """A box mesh's plane and a three-label volume's planes in one four-plane buffer, enqueued back to back on
    one stream and integrated under one table: spectrum_ref.integrate over the concatenated reference planes,
    bit for bit; the expected spectral detector over the same buffer."""
    import torch
    W, H = 67, 45
    n = W * H
    mesh, c13, su = _box_scene(W, H)
    vol = _inner_volume()
    cam = camera_kit.as_camera(c13, W, H)
    vplanes = volume_ref.volume_paths(c13, W, H, vol["labels"], vol["spacing"], vol["origin"], vol["density"], 3)
    assert all(np.count_nonzero(p) > 50 for p in vplanes)  # (every label is seen: 73, 313 and 763 pixels)
    dist = np.concatenate([su.distance, vplanes.reshape(3, n).T], axis=1)
    sign = np.concatenate([su.sign_sum, np.zeros((n, 3), np.int64)], axis=1)
    w = np.array([40.0, 25.5, 14.5], F)
    mu = np.array([[0.2059, 0.1037, 0.08], [0.5, 0.3, 0.2], [0.05, 0.0, 0.025], [1.5, 0.9, 0.4]], F)
    resp = np.array([[1, 1, 0], [0, 0, 1]], F)
    vctx.upload_scene([mesh])
    vctx.set_paths()
    upload(vctx, vol)
    d_paths = torch.full((4 * n,), 7.0, dtype=torch.float32, device="cuda")
    d_open = torch.full((n,), 3, dtype=torch.int16, device="cuda")
    d_l = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_c = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    vctx.render_paths_device(cam, 0, H, 1, d_paths.data_ptr(), d_open.data_ptr())
    vctx.volume_paths_device(cam, 0, H, 3, d_paths.data_ptr() + 4 * n)
    vctx.apply_spectrum_device(n, d_paths.data_ptr(), d_open.data_ptr(), w, mu, d_l.data_ptr())
    vctx.spectral_detector_device(n, d_paths.data_ptr(), d_open.data_ptr(), w, mu, resp, d_c.data_ptr(), gain=2.0,
                                  noisy=False)
    torch.cuda.synchronize()
    vctx.read_stats()
    planes = d_paths.cpu().numpy().reshape(4, H, W)
    opn = d_open.cpu().numpy().view(np.uint16).reshape(H, W)
    check(planes[0], su.distance.reshape(H, W), "mesh plane")
    check(planes[1:], vplanes, "volume planes")
    assert np.array_equal(opn != 0, (su.sign_sum != 0).reshape(H, W))
    want = spectrum_ref.integrate(dist, sign, w, mu)
    check(d_l.cpu().numpy(), want, "applied")
    assert np.count_nonzero(want == F(-1.0)) == np.count_nonzero(opn)
    chan = detector_ref.spectral_detector(planes, opn, w, mu, resp, gain=2.0, noisy=False)
    assert detector_ref.same(d_c.cpu().numpy().reshape(2, H, W), chan)
    vctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)


def test_a_trace_between_prepared_frames(vctx):
    """Six paths frames of one camera on the device entry (the later ones prepared ahead), once alone and once
    with volume traces enqueued between them on the same stream: the frames are bit-equal, and so is every
    trace."""
    import torch
    W, H = 67, 45
    n = W * H
    mesh, c13, su = _box_scene(W, H)
    cam = camera_kit.as_camera(c13, W, H)
    vol = vk.volume("shells3d")
    vcam = vk.camera(vol, "roll30", W, H)
    vctx.upload_scene([mesh])
    vctx.set_paths()
    upload(vctx, vol)

    def frames(with_traces):
        planes = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(6)]
        masks = [torch.full((n,), 3, dtype=torch.int16, device="cuda") for _ in range(6)]
        traces = [torch.full((3 * n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(6)]
        for k in range(6):
            vctx.render_paths_device(cam, 0, H, 1, planes[k].data_ptr(), masks[k].data_ptr())
            if with_traces:
                vctx.volume_paths_device(vcam, 0, H, 3, traces[k].data_ptr())
        torch.cuda.synchronize()
        vctx.read_stats()
        return [p.cpu().numpy() for p in planes], [m.cpu().numpy() for m in masks], [t.cpu().numpy() for t in traces]

    alone = frames(False)
    mixed = frames(True)
    want = vk.reference("shells3d", "roll30", W, H)
    for k in range(6):
        check(alone[0][k], su.distance.reshape(-1), ("alone", k))
        check(mixed[0][k], alone[0][k], ("mixed", k))
        assert np.array_equal(mixed[1][k], alone[1][k]), k
        check(mixed[2][k].reshape(3, H, W), want, ("trace", k))
    vctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)


# Measured on the CPU between the two references (spectrum_ref.sums of the box mesh, volume_ref of the same box
# in 10 x 12 x 10 voxels of 5) at 67 x 45 under the box's own camera: the largest deviation over the compared
# pixels is 2.43187e-05 = 3.1875 ulps of f32 at the largest exit distance 123.617 (ulp 2^-17).  The mesh sums
# signed f32 hit distances, the voxels f64 segments narrowed once.  The bound is four times that.
MESH_VOXEL_MEASURED_ULPS = 3.1875
MESH_VOXEL_EXIT = 123.616833667134


def test_mesh_against_voxels(vctx):
    """An axis-aligned box as a mesh (render_paths) and as a uniform one-label volume, 67 x 45: within 4 x
    MESH_VOXEL_MEASURED_ULPS ulps of the largest exit distance at every pixel whose 3 x 3 neighbourhood is
    non-zero in both planes (the silhouette's own pixels hang on f32 edge tests) and whose ray has the box's
    two mesh hits (a ray through an edge shared by two triangles hits both: the mesh model counts that face
    twice, 9 rays of this frame); the compared pixels are at least half of the box's hit pixels."""
    W, H = 67, 45
    mesh, c13, su = _box_scene(W, H)
    cam = camera_kit.as_camera(c13, W, H)
    vctx.upload_scene([mesh])
    vctx.set_paths()
    mplane = vctx.render_paths(cam)[0][0]
    vctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
    lo = np.array(BOX[0], F)
    vctx.upload_volume(np.ones((10, 12, 10), np.uint8), 5.0, lo)
    vplane = vctx.volume_paths(cam)[0]

    def interior(a):
        nz = a != 0
        out = np.zeros_like(nz)
        out[1:-1, 1:-1] = True
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                out[1:-1, 1:-1] &= nz[1 + dy:H - 1 + dy, 1 + dx:W - 1 + dx]
        return out

    sel = interior(mplane) & interior(vplane) & (su.mesh_hits.reshape(H, W) == 2)
    hit = np.count_nonzero(mplane)
    ulp = float(np.spacing(F(MESH_VOXEL_EXIT)))
    dev = np.abs(mplane.astype(np.float64) - vplane.astype(np.float64))[sel].max() / ulp
    print(f"compared {np.count_nonzero(sel)} of {hit} hit pixels, largest deviation {dev} ulps")
    assert hit > 1500 and 2 * np.count_nonzero(sel) >= hit
    assert dev <= 4.0 * MESH_VOXEL_MEASURED_ULPS, dev


def test_refusals(vctx):
    W, H = 15, 11
    vol = vk.volume("shells3")
    cam = vk.camera(vol, "base", W, H)

    def refused(call, code):
        with pytest.raises(xrt.XrtError) as e:
            call()
        assert e.value.code == code, e.value

    vctx.upload_volume(None, 1.0)
    refused(lambda: vctx.volume_paths(cam, num_labels=3), _abi.XRT_ERR_NO_MESH)          # no volume
    upload(vctx, vol)
    refused(lambda: vctx.volume_paths(cam, num_labels=2), _abi.XRT_ERR_ARGUMENT)         # the caller's buffer is of another size
    refused(lambda: vctx.volume_paths(cam, num_labels=4), _abi.XRT_ERR_ARGUMENT)
    refused(lambda: vctx.volume_paths_device(cam, 0, H, 4, 1 << 20), _abi.XRT_ERR_ARGUMENT)
    bad = vol["labels"].copy()
    bad[3, 2, 1] = 4
    refused(lambda: vctx.upload_volume(bad, vol["spacing"], vol["origin"], num_labels=3), _abi.XRT_ERR_ARGUMENT)
    check(vctx.volume_paths(cam), vk.reference("shells3", "base", W, H), "after the refusals")   # the volume stays
    vctx.upload_volume(None, 1.0)
    refused(lambda: vctx.volume_paths(cam, num_labels=3), _abi.XRT_ERR_NO_MESH)          # the freed volume
    refused(lambda: vctx.volume_paths_device(cam, 0, H, 3, 1 << 20), _abi.XRT_ERR_NO_MESH)


def test_cli_volume(tmp_path):
    """xrt_main --paths --volume on a small .mhd written here: beside a mesh (the camera of the union of the two
    boxes; the mesh's plane, then the labels'; one table over both) and alone (no -i)."""
    from test_spectrum_cpu import _write_obj
    from test_volume_cpu import _write_mhd
    W = H = 24
    vol = vk.volume("aniso")
    den = vk._density(vol["labels"].shape, 5)
    mesh = box((-3, -1, -2), (1, 1, 2))
    _write_mhd(tmp_path / "lab.mhd", vol["labels"])
    _write_mhd(tmp_path / "den.mhd", den)
    _write_obj(tmp_path / "box.obj", mesh)
    (tmp_path / "out").mkdir()
    (tmp_path / "beam.txt").write_text("40 25.5 14.5\n0.2059 0.1037 0.08\n0.05 0 0.025\n0.5 0.3 0.2\n1.5 0.9 0.4\n")

    def run(*args):
        r = subprocess.run([EXE, *args], capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert r.returncode == 0, r.stderr

    def text(plane):
        return oracle.text_bytes(np.ascontiguousarray(plane, F).reshape(-1), W, H)

    size = ["-s", str(W), str(H)]
    run("--paths", "--volume", "lab.mhd", "--volume-density", "den.mhd", "-i", "box.obj", "--spectrum", "beam.txt", *size,
        "-f", "o.txt")
    scene = xrt.load_meshes(str(tmp_path / "box.obj"))
    mlo, mhi = oracle.scene_bbox(scene)
    vlo, vhi = vk.box(vol)
    c13 = oracle.camera(np.minimum(mlo, vlo), np.maximum(mhi, vhi), W, H)
    su = spectrum_ref.sums(scene, c13, W, H)
    want = volume_ref.volume_paths(c13, W, H, vol["labels"], vol["spacing"], vol["origin"], den, 3)
    assert np.count_nonzero(su.distance) > 0 and all(np.count_nonzero(p) > 0 for p in want)
    assert (tmp_path / "out" / "o.m0.txt").read_bytes() == text(su.distance)
    for m in range(3):
        assert (tmp_path / "out" / f"o.m{1 + m}.txt").read_bytes() == text(want[m]), m
    assert not (tmp_path / "out" / "o.m4.txt").exists() and (tmp_path / "out" / "o.txt").stat().st_size > 0
    # alone: the camera of the volume's own box, no density
    run("--paths", "--volume", "lab.mhd", *size, "-f", "v.txt")
    alone = volume_ref.volume_paths(oracle.camera(vlo, vhi, W, H), W, H, vol["labels"], vol["spacing"], vol["origin"], None, 3)
    for m in range(3):
        assert (tmp_path / "out" / f"v.m{m}.txt").read_bytes() == text(alone[m]), m
    assert (tmp_path / "out" / "v.open.txt").read_bytes() == text(np.zeros((H, W), F))


def test_wave_shapes_agree(vctx):
    """The 64 x 1 row segments of the layout's timing A/B (xrt_debug_volume_wave_shape) trace the planes of the
    8 x 8 tiles, bit for bit, for every instantiation."""
    W, H = 67, 45
    try:
        for vname in ("shells1d", "shells3", "shells16d"):
            vol = vk.volume(vname)
            upload(vctx, vol)
            vctx.volume_wave_shape(True)
            check(vctx.volume_paths(vk.camera(vol, "roll30", W, H), 3, H - 2), vk.reference(vname, "roll30", W, H)[:, 3:H - 2],
                  vname)
            vctx.volume_wave_shape(False)
    finally:
        vctx.volume_wave_shape(False)
