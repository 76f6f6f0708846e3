"""The voxeliser on the GPU: k_voxel_scatter, k_voxel_tiles and k_voxel_scan bit for bit against
tests/voxel_ref.py through both entry forms over the kit's small grids, the dragon at 48^3, both scatter
schedules at once and each alone, repeated runs, poses, voxelise -> upload_volume -> volume_paths, the
refusals that need a context, and xrt_main --voxelize."""
import os
import subprocess

import numpy as np
import pytest

import simpleraytracing_amd as xrt
import voxel_kit as vk
import voxel_ref
from simpleraytracing_amd import _abi
from conftest import ROOT, bits
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
NEVER = 0xFFFFFFFF
THRESHOLD = 16                                    # kVoxelQueueColumns: footprint columns from which a triangle is queued


@pytest.fixture(scope="module")
def vctx():
    """A context of this module's own: the scenes, poses and volumes set here never reach other tests."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def sync(ctx, c, **kw):
    return ctx.voxelize(c["dims"], c["spacing"], c["origin"], value=c["value"], **kw)


def device(ctx, c, stream=0):
    """Context.voxelize_device into torch buffers preset to other values, read back as voxelize returns them."""
    import torch
    nx, ny, nz = c["dims"]
    n = nx * ny * nz
    mask = torch.full((n,), -1, dtype=torch.int16, device="cuda")
    labels = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    volume = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    odd = torch.full((_abi.XRT_MAX_MESHES,), -1, dtype=torch.int64, device="cuda")
    ctx.voxelize_device(c["dims"], c["spacing"], c["origin"], c["value"], mask.data_ptr(), labels.data_ptr(),
                        volume.data_ptr(), odd.data_ptr(), stream)
    torch.cuda.synchronize()
    odd = odd.cpu().numpy().view(np.uint64)
    assert not odd[len(c["meshes"]):].any()
    return dict(mask=mask.cpu().numpy().view(np.uint16).reshape(nz, ny, nx), labels=labels.cpu().numpy().reshape(nz, ny, nx),
                volume=volume.cpu().numpy().reshape(nz, ny, nx), odd_columns=odd[:len(c["meshes"])].copy())


@pytest.mark.parametrize("name", vk.SMALL + vk.FAST)
def test_both_forms_equal_the_reference(vctx, name):
    """Every output and odd_columns, bit for bit, through host buffers and through device buffers."""
    c = vk.case(name)
    vctx.upload_scene(c["meshes"])
    vk.assert_equal(sync(vctx, c), vk.reference(name), (name, "host buffers"))
    vk.assert_equal(device(vctx, c), vk.reference(name), (name, "device buffers"))


def _schedule(c, threshold):
    """The counters the scatter must report: triangles by path and the queue entries (four rows each)."""
    columns, rows = voxel_ref.footprints(c["meshes"], c["dims"], c["origin"], c["spacing"])
    queued = (columns >= threshold) & (columns > 0)
    return {"direct": int(np.count_nonzero((columns > 0) & ~queued)), "queued": int(np.count_nonzero(queued)),
            "entries": int(((rows[queued] + 3) // 4).sum()), "overflowed": 0}


def test_both_schedules_run_on_a_dragon_in_a_box(vctx):
    """At 14^3 the dragon's triangles cover fewer columns than the threshold and stay with their lanes; the box's
    two faces across the columns, four triangles of 84 columns, are queued for the tile waves, four
    rows of their boxes an entry (its eight side triangles are edge-on and cover nothing).  The counters say that
    both paths ran, and either schedule alone gives the same volume: the lanes alone, and every triangle queued."""
    c, ref = vk.case("dragon_in_box"), vk.reference("dragon_in_box")
    columns, _ = voxel_ref.footprints(c["meshes"], c["dims"], c["origin"], c["spacing"])
    assert columns[12:].max() < THRESHOLD <= columns[:4].min() and not columns[4:12].any()
    vctx.upload_scene(c["meshes"])
    try:
        vk.assert_equal(sync(vctx, c), ref, "default")
        n = vctx.voxelize_counters()
        print("default:", n)
        assert n == _schedule(c, THRESHOLD) and n["queued"] == 4 and n["direct"] > 500 and n["entries"] >= 4 * 3
        vctx.voxelize_threshold(NEVER)
        vk.assert_equal(sync(vctx, c), ref, "lanes alone")
        assert vctx.voxelize_counters() == _schedule(c, NEVER)
        vctx.voxelize_threshold(1)
        vk.assert_equal(sync(vctx, c), ref, "every triangle queued")
        m = vctx.voxelize_counters()
        print("all queued:", m)
        assert m == _schedule(c, 1) and m["direct"] == 0 and m["queued"] == n["queued"] + n["direct"]
    finally:
        vctx.voxelize_threshold(0)


def test_a_full_queue_leaves_the_triangles_to_their_lanes(vctx):
    """More entries than the queue's 65536: 70000 copies of one triangle, each queued at threshold 1, flip every
    crossing 70000 times -- an even number, so the volume is empty and no column is odd -- whether a copy was
    queued or not."""
    tri = np.repeat(vk.single_triangle(), 70000, axis=0)
    vctx.upload_scene([tri])
    try:
        vctx.voxelize_threshold(1)
        got = vctx.voxelize((16, 16, 8), (0.2, 0.2, 0.3), (0.0, 0.0, 0.0))
        n = vctx.voxelize_counters()
        print(n)
        assert n["overflowed"] > 0 and n["queued"] > 0 and n["queued"] + n["direct"] == 70000
        assert not got["mask"].any() and not got["odd_columns"].any()
        vctx.upload_scene([tri[:69999]])                  # an odd number of copies: the one triangle's volume
        got = vctx.voxelize((16, 16, 8), (0.2, 0.2, 0.3), (0.0, 0.0, 0.0))
        ref = vk.reference("triangle")
        assert np.array_equal(got["mask"], ref["mask"]) and np.array_equal(got["odd_columns"], ref["odd_columns"])
    finally:
        vctx.voxelize_threshold(0)


def test_two_runs_are_bitwise_equal(vctx):
    c = vk.case("dragon_in_box")
    vctx.upload_scene(c["meshes"])
    a, b = device(vctx, c), device(vctx, c)
    vk.assert_equal(a, b, "second run")


def test_outputs_are_optional_one_by_one(vctx):
    c, ref = vk.case("sixteen"), vk.reference("sixteen")
    vctx.upload_scene(c["meshes"])
    for keep in ("mask", "labels", "volume", "odd_columns"):
        got = sync(vctx, c, **{k: k == keep for k in ("mask", "labels", "volume", "odd_columns")})
        assert list(got) == [keep] and np.array_equal(got[keep], ref[keep]), keep


def test_a_pose_change_between_two_calls_is_honoured(vctx):
    """The scene of `posed` with its second mesh at rest, then under the pose on the device, then at rest again:
    each call voxelises the soup the next render would read."""
    import torch
    c, ref = vk.case("posed"), vk.reference("posed")
    box, pose = vk.turned_box()
    rest = voxel_ref.voxelize([c["meshes"][0], box], c["dims"], c["origin"], c["spacing"], c["value"])
    assert not np.array_equal(rest["mask"], ref["mask"])
    vctx.upload_scene([c["meshes"][0], box])
    try:
        vk.assert_equal(sync(vctx, c), rest, "at rest")
        launches = vctx.pose_counters()["launches"]
        vctx.set_pose(1, pose)                            # k_pose is due: the call itself enqueues it ...
        side = torch.cuda.Stream()
        vk.assert_equal(device(vctx, c, side.cuda_stream), ref, "posed, on a stream of the caller's")
        assert vctx.pose_counters()["launches"] > launches        # ... on the preparation stream
        assert np.array_equal(vctx.posed_triangles()[12:], c["meshes"][1])
        vk.assert_equal(sync(vctx, c), ref, "posed")
        assert vctx.pose_counters()["launches"] == launches + 1   # (written once)
        vctx.reset_poses()
        vk.assert_equal(device(vctx, c), rest, "at rest again")
    finally:
        vctx.reset_poses()


def test_voxelised_labels_trace_like_the_reference_labels(vctx):
    """voxelize_device's labels, uploaded as they are, trace into the planes of the reference's labels; and
    upload=True does the upload itself.  The model, the scene and a render around the calls are untouched."""
    import torch
    name = "posed"
    c, ref = vk.case(name), vk.reference(name)
    M = len(c["meshes"])
    vctx.upload_scene(c["meshes"])
    lo, hi = xrt.volume_bbox(c["dims"], c["spacing"], c["origin"])
    cam = xrt.camera_from_bbox(lo, hi, 45, 37)
    before = vctx.render_rows(cam)[0]
    nx, ny, nz = c["dims"]
    labels = torch.full((nx * ny * nz,), 255, dtype=torch.uint8, device="cuda")
    vctx.voxelize_device(c["dims"], c["spacing"], c["origin"], d_labels=labels.data_ptr())
    torch.cuda.synchronize()
    got = labels.cpu().numpy().reshape(nz, ny, nx)
    assert np.array_equal(got, ref["labels"])
    vctx.upload_volume(ref["labels"], c["spacing"], c["origin"], num_labels=M)
    want = vctx.volume_paths(cam)
    assert np.count_nonzero(want[0]) and np.count_nonzero(want[1])
    vctx.upload_volume(got, c["spacing"], c["origin"], num_labels=M)
    assert np.array_equal(bits(vctx.volume_paths(cam)), bits(want))
    vctx.upload_volume(None, 1.0)
    out = sync(vctx, c, upload=True)
    assert np.array_equal(out["labels"], ref["labels"])
    assert np.array_equal(bits(vctx.volume_paths(cam)), bits(want))
    assert np.array_equal(bits(vctx.render_rows(cam)[0]), bits(before))
    vctx.upload_volume(None, 1.0)


def test_refusals_that_need_a_context():
    """No scene: XRT_ERR_NO_MESH, after the arguments' own faults; an empty scene voxelises to nothing."""
    with xrt.Context(int(os.environ.get("XRT_DEVICE", "0"))) as ctx:
        with pytest.raises(xrt.XrtError) as e:
            ctx.voxelize((4, 4, 4), 1.0)
        assert e.value.code == _abi.XRT_ERR_NO_MESH and "no scene" in str(e.value)
        with pytest.raises(xrt.XrtError) as e:
            ctx.voxelize((4, 0, 4), 1.0)
        assert e.value.code == _abi.XRT_ERR_ARGUMENT and "dims[y]" in str(e.value)
        with pytest.raises(xrt.XrtError) as e:
            ctx.voxelize_counters()
        assert e.value.code == _abi.XRT_ERR_ARGUMENT
        ctx.upload_scene([np.zeros((0, 9), F), np.zeros((0, 9), F)])
        got = ctx.voxelize((5, 4, 3), 0.5, value=[1.0, 2.0])
        assert not got["mask"].any() and not got["labels"].any() and not bits(got["volume"]).any()
        assert got["odd_columns"].tolist() == [0, 0]
        with pytest.raises(xrt.XrtError) as e:
            ctx.voxelize((4, 4, 4), 1.0, mask=False, labels=False, odd_columns=False)
        assert e.value.code == _abi.XRT_ERR_ARGUMENT and "no output" in str(e.value)


# ------------------------------------------------------------------------------- the CLI
def test_cli_voxelizes_on_the_grid_of_reconstruct(tmp_path):
    """xrt_main --voxelize FILE.mhd:N: the header and raw file load back to the reference's labels of the loaded
    meshes on the cube about the scene's centre; FILE.mu.mhd holds --materials' coefficients summed; the grid is
    bit for bit the one --reconstruct FILE.mhd:N writes in the same run; and the option stands alone."""
    lo, hi = np.array([-5.3, -6.1, -9.2]), np.array([5.0, 4.4, 10.7])
    from scene_kit import box
    _write_obj(tmp_path / "body.obj", box(lo, hi))
    _write_obj(tmp_path / "insert.obj", box(lo + 2.5, hi - np.array([3.0, 4.0, 9.0])))
    meshes = [xrt.load_meshes(str(tmp_path / n))[0] for n in ("body.obj", "insert.obj")]
    (tmp_path / "out").mkdir()
    N = 24
    r = subprocess.run([EXE, "-s", "24", "24", "-i", str(tmp_path / "body.obj"), "-i", str(tmp_path / "insert.obj"), "-f",
                        "p.txt", "--materials", "0.25,1.5", "--voxelize", f"{tmp_path / 'truth.mhd'}:{N}"],
                       capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    labels, spacing, origin = xrt.load_volume(str(tmp_path / "truth.mhd"))
    assert labels.dtype == np.uint8 and labels.shape == (N, N, N)
    centre = 0.5 * (lo + hi)
    diagonal = np.linalg.norm(hi - lo)
    assert np.allclose(spacing, diagonal / N, rtol=1e-6) and np.allclose(origin, centre - diagonal / 2, rtol=1e-5)
    ref = voxel_ref.voxelize(meshes, (N, N, N), origin, spacing, value=[0.25, 1.5])
    assert np.array_equal(labels, ref["labels"]) and set(np.unique(labels)) == {0, 1, 2}
    mu, mu_spacing, mu_origin = xrt.load_volume(str(tmp_path / "truth.mu.mhd"))
    assert mu.dtype == F and np.array_equal(bits(mu), bits(ref["volume"]))
    assert np.array_equal(bits(mu_spacing), bits(spacing)) and np.array_equal(bits(mu_origin), bits(origin))
    # beside --reconstruct: one grid
    r = subprocess.run([EXE, "-s", "16", "16", "-i", str(tmp_path / "body.obj"), "-i", str(tmp_path / "insert.obj"), "-f",
                        "q.txt", "--turntable", "4:z", "--log-projection", "80", "--reconstruct", "recon.mhd:" + str(N),
                        "--voxelize", "truth2.mhd:" + str(N)], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    recon, r_spacing, r_origin = xrt.load_volume(str(tmp_path / "recon.mhd"))
    labels2, t_spacing, t_origin = xrt.load_volume(str(tmp_path / "truth2.mhd"))
    assert recon.shape == labels2.shape == (N, N, N)
    assert np.array_equal(bits(r_spacing), bits(t_spacing)) and np.array_equal(bits(r_origin), bits(t_origin))
    assert np.array_equal(bits(t_spacing), bits(spacing)) and np.array_equal(bits(t_origin), bits(origin))
    assert np.array_equal(labels2, labels)
    assert not os.path.exists(tmp_path / "truth2.mu.mhd")
