"""The ray table ("Ray table"): an attenuation BINNED
frame that repeats the previous one's camera, size and strip has the camera's
rays tabulated once (k_ray_table), and the frames after it read them
(k_render_binned_rays) where the others run make_ray_from.  Every frame here is
compared bit for bit -- image, L-buffer, u8, statistics -- with the same frame
computed (the table off, the brute kernel, the committed fixtures).

Further down: the table itself, read back (xrt_debug_ray_table_read) and
compared float by float, padding included, with camera_kit.ray_directions;
frames asserted to be served from the table -- general cameras, a mesh and
poses that change under it, the overflow fix-up, split tiles, the tile plan,
the packed transit layout -- against the CPU oracle; and the table's lifetime:
growth with frames in flight, the budget's boundary."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_kit as ck
import pose_ref
import ray_table_kit as rk
import simpleraytracing_amd as xrt
from camera_refs import SCENES, reference
from conftest import GOLDEN, ROOT, bits
from oracle import oracle
from scene_kit import box, second_mesh_for, synthetic_soup
from test_camera_cpu import host_footprints
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

RAY_STATS = ("rays", "hit_rays", "odd_rays", "overflow_rays", "hits", "max_hits")       # kernel-independent
ALL_STATS = RAY_STATS + ("kernel", "candidates", "tile_tests", "global_triangles")      # all but the time


def stats_of(st, names):
    return {n: getattr(st, n) for n in names}


def same_planes(a, b):
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and
            np.array_equal(a[2], b[2]))


def copy_camera(cam):
    return xrt.Camera.from_buffer_copy(cam)


def one_ulp(cam):
    """`cam` with the first origin float moved by one ulp."""
    b = copy_camera(cam)
    b.origin[0] = float(np.nextafter(np.float32(cam.origin[0]), np.float32(np.inf)))
    assert b.origin[0] != cam.origin[0]
    return b


@pytest.fixture(scope="module")
def brute(dragon):
    """Brute-force renders (no cull, no table), one per (camera, strip), kept for the module."""
    c = xrt.Context(0)
    c.set_kernel(xrt.XRT_KERNEL_BRUTE)
    c.upload_mesh(dragon)
    cache = {}

    def render(cam, r0=0, r1=None):
        r1 = cam.height if r1 is None else r1
        key = (bytes(cam), r0, r1)
        if key not in cache:
            cache[key] = c.render_rows(cam, r0, r1)
        return cache[key]
    yield render
    c.close()


@pytest.fixture()
def binned(dragon):
    c = xrt.Context(0)
    c.set_kernel(xrt.XRT_KERNEL_BINNED)
    c.upload_mesh(dragon)
    yield c
    c.close()


def render_until_cached(c, cam, r0=0, r1=None, limit=6):
    """Host-buffer frames of one key until one is served from the table; returns it."""
    before = c.ray_table_counters()["frames"]
    for _ in range(limit):
        got = c.render_rows(cam, r0, r1)
        if c.ray_table_counters()["frames"] > before:
            return got
    raise AssertionError(f"no frame from the table after {limit}: {c.ray_table_counters()}")


@pytest.mark.parametrize("size", [128, 256])
def test_cached_equals_computed(binned, brute, dragon, size):
    c = binned
    cam = xrt.camera_for_mesh(dragon, size, size)
    on = render_until_cached(c, cam)
    st_on = c.read_stats()
    n = c.ray_table_counters()
    assert n["fills"] == 1 and n["bytes"] == 12 * size * size
    c.set_ray_table(False)
    off = c.render_rows(cam)
    st_off = c.read_stats()
    assert c.ray_table_counters()["frames"] == n["frames"]
    assert same_planes(on, off)
    assert stats_of(st_on, ALL_STATS) == stats_of(st_off, ALL_STATS)
    assert stats_of(on[3], ALL_STATS) == stats_of(off[3], ALL_STATS)
    g = np.load(os.path.join(GOLDEN, f"planes_dragon_{size}.npz"), allow_pickle=False)
    assert np.array_equal(g["rows"], np.arange(size))
    assert np.array_equal(bits(on[0]), bits(g["image"]).reshape(-1))
    assert np.array_equal(bits(on[1]), bits(g["lbuffer"]).reshape(-1))
    assert np.array_equal(on[2], g["u8"].reshape(-1))
    ref = brute(cam)
    assert same_planes(on, ref) and stats_of(st_on, RAY_STATS) == stats_of(ref[3], RAY_STATS)


@pytest.mark.parametrize("W,H,r0,r1", [(100, 77, 0, 77), (33, 65, 0, 65), (96, 128, 13, 61), (96, 128, 40, 41)])
def test_partial_tiles_and_strips(binned, brute, dragon, W, H, r0, r1):
    """Frames off the tile grid and strips off it (row 13; one row): the table's
    partial tiles hold what the computing wave has."""
    cam = xrt.camera_for_mesh(dragon, W, H)
    got = render_until_cached(binned, cam, r0, r1)
    ref = brute(cam, r0, r1)
    assert same_planes(got, ref)
    assert stats_of(got[3], RAY_STATS) == stats_of(ref[3], RAY_STATS)


def test_camera_changes(binned, brute, dragon):
    """A, A, A, B, B, B, A, A, B one ulp from A: a key's first frame computes,
    its second starts the fill and reads the table behind it as the later ones
    do, and each change of key costs one fill and no more."""
    a = xrt.camera_for_mesh(dragon, 128, 128)
    b = one_ulp(a)
    # (fills, frames from the table, frames computed) after each frame
    want = [(0, 0, 1), (1, 1, 1), (1, 2, 1), (1, 2, 2), (2, 3, 2), (2, 4, 2), (2, 4, 3), (3, 5, 3)]
    for k, cam in enumerate([a, a, a, b, b, b, a, a]):
        got = binned.render_rows(cam)                  # (the host waits for every frame: no fill is postponed)
        n = binned.ray_table_counters()
        assert (n["fills"], n["frames"], n["computed"]) == want[k], (k, n)
        ref = brute(cam)
        assert same_planes(got, ref), k
        assert stats_of(got[3], RAY_STATS) == stats_of(ref[3], RAY_STATS), k


def test_size_and_strip_are_in_the_key(binned, brute, dragon):
    """The same camera floats at a second size, then a second strip: a new table each."""
    a = xrt.camera_for_mesh(dragon, 128, 128)
    assert same_planes(render_until_cached(binned, a), brute(a))
    b = copy_camera(a)
    b.width, b.height = 96, 120
    fills = binned.ray_table_counters()["fills"]
    first = binned.render_rows(b)
    assert binned.ray_table_counters()["fills"] == fills       # its first frame computed
    assert same_planes(first, brute(b))
    assert same_planes(render_until_cached(binned, b), brute(b))
    assert binned.ray_table_counters()["fills"] == fills + 1
    first = binned.render_rows(b, 13, 61)
    assert binned.ray_table_counters()["fills"] == fills + 1
    assert same_planes(first, brute(b, 13, 61))
    assert same_planes(render_until_cached(binned, b, 13, 61), brute(b, 13, 61))
    assert binned.ray_table_counters()["fills"] == fills + 2


@pytest.mark.parametrize("streams", [2, 3])
def test_frames_in_flight_across_refills(binned, brute, dragon, streams):
    """12 frames of A, 12 of B, 12 of A over two and three streams, nothing
    waited for in between: a refill never overwrites a table that a launched
    render may still read.  The last frame of each run on each stream is exact."""
    import torch
    dev = torch.device("cuda", 0)
    a = xrt.camera_for_mesh(dragon, 128, 128)
    b = one_ulp(a)
    N = 128 * 128
    runs = []
    qs = [torch.cuda.Stream(dev) for _ in range(streams)]
    for cam in (a, b, a):
        sets = [(torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev))
                for _ in range(streams)]
        binned.render_frames_device(cam, 0, 128, 12, [(i.data_ptr(), l.data_ptr(), u.data_ptr(), q.cuda_stream)
                                                      for (i, l, u), q in zip(sets, qs)])
        runs.append((cam, sets))
    torch.cuda.synchronize(dev)
    n = binned.ray_table_counters()
    assert n["frames"] + n["computed"] == 36 and n["frames"] > 0 and 1 <= n["fills"] <= 3, n
    for cam, sets in runs:
        ref = brute(cam)
        for planes in sets:
            assert same_planes([p.cpu().numpy() for p in planes], ref)


CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
import simpleraytracing_amd as xrt
tris = xrt.load_ply({ply!r})
cam = xrt.camera_for_mesh(tris, 128, 128)
with xrt.Context(0) as c:
    c.set_kernel(xrt.XRT_KERNEL_BINNED)
    c.upload_mesh(tris)
    for _ in range(4):
        img, lb, u8, st = c.render_rows(cam)
    n = c.ray_table_counters()
np.savez({out!r}, image=img, lbuffer=lb, u8=u8)
print(json.dumps(n))
"""


def test_switched_off(binned, brute, dragon, tmp_path):
    """XRT_RAY_CACHE_MB=0 (read at xrt_create: a fresh process) and
    xrt_debug_set_ray_table(0): no fill, no frame from a table, the same planes."""
    cam = xrt.camera_for_mesh(dragon, 128, 128)
    ref = brute(cam)
    out = str(tmp_path / "planes.npz")
    code = CHILD.format(root=ROOT, ply=os.path.join(ROOT, "data", "dragon.ply"), out=out)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, XRT_RAY_CACHE_MB="0"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    n = json.loads(r.stdout.strip().splitlines()[-1])
    assert n == {"fills": 0, "frames": 0, "computed": 4, "bytes": 0}
    g = np.load(out)
    assert same_planes((g["image"], g["lbuffer"], g["u8"]), ref)
    binned.set_ray_table(False)
    for _ in range(4):
        got = binned.render_rows(cam)
    assert binned.ray_table_counters() == {"fills": 0, "frames": 0, "computed": 4, "bytes": 0}
    assert same_planes(got, ref)
    binned.set_ray_table(True)                         # on again: the next repeat fills
    assert same_planes(render_until_cached(binned, cam), ref)


def test_out_of_scope_frames_compute(binned, brute, dragon):
    """With a valid table for the camera, a materials-model frame and a frame in
    the hit layout are not served from it, and are exact."""
    import torch
    from simpleraytracing_amd.strips import hit_descriptors
    W = H = 128
    cam = xrt.camera_for_mesh(dragon, W, H)
    ref = brute(cam)
    assert same_planes(render_until_cached(binned, cam), ref)
    served = binned.ray_table_counters()["frames"]
    # materials (one mesh, the dragon's coefficient): the signed model's planes
    binned.set_materials([0.1037])
    mat = binned.render_materials(cam)
    with xrt.Context(0) as c:
        c.set_kernel(xrt.XRT_KERNEL_BRUTE)
        c.upload_mesh(dragon)
        c.set_materials([0.1037])
        mat_ref = c.render_materials(cam)
    assert np.array_equal(bits(mat[1]), bits(mat_ref[1]))
    assert binned.ray_table_counters()["frames"] == served
    # the hit layout, one strip: the message unpacked equals the frame
    binned.set_model(xrt.XRT_MODEL_ATTENUATION)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lb = torch.zeros(W * H, device=dev)
    binned.render_rows_device(cam, 0, H, 0, lb.data_ptr(), 0, stream.cuda_stream)
    served = binned.ray_table_counters()["frames"]
    rmap, n_packed = binned.plan_region_map(W, H)
    hits, words = binned.plan_hit_layout()
    msg = torch.full((words + 64,), -5.0, device=dev)
    binned.set_transit_hits(msg.numel())
    try:
        for _ in range(2):
            binned.render_rows_device(cam, 0, H, 0, msg.data_ptr(), 0, stream.cuda_stream)
    finally:
        binned.set_transit_hits(0)
    torch.cuda.synchronize(dev)
    assert binned.ray_table_counters()["frames"] == served
    desc, tdesc, bases, wlist, total = hit_descriptors(W, [(0, H)], [rmap], [hits])
    rbuf = torch.zeros(total, dtype=torch.float32, device=dev)
    rbuf[bases[0]:bases[0] + words] = msg[:words]
    d_desc = torch.from_numpy(desc.reshape(-1).view(np.int32)).to(dev)
    d_tdesc = torch.from_numpy(tdesc.reshape(-1).view(np.int32)).to(dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    out = [torch.full((W * H,), -2.0, device=dev), torch.full((W * H,), -2.0, device=dev),
           torch.zeros(W * H, dtype=torch.uint8, device=dev)]
    binned.unpack_hits_device(W, len(desc), d_desc.data_ptr(), d_tdesc.data_ptr(), rbuf.data_ptr(), out[0].data_ptr(),
                              out[1].data_ptr(), out[2].data_ptr(), bad.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize(dev)
    assert int(bad.item()) == 0
    assert same_planes((out[1].cpu().numpy(), out[0].cpu().numpy(), out[2].cpu().numpy()), ref)


# =========================================================================== served frames
BINNED = xrt.XRT_KERNEL_BINNED
MAX_HITS = 12                                       # the register hit list (XRT_MAX_HITS)


def served(c, frame):
    """frame() renders one frame; asserts that it was rendered from the table."""
    before = c.ray_table_counters()
    got = frame()
    after = c.ray_table_counters()
    assert (after["frames"], after["computed"]) == (before["frames"] + 1, before["computed"]), (before, after)
    return got


def render_until_served(c, cam, r0=0, r1=None, limit=4):
    """render_until_cached, counting every frame: host-buffer frames of one key
    until one is rendered from the table (a key's first frame computes, its
    second starts the fill and reads the table behind it).  Returns that frame:
    the table's counter of served frames advanced for it and for no other."""
    for _ in range(limit):
        before = c.ray_table_counters()
        got = c.render_rows(cam, r0, r1)
        after = c.ray_table_counters()
        assert after["frames"] + after["computed"] == before["frames"] + before["computed"] + 1, (before, after)
        if after["frames"] == before["frames"] + 1:
            return got
    raise AssertionError(f"no frame from the table after {limit}: {c.ray_table_counters()}")


def assert_frame(got, ref, W, rows, what=""):
    """assert_same (image, L-buffer, u8, odd, hit rays, hits, deepest ray) and the
    other two kernel-independent statistics against the oracle's hit counts."""
    assert_same(got, ref, what)
    assert got[3].rays == W * rows, what
    assert got[3].overflow_rays == int(np.count_nonzero(ref[3] > MAX_HITS)), what


@pytest.fixture(scope="module")
def small():
    """A BINNED context over a box of 12 triangles: for the tables of cameras
    that no mesh was fitted to (the table does not depend on the mesh)."""
    c = xrt.Context(0)
    c.set_kernel(BINNED)
    c.upload_mesh(box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)))
    yield c
    c.close()


@pytest.fixture(scope="module")
def general(dragon):
    c = xrt.Context(0)
    c.set_kernel(BINNED)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle_frames(dragon):
    """The oracle's frame of the dragon under its own camera, per (W, H, r0, r1): computed once, shared."""
    cache = {}

    def get(W, H, r0=0, r1=None):
        r1 = H if r1 is None else r1
        if (W, H, r0, r1) not in cache:
            c13 = oracle.camera_for_mesh(dragon, W, H)
            ref = oracle.render_rows(dragon, c13, W, H, r0, r1)
            for a in (c13,) + tuple(ref[:4]):
                a.setflags(write=False)
            cache[W, H, r0, r1] = (c13, ref)
        return cache[W, H, r0, r1]
    return get


# --------------------------------------------------------------------------- the table, float by float
def check_table(c, c13, W, H, r0=0, r1=None, what=""):
    """Fills the table of (c13, W, H, strip) on `c`, reads it back and compares
    every float -- the padding to whole 32 x 32 regions included, rows clamped
    to H - 1 and columns to W - 1 -- with camera_kit.ray_directions: by bits,
    NaN for NaN.  Returns (table, expected)."""
    r1 = H if r1 is None else r1
    render_until_served(c, ck.as_camera(c13, W, H), r0, r1)
    table, dims = c.read_ray_table()
    assert dims == (W, H, r0, r1), what
    want = rk.expected_table(c13, W, H, r0, r1)
    assert table.size == want.size == xrt.ray_table_index(W, H, r0, r1, r0, 0)[1], what
    idx = rk.table_indices(W, r0, r1)[0]
    for row in range(r0, r1):                       # the numpy formula is the kernels' at every pixel of the strip
        for col in range(W):
            assert xrt.ray_table_index(W, H, r0, r1, row, col)[0] == idx[row - r0, col], (what, row, col)
    bad = rk.mismatches(table, want)
    assert bad.size == 0, (what, bad.size, bad[:8], table[bad[:8]], want[bad[:8]])
    return table, want


@pytest.mark.parametrize("case", ck.NAMES)
def test_table_contents_general_cameras(binned, dragon, case):
    """67 x 45, off the tile grid both ways: the padded table is 96 x 64."""
    W, H = 67, 45
    check_table(binned, ck.case_camera(case, [dragon], W, H), W, H, what=case)
    n = binned.ray_table_counters()
    assert n["fills"] == 1 and n["bytes"] == 73728 == 4 * xrt.ray_table_index(W, H, 0, H, 0, 0)[1], n


@pytest.mark.parametrize("case,W,H,r0,r1", [("all", 100, 37, 5, 30), ("mirror", 33, 65, 0, 65), ("roll30", 1, 1, 0, 1),
                                            ("roll30", 7, 13, 0, 13), ("offaxis", 96, 128, 13, 61),
                                            ("offaxis", 96, 128, 40, 41)])
def test_table_contents_sizes_and_strips(binned, dragon, case, W, H, r0, r1):
    """Strips off the tile grid (the padding rows below a strip are the image's
    next rows, clamped to H - 1, not to the strip's end), one row, one pixel."""
    check_table(binned, ck.case_camera(case, [dragon], W, H), W, H, r0, r1, what=(case, W, H, r0, r1))


def test_table_contents_random_cameras(small):
    """20 cameras with every component of up and right nonzero, scales 1e-3 to
    100, spacing of either sign, 1 to 40 pixels a side (seeded)."""
    for k, (c13, W, H) in enumerate(rk.random_cameras()):
        check_table(small, c13, W, H, what=(k, W, H, c13.tolist()))


@pytest.mark.parametrize("which", ["source_on_detector", "underflow"])
def test_table_contents_degenerate_cameras(small, which):
    """The source on the detector's centre (odd W and H): the centre pixel's
    direction is 0 / 0, NaN in its three floats and nowhere else.  Direction
    components whose squares underflow: the first length is 0, every float NaN.
    Neither reaches the second normalisation's length == 0 branch: the first
    normalisation leaves NaN or +-inf, never a vector of zero length
    (test_degenerate_cameras_have_the_expected_nan_pattern, on the CPU)."""
    c13, W, H = rk.source_on_detector_camera() if which == "source_on_detector" else rk.underflow_camera()
    table, want = check_table(small, c13, W, H, what=which)
    nan = np.isnan(want)
    assert nan.sum() == 3 if which == "source_on_detector" else nan.all()
    assert np.array_equal(np.isnan(table), nan)


def test_reader_refusals(binned, dragon):
    """No table before a fill and after a frame of another key: XRT_ERR_NO_MESH;
    a NULL or short destination: XRT_ERR_ARGUMENT.  Reading changes nothing
    that decides how the next frame takes its rays."""
    from simpleraytracing_amd import _abi
    c = binned
    cam = xrt.camera_for_mesh(dragon, 67, 45)
    with pytest.raises(xrt.XrtError) as e:
        c.read_ray_table()
    assert e.value.code == _abi.XRT_ERR_NO_MESH
    c.render_rows(cam)                                  # the key's first frame computes: still none
    with pytest.raises(xrt.XrtError) as e:
        c.read_ray_table()
    assert e.value.code == _abi.XRT_ERR_NO_MESH
    render_until_served(c, cam)
    table, dims = c.read_ray_table()
    assert dims == (67, 45, 0, 45) and table.size == 3 * 96 * 64
    buf = np.zeros(table.size, np.float32)
    assert c._lib.xrt_debug_ray_table_read(c._ctx, None, table.size, None) == _abi.XRT_ERR_ARGUMENT
    assert c._lib.xrt_debug_ray_table_read(c._ctx, buf.ctypes.data, table.size - 1, None) == _abi.XRT_ERR_ARGUMENT
    assert not buf.any()
    assert c._lib.xrt_debug_ray_table_read(c._ctx, buf.ctypes.data, table.size, None) == _abi.XRT_OK
    assert np.array_equal(bits(buf), bits(table))
    n = c.ray_table_counters()
    served(c, lambda: c.render_rows(cam))               # the read left the table valid
    assert c.ray_table_counters()["fills"] == n["fills"] == 1
    c.render_rows(one_ulp(cam))                         # another key: the table is dropped
    with pytest.raises(xrt.XrtError) as e:
        c.read_ray_table()
    assert e.value.code == _abi.XRT_ERR_NO_MESH


# --------------------------------------------------------------------------- general cameras through the table
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("case", ck.NAMES)
def test_general_camera_served(general, dragon, case, name):
    """test_general_camera_parity's matrix, each frame rendered from the table:
    equal to the oracle's, bit for bit.  The corner soup's hits at infinity
    (NaN path lengths) come from the table's directions."""
    tris, W, H, c13, ref = reference(name, case, dragon)
    assert np.count_nonzero(ref[3]) > 0
    if name == "corner" and case in ("roll45", "pitch25", "mirror"):
        assert np.isnan(ref[1]).sum() > 10
    general.upload_mesh(tris)
    got = render_until_served(general, ck.as_camera(c13, W, H))
    assert_frame(got, ref, W, H, f"{name} {case}")


def test_general_camera_ragged_strip_served(general, dragon):
    W, H, r0, r1 = 100, 37, 5, 30
    c13 = ck.case_camera("all", [dragon], W, H)
    general.upload_mesh(dragon)
    got = render_until_served(general, ck.as_camera(c13, W, H), r0, r1)
    assert_frame(got, oracle.render_rows(dragon, c13, W, H, r0, r1), W, r1 - r0)


# --------------------------------------------------------------------------- the object moves, the table stays
def test_mesh_changes_under_a_valid_table(dragon):
    """One camera, one table: the soup, the dragon moved by a few units and the
    dragon again, uploaded under it.  No upload costs a fill, every frame after
    the first two is rendered from the table and equals the oracle's frame of
    the mesh it shows."""
    W, H = 67, 45
    c13 = ck.case_camera("yaw33_pitch20_roll17", [dragon], W, H)
    cam = ck.as_camera(c13, W, H)
    centre = ck.scene_centre([dragon])
    soup = synthetic_soup(seed=9, n=2000)
    soup = (soup.reshape(-1, 3) + centre).astype(np.float32).reshape(-1, 9)       # about the dragon: in view
    moved = (dragon.reshape(-1, 3) + np.array([3.0, -2.0, 4.0], np.float32)).astype(np.float32).reshape(-1, 9)
    with xrt.Context(0) as c:
        c.set_kernel(BINNED)
        c.upload_mesh(dragon)
        first = render_until_served(c, cam)
        ref0 = oracle.render_rows(dragon, c13, W, H)
        assert_frame(first, ref0, W, H, "dragon")
        frames = []
        for what, mesh in (("soup", soup), ("moved", moved), ("dragon", dragon)):
            c.upload_mesh(mesh)
            got = served(c, lambda: c.render_rows(cam))
            ref = ref0 if mesh is dragon else oracle.render_rows(mesh, c13, W, H)
            assert np.count_nonzero(ref[3]) > 0, what
            assert_frame(got, ref, W, H, what)
            frames.append(got)
        assert c.ray_table_counters()["fills"] == 1
    assert not np.array_equal(bits(frames[0][1]), bits(frames[1][1]))
    assert not np.array_equal(bits(frames[1][1]), bits(frames[2][1]))


def test_poses_change_under_a_valid_table(dragon):
    """A 6-step turntable of the dragon (mesh 0 of two; attenuation renders it)
    under a fixed rolled camera: one fill, every step rendered from the table,
    each equal to the oracle over the posed triangles."""
    W, H = 67, 45
    meshes = [dragon, second_mesh_for(dragon)]
    c13 = ck.case_camera("roll30", meshes, W, H)
    cam = ck.as_camera(c13, W, H)
    centre = ck.scene_centre([dragon]).astype(np.float32)
    with xrt.Context(0) as c:
        c.set_kernel(BINNED)
        c.upload_scene(meshes)
        last = render_until_served(c, cam)
        assert_frame(last, oracle.render_scene_rows(meshes, c13, W, H), W, H, "rest")
        for k in range(1, 7):
            q = xrt.pose_rotation((0, 0, 1), 25.0 * k, centre)
            c.set_pose(0, q)
            got = served(c, lambda: c.render_rows(cam))
            ref = oracle.render_scene_rows(pose_ref.apply(meshes, {0: q}), c13, W, H)
            assert np.count_nonzero(ref[3]) > 0, k
            assert_frame(got, ref, W, H, f"step {k}")
            assert not np.array_equal(bits(got[1]), bits(last[1])), k
            last = got
        n = c.ray_table_counters()
        assert n["fills"] == 1 and n["frames"] >= 7, n


# --------------------------------------------------------------------------- what shares render_tile with the table
@pytest.mark.parametrize("cap", [2, 5])
def test_overflow_fixup_served(binned, oracle_frames, cap):
    """A hit list of 2 and of 5 entries: the rays past it take the exact fix-up, over the table's directions."""
    c13, ref = oracle_frames(128, 128)
    binned.set_hit_capacity(cap)
    got = render_until_served(binned, ck.as_camera(c13, 128, 128))
    want = int(np.count_nonzero(ref[3] > cap))
    assert want > 0 and got[3].overflow_rays == want
    assert_same(got, ref, f"cap {cap}")
    assert got[3].rays == 128 * 128


def planned_dragon(dragon, W, H, r0=0, r1=None):
    """(triangles, c13, the oracle's frame): a scene of the dragon that has a
    fill plan at 4 x 4 regions.  Tiles are split, and a tile plan is taken, only
    under a fill plan, which a geometry has when some region is without
    candidates.  The dragon has about a hundred triangles seen edge-on whose
    loosened footprint boxes are hundreds of pixels wide; in so small a frame
    they reach every region under every camera (measured: no fill plan at
    128 x 128 under its own camera, the off-axis one or one three times
    further out; from 160 x 160 on there is one).  So: the off-axis camera,
    which leaves the right and upper regions without a hit, and the dragon
    without the triangles whose footprint box (the cull's host build) is 32
    pixels or more either way -- they hit no pixel of these frames."""
    r1 = H if r1 is None else r1
    c13 = ck.case_camera("offaxis", [dragon], W, H)
    fp = host_footprints(c13, W, H, dragon)
    keep = (fp[:, 1] - fp[:, 0] < 32.0) & (fp[:, 3] - fp[:, 2] < 32.0)
    assert 0 < np.count_nonzero(~keep) < 200
    tris = np.ascontiguousarray(dragon[keep])
    ref = oracle.render_rows(tris, c13, W, H, r0, r1)
    assert ref[3].max() >= 6 and np.count_nonzero(ref[3]) > 500
    return tris, c13, ref


@pytest.mark.parametrize("W,H,r0,r1", [(128, 128, 0, 128), (100, 77, 13, 61)])
def test_split_tiles_served(dragon, monkeypatch, W, H, r0, r1):
    """XRT_SPLIT_MIN=1 (read at xrt_create: every region with a candidate
    renders each tile with two waves, both reading the tile's planes): the
    third frame is rendered from the table; all three are exact.  (The fill
    plan that the second frame's sizing made -- some region filled -- is what
    lets tiles split: planned_dragon.)"""
    monkeypatch.setenv("XRT_SPLIT_MIN", "1")
    tris, c13, ref = planned_dragon(dragon, W, H, r0, r1)
    cam = ck.as_camera(c13, W, H)
    with xrt.Context(0) as c:
        c.set_kernel(BINNED)
        c.upload_mesh(tris)
        for frame in range(2):
            assert_frame(c.render_rows(cam, r0, r1), ref, W, r1 - r0, f"frame {frame}")
        assert c.fill_regions() > 0
        assert_frame(served(c, lambda: c.render_rows(cam, r0, r1)), ref, W, r1 - r0, "frame 2")
        assert c.fill_regions() > 0


def test_tile_plan_and_table_together(dragon):
    """Six frames at 128 x 128 with the tile plan on (planned_dragon: a scene
    with a fill plan at this size): frames are rendered both with a tile plan
    and from the table, and every frame is exact."""
    tris, c13, ref = planned_dragon(dragon, 128, 128)
    cam = ck.as_camera(c13, 128, 128)
    both = 0
    with xrt.Context(0) as c:
        c.set_kernel(BINNED)
        c.upload_mesh(tris)
        c.set_tile_plan(True)
        for k in range(6):
            t0, n0 = c.tile_plan_counters()["frames"], c.ray_table_counters()["frames"]
            assert_frame(c.render_rows(cam), ref, 128, 128, f"frame {k}")
            t1, n1 = c.tile_plan_counters()["frames"], c.ray_table_counters()["frames"]
            both += t1 == t0 + 1 and n1 == n0 + 1
        n = c.ray_table_counters()
        assert (n["fills"], n["frames"], n["computed"]) == (1, 5, 1), n
        assert c.tile_plan_counters()["plans"] == 1 and c.tile_plan_counters()["frames"] >= 3 and both >= 3, \
            (c.tile_plan_counters(), both)


def test_packed_transit_served(binned, dragon):
    """A strip of a 96 x 128 frame rendered into the packed transit layout
    (xrt_set_transit_layout: in the table's scope) twice under a live table:
    both rendered from it, and the blocks unpacked equal the direct render,
    which equals the oracle's.  (The packed layout needs a fill plan:
    planned_dragon, rows 5 to 61, whose upper regions are without candidates.)"""
    import torch
    W, H, r0, r1 = 96, 128, 5, 61
    rows = r1 - r0
    tris, c13, ref = planned_dragon(dragon, W, H, r0, r1)
    cam = ck.as_camera(c13, W, H)
    c = binned
    c.upload_mesh(tris)
    direct = render_until_served(c, cam, r0, r1)
    assert_frame(direct, ref, W, rows)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lb = torch.full((W * rows,), -1.0, device=dev)
    c.set_miss_code(xrt._abi.XRT_MISS_TRANSIT)
    try:
        served(c, lambda: c.render_rows_device(cam, r0, r1, 0, lb.data_ptr(), 0, stream.cuda_stream))
        rmap, n_packed = c.plan_region_map(W, rows)
        n_fill = c.fill_regions()
        assert n_packed == len(rmap) - n_fill and n_packed > 0 and n_fill > 0
        packed = torch.full((n_packed * 1024,), -3.0, device=dev)
        c.set_transit_layout(packed.numel())
        try:
            for _ in range(2):
                served(c, lambda: c.render_rows_device(cam, r0, r1, 0, packed.data_ptr(), 0, stream.cuda_stream))
                assert c.fill_regions() == n_fill
        finally:
            c.set_transit_layout(0)
    finally:
        c.set_miss_code(0)
    assert c.ray_table_counters()["fills"] == 1
    d_map = torch.from_numpy(rmap.view(np.int32)).to(dev)
    out = [torch.full((W * rows,), -2.0, device=dev), torch.zeros(W * rows, device=dev),
           torch.zeros(W * rows, dtype=torch.uint8, device=dev)]
    c.unpack_regions_device(W, rows, d_map.data_ptr(), packed.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                            out[2].data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize(dev)
    assert same_planes((out[1].cpu().numpy(), out[0].cpu().numpy(), out[2].cpu().numpy()), direct)


# --------------------------------------------------------------------------- lifetime
def test_table_grows_with_frames_in_flight(binned, oracle_frames):
    """12 frames at 64 x 64, 12 at 160 x 128, 12 at 64 x 64 again over two
    streams, nothing waited for in between: the second key's table is larger,
    so its fill frees and allocates -- only once no launched render reads the
    old buffer and no fill writes it.  The last frame of each run on each
    stream is exact, and the buffer is the largest table's."""
    import torch
    dev = torch.device("cuda", 0)
    qs = [torch.cuda.Stream(dev) for _ in range(2)]
    runs = []
    for W, H in ((64, 64), (160, 128), (64, 64)):
        c13, ref = oracle_frames(W, H)
        sets = [(torch.zeros(W * H, device=dev), torch.zeros(W * H, device=dev),
                 torch.zeros(W * H, dtype=torch.uint8, device=dev)) for _ in qs]
        binned.render_frames_device(ck.as_camera(c13, W, H), 0, H, 12,
                                    [(i.data_ptr(), l.data_ptr(), u.data_ptr(), q.cuda_stream)
                                     for (i, l, u), q in zip(sets, qs)])
        runs.append((ref, sets))
    torch.cuda.synchronize(dev)
    n = binned.ray_table_counters()
    assert n["frames"] + n["computed"] == 36 and 1 <= n["fills"] <= 3, n
    assert n["bytes"] == 12 * 160 * 128 == 4 * xrt.ray_table_index(160, 128, 0, 128, 0, 0)[1], n
    for ref, sets in runs:
        for planes in sets:
            assert same_planes([p.cpu().numpy() for p in planes], ref)


BUDGET_CHILD = """
import json, os, sys
import numpy as np
sys.path.insert(0, {root!r})
import simpleraytracing_amd as xrt
from oracle import oracle
threads = min(16, os.cpu_count() or 1)
tris = oracle.load_ply({ply!r})
log = []
with xrt.Context(0) as c:
    c.set_kernel(xrt.XRT_KERNEL_BINNED)
    c.upload_mesh(tris)
    for size, frames in ((256, 3), (320, 4), (256, 2)):
        c13 = oracle.camera_for_mesh(tris, size, size)
        ref = oracle.render_rows(tris, c13, size, size, threads=threads)
        cam = xrt.camera_for_mesh(tris, size, size)
        for _ in range(frames):
            img, lb, u8, st = c.render_rows(cam)
            exact = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((img, lb, u8), ref[:3]))
            exact = exact and st.hits == int(ref[3].sum()) and st.hit_rays == int(np.count_nonzero(ref[3]))
            log.append([size, bool(exact), c.ray_table_counters()])
print(json.dumps(log))
"""


def test_budget_boundary():
    """XRT_RAY_CACHE_MB=1 (read at xrt_create: a fresh process).  A 256 x 256
    table fits the budget: filled, its frames rendered from it.  A 320 x 320
    table does not: four frames compute, nothing is filled or allocated.  256
    x 256 again: one more fill.  Every frame equals the oracle's."""
    b256 = 4 * xrt.ray_table_index(256, 256, 0, 256, 0, 0)[1]
    b320 = 4 * xrt.ray_table_index(320, 320, 0, 320, 0, 0)[1]
    assert b256 <= 1 << 20 < b320
    code = BUDGET_CHILD.format(root=ROOT, ply=os.path.join(ROOT, "data", "dragon.ply"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, XRT_RAY_CACHE_MB="1"), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    log = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(exact for _, exact, _ in log), [(s, e) for s, e, _ in log]
    got = [(s, n["fills"], n["frames"], n["computed"], n["bytes"]) for s, _, n in log]
    want = [(256, 0, 0, 1, 0), (256, 1, 1, 1, b256), (256, 1, 2, 1, b256),
            (320, 1, 2, 2, b256), (320, 1, 2, 3, b256), (320, 1, 2, 4, b256), (320, 1, 2, 5, b256),
            (256, 1, 2, 6, b256), (256, 2, 3, 6, b256)]
    assert got == want, got
