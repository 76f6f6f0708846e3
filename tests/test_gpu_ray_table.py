"""The ray table ("Ray table"): an attenuation BINNED
frame that repeats the previous one's camera, size and strip has the camera's
rays tabulated once (k_ray_table), and the frames after it read them
(k_render_binned_rays) where the others run make_ray_from.  Every frame here is
compared bit for bit -- image, L-buffer, u8, statistics -- with the same frame
computed (the table off, the brute kernel, the committed fixtures)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import simpleraytracing_amd as xrt
from conftest import GOLDEN, ROOT, bits

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
