"""The ray table's index function ("Ray table"), through
xrt_debug_ray_table_index: host code, the function k_ray_table and the render
address the table with.  No GPU."""
import numpy as np
import pytest

import simpleraytracing_amd as xrt

CASES = [(8, 8, 0, 8), (100, 77, 0, 77), (33, 65, 0, 65), (33, 65, 13, 61), (33, 65, 32, 33)]


@pytest.mark.parametrize("W,H,r0,r1", CASES)
def test_every_pixel_has_its_own_place(W, H, r0, r1):
    """Every pixel of the strip maps to a distinct index, and its dz (128
    floats past its dx) still lies below the allocated size; the size is 12
    bytes per pixel of the strip padded to whole 32 x 32 regions."""
    seen = set()
    floats = None
    for row in range(r0, r1):
        for col in range(W):
            i, n = xrt.ray_table_index(W, H, r0, r1, row, col)
            floats = n if floats is None else floats
            assert n == floats
            assert i + 128 < n, (row, col, i, n)
            # the three planes of a tile are 64 floats each: dx indices never meet dy / dz ones
            assert i % 192 < 64
            seen.add(i)
    assert len(seen) == (r1 - r0) * W
    pad = lambda v: (v + 31) // 32 * 32
    assert floats == 3 * pad(W) * pad(r1 - r0)


def test_layout_is_tile_major_in_lane_order():
    """Tile (tx, ty) owns 192 contiguous floats, lane = (row & 7) * 8 + (col & 7)
    relative to the strip's first row."""
    W, H, r0, r1 = 100, 77, 13, 61
    tiles_x = (W + 31) // 32 * 4
    for row, col in [(13, 0), (13, 7), (14, 0), (20, 99), (21, 8), (60, 99)]:
        r = row - r0
        want = ((r // 8) * tiles_x + col // 8) * 192 + (r & 7) * 8 + (col & 7)
        assert xrt.ray_table_index(W, H, r0, r1, row, col)[0] == want


def test_rejects_pixels_outside_the_strip():
    for args in [(33, 65, 13, 61, 12, 0), (33, 65, 13, 61, 61, 0), (33, 65, 13, 61, 13, 33), (33, 65, 13, 66, 13, 0),
                 (33, 65, 13, 13, 13, 0)]:
        with pytest.raises(xrt.XrtError):
            xrt.ray_table_index(*args)


@pytest.mark.parametrize("W,H,r0,r1", CASES + [(1, 1, 0, 1), (67, 45, 0, 45), (100, 37, 5, 30), (96, 128, 40, 41)])
def test_numpy_restatement_of_the_layout(W, H, r0, r1):
    """ray_table_kit.table_indices (the GPU suite builds the whole expected
    table with it) agrees with the kernels' function at every pixel of the
    strip, and covers the padded table's every float exactly once."""
    import ray_table_kit as rk
    idx, r, c = rk.table_indices(W, r0, r1)
    assert idx.shape == (rk.pad32(r1 - r0), rk.pad32(W))
    floats = xrt.ray_table_index(W, H, r0, r1, r0, 0)[1]
    assert floats == 3 * idx.size
    for row in range(r0, r1):
        for col in range(W):
            assert xrt.ray_table_index(W, H, r0, r1, row, col)[0] == idx[row - r0, col]
    every = np.concatenate([idx.ravel() + 64 * k for k in range(3)])
    assert np.array_equal(np.sort(every), np.arange(floats))


def test_degenerate_cameras_have_the_expected_nan_pattern():
    """The two degenerate cameras of the GPU suite, on the CPU: the source on
    the detector's centre has NaN at the centre pixel only, the underflowing
    camera everywhere; neither reaches the second normalisation's zero-length
    branch (no direction is (0, 0, 0)).  The random cameras are all finite."""
    import camera_kit as ck
    import ray_table_kit as rk
    c13, W, H = rk.source_on_detector_camera()
    d = ck.ray_directions(c13, W, H)
    nan = np.isnan(d)
    assert nan[H // 2, W // 2].all() and nan.sum() == 3 and np.isfinite(d[~nan]).all()
    assert not (d == 0).all(axis=2).any()
    c13, W, H = rk.underflow_camera()
    d = ck.ray_directions(c13, W, H)
    assert np.isnan(d).all()
    raw = c13[3:6] - c13[0:3]
    assert (np.abs(raw) > np.finfo(np.float32).tiny).all() and (raw * raw == 0).all()
    for c13, W, H in rk.random_cameras():
        assert np.isfinite(ck.ray_directions(c13, W, H)).all()


def test_reader_refuses_without_a_context():
    from simpleraytracing_amd import _abi
    buf = np.zeros(4, np.float32)
    assert _abi.load().xrt_debug_ray_table_read(None, buf.ctypes.data, 4, None) == _abi.XRT_ERR_ARGUMENT


def test_cached_render_keeps_eight_waves_without_scratch():
    """k_render_binned_rays keeps 8 waves per SIMD -- at most 64 VGPRs of 512, 8 KB of
    LDS for its four waves -- and spills nothing into scratch, as the computing
    instantiation beside it; k_ray_table uses no scratch either.
    (profiles/ray_table/resources.txt has every kernel's figures.)"""
    from test_materials_cpu import _render_kernel_metadata
    meta = _render_kernel_metadata()
    rays = [f for k, f in meta.items() if "k_render_binned_rays" in k]
    computing = [f for k, f in meta.items() if "k_render_binnedILj0E" in k]
    fill = [f for k, f in meta.items() if "k_ray_table" in k]
    assert len(rays) == 1 and len(computing) == 1 and len(fill) == 1, sorted(meta)
    for f in rays + computing:
        assert f["vgpr_count"] <= 64 and f["group_segment_fixed_size"] == 8192, f
    for f in rays + computing + fill:
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, f


def test_size_at_the_headline_frames():
    """48 MiB at 2048^2 and 192 MiB at 4096^2: inside the default budget of 256 MiB."""
    assert xrt.ray_table_index(2048, 2048, 0, 2048, 0, 0)[1] * 4 == 48 << 20
    assert xrt.ray_table_index(4096, 4096, 0, 4096, 0, 0)[1] * 4 == 192 << 20
    assert np.uint64(xrt.ray_table_index(4096, 4096, 0, 4096, 4095, 4095)[0]) < np.uint64(48 << 20)
