"""FDK reconstruction on the GPU: k_fdk_filter and k_backproject against
tests/fdk_ref.py bit for bit through both entry forms, the ball scan through Context.fdk,
and xrt_main --reconstruct end to end."""
import os
import subprocess

import numpy as np
import pytest

import camera_kit
import fdk_kit
import fdk_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import ROOT, bits
from scene_kit import box
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
# k_fdk_filter (csrc/kernels/xrt_kernels.h): a wave owns 448 outputs, a workgroup 2240
WAVE_OUT, SEGMENT = 448, 2240
# rows past one wave, past one workgroup, and the widest with the longest table (one stack, to stay quick)
WIDE_PLANES = [(WAVE_OUT + 1, 2), (SEGMENT + 1, 2), (xrt.XRT_MAX_RAMP_WIDTH, 1)]
# a row of voxels past one wave's span of 256 (csrc/kernels/xrt_kernels.h: kBackprojectSpan)
BP_DIMS = fdk_kit.BP_DIMS + [(261, 2, 2)]


@pytest.fixture(scope="module")
def fctx():
    """A context of this module's own."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def same(got, want, what):
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    if not fdk_kit.same_bits(got, want):
        bad = np.argwhere((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError((what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ------------------------------------------------------------------------------- the filter
@pytest.mark.parametrize("W,H", fdk_kit.FILTER_PLANES + WIDE_PLANES)
def test_filter_equals_the_reference(fctx, W, H):
    wide = (W, H) in WIDE_PLANES
    for P in ([1] if wide else fdk_kit.FILTER_STACKS):
        for T in ([2 * W - 1] if wide else fdk_kit.filter_tap_counts(W)):
            for weighted in ([True] if wide else [False, True]):
                a = fdk_kit.filter_image(W * 100 + H + T, P, H, W)
                taps = fdk_kit.filter_taps(T, T)
                wt = fdk_kit.filter_weight(W, H, W) if weighted else None
                same(fctx.fdk_filter(a, taps, wt), fdk_ref.fdk_filter(a, taps, wt), (W, H, P, T, weighted))


@pytest.mark.parametrize("W,H,T", [(xrt.XRT_MAX_RAMP_WIDTH, 1, 3), (SEGMENT + 1, 2, 9), (SEGMENT + 1, 2, 2 * 300 + 1)])
def test_filter_short_table_over_a_wide_row(fctx, W, H, T):
    """A row wider than one workgroup's 2240 outputs under a table shorter than the row: the second segment's LDS
    window begins inside the row (x0 - r > 0)."""
    a = fdk_kit.filter_image(W + T, 1, H, W)
    taps = fdk_kit.filter_taps(T, T)
    same(fctx.fdk_filter(a, taps), fdk_ref.fdk_filter(a, taps), (W, H, T))


@pytest.mark.parametrize("W,H", [(1, 1), (7, 13), (67, 3), (WAVE_OUT + 1, 3), (2049, 2), (xrt.XRT_MAX_RAMP_WIDTH, 1)])
def test_filter_under_ramp_tables(fctx, W, H):
    """The library's own tables, 2 W - 1 taps and longer (k_fdk_filter_wide).  Ram-Lak's taps at even distances
    from the centre are zeros, which the kernel leaves out where the rows are finite; a Hann window's are not;
    one more even tap, a NaN or an infinity in a row (0 * inf is NaN), or a -0.0 tap, and the bits are still the
    reference's.  An odd number of rows: the last workgroup's second row does not exist."""
    for T in (2 * W - 1, min(2 * W + 5, 2 * xrt.XRT_MAX_RAMP_WIDTH - 1)):
        for window in (xrt.XRT_RAMP_RAMLAK, xrt.XRT_RAMP_HANN):
            taps = xrt.ramp_filter(T, window)
            a = fdk_kit.filter_image(W + T + window, 1 if W > 2048 else 3, H, W)
            wt = fdk_kit.filter_weight(W, H, W)
            same(fctx.fdk_filter(a, taps, wt), fdk_ref.fdk_filter(a, taps, wt), (W, H, T, window))
            bad = a.copy()
            bad[0, 0, W // 2] = np.inf
            bad[-1, -1, 0] = np.nan
            same(fctx.fdk_filter(bad, taps), fdk_ref.fdk_filter(bad, taps), (W, H, T, window, "non-finite"))
        taps = xrt.ramp_filter(T, xrt.XRT_RAMP_RAMLAK)
        r = (T - 1) // 2
        signed = taps.copy()
        signed[r % 2::2][signed[r % 2::2] == 0] = F(-0.0)               # the zeros at even distances, negative
        assert (bits(signed) == 0x80000000).any() or T < 5
        same(fctx.fdk_filter(a, signed), fdk_ref.fdk_filter(a, signed), (W, H, T, "-0.0 taps"))
        if T >= 5:
            dense = taps.copy()
            dense[r + 2] = F(0.125)                                      # one tap at an even distance
            same(fctx.fdk_filter(a, dense), fdk_ref.fdk_filter(a, dense), (W, H, T, "one even tap"))


@pytest.mark.parametrize("W,H", [(7, 13), (67, 45), (WAVE_OUT + 1, 2)])
def test_filter_carries_nan_inf_and_negative_zero(fctx, W, H):
    """NaN, +-inf and -0.0 among the pixels: what IEEE arithmetic makes of them in the written order (a NaN's
    sign and payload apart); the zeros the kernel pads its row with never meet them."""
    for T in (1, 3, 2 * W - 1):
        a = fdk_kit.filter_image(W + T, 2, H, W, specials=True)
        assert np.isnan(a).any() and np.isinf(a).any() and (bits(a) == 0x80000000).any()
        taps = fdk_kit.filter_taps(T + 1, T)
        wt = fdk_kit.filter_weight(W, H, W)
        same(fctx.fdk_filter(a, taps), fdk_ref.fdk_filter(a, taps), (W, H, T))
        same(fctx.fdk_filter(a, taps, wt), fdk_ref.fdk_filter(a, taps, wt), (W, H, T, "weighted"))
    z = fctx.fdk_filter(np.full((1, 3), -0.0, F), [1.0])
    assert not bits(z).any()                                             # the sum starts at +0.0


def test_filter_device_form(fctx):
    """Device pointers for the image, the weight, the taps and out, two calls back to back on one stream."""
    import torch
    W, H, P = 67, 45, 3
    a = fdk_kit.filter_image(5, P, H, W)
    wt = fdk_kit.filter_weight(5, H, W)
    t1, t2 = fdk_kit.filter_taps(1, 2 * W - 1), fdk_kit.filter_taps(2, 9)
    d_a, d_w = torch.from_numpy(a).to("cuda"), torch.from_numpy(wt).to("cuda")
    d_t1, d_t2 = torch.from_numpy(t1).to("cuda"), torch.from_numpy(t2).to("cuda")
    outs = [torch.full((P, H, W), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    with pytest.raises(xrt.XrtError) as e:
        fctx.fdk_filter_device(W, H, P, d_a.data_ptr(), d_t1.data_ptr(), t1.size, d_a.data_ptr() + 4 * (P * H * W - 1))
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)
    fctx.fdk_filter_device(W, H, P, d_a.data_ptr(), d_t1.data_ptr(), t1.size, outs[0].data_ptr(), d_w.data_ptr())
    fctx.fdk_filter_device(W, H, P, d_a.data_ptr(), d_t2.data_ptr(), t2.size, outs[1].data_ptr())
    torch.cuda.synchronize()
    same(outs[0].cpu().numpy(), fdk_ref.fdk_filter(a, t1, wt), "first taps")
    same(outs[1].cpu().numpy(), fdk_ref.fdk_filter(a, t2), "second taps")


# ------------------------------------------------------------------------------- the backprojector
@pytest.mark.parametrize("dims", BP_DIMS)
def test_backprojector_equals_the_reference(fctx, dims):
    for W, H in fdk_kit.BP_PLANES:
        for P in fdk_kit.BP_STACKS:
            proj = fdk_kit.projections(W + H + P, P, H, W)
            mats = fdk_kit.general_matrices(P, dims, W, H, seed=P)
            want = fdk_ref.backproject(proj, mats, dims, 0.37)
            same(fctx.backproject(proj, mats, dims, 0.37), want, (dims, W, H, P))
            assert np.abs(want).max() > 0, (dims, W, H, P)               # the grid is in view


@pytest.mark.parametrize("W,H", [(7, 5), (67, 45)])
def test_backprojector_edges_nan_slabs_and_accumulation(fctx, W, H):
    """Hand-built matrices: voxels exactly on col (row) = -1, 0, W - 1 (H - 1) and W (H), outside, on half
    pixels, and with c = 0 and c < 0; a NaN plane; slabs against the whole volume; two halves of the planes
    accumulated against the reference of the same two steps."""
    mats, dims = fdk_kit.edge_matrices(W, H)
    proj = fdk_kit.projections(3, 3, H, W)
    whole = fdk_ref.backproject(proj, mats, dims, 2.0)
    same(fctx.backproject(proj, mats, dims, 2.0), whole, "whole")
    first = fctx.backproject(proj[:1], mats[:1], dims, 1.0)
    assert np.array_equal(first[0, 1:H + 1, 1:W + 1], proj[0]) and not first[1].any()
    assert not first[0, 0].any() and not first[0, :, 0].any() and not first[0, H + 1:].any() and not first[0, :, W + 1:].any()
    nan = fdk_kit.projections(4, 3, H, W, nan_plane=1)
    want = fdk_ref.backproject(nan, mats, dims, 1.0)
    assert np.isnan(want).any() and not np.isnan(want).all()
    same(fctx.backproject(nan, mats, dims, 1.0), want, "NaN plane")
    for slabs in ((0, 1), (1, 2), (2, dims[2]), (1, 1)):
        got = fctx.backproject(proj, mats, dims, 2.0, slabs=slabs)
        same(got, whole[slabs[0]:slabs[1]], slabs)
    half = fdk_ref.backproject(proj[:2], mats[:2], dims, 2.0)
    both = fdk_ref.backproject(proj[2:], mats[2:], dims, 2.0, volume=half, accumulate=True)
    got = fctx.backproject(proj[2:], mats[2:], dims, 2.0, volume=fctx.backproject(proj[:2], mats[:2], dims, 2.0),
                           accumulate=True)
    same(got, both, "accumulated")


def test_backprojector_slabs_of_a_deeper_volume(fctx):
    dims, (W, H), P = (67, 9, 3), (67, 45), 3
    proj = fdk_kit.projections(8, P, H, W)
    mats = fdk_kit.general_matrices(P, dims, W, H)
    whole = fdk_ref.backproject(proj, mats, dims, 1.5)
    for slabs in ((0, 1), (1, 2), (2, 3), (3, 3)):
        same(fctx.backproject(proj, mats, dims, 1.5, slabs=slabs), whole[slabs[0]:slabs[1]], slabs)


def test_backprojector_device_form(fctx):
    """Device pointers; a slab range into a buffer of its own size with guard words behind it; accumulation in
    place on the device."""
    import torch
    dims, (W, H), P = (67, 9, 3), (67, 45), 3
    proj = fdk_kit.projections(9, P, H, W)
    mats = fdk_kit.general_matrices(P, dims, W, H)
    whole = fdk_ref.backproject(proj, mats, dims, 0.5)
    d_p, d_m = torch.from_numpy(proj).to("cuda"), torch.from_numpy(mats.reshape(-1)).to("cuda")
    n = dims[0] * dims[1]
    d_v = torch.full((2 * n + 16,), -7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(xrt.XrtError) as e:
        fctx.backproject_device(W, H, P, d_p.data_ptr(), d_m.data_ptr(), dims, 0, 3, 0.5, False, d_p.data_ptr() + 64)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)
    fctx.backproject_device(W, H, P, d_p.data_ptr(), d_m.data_ptr(), dims, 1, 3, 0.5, False, d_v.data_ptr())
    fctx.backproject_device(W, H, P, d_p.data_ptr(), d_m.data_ptr(), dims, 2, 2, 0.5, False, d_v.data_ptr() + 8 * n)   # empty: nothing written
    torch.cuda.synchronize()
    got = d_v.cpu().numpy()
    same(got[:2 * n].reshape(2, dims[1], dims[0]), whole[1:3], "slabs 1..3")
    assert (got[2 * n:] == -7.0).all()                                   # nothing behind the slabs
    fctx.backproject_device(W, H, P, d_p.data_ptr(), d_m.data_ptr(), dims, 1, 3, 0.5, True, d_v.data_ptr())
    torch.cuda.synchronize()
    twice = fdk_ref.backproject(proj, mats, dims, 0.5, slabs=(1, 3), volume=whole[1:3], accumulate=True)
    same(d_v.cpu().numpy()[:2 * n].reshape(2, dims[1], dims[0]), twice, "accumulated on the device")


# ------------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("posed", [False, True], ids=["turning-camera", "posed-object"])
def test_ball_scan_through_the_context(fctx, posed):
    """tests/test_fdk_cpu.py's scan through Context.fdk: bit-equal to the reference (fed the library's own
    matrices: two routes to one inverse differ in their last bits), and within the same bounds."""
    proj, cams, poses = fdk_kit.scan(posed)
    W, H = fdk_kit.SCAN_W, fdk_kit.SCAN_H
    cs = [camera_kit.as_camera(c, W, H) for c in cams]
    vol = fctx.fdk(proj, cs[0] if posed else cs, poses, fdk_kit.SCAN_DIMS, fdk_kit.SCAN_ORIGIN, fdk_kit.SCAN_SPACING,
                   fdk_kit.SCAN_AXIS_POINT)
    mats = np.stack([xrt.backprojection_matrix(cs[p], fdk_kit.SCAN_ORIGIN, fdk_kit.SCAN_SPACING,
                                               poses[p] if posed else None) for p in range(len(cs))])
    same(vol, fdk_kit.scan_reference(posed, matrices=mats), "scan")
    fdk_kit.check_ball(vol)


# ------------------------------------------------------------------------------- the CLI
def test_cli_reconstructs_a_box(tmp_path):
    """xrt_main --turntable 24:z --log-projection 80 --reconstruct: the .mhd loads, and the interior of the box
    holds the attenuation model's coefficient per scene length unit (0.3971 per cm, a unit being a mm) within
    5 % -- loose on purpose: 24 projections of traced rays; this checks the wiring, not the accuracy.  The box is
    taller than wide, so that its shadow stays on the detector under every turn (the scene's camera fits the
    detector to the box at rest; a truncated row reconstructs too high), and its corners are no round numbers: a
    ray that meets the shared edge of a face's two triangles exactly is a hole in the render, and symmetric
    geometry turned by 90 degrees puts pixels there.  Measured: interior mean 0.9946 mu."""
    lo, hi = np.array([-5.3, -6.1, -9.2]), np.array([5.0, 4.4, 10.7])
    _write_obj(tmp_path / "box.obj", box(lo, hi))
    (tmp_path / "out").mkdir()
    r = subprocess.run([EXE, "-s", "96", "96", "-i", str(tmp_path / "box.obj"), "-f", "p.txt", "--turntable", "24:z",
                        "--log-projection", "80", "--reconstruct", str(tmp_path / "box.mhd") + ":48"],
                       capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE, "-s", "16", "16", "-i", str(tmp_path / "box.obj"), "-f", "q.txt", "--turntable", "4",
                        "--log-projection", "80", "--reconstruct", "y.mhd:8"], capture_output=True, text=True,
                       cwd=tmp_path, timeout=300)
    assert r.returncode == 1 and "parallel to the detector's up" in r.stderr      # (the default axis, y, lies along the rows)
    vol, spacing, origin = xrt.load_volume(str(tmp_path / "box.mhd"))
    assert vol.dtype == F and vol.shape == (48, 48, 48)
    centre = 0.5 * (lo + hi)
    diagonal = np.linalg.norm(hi - lo)
    assert np.allclose(spacing, diagonal / 48, rtol=1e-6) and np.allclose(origin, centre - diagonal / 2, rtol=1e-5)
    kk, jj, ii = np.meshgrid(*[np.arange(48)] * 3, indexing="ij")
    X = origin.astype(D) + (np.stack([ii, jj, kk], -1) + 0.5) * spacing.astype(D)
    inner = np.all((X > lo + 3.0) & (X < hi - 3.0), axis=-1)
    outer = np.any((X < lo - 3.0) | (X > hi + 3.0), axis=-1) & (np.linalg.norm(X - centre, axis=-1) < diagonal / 2 - 3)
    mu = 0.3971 * 0.1
    mean = float(vol[inner].mean())
    print(f"box: interior mean {mean:.5f} (mu {mu:.5f}), outside mean {float(vol[outer].mean()):.5f}, {inner.sum()} voxels")
    assert inner.sum() > 1000 and abs(mean / mu - 1.0) <= 0.05, mean
    # refused where --sinogram is: before anything is loaded
    for args in (["--turntable", "24"], ["--log-projection", "80"], ["--turntable", "24:y:0", "--log-projection", "80"]):
        r = subprocess.run([EXE, "-i", str(tmp_path / "box.obj"), *args, "--reconstruct", "x.mhd"], capture_output=True,
                           text=True, cwd=tmp_path, timeout=120)
        assert r.returncode == 1 and "--reconstruct needs" in r.stderr and "Loading" not in r.stdout, r.stderr
