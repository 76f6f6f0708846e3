"""TV-regularised SIRT on the GPU: k_tv_gradient, the sum of squares and the
descent against tests/tv_ref.py bit for bit through both entry forms, Context.sirt with tv on
the small scan and on the noisy ball scan, and xrt_main --reconstruct --sirt --tv end to end."""
import os
import subprocess

import numpy as np
import pytest

import camera_kit
import fdk_kit
import sirt_kit
import tv_kit
import tv_ref
import simpleraytracing_amd as xrt
from conftest import ROOT, bits
from scene_kit import box
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


@pytest.fixture(scope="module")
def tctx():
    """A context of this module's own."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def same(got, want, what):
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    if not fdk_kit.same_bits(got, want):
        bad = np.argwhere((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError((what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def device_gradient(ctx, vol, eps):
    """Context.tv_gradient_device over buffers of exactly the volume's size plus guard words."""
    import torch
    d_v = torch.from_numpy(np.array(vol, F)).to("cuda")
    out = torch.full((vol.size + 16,), -7.0, dtype=torch.float32, device="cuda")
    ctx.tv_gradient_device(d_v.data_ptr(), vol.shape[::-1], out.data_ptr(), eps)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[vol.size:] == -7.0).all()
    return got[:vol.size].reshape(vol.shape)


def gradient_both_forms(ctx, vol, eps, what):
    want = tv_ref.gradient(vol, eps)
    same(ctx.tv_gradient(vol, eps), want, (what, "host form"))
    same(device_gradient(ctx, vol, eps), want, (what, "device form"))


# ------------------------------------------------------------------------------- the gradient
@pytest.mark.parametrize("dims", tv_kit.GRIDS)
def test_gradient_equals_the_reference(tctx, dims):
    """The small grids: plain and NaN, +-inf and -0.0 voxels, every eps."""
    for specials in (False, True):
        vol = tv_kit.volume(sum(dims), dims, specials)
        for eps in tv_kit.EPSILONS:
            gradient_both_forms(tctx, vol, eps, (dims, specials, eps))


@pytest.mark.parametrize("dims", tv_kit.tile_grids())
def test_gradient_about_the_tile(tctx, dims):
    """One voxel below, at and above the tile's extent on each axis (the rim and halo lanes, the chunk's first slice
    and the slice under it), and a grid of more than two tiles a side and more than one chunk: the kernel's loop along
    z past a chunk's end."""
    vol = tv_kit.volume(sum(dims), dims, specials=True)
    gradient_both_forms(tctx, vol, 1e-8, dims)


def test_gradient_refuses_overlap_on_the_device(tctx):
    import torch
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    with pytest.raises(xrt.XrtError) as e:
        tctx.tv_gradient_device(buf.data_ptr(), (5, 3, 2), buf.data_ptr() + 64)
    assert e.value.code == xrt._abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)


# ------------------------------------------------------------------------------- the sum of squares
@pytest.mark.parametrize("n", tv_kit.SUMSQ_LENGTHS + [tv_kit.SUMSQ_LONG])
def test_sumsq_equals_the_reference(tctx, n):
    """One, two and (2^24 + 4097 entries) three levels, with and without b, both forms."""
    import torch
    a, b = tv_kit.sumsq_vectors(n)
    d_a, d_b = torch.from_numpy(a.copy()).to("cuda"), torch.from_numpy(b.copy()).to("cuda")
    for with_b in (False, True):
        want = tv_kit.sumsq_reference(n, with_b)
        got = tctx.volume_sumsq(a, b if with_b else None)
        assert tv_kit.same_double(got, want), (n, with_b, "host form", got, want)
        out = torch.full((3,), -7.0, dtype=torch.float64, device="cuda")
        tctx.volume_sumsq_device(n, d_a.data_ptr(), d_b.data_ptr() if with_b else 0, out.data_ptr() + 8)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert tv_kit.same_double(o[1], want) and o[0] == -7.0 and o[2] == -7.0, (n, with_b, "device form", o, want)


def test_sumsq_of_special_values(tctx):
    a = np.array([1.0, np.inf, -2.0], F)
    assert tctx.volume_sumsq(a) == np.inf and np.isnan(tctx.volume_sumsq(a, a)) and np.isnan(tctx.volume_sumsq(np.array([np.nan], F)))


# ------------------------------------------------------------------------------- the descent
def device_descend(ctx, vol, steps, length, eps, lo, hi):
    import torch
    d_v = torch.from_numpy(np.concatenate([vol.reshape(-1), np.full(8, -7.0, F)])).to("cuda")
    ctx.tv_descend_device(d_v.data_ptr(), vol.shape[::-1], steps, length, eps, lo, hi)
    torch.cuda.synchronize()
    got = d_v.cpu().numpy()
    assert (got[vol.size:] == -7.0).all()
    return got[:vol.size].reshape(vol.shape)


@pytest.mark.parametrize("dims", tv_kit.DESCEND_GRIDS)
def test_descend_equals_the_reference(tctx, dims):
    vol = tv_kit.descend_volume(dims)
    args = (tv_kit.DESCEND_STEPS, tv_kit.DESCEND_LENGTH, 1e-8, tv_kit.DESCEND_LO, tv_kit.DESCEND_HI)
    want = tv_ref.descend(vol, *args)
    assert (want == tv_kit.DESCEND_LO).any() and ((want == tv_kit.DESCEND_HI).any() or dims[0] < 16)
    assert ((want > tv_kit.DESCEND_LO) & (want < tv_kit.DESCEND_HI)).any()
    same(tctx.tv_descend(vol, *args), want, (dims, "host form"))
    same(device_descend(tctx, vol, *args), want, (dims, "device form"))


def test_descend_leaves_a_constant_volume_and_a_zero_length(tctx):
    flat = np.full((3, 9, 67), 0.75, F)
    for form in (tctx.tv_descend, lambda *a: device_descend(tctx, *a)):
        assert np.array_equal(bits(form(flat, 3, 0.7, 1e-8, -np.inf, np.inf)), bits(flat))           # G = 0
        vol = tv_kit.volume(4, (67, 9, 3), specials=False)
        assert np.array_equal(bits(form(vol, 3, 0.0, 1e-8, -np.inf, np.inf)), bits(vol))              # c = 0


# ------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize("subsets", [1, 3])
def test_sirt_tv_small_scan_equals_the_reference(tctx, subsets):
    proj, A, spacing = sirt_kit.small_scan()
    got = tctx.sirt_matrices(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, subsets, relax=0.9, lo=0.0, tv=tv_kit.SMALL_TV)
    same(got, tv_kit.small_reference(subsets), subsets)
    assert not np.array_equal(got, sirt_kit.small_reference(subsets))


def test_sirt_tv_without_steps_is_sirt(tctx):
    proj, A, spacing = sirt_kit.small_scan()
    plain = tctx.sirt_matrices(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, 3, relax=0.9, lo=0.0)
    same(plain, sirt_kit.small_reference(3), "plain")
    none = tctx.sirt_matrices(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, 3, relax=0.9, lo=0.0, tv=(0, np.nan, 7.0, -1.0))
    assert np.array_equal(bits(none), bits(plain))


def test_sirt_tv_device_form(tctx):
    """Device projections and volume, a start that is not zero, twice back to back on one context: the second call
    takes over the working set, with and without x0."""
    import torch
    proj, A, spacing = sirt_kit.small_scan()
    start = sirt_kit.volume(1, sirt_kit.SMALL_DIMS)
    P, H, W = proj.shape
    d_p = torch.from_numpy(proj.copy()).to("cuda")
    vols = [torch.from_numpy(start.copy()).to("cuda") for _ in range(3)]
    tv = (3, 0.25, 0.5, 1e-4)
    tctx.sirt_device(W, H, P, d_p.data_ptr(), A, sirt_kit.SMALL_DIMS, spacing, 2, vols[0].data_ptr(), subsets=3, relax=0.9, tv=tv)
    tctx.sirt_device(W, H, P, d_p.data_ptr(), A, sirt_kit.SMALL_DIMS, spacing, 2, vols[1].data_ptr(), subsets=1, lo=-np.inf, tv=tv)
    tctx.sirt_device(W, H, P, d_p.data_ptr(), A, sirt_kit.SMALL_DIMS, spacing, 2, vols[2].data_ptr(), subsets=3, relax=0.9)
    torch.cuda.synchronize()
    same(vols[0].cpu().numpy(), tv_ref.sirt_tv(proj, A, sirt_kit.SMALL_DIMS, spacing, 2, 3, 0.9, 0.0, start=start, tv=tv), "three subsets")
    same(vols[1].cpu().numpy(), tv_ref.sirt_tv(proj, A, sirt_kit.SMALL_DIMS, spacing, 2, 1, 1.0, -np.inf, start=start, tv=tv), "one subset")
    same(vols[2].cpu().numpy(), tv_ref.sirt_tv(proj, A, sirt_kit.SMALL_DIMS, spacing, 2, 3, 0.9, 0.0, start=start), "plain behind TV")


def test_noisy_ball_scan_through_the_context(tctx):
    """tests/test_tv_cpu.py's noisy 12-view ball scan through Context.sirt (cameras, no poses) with tv: bit-equal to
    the reference, its figures within the CPU test's bounds against plain SIRT through the same entry."""
    import test_tv_cpu
    proj, _ = tv_kit.noisy_scan()
    cams = [camera_kit.as_camera(c, sirt_kit.BALL_W, sirt_kit.BALL_H) for c in sirt_kit.ball_scan(sirt_kit.FEW_P)[1]]
    args = (proj, cams, None, sirt_kit.BALL_DIMS, sirt_kit.BALL_ORIGIN, sirt_kit.BALL_SPACING, sirt_kit.FEW_K)
    plain, smooth = tctx.sirt(*args), tctx.sirt(*args, tv=tv_kit.BALL_TV)
    same(plain, tv_kit.noisy_reference(False), "plain")
    same(smooth, tv_kit.noisy_reference(True), "tv")
    test_tv_cpu.check_denoised(plain, smooth)


# ------------------------------------------------------------------------------- the CLI
def test_cli_reconstructs_a_box_by_sirt_with_tv(tmp_path):
    """tests/test_gpu_sirt.py's box with --tv 5: the .mhd loads and the interior still holds the attenuation model's
    coefficient within that test's 5 %: the wiring, and a level that the default alpha does not flatten."""
    lo, hi = np.array([-5.3, -6.1, -9.2]), np.array([5.0, 4.4, 10.7])
    _write_obj(tmp_path / "box.obj", box(lo, hi))
    (tmp_path / "out").mkdir()
    r = subprocess.run([EXE, "-s", "64", "64", "-i", str(tmp_path / "box.obj"), "-f", "p.txt", "--turntable", "16:z",
                        "--log-projection", "80", "--reconstruct", str(tmp_path / "box.mhd") + ":32", "--sirt", "12:4",
                        "--tv", "5"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    vol, spacing, origin = xrt.load_volume(str(tmp_path / "box.mhd"))
    assert vol.dtype == F and vol.shape == (32, 32, 32) and vol.min() >= 0.0
    kk, jj, ii = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    X = origin.astype(D) + (np.stack([ii, jj, kk], -1) + 0.5) * spacing.astype(D)
    inner = np.all((X > lo + 3.0) & (X < hi - 3.0), axis=-1)
    mu = 0.3971 * 0.1
    mean = float(vol[inner].mean())
    print(f"box by SIRT with TV: interior mean {mean:.5f} (mu {mu:.5f}), {inner.sum()} voxels")
    assert inner.sum() > 200 and abs(mean / mu - 1.0) <= 0.05, mean
