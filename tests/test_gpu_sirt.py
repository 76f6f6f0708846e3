"""SIRT / OS-SART on the GPU: k_forward_project and k_volume_update against
tests/sirt_ref.py bit for bit through both entry forms, Context.sirt on the small scan and
on the ball scan, and xrt_main --reconstruct --sirt end to end."""
import os
import subprocess

import numpy as np
import pytest

import camera_kit
import fdk_kit
import sirt_kit
import sirt_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import ROOT, bits
from scene_kit import box
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


@pytest.fixture(scope="module")
def sctx():
    """A context of this module's own."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def same(got, want, what):
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    if not fdk_kit.same_bits(got, want):
        bad = np.argwhere((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError((what, len(bad), bad[:6].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def device_forward(ctx, vol, spacing, R, shape, mode=xrt.XRT_FP_PROJECT, meas=None):
    """Context.forward_project_device over buffers of exactly the arguments' sizes: (P, H, W) f32."""
    import torch
    H, W = shape
    R = np.ascontiguousarray(R, D).reshape(-1, 12)
    P = R.shape[0]
    d_v, d_r = torch.from_numpy(np.array(vol, F)).to("cuda"), torch.from_numpy(R.reshape(-1).copy()).to("cuda")
    d_m = torch.from_numpy(np.array(meas, F)).to("cuda") if meas is not None else None
    out = torch.full((P, H, W), -7.0, dtype=torch.float32, device="cuda")
    ctx.forward_project_device(W, H, P, d_v.data_ptr(), vol.shape[::-1], spacing, d_r.data_ptr(), out.data_ptr(), mode,
                               d_m.data_ptr() if d_m is not None else 0)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def both_forms(ctx, vol, spacing, R, shape, want_project, meas, want_residual, what):
    """The host form and the _device form, both modes, against the reference's planes."""
    same(ctx.forward_project(vol, spacing, R, shape), want_project, (what, "project"))
    same(device_forward(ctx, vol, spacing, R, shape), want_project, (what, "project, device form"))
    same(ctx.forward_project(vol, spacing, R, mode=xrt.XRT_FP_RESIDUAL, meas=meas), want_residual, (what, "residual"))
    same(device_forward(ctx, vol, spacing, R, shape, xrt.XRT_FP_RESIDUAL, meas), want_residual, (what, "residual, device form"))


# ------------------------------------------------------------------------------- the forward projector
@pytest.mark.parametrize("dims", sirt_kit.FP_DIMS)
def test_forward_projector_equals_the_reference(sctx, dims):
    """Every grid on every detector (1 x 1 to more than one tile a side, ragged edges), stacks of 1, 3 and 17
    planes in turn, both modes, NaN, +-inf and -0.0 voxels on the last detector."""
    for n, (W, H) in enumerate(sirt_kit.FP_PLANES):
        P = sirt_kit.FP_STACKS[n % len(sirt_kit.FP_STACKS)] if (W, H) != (67, 45) else 3
        R, spacing = sirt_kit.general_rays(P, dims, W, H, seed=P)
        vol = sirt_kit.volume(W + H, dims, specials=(W, H) == (67, 45))
        meas = sirt_kit.measured(W, P, H, W)
        both_forms(sctx, vol, spacing, R, (H, W), sirt_ref.forward_project(vol, spacing, R, (H, W)), meas,
                   sirt_ref.forward_project(vol, spacing, R, mode=sirt_ref.RESIDUAL, meas=meas), (dims, W, H, P))


@pytest.mark.parametrize("P", sirt_kit.FP_STACKS)
def test_forward_projector_stacks(sctx, P):
    dims, (W, H) = (67, 9, 3), (7, 13)
    R, spacing = sirt_kit.general_rays(P, dims, W, H, seed=1)
    vol, meas = sirt_kit.volume(3, dims), sirt_kit.measured(P, P, H, W)
    both_forms(sctx, vol, spacing, R, (H, W), sirt_ref.forward_project(vol, spacing, R, (H, W)), meas,
               sirt_ref.forward_project(vol, spacing, R, mode=sirt_ref.RESIDUAL, meas=meas), P)


@pytest.mark.parametrize("name", list(sirt_kit.hand_rays()))
def test_forward_projector_hand_built_rays(sctx, name):
    """Rays inside voxel faces, through edges and corners, a source on the boundary and inside the grid, misses,
    L = 0 and a ray that does not move: both modes, plain and special voxels."""
    R, (H, W) = sirt_kit.hand_rays()[name]
    for specials in (False, True):
        vol = sirt_kit.volume(9, sirt_kit.HAND_DIMS, specials)
        meas = sirt_kit.measured(4, 1, H, W)
        both_forms(sctx, vol, sirt_kit.HAND_SPACING, R, (H, W), sirt_ref.forward_project(vol, sirt_kit.HAND_SPACING, R, (H, W)),
                   meas, sirt_ref.forward_project(vol, sirt_kit.HAND_SPACING, R, mode=sirt_ref.RESIDUAL, meas=meas),
                   (name, specials))


def test_forward_projector_device_form(sctx):
    """Device pointers, both modes back to back on one stream, guard words behind the planes."""
    import torch
    dims, (W, H), P = (67, 9, 3), (67, 45), 3
    R, spacing = sirt_kit.general_rays(P, dims, W, H)
    vol, meas = sirt_kit.volume(5, dims), sirt_kit.measured(6, P, H, W)
    d_v, d_r, d_m = (torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (vol, R.reshape(-1), meas))
    n = P * H * W
    outs = [torch.full((n + 16,), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    with pytest.raises(xrt.XrtError) as e:
        sctx.forward_project_device(W, H, P, d_v.data_ptr(), dims, spacing, d_r.data_ptr(), d_m.data_ptr() + 64,
                                    xrt.XRT_FP_RESIDUAL, d_m.data_ptr())
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)
    sctx.forward_project_device(W, H, P, d_v.data_ptr(), dims, spacing, d_r.data_ptr(), outs[0].data_ptr())
    sctx.forward_project_device(W, H, P, d_v.data_ptr(), dims, spacing, d_r.data_ptr(), outs[1].data_ptr(),
                                xrt.XRT_FP_RESIDUAL, d_m.data_ptr())
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    same(got[0][:n].reshape(P, H, W), sirt_ref.forward_project(vol, spacing, R, (H, W)), "project")
    same(got[1][:n].reshape(P, H, W), sirt_ref.forward_project(vol, spacing, R, mode=sirt_ref.RESIDUAL, meas=meas), "residual")
    assert (got[0][n:] == -7.0).all() and (got[1][n:] == -7.0).all()


# ------------------------------------------------------------------------------- the update
@pytest.mark.parametrize("n", sirt_kit.UPDATE_LENGTHS + [sirt_kit.UPDATE_LONG])
def test_volume_update_equals_the_reference(sctx, n):
    """The lengths about a wave and a workgroup, and one past the 2^22 voxels that a launch's workgroups cover in
    one pass (kUpdateBlocks * kUpdateThreads in csrc/kernels/xrt_kernels.h): the lanes' second pass."""
    import torch
    x, corr, norm, lo, hi = sirt_kit.update_vectors(n)
    for relax, a, b in ((1.0, lo, hi), (0.7, -np.inf, np.inf), (1.0, lo, np.inf)):
        want = sirt_ref.volume_update(x, corr, norm, relax, a, b)
        same(sctx.volume_update(x, corr, norm, relax, a, b), want, (n, relax, "host form"))
        d_x = torch.from_numpy(np.concatenate([x, np.full(8, -7.0, F)])).to("cuda")
        d_c, d_n = torch.from_numpy(corr).to("cuda"), torch.from_numpy(norm).to("cuda")
        sctx.volume_update_device(n, d_x.data_ptr(), d_c.data_ptr(), d_n.data_ptr(), relax, a, b)
        torch.cuda.synchronize()
        got = d_x.cpu().numpy()
        same(got[:n], want, (n, relax, "device form"))
        assert (got[n:] == -7.0).all()


# ------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize("subsets", [1, 3])
def test_sirt_small_scan_equals_the_reference(sctx, subsets):
    proj, A, spacing = sirt_kit.small_scan()
    got = sctx.sirt_matrices(proj, A, sirt_kit.SMALL_DIMS, spacing, 3, subsets, relax=0.9, lo=0.0)
    same(got, sirt_kit.small_reference(subsets), subsets)


def test_sirt_device_form(sctx):
    """Device projections and volume, a start that is not zero, twice back to back (the second call takes over the
    context's working set)."""
    import torch
    proj, A, spacing = sirt_kit.small_scan()
    start = sirt_kit.volume(1, sirt_kit.SMALL_DIMS)
    P, H, W = proj.shape
    d_p = torch.from_numpy(proj.copy()).to("cuda")
    vols = [torch.from_numpy(start.copy()).to("cuda") for _ in range(2)]
    sctx.sirt_device(W, H, P, d_p.data_ptr(), A, sirt_kit.SMALL_DIMS, spacing, 2, vols[0].data_ptr(), subsets=3, relax=0.9)
    sctx.sirt_device(W, H, P, d_p.data_ptr(), A, sirt_kit.SMALL_DIMS, spacing, 1, vols[1].data_ptr(), subsets=1, lo=-np.inf)
    torch.cuda.synchronize()
    same(vols[0].cpu().numpy(), sirt_ref.sirt(proj, A, sirt_kit.SMALL_DIMS, spacing, 2, 3, 0.9, 0.0, start=start), "three subsets")
    same(vols[1].cpu().numpy(), sirt_ref.sirt(proj, A, sirt_kit.SMALL_DIMS, spacing, 1, 1, 1.0, -np.inf, start=start), "one subset")


def test_ball_scan_through_the_context(sctx):
    """tests/test_sirt_cpu.py's ball scan through Context.sirt (cameras, no poses): bit-equal to the reference, its
    figures within the CPU test's bounds."""
    import test_sirt_cpu
    proj, cams, A = sirt_kit.ball_scan(sirt_kit.BALL_P)
    cs = [camera_kit.as_camera(c, sirt_kit.BALL_W, sirt_kit.BALL_H) for c in cams]
    vol = sctx.sirt(proj, cs, None, sirt_kit.BALL_DIMS, sirt_kit.BALL_ORIGIN, sirt_kit.BALL_SPACING, sirt_kit.BALL_K)
    same(vol, sirt_kit.ball_reference(sirt_kit.BALL_P, sirt_kit.BALL_K)[0], "ball")
    test_sirt_cpu.check_ball(vol)


# ------------------------------------------------------------------------------- the CLI
def test_cli_reconstructs_a_box_by_sirt(tmp_path):
    """xrt_main --turntable 16:z --log-projection 80 --reconstruct box.mhd:32 --sirt 12:4: the .mhd loads (what
    loadMetaImage reads back), and the interior of tests/test_gpu_fdk.py's box holds the attenuation model's
    coefficient per scene length unit within 5 %, as that test bounds its FDK: the wiring, not the accuracy."""
    lo, hi = np.array([-5.3, -6.1, -9.2]), np.array([5.0, 4.4, 10.7])
    _write_obj(tmp_path / "box.obj", box(lo, hi))
    (tmp_path / "out").mkdir()
    r = subprocess.run([EXE, "-s", "64", "64", "-i", str(tmp_path / "box.obj"), "-f", "p.txt", "--turntable", "16:z",
                        "--log-projection", "80", "--reconstruct", str(tmp_path / "box.mhd") + ":32", "--sirt", "12:4"],
                       capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    vol, spacing, origin = xrt.load_volume(str(tmp_path / "box.mhd"))
    assert vol.dtype == F and vol.shape == (32, 32, 32) and vol.min() >= 0.0
    kk, jj, ii = np.meshgrid(*[np.arange(32)] * 3, indexing="ij")
    X = origin.astype(D) + (np.stack([ii, jj, kk], -1) + 0.5) * spacing.astype(D)
    inner = np.all((X > lo + 3.0) & (X < hi - 3.0), axis=-1)
    mu = 0.3971 * 0.1
    mean = float(vol[inner].mean())
    print(f"box by SIRT: interior mean {mean:.5f} (mu {mu:.5f}), {inner.sum()} voxels")
    assert inner.sum() > 200 and abs(mean / mu - 1.0) <= 0.05, mean
