"""OS-MLTR on the GPU: k_poisson_project and k_backproject_update against
tests/mltr_ref.py bit for bit through both entry forms, the fused backprojector against the
entries it replaces, Context.mltr on the small scans (subsets, background, TV, the shared
working set), the two ball scans that show what the solver is for, and xrt_main
--reconstruct --mltr end to end."""
import os
import subprocess

import numpy as np
import pytest

import mltr_kit
import sirt_kit
import tv_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import ROOT
from mltr_kit import same
from scene_kit import box
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


@pytest.fixture(scope="module")
def mctx():
    """A context of this module's own."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda")


def device_pairs(ctx, vol, spacing, R, y, f, b):
    """Context.poisson_project_device over buffers of the arguments' sizes and guard words: (P, H, W, 2) f32."""
    import torch
    P, H, W = y.shape
    d_v, d_r, d_y, d_f = _dev(vol), _dev(np.asarray(R, D).reshape(-1)), _dev(y), _dev(f)
    d_b = _dev(b) if b is not None else None
    n = 2 * P * H * W
    out = torch.full((n + 16,), -7.0, dtype=torch.float32, device="cuda")
    ctx.poisson_project_device(W, H, P, d_v.data_ptr(), vol.shape[::-1], spacing, d_r.data_ptr(), d_y.data_ptr(),
                               d_f.data_ptr(), out.data_ptr(), d_b.data_ptr() if d_b is not None else 0)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n:] == -7.0).all()
    return got[:n].reshape(P, H, W, 2)


# ------------------------------------------------------------------------------- the pixel stage
@pytest.mark.parametrize("name", list(mltr_kit.PIXEL_CASES))
def test_pixel_stage_equals_the_reference(mctx, name):
    vol, spacing, R, y, f, b, want = mltr_kit.pixel_case(name)
    y3 = y.reshape(-1, *y.shape[-2:])
    same(mctx.poisson_project(vol, spacing, R, y, f, b), want, (name, "host form"))
    same(device_pairs(mctx, vol, spacing, R, y3, f, b), want, (name, "device form"))


def test_null_background_equals_a_zero_background(mctx):
    for name in ("stack3", "hand-faces-plain", "grid(67, 9, 3)-plane(67, 45)"):
        vol, spacing, R, y, f, _, _ = mltr_kit.pixel_case(name)
        none = mctx.poisson_project(vol, spacing, R, y, f, None)
        same(mctx.poisson_project(vol, spacing, R, y, f, np.zeros_like(y)), none, name)
        same(device_pairs(mctx, vol, spacing, R, y, f, np.zeros_like(y)), none, (name, "device form"))


# ------------------------------------------------------------------------------- the fused backprojector
def device_update(ctx, pr, A, dims, start, relax, lo, hi):
    import torch
    P, H, W = pr.shape[:3]
    d_p, d_a = _dev(pr), _dev(np.asarray(A, D).reshape(-1))
    d_x = _dev(np.concatenate([start.reshape(-1), np.full(16, -7.0, F)]))
    ctx.backproject_update_device(W, H, P, d_p.data_ptr(), d_a.data_ptr(), dims, d_x.data_ptr(), relax, lo, hi)
    torch.cuda.synchronize()
    got = d_x.cpu().numpy()
    assert (got[start.size:] == -7.0).all()
    return got[:start.size].reshape(start.shape)


def composed_update(ctx, pr, A, dims, start, relax, lo, hi):
    """xrt_backproject of each component and xrt_volume_update, through the _device entries on one stream."""
    import torch
    P, H, W = pr.shape[:3]
    d_n, d_d = _dev(pr[..., 0]), _dev(pr[..., 1])
    d_a, d_x = _dev(np.asarray(A, D).reshape(-1)), _dev(start)
    corr, norm = (torch.empty(start.size, dtype=torch.float32, device="cuda") for _ in range(2))
    ctx.backproject_device(W, H, P, d_n.data_ptr(), d_a.data_ptr(), dims, 0, dims[2], 1.0, False, corr.data_ptr())
    ctx.backproject_device(W, H, P, d_d.data_ptr(), d_a.data_ptr(), dims, 0, dims[2], 1.0, False, norm.data_ptr())
    ctx.volume_update_device(start.size, d_x.data_ptr(), corr.data_ptr(), norm.data_ptr(), relax, lo, hi)
    torch.cuda.synchronize()
    return d_x.cpu().numpy()


@pytest.mark.parametrize("name", list(mltr_kit.UPDATE_CASES))
def test_backproject_update_equals_the_reference_and_its_composition(mctx, name):
    pr, A, dims, start, relax, lo, hi, want = mltr_kit.update_case(name)
    same(mctx.backproject_update(pr, A, dims, start, relax, lo, hi), want, (name, "host form"))
    same(device_update(mctx, pr, A, dims, start, relax, lo, hi), want, (name, "device form"))
    same(composed_update(mctx, pr, A, dims, start, relax, lo, hi), want, (name, "the entries it replaces"))


def test_unseen_voxels_keep_their_bits(mctx):
    pr, A, dims, start, relax, lo, hi, _ = mltr_kit.update_case("edge(7, 13)")
    got = mctx.backproject_update(pr[:2], A[:2], dims, start, relax, lo, hi)
    assert np.array_equal(got[1].view(np.uint32), start[1].view(np.uint32))
    assert np.isnan(start[1]).any() and (start[1].view(np.uint32) == 0x80000000).any()


# ------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize("subsets", [1, 3])
@pytest.mark.parametrize("with_bg", [False, True])
def test_mltr_small_scan_equals_the_reference(mctx, subsets, with_bg):
    y, flat, bg, A, spacing = mltr_kit.small_scan(with_bg)
    got = mctx.mltr_matrices(y, flat, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, subsets, mltr_kit.SMALL_RELAX, 0.0,
                             background=bg)
    same(got, mltr_kit.small_reference(subsets, with_bg), (subsets, with_bg))


def test_mltr_with_tv(mctx):
    y, flat, bg, A, spacing = mltr_kit.small_scan(True)
    args = (y, flat, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, 3, mltr_kit.SMALL_RELAX, 0.0)
    same(mctx.mltr_matrices(*args, tv=mltr_kit.SMALL_TV, background=bg), mltr_kit.small_reference(3, True, mltr_kit.SMALL_TV), "tv")
    same(mctx.mltr_matrices(*args, tv=(0, 0.2, 0.9, 1e-8), background=bg), mltr_kit.small_reference(3, True), "tv without steps")


def device_mltr(ctx, y, flat, bg, A, dims, spacing, K, S, relax, tv=None):
    import torch
    P, H, W = y.shape
    d_y, d_f = _dev(y), _dev(flat)
    d_b = _dev(bg) if bg is not None else None
    d_x = torch.zeros(int(np.prod(dims)), dtype=torch.float32, device="cuda")
    ctx.mltr_device(W, H, P, d_y.data_ptr(), d_f.data_ptr(), A, dims, spacing, K, d_x.data_ptr(), subsets=S, relax=relax,
                    tv=tv, d_background=d_b.data_ptr() if d_b is not None else 0)
    torch.cuda.synchronize()
    return d_x.cpu().numpy().reshape(dims[::-1])


def test_mltr_device_form(mctx):
    """Device buffers; three subsets read the counts and the background at the subsets' stride."""
    for with_bg, tv in ((True, None), (False, None), (True, mltr_kit.SMALL_TV)):
        y, flat, bg, A, spacing = mltr_kit.small_scan(with_bg)
        got = device_mltr(mctx, y, flat, bg, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, 3, mltr_kit.SMALL_RELAX, tv)
        same(got, mltr_kit.small_reference(3, with_bg, tv), (with_bg, tv))


def test_the_working_set_grows_and_is_reused():
    """A larger call, then a smaller one, on a context that has solved the small scan: each equals a fresh context's
    result (the reference's)."""
    y, flat, bg, A, spacing = mltr_kit.small_scan(True)
    Y, FL, BG, AA, SP, dims = mltr_kit.large_scan()
    with xrt.Context(int(os.environ.get("XRT_DEVICE", "0"))) as c:
        small = lambda: c.mltr_matrices(y, flat, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, 3, mltr_kit.SMALL_RELAX,
                                        0.0, background=bg)
        same(small(), mltr_kit.small_reference(3, True), "first")
        same(c.mltr_matrices(Y, FL, AA, dims, SP, 2, 2, 1.0, 0.0, background=BG), mltr_kit.large_reference(), "larger")
        same(small(), mltr_kit.small_reference(3, True), "smaller again")


def test_the_working_set_is_shared_with_sirt():
    """xrt_mltr after xrt_sirt_tv on one context, and the reverse: each equals a fresh context's result."""
    y, flat, bg, A, spacing = mltr_kit.small_scan(True)
    proj = sirt_kit.small_scan()[0]
    sirt_want = tv_ref.sirt_tv(proj, A, sirt_kit.SMALL_DIMS, spacing, 2, 3, 0.9, 0.0, tv=mltr_kit.SMALL_TV)
    with xrt.Context(int(os.environ.get("XRT_DEVICE", "0"))) as c:
        sirt = lambda: c.sirt_matrices(proj, A, sirt_kit.SMALL_DIMS, spacing, 2, 3, relax=0.9, lo=0.0, tv=mltr_kit.SMALL_TV)
        mltr = lambda: c.mltr_matrices(y, flat, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, 3, mltr_kit.SMALL_RELAX,
                                       0.0, background=bg, tv=mltr_kit.SMALL_TV)
        same(sirt(), sirt_want, "SIRT first")
        same(mltr(), mltr_kit.small_reference(3, True, mltr_kit.SMALL_TV), "MLTR after SIRT")
        same(sirt(), sirt_want, "SIRT after MLTR")


def test_refusals_come_before_the_context(mctx):
    """The checks themselves are tests/test_mltr_cpu.py's, on a NULL context; here a live context refuses the same
    and stays usable."""
    y, flat, bg, A, spacing = mltr_kit.small_scan(True)
    with pytest.raises(xrt.XrtError) as e:
        mctx.mltr_matrices(y, flat, A, sirt_kit.SMALL_DIMS, spacing, 0, 1)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "iterations" in str(e.value)
    with pytest.raises(xrt.XrtError) as e:
        mctx.mltr_matrices(y, flat, A, sirt_kit.SMALL_DIMS, spacing, 1, 9)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "subsets" in str(e.value)
    with pytest.raises(xrt.XrtError) as e:
        mctx.backproject_update(np.zeros((1, 3, 4, 2), F), A[:1], (5, 4, 3), np.zeros((3, 4, 5), F), relax=np.nan)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "relax" in str(e.value)
    same(mctx.mltr_matrices(y, flat, A, sirt_kit.SMALL_DIMS, spacing, mltr_kit.SMALL_K, 1, mltr_kit.SMALL_RELAX, 0.0,
                            background=bg), mltr_kit.small_reference(1, True), "after the refusals")


# ------------------------------------------------------------------------------- what it is for
def test_starved_counts(mctx):
    """A flat field of 100 counts on sirt_kit's ball, 4 iterations of 8 subsets from zeros: bit-equal to the
    reference, the inner mean within 0.1 of 1; SIRT on xrt_log_projection of the same counts (t_min = 0.5 / flat)
    at the same iterations and subsets stays below 0.75."""
    y, A = mltr_kit.starved_scan()
    got = mctx.mltr_matrices(y, mltr_kit.STARVED_FLAT, A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING, mltr_kit.STARVED_K,
                             mltr_kit.BALL_S, 1.0, 0.0)
    same(got, mltr_kit.starved_reference(), "starved")
    mean = sirt_kit.ball_figures(got)[0]
    line = mctx.log_projection(y, flat_value=mltr_kit.STARVED_FLAT, t_min=0.5 / mltr_kit.STARVED_FLAT)
    same(line, mltr_kit.starved_line_integrals(), "the logarithm")
    below = sirt_kit.ball_figures(mctx.sirt_matrices(line, A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING, mltr_kit.STARVED_K,
                                                     mltr_kit.BALL_S, 1.0, 0.0))[0]
    print(f"starved counts: inner mean MLTR {mean:.4f}, SIRT on the logarithm {below:.4f}")
    assert abs(mean - 1.0) <= 0.1, mean
    assert below < 0.75, below


def test_known_background(mctx):
    """A flat field of 1000 counts over a background of 20, 3 iterations of 8 subsets: modelled, the inner mean lies
    in [0.9, 1.2]; with background=None it stays below 0.7.  Both bit-equal to the reference."""
    y, A = mltr_kit.background_scan()
    figures = []
    for modelled in (True, False):
        got = mctx.mltr_matrices(y, mltr_kit.BG_FLAT, A, sirt_kit.BALL_DIMS, sirt_kit.BALL_SPACING, mltr_kit.BG_K,
                                 mltr_kit.BALL_S, 1.0, 0.0, background=mltr_kit.BG_LEVEL if modelled else None)
        same(got, mltr_kit.background_reference(modelled), modelled)
        figures.append(sirt_kit.ball_figures(got)[0])
    print(f"known background: inner mean modelled {figures[0]:.4f}, ignored {figures[1]:.4f}")
    assert 0.9 <= figures[0] <= 1.2, figures
    assert figures[1] < 0.7, figures


# ------------------------------------------------------------------------------- the CLI
def test_cli_reconstructs_a_box_by_mltr(tmp_path):
    """xrt_main --turntable 16:z --noise 1:7 --log-projection 80 --reconstruct box.mhd:16 --mltr 3:4: the volume
    file equals Context.mltr on the planes the solver received -- the intensities just before the logarithm, which
    the run keeps in box.counts.mhd beside the volume -- under the run's camera, poses and grid.  --mltr with --sirt
    is refused."""
    lo, hi = np.array([-5.3, -6.1, -9.2]), np.array([5.0, 4.4, 10.7])
    _write_obj(tmp_path / "box.obj", box(lo, hi))
    (tmp_path / "out").mkdir()
    base = [EXE, "-s", "64", "64", "-i", str(tmp_path / "box.obj"), "-f", "p.txt", "--turntable", "16:z", "--noise", "1:7",
            "--log-projection", "80", "--reconstruct", str(tmp_path / "box.mhd") + ":16"]
    r = subprocess.run(base + ["--mltr", "3:4", "--sirt", "3:4"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode != 0 and "--mltr" in r.stderr and "--sirt" in r.stderr, r.stderr
    r = subprocess.run(base + ["--mltr", "3:4"], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert r.returncode == 0, r.stderr
    vol, spacing, origin = xrt.load_volume(str(tmp_path / "box.mhd"))
    assert vol.dtype == F and vol.shape == (16, 16, 16) and vol.min() >= 0.0
    counts, _, _ = xrt.load_volume(str(tmp_path / "box.counts.mhd"))
    assert counts.shape == (16, 64, 64)
    tris = xrt.load_meshes(str(tmp_path / "box.obj"))
    cam = xrt.camera_for_scene(tris, 64, 64)
    lower, upper = (np.asarray(v, F) for v in xrt.scene_bbox(tris))
    centre = lower + ((upper - lower).astype(D) / 2.0).astype(F)          # the turntable's centre, as xrt_main forms it
    poses = [xrt.pose_rotation((0.0, 0.0, 1.0), p * 360.0 / 16, centre) for p in range(16)]
    with xrt.Context(int(os.environ.get("XRT_DEVICE", "0"))) as c:
        want = c.mltr(counts, 80.0, cam, poses, (16, 16, 16), origin, spacing, 3, 4)
    same(vol, want, "the CLI's volume")
    assert float(vol.max()) > 0.0
