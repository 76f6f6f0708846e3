"""The detector response (xrt_detector_response, k_lsf) on the GPU: every plane is compared
bit for bit with tests/lsf_ref.py, the f32 image and the 8-bit one.  Inputs and taps are
finite, so no pixel is left out of a comparison (the rendered phantom may hold NaNs: those
are compared by class and counted)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import lsf_ref
import materials_kit as kit
import simpleraytracing_amd as xrt
import spectrum_kit as skit
from simpleraytracing_amd import _abi
from oracle import oracle
from conftest import ROOT, bits
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
TILE = 64                                               # kLsfTile (csrc/kernels/xrt_kernels.h): a workgroup's tile
PLANES = [(1, 1), (7, 13), (13, 7), (63, 5), (64, 64), (65, 33), (257, 131), (33, TILE - 1), (33, TILE + 1)]
TAPS = [(1, 1), (3, 1), (1, 3), (5, 9), (41, 41), (129, 129)]


@pytest.fixture(scope="module")
def lctx():
    """A context of this module's own: the models and scenes set here never reach other tests."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def tap_pair(nx, ny):
    return lsf_ref.taps(nx, nx), lsf_ref.taps(ny + 1, ny)


@functools.lru_cache(maxsize=None)
def case(W, H, nx, ny, P=None):
    """(input, hx, hy, reference out, reference u8), computed once."""
    a = lsf_ref.plane(1000 * W + H, W, H, P)
    assert np.isfinite(a).all()
    hx, hy = tap_pair(nx, ny)
    return (a, hx, hy) + lsf_ref.apply(a, hx, hy)


def check(got, want, what):
    (g, gu), (w, wu) = got, want
    ok, nans = lsf_ref.same(g, w)
    assert nans == 0, what
    assert ok, (what, np.argwhere(bits(g) != bits(w))[:8])
    assert gu.dtype == np.uint8 and np.array_equal(gu, wu), (what, np.argwhere(gu != wu)[:8])


@pytest.mark.parametrize("W,H", PLANES)
def test_planes_and_taps(lctx, W, H):
    for nx, ny in TAPS:
        a, hx, hy, w, wu = case(W, H, nx, ny)
        check(lctx.detector_response(a, hx, hy), (w, wu), (W, H, nx, ny))


def test_identity_and_orientation(lctx):
    a = lsf_ref.plane(3, 70, 19)
    got, _ = lctx.detector_response(a, [1.0])
    assert np.array_equal(bits(got), bits(a))           # -0.0 and denormals included
    got, _ = lctx.detector_response(a, [1.0, 0.0, 0.0], [1.0])
    assert np.array_equal(got, np.concatenate([a[:, :1], a[:, :-1]], axis=1))   # hx[0] meets the LEFT pixel
    got, _ = lctx.detector_response(a, [1.0], [0.0, 0.0, 1.0])
    assert np.array_equal(got, np.concatenate([a[1:], a[-1:]], axis=0))


def test_three_planes_in_one_launch(lctx):
    a, hx, hy, w, wu = case(65, 33, 41, 41, 3)
    got, gu = lctx.detector_response(a, hx, hy)
    check((got, gu), (w, wu), "stack")
    for p in range(3):                                  # a plane's edge does not read its neighbour
        check(lctx.detector_response(a[p], hx, hy), (got[p], gu[p]), p)
        check((got[p], gu[p]), lsf_ref.apply(a[p], hx, hy), p)


def test_either_output_alone(lctx):
    a, hx, hy, w, wu = case(65, 33, 5, 9)
    got, gu = lctx.detector_response(a, hx, hy, u8=False)
    assert gu is None and np.array_equal(bits(got), bits(w))
    got, gu = lctx.detector_response(a, hx, hy, out=False)
    assert got is None and np.array_equal(gu, wu)
    with pytest.raises(xrt.XrtError) as e:
        lctx.detector_response(a, hx, hy, out=False, u8=False)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT


def test_device_entry(lctx):
    """Device buffers: an overlap is refused; two launches with different taps back to back on
    one stream, no host wait between them, each give their own reference (the taps travel by
    value with the launch)."""
    import torch
    W, H = 257, 131
    a, hx1, hy1, w1, wu1 = case(W, H, 41, 41)
    _, hx2, hy2, w2, wu2 = case(W, H, 5, 9)
    assert not np.array_equal(bits(w1), bits(w2))
    d_in = torch.from_numpy(a).to("cuda")
    outs = [torch.zeros(H * W, dtype=torch.float32, device="cuda") for _ in range(2)]
    u8s = [torch.zeros(H * W, dtype=torch.uint8, device="cuda") for _ in range(2)]
    for d_out, d_u8 in ((d_in.data_ptr(), 0), (d_in.data_ptr() + 4 * (H * W - 1), 0), (0, d_in.data_ptr() + 4 * H * W - 1)):
        with pytest.raises(xrt.XrtError) as e:
            lctx.detector_response_device(W, H, 1, d_in.data_ptr(), hx1, hy1, d_out, d_u8)
        assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)
    lctx.detector_response_device(W, H, 1, d_in.data_ptr(), hx1, hy1, outs[0].data_ptr(), u8s[0].data_ptr())
    lctx.detector_response_device(W, H, 1, d_in.data_ptr(), hx2, hy2, outs[1].data_ptr(), u8s[1].data_ptr())
    torch.cuda.synchronize()
    check((outs[0].cpu().numpy().reshape(H, W), u8s[0].cpu().numpy().reshape(H, W)), (w1, wu1), "first taps")
    check((outs[1].cpu().numpy().reshape(H, W), u8s[1].cpu().numpy().reshape(H, W)), (w2, wu2), "second taps")
    assert np.array_equal(bits(d_in.cpu().numpy()), bits(a))            # the input is only read


def test_phantom_end_to_end_and_device_chain(lctx):
    """render_spectrum -> image -> detector_response equals the reference of the rendered image;
    the device chain paths render -> apply_spectrum_device -> hole_fill_device ->
    detector_response_device on one stream equals it too."""
    import torch
    W, H = 96, 80
    n = W * H
    meshes = kit.phantom()
    w, mu = skit.phantom_table(4)
    hx, hy = xrt.lsf_gaussian(1.5, 13), tap_pair(5, 7)[1]
    cam = xrt.camera_for_scene(meshes, W, H)
    try:
        lctx.set_kernel(xrt.XRT_KERNEL_BINNED)
        lctx.upload_scene(meshes)
        lctx.set_spectrum(w, mu)
        img, lb, u8, _ = lctx.render_spectrum(cam)
        assert np.count_nonzero(lb == F(-1.0)) > 0      # the hole fill had work
        got = lctx.detector_response(img.reshape(H, W), hx, hy)
        want = lsf_ref.apply(img.reshape(H, W), hx, hy)
        ok, nans = lsf_ref.same(got[0], want[0])
        fin = ~np.isnan(want[0])
        assert ok and np.array_equal(got[1][fin], want[1][fin]), f"{nans} NaN pixels compared by class"
        print("NaN pixels in the blurred phantom:", nans, "of", n)
        assert not np.array_equal(bits(got[0]), bits(img.reshape(H, W)))

        lctx.set_paths()
        d_paths = torch.zeros(5 * n, dtype=torch.float32, device="cuda")
        d_open = torch.zeros(n, dtype=torch.int16, device="cuda")
        d_lb = torch.zeros(n, dtype=torch.float32, device="cuda")
        d_img = torch.zeros(n, dtype=torch.float32, device="cuda")
        d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
        d_u8 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        lctx.render_paths_device(cam, 0, H, 5, d_paths.data_ptr(), d_open.data_ptr())
        lctx.apply_spectrum_device(n, d_paths.data_ptr(), d_open.data_ptr(), w, mu, d_lb.data_ptr())
        lctx.hole_fill_device(W, H, d_lb.data_ptr(), d_img.data_ptr(), 0)
        lctx.detector_response_device(W, H, 1, d_img.data_ptr(), hx, hy, d_out.data_ptr(), d_u8.data_ptr())
        torch.cuda.synchronize()
        lctx.read_stats()
        assert np.array_equal(bits(d_lb.cpu().numpy()), bits(lb))       # the unblurred planes stay as rendered
        chain = d_out.cpu().numpy().reshape(H, W)
        ok, _ = lsf_ref.same(chain, got[0])
        assert ok and np.array_equal(d_u8.cpu().numpy().reshape(H, W)[fin], got[1][fin])
    finally:
        lctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
        lctx.set_kernel(xrt.XRT_KERNEL_AUTO)


def test_context_state_is_untouched(lctx, dragon):
    """The model, the scene and the frame pipeline: a render after the call is served as before."""
    import torch
    W = H = 64
    cam = xrt.camera_for_mesh(dragon, W, H)
    lctx.upload_mesh(dragon)
    lctx.set_kernel(xrt.XRT_KERNEL_BINNED)
    try:
        n = W * H
        planes = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(2)]
        d_u8 = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(n, dtype=torch.float32, device="cuda")
        for _ in range(4):                              # repeated frames are served from preparations made ahead
            lctx.render_rows_device(cam, 0, H, planes[0].data_ptr(), planes[1].data_ptr(), d_u8.data_ptr())
        torch.cuda.synchronize()
        before = lctx.pipeline_counters()
        assert before["ahead_used"] >= 1, before
        first = planes[0].cpu().numpy().copy()
        hx, hy = tap_pair(9, 5)
        lctx.detector_response_device(W, H, 1, planes[0].data_ptr(), hx, hy, d_out.data_ptr(), 0)
        lctx.detector_response(first.reshape(H, W), hx, hy)
        torch.cuda.synchronize()
        assert lctx.pipeline_counters() == before
        lctx.render_rows_device(cam, 0, H, planes[0].data_ptr(), planes[1].data_ptr(), d_u8.data_ptr())
        torch.cuda.synchronize()
        after = lctx.pipeline_counters()
        assert after["ahead_used"] == before["ahead_used"] + 1 and after["ahead_dropped"] == before["ahead_dropped"]
        assert np.array_equal(bits(planes[0].cpu().numpy()), bits(first))
        ref, _ = lsf_ref.apply(first.reshape(H, W), hx, hy)
        assert lsf_ref.same(d_out.cpu().numpy().reshape(H, W), ref)[0]
    finally:
        lctx.set_kernel(xrt.XRT_KERNEL_AUTO)


def test_cli(tmp_path, lctx):
    """--spectrum F --lsf G writes the reference of its own unblurred output: the text image
    and the PGM; --lbuffer's file stays unblurred."""
    meshes = kit.phantom()
    _write_obj(tmp_path / "a.obj", meshes[0])
    _write_obj(tmp_path / "b.obj", meshes[4])
    (tmp_path / "out").mkdir()
    (tmp_path / "beam.txt").write_text("40 25.5 14.5\n0.2059 0.1037 0.08\n0.05 0 0.025\n")
    (tmp_path / "lsf.txt").write_text("# x, then y\n0.0625 0.25 0.4375 0.1875 0.0625\n0.5 0.375 0.125\n")
    hx, hy = np.array([0.0625, 0.25, 0.4375, 0.1875, 0.0625], F), np.array([0.5, 0.375, 0.125], F)
    W = H = 24
    common = ["--spectrum", str(tmp_path / "beam.txt"), "-i", str(tmp_path / "a.obj"), "-i", str(tmp_path / "b.obj"),
              "-s", str(W), str(H)]

    def run(*args):
        r = subprocess.run([EXE, *args], capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert r.returncode == 0, r.stderr

    run(*common, "-f", "plain.txt", "--lbuffer", "plain.raw")
    run(*common, "--lsf", str(tmp_path / "lsf.txt"), "-f", "blur.txt", "--lbuffer", "blur.raw", "--u8", "blur.pgm")
    assert (tmp_path / "blur.raw").read_bytes() == (tmp_path / "plain.raw").read_bytes()
    lb = np.fromfile(tmp_path / "plain.raw", F)
    assert np.count_nonzero(lb == F(-1.0)) > 0
    image, _ = lctx.hole_fill(lb, W, H)                 # the unblurred image, bit for bit
    assert (tmp_path / "out" / "plain.txt").read_bytes() == oracle.text_bytes(image, W, H)
    want, want_u8 = lsf_ref.apply(image.reshape(H, W), hx, hy)
    assert not np.isnan(want).any()
    assert (tmp_path / "out" / "blur.txt").read_bytes() == oracle.text_bytes(want.reshape(-1), W, H)
    assert (tmp_path / "out" / "blur.txt").read_bytes() != (tmp_path / "out" / "plain.txt").read_bytes()
    pgm = (tmp_path / "blur.pgm").read_bytes()
    assert pgm[-W * H:] == want_u8.tobytes()
    # --paths --spectrum F --lsf G: the same image, the planes as rendered
    run("--paths", *common, "--lsf", str(tmp_path / "lsf.txt"), "-f", "p.txt")
    assert (tmp_path / "out" / "p.txt").read_bytes() == (tmp_path / "out" / "blur.txt").read_bytes()
    run("--paths", *common, "-f", "q.txt")
    assert (tmp_path / "out" / "p.m1.txt").read_bytes() == (tmp_path / "out" / "q.m1.txt").read_bytes()
    # a Gaussian by its sigma
    run(*common, "--lsf-gaussian", "1.25:9", "-f", "g.txt")
    g = xrt.lsf_gaussian(1.25, 9)
    want_g, _ = lsf_ref.apply(image.reshape(H, W), g, g)
    assert (tmp_path / "out" / "g.txt").read_bytes() == oracle.text_bytes(want_g.reshape(-1), W, H)
