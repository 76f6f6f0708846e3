"""The spectral detector on the device: k_spectral_detector bit for bit against
tests/detector_ref.py -- the numpy restatement of the contract in include/xrt.h -- over every quad
edge, mesh and channel bound, gains on either side of the sampler's threshold, the wave shapes the
kernel treats apart, first indices that carry into the counter's second word, device buffers, the
rendered phantom and the CLI."""
import functools
import os
import subprocess

import numpy as np
import pytest

import detector_kit as dkit
import detector_ref
import materials_kit as kit
import simpleraytracing_amd as xrt
import spectrum_kit as skit
from simpleraytracing_amd import _abi
from oracle import oracle
from conftest import ROOT, bits
from test_detector_cpu import GRID
from test_spectrum_cpu import _write_obj

pytestmark = pytest.mark.gpu
F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
SEED = 0x0123456789ABCDEF


@pytest.fixture(scope="module")
def pctx():
    """A context of this module's own."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


def check(got, want, what):
    assert detector_ref.same(got, want), (what, np.argwhere(bits(got) != bits(want))[:8])


@pytest.mark.parametrize("shape,K,M,C", GRID, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_crafted_planes(pctx, shape, K, M, C):
    """Sizes 1, 63, 64, 65, 257 and 7 x 13, K over the quad edges, M and C over both mesh bounds and the
    three channel bounds; per case the four gain classes (a wave of small means only, of large means only,
    both within a lane's quad, dark), both draw modes, both output modes, read noise on and off."""
    paths, opn = dkit.planes(shape, M, far=dkit.FAR[M])
    w, mu = dkit.table(M, K)
    r = dkit.response(C, K)
    for name, gain in dkit.gains(w, mu, dkit.FAR[M]).items():
        for noisy, counts, rn in [(True, True, 0.0), (True, False, 12.5), (False, True, 0.0), (False, False, 0.0)]:
            got = pctx.spectral_detector(paths, opn, w, mu, r, gain, 99, noisy, counts, rn, 2 ** 32 - 3)
            want = detector_ref.spectral_detector(paths, opn, w, mu, r, gain, 99, noisy, counts, rn, 2 ** 32 - 3)
            assert got.shape == (C,) + tuple(shape)
            check(got, want, (name, noisy, counts, rn))
    got = pctx.spectral_detector(paths, None, w, mu, r, 1.0, 99)                 # open NULL
    check(got, detector_ref.spectral_detector(paths, None, w, mu, r, 1.0, 99), "open NULL")


@pytest.mark.parametrize("M", [3, 16])
@pytest.mark.parametrize("name", ["misses", "one lane", "flagged lane", "minus zero", "far", "nan", "infinite"])
def test_wave_shapes(pctx, name, M):
    """A wave of misses under both draw modes (a noisy miss still draws), a wave of zeros but for one lane,
    a flagged lane in a wave of zeros, a plane of -0.0, exponents through exp's special cases, a NaN and
    infinite paths: the device equals the reference and the host hook."""
    K, C = 5, 2
    paths, opn = dkit.wave_shapes(M, K)[name]
    w, mu = dkit.table(M, K)
    r = dkit.response(C, K)
    for noisy in (True, False):
        for gain in (0.5, 400.0):
            got = pctx.spectral_detector(paths, opn, w, mu, r, gain, 3, noisy)
            check(got, detector_ref.spectral_detector(paths, opn, w, mu, r, gain, 3, noisy), (name, noisy, gain))
            check(got, xrt.host_spectral_detector(paths, opn, w, mu, r, gain, 3, noisy), (name, noisy, gain, "hook"))
    if name == "misses":
        noisy = pctx.spectral_detector(paths, opn, w, mu, r, 400.0, 3, True)
        assert len(np.unique(noisy[0])) > 8                                       # every miss drew its own counts


@functools.lru_cache(maxsize=None)
def scan():
    """Three waves and a ragged fourth, M = 3, K = 5, C = 3, means on both sides of 64."""
    paths, opn = dkit.planes((2, 113), 3)
    w, mu = dkit.table(3, 5)
    for a in (paths, opn, w, mu):
        a.setflags(write=False)
    return paths, opn, w, mu, dkit.response(3, 5), dkit.gains(w, mu)["mixed"]


@pytest.mark.parametrize("first_index", dkit.FIRST)
def test_first_index_and_pieces(pctx, first_index):
    """First indices 0, 1, 2^32 - 3 (the carry into the counter's second word) and 2^40 + 5; a buffer drawn
    in two pieces, each under its own first index, equals the whole."""
    paths, opn, w, mu, r, gain = scan()
    whole = pctx.spectral_detector(paths, opn, w, mu, r, gain, SEED, True, True, 4.0, first_index)
    check(whole, detector_ref.spectral_detector(paths, opn, w, mu, r, gain, SEED, True, True, 4.0, first_index), first_index)
    for p in range(2):
        piece = pctx.spectral_detector(paths[:, p], opn[p], w, mu, r, gain, SEED, True, True, 4.0, first_index + p * 113)
        assert np.array_equal(bits(piece), bits(whole[:, p])), p


@pytest.mark.parametrize("seed", dkit.SEEDS)
def test_seeds(pctx, seed):
    paths, opn, w, mu, r, gain = scan()
    got = pctx.spectral_detector(paths, opn, w, mu, r, gain, seed, read_noise=2.0)
    check(got, detector_ref.spectral_detector(paths, opn, w, mu, r, gain, seed, read_noise=2.0), seed)
    other = pctx.spectral_detector(paths, opn, w, mu, r, gain, seed ^ (1 << 32), read_noise=2.0)
    keep = opn == 0
    assert np.count_nonzero(got[0][keep] != other[0][keep]) > np.count_nonzero(keep) // 2
    expected = pctx.spectral_detector(paths, opn, w, mu, r, gain, seed, noisy=False)        # the seed is ignored
    assert np.array_equal(bits(expected), bits(pctx.spectral_detector(paths, opn, w, mu, r, gain, 0, noisy=False)))


def test_device_entry_offset_buffers_and_two_tables(pctx):
    """Torch buffers that begin one float past an aligned address: the same bits, nothing written outside
    the output, the inputs untouched.  Then two launches back to back on one stream with other tables and
    responses, before one synchronise: each launch owns its copies.  The host entry and the module-level
    call equal the device entry."""
    import torch
    paths, opn, w, mu, r, gain = scan()
    M, n = 3, opn.size
    flat, mask = paths.reshape(M, n), opn.reshape(n)
    d_paths = torch.zeros(M * n + 2, dtype=torch.float32, device="cuda")
    d_open = torch.zeros(n + 2, dtype=torch.int16, device="cuda")
    d_out = torch.zeros(3 * n + 2, dtype=torch.float32, device="cuda")
    d_out2 = torch.zeros(2 * n + 2, dtype=torch.float32, device="cuda")
    d_paths[1:1 + M * n].copy_(torch.from_numpy(flat.reshape(-1).copy()))
    d_open[1:1 + n].copy_(torch.from_numpy(mask.view(np.int16).copy()))
    w2, mu2 = dkit.table(3, 8, seed=4)
    r2 = dkit.windows(2, 8)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    pctx.spectral_detector_device(n, d_paths.data_ptr() + 4, d_open.data_ptr() + 2, w, mu, r, d_out.data_ptr() + 4, gain,
                                  SEED, True, False, 3.0, 7, stream)
    pctx.spectral_detector_device(n, d_paths.data_ptr() + 4, 0, w2, mu2, r2, d_out2.data_ptr() + 4, 2.0, SEED, True, True,
                                  0.0, 7, stream)
    torch.cuda.synchronize()
    first = d_out.cpu().numpy()
    second = d_out2.cpu().numpy()
    want = detector_ref.spectral_detector(flat, mask, w, mu, r, gain, SEED, True, False, 3.0, 7)
    check(first[1:-1].reshape(3, n), want, "offset buffers")
    check(second[1:-1].reshape(2, n), detector_ref.spectral_detector(flat, None, w2, mu2, r2, 2.0, SEED, True, True, 0.0, 7),
          "the second table")
    assert first[0] == 0 and first[-1] == 0 and second[0] == 0 and second[-1] == 0
    assert np.array_equal(bits(d_paths.cpu().numpy()[1:-1]), bits(flat.reshape(-1)))
    host = pctx.spectral_detector(flat, mask, w, mu, r, gain, SEED, True, False, 3.0, 7)
    assert np.array_equal(bits(host), bits(first[1:-1].reshape(3, n)))
    assert np.array_equal(bits(xrt.spectral_detector(flat, mask, w, mu, r, gain, SEED, True, False, 3.0, 7)), bits(host))
    with pytest.raises(xrt.XrtError) as e:                  # the output over the last path
        pctx.spectral_detector_device(n, d_paths.data_ptr() + 4, 0, w, mu, r, d_paths.data_ptr() + 4 * M * n)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps paths" in str(e.value)


def test_expected_with_ones_is_apply_spectrum(pctx):
    """EXPECTED, COUNTS, gain 1, one channel of ones: apply_spectrum_device's plane on the same buffers,
    bit for bit (no NaN among them), at M = 3 and at M = 16 with more than four live meshes."""
    import torch
    for M, K in ((3, 8), (16, 5)):
        paths, opn = dkit.planes((5, 77), M, far=30.0)
        w, mu = skit.table(M, K)
        n = opn.size
        d_paths = torch.from_numpy(paths.reshape(-1).copy()).to("cuda")
        d_open = torch.from_numpy(opn.reshape(-1).view(np.int16).copy()).to("cuda")
        d_lb = torch.empty(n, dtype=torch.float32, device="cuda")
        d_out = torch.empty(n, dtype=torch.float32, device="cuda")
        pctx.apply_spectrum_device(n, d_paths.data_ptr(), d_open.data_ptr(), w, mu, d_lb.data_ptr())
        pctx.spectral_detector_device(n, d_paths.data_ptr(), d_open.data_ptr(), w, mu, np.ones((1, K), F), d_out.data_ptr(),
                                      1.0, 0, False, True)
        torch.cuda.synchronize()
        lb = d_lb.cpu().numpy()
        assert not np.isnan(lb).any() and (lb == -1).any() and len(np.unique(lb)) > n // 2
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(lb)), M


@pytest.mark.parametrize("W,H", [(67, 45), (96, 80)])
def test_rendered_phantom(pctx, W, H):
    """render_paths -> the detector, against the reference over spectrum_kit.phantom_sums' planes, flagged
    rays included: an energy-integrating row and two windows, noisy and expected."""
    meshes = kit.phantom()
    su = skit.phantom_sums(W, H)
    w, mu = skit.phantom_table(4)
    r = np.array([[20.0, 40.0, 60.0, 80.0], [1.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0]], F)
    want_paths = np.ascontiguousarray(su.distance.T).reshape(5, H, W)
    mask = ((su.sign_sum != 0).astype(np.uint32) << np.arange(5, dtype=np.uint32)).sum(1).astype(np.uint16).reshape(H, W)
    assert np.count_nonzero(mask) > 0
    cam = xrt.camera_for_scene(meshes, W, H)
    try:
        pctx.upload_scene(meshes)
        pctx.set_paths()
        paths, opn, _ = pctx.render_paths(cam)
    finally:
        pctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
    assert np.array_equal(bits(paths), bits(want_paths)) and np.array_equal(opn, mask)
    for noisy, gain in ((True, 25.0), (False, 1.0)):
        got = pctx.spectral_detector(paths, opn, w, mu, r, gain, 11, noisy, first_index=W * H)
        want = detector_ref.spectral_detector(want_paths, mask, w, mu, r, gain, 11, noisy, first_index=W * H)
        check(got, want, (W, H, noisy))
        assert (got[:, mask != 0] == -1).all()
        if noisy:
            keep = mask == 0
            assert np.array_equal(got[1][keep] + got[2][keep], pctx.spectral_detector(
                paths, opn, w, mu, np.ones((1, 4), F), gain, 11, True, first_index=W * H)[0][keep])


def test_cli_detector(tmp_path, pctx):
    """xrt_main --paths --spectrum --detector over a --turntable 2 scan: NAME.c<c>.EXT is the Python
    entry's channel after the hole fill -- expected values at gain 1 without --noise; with --noise GAIN:SEED
    and --read-noise the draw inside the detector, in intensity mode, projection p under first_index =
    p W H --, NAME.EXT and the planes stay what --paths --spectrum writes, and without the option the
    bytes are as before."""
    W = H = 24
    meshes = kit.phantom()
    _write_obj(tmp_path / "a.obj", meshes[0])
    _write_obj(tmp_path / "b.obj", meshes[4])
    (tmp_path / "out").mkdir()
    (tmp_path / "beam.txt").write_text("40 25.5 14.5\n0.2059 0.1037 0.08\n0.05 0 0.025\n")
    (tmp_path / "det.txt").write_text("# an energy-integrating row, then two windows\n30 60 90\n1 1 0\n0 0 1\n")
    w, mu = np.array([40, 25.5, 14.5], F), np.array([[0.2059, 0.1037, 0.08], [0.05, 0, 0.025]], F)
    r = np.array([[30, 60, 90], [1, 1, 0], [0, 0, 1]], F)
    common = ["--paths", "--spectrum", "beam.txt", "-i", "a.obj", "-i", "b.obj", "-s", str(W), str(H)]

    def run(*args):
        res = subprocess.run([EXE, *args], capture_output=True, text=True, cwd=tmp_path, timeout=300)
        assert res.returncode == 0, res.stderr

    def text(name):
        return (tmp_path / "out" / name).read_bytes()

    run(*common, "-f", "plain.txt")
    run(*common, "-f", "e.txt", "--detector", "det.txt", "--turntable", "2")
    run(*common, "-f", "n.txt", "--detector", "det.txt", "--turntable", "2", "--noise", "2.5:7", "--read-noise", "3")
    run(*common, "-f", "one.txt", "--detector", "det.txt", "--noise", "2.5:7", "--read-noise", "3")
    scene = [xrt.load_meshes(str(tmp_path / "a.obj"))[0], xrt.load_meshes(str(tmp_path / "b.obj"))[0]]
    cam = xrt.camera_for_scene(scene, W, H)
    lo, hi = xrt.scene_bbox(scene)
    centre = (lo + ((hi - lo).astype(np.float64) / 2.0).astype(F)).astype(F)
    try:
        pctx.upload_scene(scene)
        pctx.set_paths()
        views = [pctx.render_paths(cam)[:2]]
        turn = xrt.pose_rotation((0, 1, 0), 180.0, centre)
        for m in range(2):
            pctx.set_pose(m, turn)
        views.append(pctx.render_paths(cam)[:2])
    finally:
        pctx.reset_poses()
        pctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
    assert not np.array_equal(views[0][0], views[1][0])
    for p, (paths, opn) in enumerate(views):
        image = oracle.hole_fill(pctx.apply_spectrum(paths, opn, w, mu), W, H)
        for name in ("e", "n"):
            assert text(f"{name}.p{p:03d}.txt") == oracle.text_bytes(image, W, H), (name, p)
            assert text(f"{name}.p{p:03d}.m1.txt") == oracle.text_bytes(paths[1].reshape(-1), W, H), (name, p)
        expected = pctx.spectral_detector(paths, opn, w, mu, r, 1.0, 0, noisy=False, counts=False)
        noisy = pctx.spectral_detector(paths, opn, w, mu, r, 2.5, 7, True, False, 3.0, p * W * H)
        for c in range(3):
            assert text(f"e.p{p:03d}.c{c}.txt") == oracle.text_bytes(oracle.hole_fill(expected[c], W, H), W, H), (p, c)
            assert text(f"n.p{p:03d}.c{c}.txt") == oracle.text_bytes(oracle.hole_fill(noisy[c], W, H), W, H), (p, c)
        assert text(f"e.p{p:03d}.c0.txt") != text(f"n.p{p:03d}.c0.txt")
    assert text("n.p000.txt") == text("plain.txt") and text("one.txt") == text("plain.txt")
    for c in range(3):
        assert text(f"one.c{c}.txt") == text(f"n.p000.c{c}.txt")
    assert not (tmp_path / "out" / "plain.c0.txt").exists()
