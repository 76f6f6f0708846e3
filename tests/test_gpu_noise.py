"""Photon noise on the device: k_photon_noise bit for bit against tests/noise_ref.py --
the numpy restatement of the contract in include/xrt.h -- over ragged sizes, first indices that cut a
Philox group and cross into the counter's high word, misaligned device buffers, in place, both modes,
every class of mean, a scan done in pieces, and the sampler's device probe over the CPU suite's
words."""
import functools
import os
import subprocess

import numpy as np
import pytest

import noise_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import bits

pytestmark = pytest.mark.gpu
F = np.float32
GAIN, SEED = 1.75, 0x0123456789ABCDEF
FIRST = [0, 1, 2, 3, 2 ** 34 - 3]
STACK = (3, 67, 70)                                     # (P, H, W): odd sizes, 14070 pixels, 14 workgroups


@pytest.fixture(scope="module")
def pctx():
    """A context of this module's own."""
    c = xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def stack():
    """Means on both sides of 64 in every wave: image * GAIN from 0 to about 1300, some pixels exactly 0."""
    rng = np.random.default_rng(11)
    a = (rng.uniform(0.0, 3.0, STACK) ** 6).astype(F)
    a.reshape(-1)[rng.integers(0, a.size, a.size // 16)] = F(0.0)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(first_index, counts, seed=SEED):
    """The reference over the stack, computed once and left unchanged."""
    want = noise_ref.photon_noise(stack(), GAIN, seed, counts, first_index)
    assert np.isfinite(want).all()
    want.setflags(write=False)
    return want


def check(got, want, what):
    assert got.shape == want.shape and noise_ref.same(got, want), (what, np.argwhere(bits(got) != bits(want))[:8])


@pytest.mark.parametrize("first_index", FIRST)
@pytest.mark.parametrize("counts", [False, True])
def test_stack_and_ragged_sizes(pctx, first_index, counts):
    """The 70 x 67 x 3 stack and n = 1, 2, 3, 5 under every first index, both modes."""
    check(pctx.photon_noise(stack(), GAIN, SEED, counts, first_index), reference(first_index, counts), "stack")
    flat = stack().reshape(1, -1)
    for n in (1, 2, 3, 5):
        piece = flat[:, 1000:1000 + n]
        want = noise_ref.photon_noise(piece, GAIN, SEED, counts, first_index)
        check(pctx.photon_noise(piece, GAIN, SEED, counts, first_index), want, n)


@pytest.mark.parametrize("offs", [(0, 0), (1, 0), (0, 1), (1, 1), (3, 3), (3, 2)])
def test_device_buffers_offset_and_in_place(pctx, offs):
    """Torch buffers that begin `offs` floats past an aligned address (input, output): the same bits,
    nothing written outside the output, the input untouched; then in place."""
    import torch
    P, H, W = STACK
    n = P * H * W
    image = stack().reshape(-1)
    for first_index in (0, 3, 2 ** 34 - 3):
        want = reference(first_index, False).reshape(-1)
        bufs = [torch.zeros(n + 8, dtype=torch.float32, device="cuda") for _ in range(2)]
        d_img, d_out = (b[o:o + n] for b, o in zip(bufs, offs))
        d_img.copy_(torch.from_numpy(image.copy()))
        pctx.photon_noise_device(W, H, P, d_img.data_ptr(), d_out.data_ptr(), GAIN, SEED, False, first_index)
        torch.cuda.synchronize()
        check(d_out.cpu().numpy(), want, (offs, first_index))
        for b, o in zip(bufs, offs):
            guard = b.cpu().numpy()
            assert (guard[:o] == 0).all() and (guard[o + n:] == 0).all(), offs
        assert np.array_equal(bits(d_img.cpu().numpy()), bits(image))
        pctx.photon_noise_device(W, H, P, d_img.data_ptr(), d_img.data_ptr(), GAIN, SEED, False, first_index)
        torch.cuda.synchronize()
        check(d_img.cpu().numpy(), want, (offs, first_index, "in place"))
    with pytest.raises(xrt.XrtError) as e:                  # a partial overlap
        pctx.photon_noise_device(W, H, P, d_img.data_ptr(), d_img.data_ptr() + 4, GAIN, SEED)
    assert e.value.code == _abi.XRT_ERR_ARGUMENT and "overlaps" in str(e.value)


def test_plane_of_every_class(pctx):
    """One plane mixing every class of mean the contract names, each under many words, both modes."""
    plane = np.tile(noise_ref.LAMBDAS, 97 * 5).reshape(97, -1)             # (97, 65): odd sizes
    for counts in (False, True):
        for first_index in (0, 1):
            want = noise_ref.photon_noise(plane, 1.0, 5, counts, first_index)
            got = pctx.photon_noise(plane, 1.0, 5, counts, first_index)
            check(got, want, (counts, first_index))
            lam = plane.reshape(-1)
            g = got.reshape(-1)
            assert np.isnan(g[np.isnan(lam) | (lam < 0)]).all() and (g[lam == np.inf] == np.inf).all()
            assert (bits(g[(lam == 0) | (lam == F(1e-45))]) == 0).all()     # -0.0 counts as 0: +0.0 out
    want = noise_ref.photon_noise(plane, 0.5, 5)                            # a gain that moves the means
    check(pctx.photon_noise(plane, 0.5, 5), want, "gain 0.5")


def test_scan_in_pieces(pctx):
    """Three calls, each with its plane's first_index, equal one call over the stack."""
    P, H, W = STACK
    for base in (0, 2 ** 34 - 3):
        whole = pctx.photon_noise(stack(), GAIN, SEED, False, base)
        check(whole, reference(base, False), "whole")
        for p in range(P):
            one = pctx.photon_noise(stack()[p], GAIN, SEED, False, base + p * H * W)
            check(one, whole[p], ("piece", p))


def test_seeds(pctx):
    """Two seeds differ -- in the key's low and in its high word --, and the same seed repeats."""
    a = pctx.photon_noise(stack(), GAIN, SEED)
    again = pctx.photon_noise(stack(), GAIN, SEED)
    assert np.array_equal(bits(a), bits(again))
    for other in (SEED ^ 1, SEED ^ (1 << 63)):
        b = pctx.photon_noise(stack(), GAIN, other)
        check(b, reference(0, False, other), "other seed")
        assert np.count_nonzero(a != b) > a.size // 2


def test_host_entry_equals_device_entry(pctx):
    import torch
    P, H, W = STACK
    host = pctx.photon_noise(stack(), GAIN, SEED, True, 2)
    d_img = torch.from_numpy(stack().reshape(-1).copy()).to("cuda")
    d_out = torch.empty_like(d_img)
    pctx.photon_noise_device(W, H, P, d_img.data_ptr(), d_out.data_ptr(), GAIN, SEED, True, 2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(host.reshape(-1)), bits(d_out.cpu().numpy()))
    assert np.array_equal(bits(xrt.photon_noise(stack()[0], GAIN, SEED, True, 2)), bits(host[0]))


def test_cli_noise(tmp_path, pctx):
    """xrt_main --noise GAIN:SEED: NAME.EXT receives the reference's noise of the rendered image, in
    intensity mode, projection p of a --turntable with first_index = p W H, ahead of --log-projection;
    --u8 stays as rendered; SEED defaults to 0."""
    import logf_ref
    from oracle import oracle
    from conftest import DRAGON, ROOT
    exe = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")
    W, H = 48, 40
    (tmp_path / "out").mkdir()

    def run(*args):
        r = subprocess.run([exe, "-s", str(W), str(H), "-i", DRAGON, *args], capture_output=True, text=True,
                           cwd=tmp_path, timeout=300)
        assert r.returncode == 0, r.stderr

    def text(name):
        return (tmp_path / "out" / name).read_bytes()

    run("-f", "plain.txt", "--u8", "plain.pgm")
    run("-f", "n.txt", "--u8", "n.pgm", "--noise", "2.5:7")
    run("-f", "z.txt", "--noise", "2.5")
    run("-f", "l.txt", "--noise", "2.5:7", "--log-projection", "80")
    run("-f", "t.txt", "--noise", "2.5:7", "--turntable", "2")
    tris = xrt.load_ply(DRAGON)
    cam = xrt.camera_for_mesh(tris, W, H)
    lo, hi = xrt.mesh_bbox(tris)
    centre = (lo + ((hi - lo).astype(np.float64) / 2.0).astype(F)).astype(F)
    try:
        pctx.upload_scene([tris])
        images = [pctx.render_rows(cam)[0].reshape(H, W)]
        pctx.set_pose(0, xrt.pose_rotation((0, 1, 0), 180.0, centre))
        images.append(pctx.render_rows(cam)[0].reshape(H, W))
    finally:
        pctx.reset_poses()
    assert text("plain.txt") == oracle.text_bytes(images[0].reshape(-1), W, H)
    noisy = noise_ref.photon_noise(images[0], 2.5, 7)
    assert not np.array_equal(noisy, images[0])
    assert text("n.txt") == oracle.text_bytes(noisy.reshape(-1), W, H)
    assert (tmp_path / "n.pgm").read_bytes() == (tmp_path / "plain.pgm").read_bytes()
    assert text("z.txt") == oracle.text_bytes(noise_ref.photon_noise(images[0], 2.5, 0).reshape(-1), W, H)
    assert text("l.txt") == oracle.text_bytes(logf_ref.pixels(noisy, None, None, 80.0).reshape(-1), W, H)
    assert text("t.p000.txt") == text("n.txt")
    second = noise_ref.photon_noise(images[1], 2.5, 7, first_index=W * H)
    assert text("t.p001.txt") == oracle.text_bytes(second.reshape(-1), W, H)


def test_device_probe_over_the_word_set(pctx):
    """xrt_debug_poisson_batch: every class of mean under the CPU suite's words (the edges, both
    |q| = 0.425 crossings, a stride of 4099 over all 2^32 words)."""
    words = noise_ref.word_set()
    total = 0
    for lam in noise_ref.LAMBDAS.astype(np.float64):
        got = pctx.debug_poisson(lam, words)
        want = noise_ref.poisson_from_word(lam, words)
        nan = np.isnan(want)
        assert np.array_equal(got[~nan], want[~nan]) and np.isnan(got[nan]).all(), lam
        total += words.size
    assert total > 13_000_000
