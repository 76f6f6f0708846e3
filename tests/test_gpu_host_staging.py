"""The host-buffer entry points' staging (per-call device scratch for the operators, the context's
staging planes for the renders and the hole fill): a host entry gives the bits of its _device entry
over torch buffers; the staging planes grow and are reused on one context without changing a
result; calls with no work leave their output arrays alone.  Nothing here checks a kernel's
arithmetic (the operators' own test files do): the shapes are just large enough that a wrong byte
count, a swapped plane or a missing optional buffer shows -- three planes of 70 x 67 (one k_lsf tile
plus a ragged edge on both axes)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import logf_ref
import materials_kit as kit
import simpleraytracing_amd as xrt
import spectrum_kit as skit
from simpleraytracing_amd import _abi
from conftest import bits

pytestmark = pytest.mark.gpu
F = np.float32
W, H, P = 70, 67, 3
N = W * H
CANARY = 0xA5


def new_context():
    return xrt.Context(int(os.environ.get("XRT_DEVICE", "0")))


@pytest.fixture(scope="module")
def pctx():
    """A context of this module's own: the models and scenes set here never reach other tests."""
    c = new_context()
    yield c
    c.close()


def scene():
    """Three meshes of the phantom: tissue, bone and the open quads (flagged rays for the hole fill)."""
    meshes = kit.phantom()
    return [meshes[0], meshes[1], meshes[4]]


@functools.lru_cache(maxsize=None)
def stack():
    """(image (P, H, W), flat plane, dark plane, flat_value), computed once and left unchanged."""
    out = logf_ref.planes(4242, W, H, P, True, True)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def traced(pctx):
    """(paths (3, H, W), open (H, W), weights, mu, lbuffer (H, W)) of the scene at W x H: the apply's and
    the hole fill's inputs, rendered once."""
    meshes = scene()
    w, mu = skit.table(3, 8)
    try:
        pctx.upload_scene(meshes)
        pctx.set_paths()
        paths, opn, _ = pctx.render_paths(xrt.camera_for_scene(meshes, W, H))
    finally:
        pctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
    lb = pctx.apply_spectrum(paths, opn, w, mu)
    assert np.count_nonzero(opn) > 0 and np.count_nonzero(lb == F(-1.0)) > 0      # the hole fill has work
    assert all(np.count_nonzero(paths[m]) > 0 for m in range(3))
    for a in (paths, opn, lb):
        a.setflags(write=False)
    return paths, opn, w, mu, lb


def on_device(a):
    import torch
    a = np.array(a, copy=True, order="C")                     # (the fixtures' arrays are read-only)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to("cuda")


def device_out(n, dtype=None):
    import torch
    return torch.full((n,), CANARY if dtype is not None else 7.0, dtype=dtype or torch.float32, device="cuda")


def fetch(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want, what):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.dtype == want.dtype and got.size == want.size, what
    assert np.array_equal(bits(got), bits(want)), (what, np.nonzero(bits(got) != bits(want))[0][:8])


# ----------------------------------------------------- host entry == device entry
@pytest.mark.parametrize("masks", [True, False], ids=["open", "no-open"])
def test_apply_spectrum(pctx, traced, masks):
    paths, opn, w, mu, lb = traced
    got = pctx.apply_spectrum(paths, opn if masks else None, w, mu)
    assert got.shape == (H, W) and got.dtype == F
    d_paths, d_open, d_lb = on_device(paths), on_device(opn), device_out(N)
    pctx.apply_spectrum_device(N, d_paths.data_ptr(), d_open.data_ptr() if masks else 0, w, mu, d_lb.data_ptr())
    same(got, fetch(d_lb), "lbuffer")
    if masks:
        same(got, lb, "the fixture's")
    else:
        assert not np.array_equal(bits(got), bits(lb))          # (the masks matter in this scene)


def test_hole_fill(pctx, traced):
    import torch
    lb = traced[4]
    img, u8 = pctx.hole_fill(lb, W, H)
    assert img.dtype == F and u8.dtype == np.uint8 and img.size == N and u8.size == N
    d_lb, d_img, d_u8 = on_device(lb), device_out(N), device_out(N, torch.uint8)
    pctx.hole_fill_device(W, H, d_lb.data_ptr(), d_img.data_ptr(), d_u8.data_ptr())
    same(img, fetch(d_img), "image")
    same(u8, fetch(d_u8), "u8")
    assert not np.array_equal(bits(img), bits(lb.reshape(-1)))  # (holes were filled)


@pytest.mark.parametrize("out,u8", [(True, True), (True, False), (False, True)], ids=["both", "out", "u8"])
def test_detector_response(pctx, out, u8):
    import torch
    image = stack()[0]
    hx, hy = xrt.lsf_gaussian(1.25, 9), xrt.lsf_gaussian(0.8, 5)
    o, u = pctx.detector_response(image, hx, hy, out=out, u8=u8)
    assert (o is not None) == out and (u is not None) == u8
    d_image, d_o, d_u = on_device(image), device_out(P * N), device_out(P * N, torch.uint8)
    pctx.detector_response_device(W, H, P, d_image.data_ptr(), hx, hy, d_o.data_ptr() if out else 0,
                                  d_u.data_ptr() if u8 else 0)
    if out:
        assert o.shape == (P, H, W)
        same(o, fetch(d_o), "out")
        assert not any(np.array_equal(bits(o[p]), bits(o[q])) for p in range(P) for q in range(p))
    else:
        assert (fetch(d_o) == 7.0).all()
    if u8:
        assert u.shape == (P, H, W)
        same(u, fetch(d_u), "u8")
    else:
        assert (fetch(d_u) == CANARY).all()


@pytest.mark.parametrize("planes,sino", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["scalar", "flat-dark", "scalar-sinograms", "flat-dark-sinograms"])
def test_log_projection(pctx, planes, sino):
    image, flat, dark, fv = stack()
    f, d = (flat, dark) if planes else (None, None)
    got = pctx.log_projection(image, f, d, None if planes else fv, 0.01, sino)
    assert got.shape == ((H, P, W) if sino else (P, H, W))
    d_image, d_out = on_device(image), device_out(P * N)
    d_f, d_d = (on_device(flat), on_device(dark)) if planes else (None, None)
    pctx.log_projection_device(W, H, P, d_image.data_ptr(), d_out.data_ptr(), d_f.data_ptr() if planes else 0,
                               d_d.data_ptr() if planes else 0, 0.0 if planes else fv, 0.01, sino)
    same(got, fetch(d_out), (planes, sino))
    same(got, logf_ref.apply(image, f, d, fv, 0.01, sino), "reference")


# ------------------------------------------- staging growth and reuse on one context
def test_staging_grows_and_is_reused(traced):
    """render_rows at 8 x 8, hole_fill at 70 x 67 (the planes grow), render_paths of three meshes at
    16 x 16 (smaller than the planes: n * max(num_meshes, 2) elements, the masks in the 8-bit plane),
    render_rows at 8 x 8 again -- each equals the same call on a fresh context."""
    lb = traced[4]
    meshes = scene()
    cam8, cam16 = xrt.camera_for_scene(meshes, 8, 8), xrt.camera_for_scene(meshes, 16, 16)

    def rows(c):
        img, lbuf, u8, st = c.render_rows(cam8)
        assert st.rays == 64 and st.hit_rays > 0
        return img, lbuf, u8, np.array([st.rays, st.hit_rays, st.hits])

    def fill(c):
        return c.hole_fill(lb, W, H)

    def paths(c):
        try:
            c.set_paths()
            p, o, st = c.render_paths(cam16)
        finally:
            c.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
        assert p.shape == (3, 16, 16) and o.shape == (16, 16) and st.hit_rays > 0
        return p, o, np.array([st.rays, st.hit_rays, st.hits, st.odd_rays])

    with new_context() as one:
        one.upload_scene(meshes)
        for step, call in enumerate((rows, fill, paths, rows)):
            got = call(one)
            with new_context() as fresh:
                fresh.upload_scene(meshes)
                want = call(fresh)
            assert len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                same(g, w, (step, call.__name__, k))


# ------------------------------------------------------------------- empty work
def canary(n, dtype):
    a = np.empty(n, dtype)
    a.view(np.uint8)[:] = CANARY
    return a


def untouched(*arrays):
    return all((a.view(np.uint8) == CANARY).all() for a in arrays)


def test_empty_calls_leave_the_outputs_alone(pctx):
    lib, c = pctx._lib, pctx._ctx
    w, mu = skit.table(3, 8)
    paths, opn, out = canary(3 * 16, F), canary(16, np.uint16), canary(16, F)
    rc = lib.xrt_apply_spectrum(c, 0, 3, xrt._fptr(paths), xrt._u16ptr(opn), xrt._fptr(w), xrt._fptr(mu), w.size,
                                xrt._fptr(out))
    assert rc == _abi.XRT_OK and untouched(paths, opn, out)

    lb, img, u8 = canary(16, F), canary(16, F), canary(16, np.uint8)
    rc = lib.xrt_hole_fill(c, 0, 0, xrt._fptr(lb), xrt._fptr(img), xrt._u8ptr(u8))
    assert rc == _abi.XRT_OK and untouched(lb, img, u8)

    meshes = scene()
    cam = xrt.camera_for_scene(meshes, 16, 16)
    st = xrt.Stats()
    try:
        pctx.upload_scene(meshes)
        pctx.set_paths()
        rc = lib.xrt_render_paths(c, ctypes.byref(cam), 5, 5, 3, xrt._fptr(paths), xrt._u16ptr(opn), ctypes.byref(st))
    finally:
        pctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
    assert rc == _abi.XRT_OK and untouched(paths, opn)
    assert st.rays == 0 and st.hits == 0
