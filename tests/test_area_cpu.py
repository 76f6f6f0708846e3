"""Area sampling without a GPU: the pass compiled for the host (xrt_host_area_integrate)
bit for bit against tests/area_ref.py; the two camera helpers against their f32 restatement; the
argument errors that need no device; geometric unsharpness and pixel-area means through the oracle
alone; the CLI's refusals, k_area_integrate's code-object metadata and a stand-alone sanitizer build
of the host code."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import area_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from conftest import DRAGON, ROOT, bits
from test_materials_cpu import _render_kernel_metadata
from test_pose_cpu import _sanitizer_runtime

F = np.float32
EXE = os.path.join(ROOT, "simpleraytracing_amd", "lib", "xrt_main")


# --------------------------------------------------------------------------- the hook against the reference
@pytest.mark.parametrize("size", area_ref.SIZES, ids=str)
def test_host_pass_equals_the_reference(size):
    """Every bin, source count and plane count of the matrix at one output size, with unequal weights
    (one of them zero from three sources on); a stacked call equals the per-plane calls."""
    W, H = size
    for bx, by, S, P in area_ref.matrix(size):
        a, w = area_ref.planes(W, H, bx, by, S, P), area_ref.weights(S)
        got, u8 = xrt.host_area_integrate(a, (by, bx), w, u8=True)
        want = area_ref.reference(W, H, bx, by, S, P)
        assert got.shape == (P, H, W) and np.array_equal(bits(got), bits(want)), (size, bx, by, S, P)
        assert np.array_equal(u8, area_ref.lut_u8(want)), (size, bx, by, S, P)
        if P > 1:
            for p in range(P):
                assert np.array_equal(bits(xrt.host_area_integrate(a[p], (by, bx), w)), bits(want[p]))


def test_identity_returns_the_inputs_bits():
    """Bin 1 x 1, one source of weight 1.0: every finite bit pattern class comes back, -0.0 and denormals too."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, 2 ** 32, (37, 53), dtype=np.uint64).astype(np.uint32).view(F)
    a[~np.isfinite(a)] = F(-0.0)
    a[0, :4] = np.array([0x80000000, 1, 0x807FFFFF, 0x7F7FFFFF], np.uint32).view(F)
    assert np.array_equal(bits(xrt.host_area_integrate(a)), bits(a))
    assert np.array_equal(bits(area_ref.integrate(a)), bits(a))
    assert np.array_equal(bits(xrt.host_area_integrate(a[None], 1, [1.0])), bits(a))


@pytest.mark.parametrize("S", area_ref.SOURCES + (64,))
def test_a_flat_field_stays_flat(S):
    """Unit weights over a constant 80.0 return 80.0 exactly under every bin; its line integral is +0.0."""
    for bx, by in area_ref.BINS:
        a = np.full((S, 3 * by, 5 * bx), 80.0, F)
        out = xrt.host_area_integrate(a, (by, bx))
        assert np.array_equal(bits(out), bits(np.full((3, 5), 80.0, F))), (bx, by, S)
        assert not bits(xrt.host_log_projection(out, flat_value=80.0)).any()


def test_specials():
    a = area_ref.specials()
    w = area_ref.weights(a.shape[0])
    want = area_ref.integrate(a, 2, w)
    got = xrt.host_area_integrate(a, 2, w)
    assert area_ref.same(got, want)
    assert np.isnan(want).sum() > 0 and (want == np.inf).sum() > 0 and (want == -np.inf).sum() > 0
    assert (want == F(3.0e38)).sum() > 0                                    # the f64 sum passed f32's range


# --------------------------------------------------------------------------- the helpers
def _random_camera(rng, W, H):
    cam = xrt.Camera()
    for name in ("origin", "detector", "up", "right"):
        v = rng.normal(0, 100, 3).astype(F)
        for k in range(3):
            getattr(cam, name)[k] = float(v[k])
    cam.pixel_spacing, cam.width, cam.height = float(F(rng.uniform(1e-3, 2.0))), W, H
    return cam


def _cameras(dragon):
    rng = np.random.default_rng(17)
    cams = [xrt.camera_for_mesh(dragon, W, H) for W, H in ((64, 48), (128, 128), (333, 77), (2048, 2048))]
    return cams + [_random_camera(rng, 31, 17) for _ in range(20)]


def test_helpers_equal_the_f32_restatement(dragon):
    for cam in _cameras(dragon):
        for b in range(1, xrt.XRT_MAX_BIN + 1):
            assert area_ref.camera_fields(xrt.supersampled_camera(cam, b)) == area_ref.camera_fields(area_ref.supersample(cam, b))
        for su, sv, nu, nv in ((0.5, 0.25, 3, 3), (1.0, 0.0, 5, 1), (0.0, 0.0, 1, 1), (0.3, 0.7, 8, 8), (2.0, 1.0, 2, 7)):
            got, w = xrt.focal_spot(cam, su, sv, nu, nv)
            want, ww = area_ref.focal_spot(cam, su, sv, nu, nv)
            assert [area_ref.camera_fields(c) for c in got] == [area_ref.camera_fields(c) for c in want]
            assert np.array_equal(w, ww) and w.dtype == F and (w == 1).all()
    one, w = xrt.focal_spot(cam, 0.0, 0.0, 1, 1)                              # the point source
    assert area_ref.camera_fields(one[0]) == area_ref.camera_fields(cam)


def test_supersampled_spacing_is_the_larger_images(dragon):
    """By 2, 4 and 8 the spacing is what camera_from_bbox computes for the larger image (a division by a power of
    two commutes with the prologue's roundings)."""
    lo, hi = xrt.mesh_bbox(dragon)
    for W, H in ((64, 48), (100, 37), (2048, 2048)):
        cam = xrt.camera_from_bbox(lo, hi, W, H)
        for b in (2, 4, 8):
            assert area_ref.camera_fields(xrt.supersampled_camera(cam, b)) == \
                area_ref.camera_fields(xrt.camera_from_bbox(lo, hi, W * b, H * b))


def test_sub_pixel_centres_average_to_the_pixel_centre(dragon):
    """u(c) = spacing * (0.5 + c - W / 2): the bin sub-centres of pixel c average to u(c), in exact arithmetic
    on the f32 spacings."""
    from fractions import Fraction
    cam = xrt.camera_for_mesh(dragon, 64, 48)
    for b in (2, 4):
        fine = xrt.supersampled_camera(cam, b)
        ps, pf = Fraction(float(F(cam.pixel_spacing))), Fraction(float(F(fine.pixel_spacing)))
        for c in (0, 1, 31, 32, 63):
            centre = ps * (Fraction(1, 2) + c - Fraction(cam.width, 2))
            subs = [pf * (Fraction(1, 2) + (c * b + k) - Fraction(fine.width, 2)) for k in range(b)]
            assert sum(subs) / b == centre


def test_spot_is_symmetric_and_in_the_detectors_directions(dragon):
    cam = xrt.camera_for_mesh(dragon, 64, 48)
    o = np.array(list(cam.origin), np.float64)
    r, u = np.array(list(cam.right), np.float64), np.array(list(cam.up), np.float64)
    n = np.cross(r, u)
    cams, _ = xrt.focal_spot(cam, 0.6, 0.4, 4, 3)
    pos = np.array([list(c.origin) for c in cams], np.float64)
    scale = np.abs(o).max()
    assert np.abs(pos + pos[::-1] - 2 * o).max() <= 4 * np.finfo(F).eps * scale          # s and its mirror image
    assert np.abs((pos - o) @ n).max() <= 4 * np.finfo(F).eps * scale                    # nothing along the beam
    assert np.abs((pos - o) @ r).max() <= 0.3 + 1e-5 and np.abs((pos - o) @ u).max() <= 0.2 + 1e-5
    for c in cams:
        assert area_ref.camera_fields(c)[3:] == area_ref.camera_fields(cam)[3:]           # only the origin moves


# --------------------------------------------------------------------------- refusals
def _call(lib, entry, w, h, bx, by, s, p, weight, image, out, out_u8):
    def ptr(a, t=_abi._fp):
        return None if a is None else a.ctypes.data_as(t)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    if entry == "device":
        cast = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
        return lib.xrt_area_integrate_device(None, w, h, bx, by, s, p, ptr(weight), cast(image), cast(out), cast(out_u8), None)
    if entry == "host":
        return lib.xrt_area_integrate(None, w, h, bx, by, s, p, ptr(weight), ptr(image), ptr(out), ptr(out_u8, u8p))
    return lib.xrt_host_area_integrate(w, h, bx, by, s, p, ptr(weight), ptr(image), ptr(out), ptr(out_u8, u8p))


@pytest.mark.parametrize("entry", ["host", "device", "hook"])
def test_argument_errors_without_a_device(entry):
    """Every check comes before the context is looked at: with a NULL context each is XRT_ERR_ARGUMENT with its
    own message (the entries), or XRT_ERR_ARGUMENT (the hook)."""
    lib = _abi.load()
    img, out, u8 = np.zeros(96, F), np.zeros(24, F), np.zeros(24, np.uint8)
    ones = np.ones(64, F)

    def wt(*v):
        w = ones.copy()
        w[:len(v)] = v
        return w
    nan, inf = float("nan"), float("inf")
    cases = [
        ((4, 3, 2, 2, 1, 2, ones, None, out, u8), "image is NULL"),
        ((4, 3, 2, 2, 1, 2, None, img, out, u8), "weight is NULL"),
        ((4, 3, 2, 2, 1, 2, ones, img, None, None), "both NULL"),
        ((0, 3, 2, 2, 1, 2, ones, img, out, u8), "is 0"),
        ((4, 0, 2, 2, 1, 2, ones, img, out, u8), "is 0"),
        ((4, 3, 2, 2, 1, 0, ones, img, out, u8), "is 0"),
        ((4, 3, 0, 2, 1, 2, ones, img, out, u8), "bin_x"),
        ((4, 3, 9, 2, 1, 2, ones, img, out, u8), "bin_x"),
        ((4, 3, 2, 0, 1, 2, ones, img, out, u8), "bin_y"),
        ((4, 3, 2, 9, 1, 2, ones, img, out, u8), "bin_y"),
        ((4, 3, 2, 2, 0, 2, ones, img, out, u8), "num_sources"),
        ((4, 3, 2, 2, 65, 2, ones, img, out, u8), "num_sources"),
        ((2, 1, 1, 1, 2, 1, wt(1, nan), img, out, u8), "weight is NaN"),
        ((2, 1, 1, 1, 2, 1, wt(inf, 1), img, out, u8), "weight is NaN"),
        ((2, 1, 1, 1, 2, 1, wt(1, -1), img, out, u8), "negative"),
        ((2, 1, 1, 1, 2, 1, wt(0, 0), img, out, u8), "weight sum"),
        ((0x40000000, 1, 2, 1, 1, 1, ones, img, out, u8), "width * bin_x"),            # 2^31
        ((1, 0x40000000, 1, 2, 1, 1, ones, img, out, u8), "height * bin_y"),
        ((1, 0x10000, 1, 1, 1, 0x10000, ones, img, out, u8), "num_planes * height"),   # 2^32 rows
        ((0x10000000, 0x100000, 1, 1, 1, 1, ones, img, out, u8), "workgroups"),         # 2^38 of them
        ((0x7FFFFFFF, 0x7FFFFFFF, 1, 1, 64, 0xFFFFFFFF, ones, img, out, u8), "num_planes * height"),
        ((4, 3, 2, 2, 1, 2, ones, img, img, u8), "overlaps"),                           # in place
        ((4, 3, 2, 2, 1, 2, ones, img, img[95:], u8), "overlaps"),                      # the last input pixel
        ((4, 3, 2, 2, 1, 1, ones, img[11:], img, u8), "overlaps"),
        ((4, 3, 2, 2, 1, 1, ones, img, out, img.view(np.uint8)[191:]), "overlaps"),
    ]
    for args, word in cases:
        assert _call(lib, entry, *args) == _abi.XRT_ERR_ARGUMENT, (word, args[:6])
        if entry != "hook":
            assert word.encode() in lib.xrt_last_error(None), (word, lib.xrt_last_error(None))
    # arguments in order: the entries then fail on the context alone, the hook computes
    for ok in ((4, 3, 2, 2, 1, 2, ones, img, out, u8),
               (4, 3, 2, 2, 1, 2, ones, img, None, u8),
               (4, 3, 2, 2, 1, 1, ones, img, img[48:], None),                            # side by side
               (2, 1, 1, 1, 2, 1, wt(0, 1), img, out, u8),                               # a zero weight among positive ones
               (1, 1, 8, 8, 64, 1, wt(0.5), np.zeros(4096, F), out, u8)):
        rc = _call(lib, entry, *ok)
        if entry == "hook":
            assert rc == _abi.XRT_OK
        else:
            assert rc == _abi.XRT_ERR_ARGUMENT and b"context is NULL" in lib.xrt_last_error(None)


def test_helper_refusals():
    cam = xrt.Camera()
    cam.width, cam.height, cam.pixel_spacing = 8, 8, 1.0
    for b in (0, 9):
        with pytest.raises(xrt.XrtError):
            xrt.supersampled_camera(cam, b)
    big = xrt.Camera()
    big.width, big.height = 2 ** 30, 1
    with pytest.raises(xrt.XrtError):
        xrt.supersampled_camera(big, 2)
    lib = _abi.load()
    assert lib.xrt_camera_supersample(None, 2, ctypes.byref(cam)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_camera_supersample(ctypes.byref(cam), 2, None) == _abi.XRT_ERR_ARGUMENT
    for args in ((-1.0, 1.0, 1, 1), (1.0, float("inf"), 1, 1), (float("nan"), 1.0, 1, 1), (1.0, 1.0, 0, 1),
                 (1.0, 1.0, 1, 0), (1.0, 1.0, 65, 1), (1.0, 1.0, 9, 8)):
        with pytest.raises(xrt.XrtError):
            xrt.focal_spot(cam, *args)
    w = np.ones(1, F)
    assert lib.xrt_focal_spot(None, 1.0, 1.0, 1, 1, ctypes.byref(cam), w.ctypes.data_as(_abi._fp)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_focal_spot(ctypes.byref(cam), 1.0, 1.0, 1, 1, None, w.ctypes.data_as(_abi._fp)) == _abi.XRT_ERR_ARGUMENT
    assert lib.xrt_focal_spot(ctypes.byref(cam), 1.0, 1.0, 1, 1, ctypes.byref(cam), None) == _abi.XRT_ERR_ARGUMENT
    with pytest.raises(ValueError):
        xrt.host_area_integrate(np.zeros((5, 5), F), 2)
    with pytest.raises(ValueError):
        xrt.host_area_integrate(np.zeros((2, 4, 4), F), 2, [1.0])
    with pytest.raises(xrt.XrtError):
        xrt.host_area_integrate(np.zeros((2, 4, 4), F), 2, [0.0, 0.0])


# --------------------------------------------------------------------------- physics, through the oracle alone
# Powers of two throughout, so that the tracer's f32 hit distances are exact: rays within 1.6e-4 rad of the axis reach
# the faces at 512 (1 + 1.3e-8), which rounds to 512, and the plate's path length is 1.0 for every ray through both
# faces -- the image has exactly two plateaus, 80 and 80 expf(-0.03971).
D_DETECTOR = 1024.0             # source to detector
SPACING = 1.0 / 256.0           # a 0.25 wide detector
THICKNESS = 1.0
EDGE = 0.0005                   # the plate covers x >= EDGE: its shadow's edge lies off every sample's centre
DISTANCES = [512.0, 256.0]      # source to the plate's front face: magnifications 2 and 4
SPOTS = [4 * SPACING, 8 * SPACING]


def plate(d):
    """A closed box of 12 triangles, normal to the beam axis z, front face at distance d, covering x >= EDGE."""
    x0, x1, y0, y1, z0, z1 = EDGE, 60.0, -45.0, 50.0, d, d + THICKNESS
    v = [(x, y, z) for z in (z0, z1) for y in (y0, y1) for x in (x0, x1)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([v[a] + v[b] + v[c] for q in quads for a, b, c in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], F)


def plate_camera(W=64, H=4):
    cam = xrt.Camera()
    for k, (o, d, u, r) in enumerate(zip((0, 0, 0), (0, 0, D_DETECTOR), (0, 1, 0), (1, 0, 0))):
        cam.origin[k], cam.detector[k], cam.up[k], cam.right[k] = o, d, u, r
    cam.pixel_spacing, cam.width, cam.height = SPACING, W, H
    return cam


def cam13(cam):
    return np.array(list(cam.origin) + list(cam.detector) + list(cam.up) + list(cam.right) + [cam.pixel_spacing], F)


def oracle_render(tris, cam):
    from oracle import oracle
    return oracle.render_rows(tris, cam13(cam), cam.width, cam.height)[0].reshape(cam.height, cam.width)


def plate_spot_reference(d, size_u, n):
    """area_ref over the oracle's renders of a line spot's n sub-cameras."""
    cams, w = xrt.focal_spot(plate_camera(), size_u, 0.0, n, 1)
    return area_ref.integrate(np.stack([oracle_render(plate(d), c) for c in cams]), 1, w)


def transition_width(row):
    """Pixels strictly between the plateaus.  The plateaus are the row's two extremes; a mean over k of n
    sub-sources lies at least (hi - lo) / n = 0.6 from both for n = 5, so a relative 1e-4 separates them."""
    lo, hi = float(row.min()), float(row.max())
    return int(np.count_nonzero((row > lo * (1 + 1e-4)) & (row < hi * (1 - 1e-4))))


@pytest.mark.parametrize("d", DISTANCES)
@pytest.mark.parametrize("size_u", SPOTS)
def test_penumbra_width(d, size_u):
    """An edge at magnification M = D / d under a line spot of n sub-sources spread over size_u (n - 1) / n throws
    a penumbra of that times (M - 1); counted in pixels, within one of it."""
    n = 5
    img = plate_spot_reference(d, size_u, n)
    want = size_u * (n - 1) / n * (D_DETECTOR - d) / d / SPACING
    for row in img:
        got = transition_width(row)
        print(d, size_u, got, want)
        assert abs(got - want) <= 1.0
        assert row[0] == F(80.0) and row[-1] < F(77.0)
    point = plate_spot_reference(d, size_u, 1)
    assert all(transition_width(row) <= 1 for row in point)
    assert np.array_equal(bits(point), bits(oracle_render(plate(d), plate_camera())))


def test_supersampled_silhouette():
    """The plate at d = 512 under a point source, supersampled by 4: the edge's shadow falls at x = 0.001, inside
    pixel 32 (0 to 1/256), between its first and second columns of samples; that pixel is the mean of its 16 oracle samples and every other pixel keeps the plain render's bits."""
    cam = plate_camera()
    tris = plate(DISTANCES[0])
    plain = oracle_render(tris, cam)
    fine = oracle_render(tris, xrt.supersampled_camera(cam, 4))
    got = xrt.host_area_integrate(fine, 4)
    assert np.array_equal(bits(got), bits(area_ref.integrate(fine, 4)))
    lo, hi = F(plain.min()), F(80.0)
    for y in range(cam.height):
        block = fine[4 * y:4 * y + 4, 128:132].astype(np.float64)
        assert got[y, 32] == F(block.sum() / 16.0) and lo < got[y, 32] < hi
        assert 0 < np.count_nonzero(block == 80.0) < 16
    away = np.ones(cam.width, bool)
    away[32] = False
    assert np.array_equal(bits(got[:, away]), bits(plain[:, away]))
    assert (plain[:, :32] == hi).all() and (plain[:, 32:] == lo).all()


# --------------------------------------------------------------------------- symbols, metadata, CLI, sanitizers
def test_symbols_are_declared_and_bound():
    """The pass and the helpers in xrt.h, the hook in xrt_debug.h only; every one bound; the ABI version stays."""
    pub = open(os.path.join(ROOT, "include", "xrt.h")).read()
    dbg = open(os.path.join(ROOT, "include", "xrt_debug.h")).read()
    for name in ("xrt_area_integrate(", "xrt_area_integrate_device(", "xrt_camera_supersample(", "xrt_focal_spot(",
                 "#define XRT_MAX_SOURCES 64", "#define XRT_MAX_BIN 8"):
        assert name in pub
    assert pub.index("xrt_photon_noise_device(") < pub.index("xrt_area_integrate(") < pub.index("xrt_multi_create")
    assert "xrt_host_area_integrate(" in dbg and "xrt_host_area_integrate" not in pub
    for name in ("xrt_area_integrate", "xrt_area_integrate_device", "xrt_host_area_integrate", "xrt_camera_supersample",
                 "xrt_focal_spot"):
        assert name in _abi.XRT_SYMBOLS
    assert _abi.load().xrt_abi_version() == 5 and "#define XRT_ABI_VERSION 5" in pub
    assert (_abi.XRT_MAX_SOURCES, _abi.XRT_MAX_BIN) == (64, 8)
    assert not [name for name in _abi.XRT_SYMBOLS if name.startswith("xrt_multi_") and "area" in name]


def test_k_area_integrate_metadata():
    """k_area_integrate's instantiations in the gfx950 code object: no scratch, no spills, no LDS, <= 128 VGPRs;
    k_probe_math, k_lsf and k_photon_noise stay one kernel each."""
    meta = _render_kernel_metadata()
    area = {k: v for k, v in meta.items() if "k_area_integrate" in k}
    assert len(area) == 10, sorted(meta)                                      # bin_x 0 (any), 1, 2, 4, 8; narrow and wide
    for name, f in area.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (name, f)
        assert f["group_segment_fixed_size"] == 0 and f["vgpr_count"] <= 128, (name, f)
    for one in ("k_probe_math", "k_lsf", "k_photon_noise"):
        assert len([k for k in meta if one + "E" in k]) == 1, one


def test_cli_help_lists_the_options():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--supersample B" in r.stderr and "--focal-spot UxV[:NUxNV]" in r.stderr


@pytest.mark.parametrize("args,word", [
    (["--supersample", "0"], "--supersample"),
    (["--supersample", "9"], "--supersample"),
    (["--supersample", "-2"], "--supersample"),
    (["--supersample", "2x"], "--supersample"),
    (["--supersample", "1.5"], "--supersample"),
    (["--focal-spot", "1"], "--focal-spot"),
    (["--focal-spot", "1x"], "--focal-spot"),
    (["--focal-spot", "1x-1"], "--focal-spot"),
    (["--focal-spot", "nanx1"], "--focal-spot"),
    (["--focal-spot", "1xinf"], "--focal-spot"),
    (["--focal-spot", "1x1x1"], "--focal-spot"),
    (["--focal-spot", "1x1:3"], "--focal-spot"),
    (["--focal-spot", "1x1:0x3"], "--focal-spot"),
    (["--focal-spot", "1x1:9x8"], "--focal-spot"),
    (["--focal-spot", "1x1:3x3:1"], "--focal-spot"),
    (["--supersample", "2", "-g", "2"], "--supersample"),
    (["--supersample", "2", "--rows", "0:4"], "--supersample"),
    (["--supersample", "2", "--batch", "3"], "--supersample"),
    (["--supersample", "2", "--paths"], "--supersample"),
    (["--supersample", "2", "--lbuffer", "l.raw"], "--supersample"),
    (["--focal-spot", "1x1", "-g", "2"], "--focal-spot"),
    (["--focal-spot", "1x1", "--rows", "0:4"], "--focal-spot"),
    (["--focal-spot", "1x1", "--batch", "3"], "--focal-spot"),
    (["--focal-spot", "1x1", "--paths"], "--focal-spot"),
    (["--focal-spot", "1x1", "--lbuffer", "l.raw"], "--focal-spot"),
])
def test_cli_errors(tmp_path, args, word):
    """Each is an error before any device is opened: exit 1, stderr 'ERROR: ...' naming the option."""
    r = subprocess.run([EXE, "-s", "16", "16", "-i", DRAGON] + args, capture_output=True, text=True, cwd=tmp_path,
                       timeout=120)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert r.stderr.startswith("ERROR:") and word in r.stderr and "xrt_create" not in r.stderr, r.stderr


def test_host_code_under_sanitizers(tmp_path):
    """tools/area_san.cpp: a stand-alone program over csrc/xrt_area_host.inc (the checks, the helpers, the pass over
    ragged sizes, every bin and the longest source loop) with AddressSanitizer and UBSan.  Nothing is loaded into
    Python."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc) or not _sanitizer_runtime(hipcc):
        pytest.skip("no host sanitizer runtime beside hipcc")
    exe = str(tmp_path / "area_san")
    b = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-O1", "-g", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "simpleraytracing_amd", "csrc"),
                        os.path.join(ROOT, "tools", "area_san.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "area_san: OK" in r.stdout, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out, out[-3000:]
