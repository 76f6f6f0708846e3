"""GPU: general cameras (tests/camera_kit.py) -- rolled, pitched, skewed,
anisotropic, mirrored and off-centre, up and right mixing on one axis --
through every render kernel, the cull's device footprints, a moving general
camera and row strips, against the CPU oracle bit for bit.  Tiny frames."""
import ctypes

import numpy as np
import pytest

import camera_kit as ck
import materials_ref
import simpleraytracing_amd as xrt
from simpleraytracing_amd import _abi
from oracle import oracle
from camera_refs import reference
from conftest import bits
from scene_kit import second_mesh_for, striped_sheets, synthetic_soup
from test_camera_cpu import assert_footprints_contain_hits, host_footprints, never_cull
from test_gpu_parity import KERNELS, KNAME, assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def references(dragon):
    """The oracle's frame of every (scene, case), computed once and shared
    (camera_refs: with the ray table's suite too)."""
    return lambda name, case: reference(name, case, dragon)


# --------------------------------------------------------------------------- a. parity
@pytest.mark.parametrize("name", ["dragon", "soup", "corner", "inside"])
@pytest.mark.parametrize("case", ck.NAMES)
def test_general_camera_parity(ctx, references, case, name):
    """Every kernel's frame under a general camera equals the oracle's: image,
    L-buffer, u8 and hit statistics, bit for bit."""
    tris, W, H, c13, ref = references(name, case)
    assert np.count_nonzero(ref[3]) > 0
    if name == "corner" and case in ("roll45", "pitch25", "mirror"):
        assert np.isnan(ref[1]).sum() > 10                # hits at infinity: NaN path lengths
    ctx.upload_mesh(tris)
    for kernel in KERNELS:
        ctx.set_kernel(kernel)
        assert_same(ctx.render_rows(ck.as_camera(c13, W, H)), ref, f"{KNAME[kernel]} {name} {case}")
    ctx.set_kernel(xrt.XRT_KERNEL_AUTO)


@pytest.mark.parametrize("kernel", KERNELS)
def test_general_camera_ragged_strip(ctx, dragon, kernel):
    W, H, r0, r1 = 100, 37, 5, 30
    c13 = ck.case_camera("all", [dragon], W, H)
    ctx.set_kernel(kernel)
    ctx.upload_mesh(dragon)
    assert_same(ctx.render_rows(ck.as_camera(c13, W, H), r0, r1), oracle.render_rows(dragon, c13, W, H, r0, r1))
    ctx.set_kernel(xrt.XRT_KERNEL_AUTO)


@pytest.fixture
def signed(ctx):
    ctx.set_model(xrt.XRT_MODEL_SIGNED, 0.1037)
    try:
        yield ctx
    finally:
        ctx.set_model(xrt.XRT_MODEL_ATTENUATION, 0.0)
        ctx.set_kernel(xrt.XRT_KERNEL_AUTO)


@pytest.mark.parametrize("case", ["roll30", "all"])
def test_general_camera_signed_model(signed, case):
    """The signed model on the striped sheets, 96 x 80, by the kernels that
    render it (BRUTE and BINNED; TILED refuses the model)."""
    meshes, W, H = [striped_sheets()], 96, 80
    c13 = ck.case_camera(case, meshes, W, H)
    rlb, rnh, flagged = oracle.render_signed_rows(meshes, c13, W, H)
    assert flagged > 0
    rimg = oracle.hole_fill(rlb, W, H)
    signed.upload_mesh(meshes[0])
    for kernel in (xrt.XRT_KERNEL_BRUTE, xrt.XRT_KERNEL_BINNED):
        signed.set_kernel(kernel)
        img, lb, u8, st = signed.render_signed(ck.as_camera(c13, W, H))
        assert np.array_equal(bits(lb), bits(rlb)), (KNAME[kernel], np.nonzero(bits(lb) != bits(rlb))[0][:8])
        assert np.array_equal(bits(img), bits(rimg))
        assert np.array_equal(u8, oracle.lut_u8_array(rimg))
        assert st.odd_rays == flagged and st.hits == int(rnh.sum()) and st.hit_rays == int(np.count_nonzero(rnh))
    signed.set_kernel(xrt.XRT_KERNEL_TILED)
    with pytest.raises(xrt.XrtError):
        signed.render_signed(ck.as_camera(c13, W, H))


@pytest.mark.parametrize("kernel", [xrt.XRT_KERNEL_BRUTE, xrt.XRT_KERNEL_BINNED])
def test_general_camera_materials(dragon, kernel):
    """Two meshes with their own coefficients under the off-axis camera."""
    meshes, mu, W, H = [dragon, second_mesh_for(dragon)], [0.1037, 0.3971], 67, 45
    c13 = ck.case_camera("offaxis", meshes, W, H)
    ref = materials_ref.render(meshes, mu, c13, W, H)
    assert np.count_nonzero(ref.mesh_hits[:, 1]) > 0          # the second mesh is in view
    rimg = oracle.hole_fill(ref.lbuffer, W, H)
    with xrt.Context(0) as c:
        c.set_kernel(kernel)
        c.upload_scene(meshes)
        c.set_materials(mu)
        img, lb, u8, st = c.render_materials(ck.as_camera(c13, W, H))
    assert np.array_equal(bits(lb), bits(ref.lbuffer))
    assert np.array_equal(bits(img), bits(rimg)) and np.array_equal(u8, oracle.lut_u8_array(rimg))
    assert st.odd_rays == ref.flagged
    assert st.hits == int(ref.nhits.sum()) and st.hit_rays == int(np.count_nonzero(ref.nhits))


# --------------------------------------------------------------------------- b. device footprints
def footprint_class(fp):
    """0 culled (an empty box), 1 never culled, 2 without a bounded box, 3 boxed."""
    culled = fp[:, 0] > fp[:, 1]
    boxed = np.isfinite(fp[:, 0:4]).all(axis=1) & ~culled
    return np.where(culled, 0, np.where(never_cull(fp), 1, np.where(boxed, 3, 2)))


def assert_device_matches_host(fp, hfp, what):
    """Device and host footprints: the same class per triangle; the relaxed
    edges' a, b within 2^-20 and c within 2^-20 (|c| + 8).  (v_rsq_f32 is within
    1 ulp, 2^-23 relative, of the host's correctly rounded 1 / sqrtf; a and b
    are at most 1 in magnitude and rounded once to f32, 2^-25; c scales with
    the same reciprocal, is rounded to f32 and carries 3.5 (|a| + |b|) <= 7,
    hence the 8: 2^-22 of each bound, with 4x slack.  Boxes are not compared:
    they are ill-conditioned for slivers.)"""
    cd, ch = footprint_class(fp), footprint_class(hfp)
    assert np.array_equal(cd, ch), (what, np.nonzero(cd != ch)[0][:8], cd[cd != ch][:8], ch[cd != ch][:8])
    live = cd >= 2
    for k in range(3):
        for j in (4 + 4 * k, 5 + 4 * k):
            d = np.abs(fp[live, j].astype(np.float64) - hfp[live, j])
            assert d.max(initial=0.0) <= 2.0 ** -20, (what, k, j, d.max())
        c, hc = fp[live, 6 + 4 * k].astype(np.float64), hfp[live, 6 + 4 * k].astype(np.float64)
        same_inf = np.isinf(c) & (c == hc)
        with np.errstate(invalid="ignore"):
            ok = same_inf | (np.abs(c - hc) <= 2.0 ** -20 * (np.abs(hc) + 8.0))
        assert ok.all(), (what, k, c[~ok][:4], hc[~ok][:4])


@pytest.mark.parametrize("name", ["dragon", "soup"])
@pytest.mark.parametrize("case", ck.NAMES)
def test_device_footprints_general_cameras(ctx, dragon, case, name):
    """k_prep's footprints under a general camera contain every hit the oracle
    reports, are of the host build's class per triangle and agree with its
    edges; the dragon has none the cull gave up on."""
    tris = dragon if name == "dragon" else synthetic_soup()
    W, H = 67, 45
    c13 = ck.case_camera(case, [tris], W, H)
    ctx.upload_mesh(tris)
    _, fp = ctx.probe_prep(ck.as_camera(c13, W, H), len(tris))
    assert assert_footprints_contain_hits(fp, tris, c13, W, H) > 0
    assert_device_matches_host(fp, host_footprints(c13, W, H, tris), (name, case))
    if name == "dragon":
        assert not never_cull(fp).any()


def test_no_dragon_footprint_is_never_cull_at_512(ctx, dragon):
    """k_prep only: at 512 x 512 too, no case leaves the cull a triangle of the
    dragon it gave up on (the base camera neither)."""
    W = H = 512
    ctx.upload_mesh(dragon)
    cams = {"base": oracle.camera_for_mesh(dragon, W, H)}
    cams.update({case: ck.case_camera(case, [dragon], W, H) for case in ck.NAMES})
    for case, c13 in cams.items():
        _, fp = ctx.probe_prep(ck.as_camera(c13, W, H), len(dragon))
        assert int(never_cull(fp).sum()) == 0, case
        assert_device_matches_host(fp, host_footprints(c13, W, H, dragon), case)


# --------------------------------------------------------------------------- c. counters (recorded)
def test_binned_counters_under_general_cameras(dragon):
    """BINNED on the dragon at 512 x 512: tile tests and candidates per ray for
    the base camera and each case, printed (DESIGN.md section 5 records them);
    each frame equals BRUTE's."""
    W = H = 512
    cams = {"base": oracle.camera_for_mesh(dragon, W, H)}
    cams.update({case: ck.case_camera(case, [dragon], W, H) for case in ck.NAMES})
    with xrt.Context(0) as binned, xrt.Context(0) as brute:
        binned.set_kernel(xrt.XRT_KERNEL_BINNED)
        brute.set_kernel(xrt.XRT_KERNEL_BRUTE)
        binned.upload_mesh(dragon)
        brute.upload_mesh(dragon)
        for case, c13 in cams.items():
            cam = ck.as_camera(c13, W, H)
            got, ref = binned.render_rows(cam), brute.render_rows(cam)
            st = got[3]
            print(f"counters {case}: tile_tests/ray {st.tile_tests / st.rays:.3f} candidates/ray "
                  f"{st.candidates / st.rays:.3f} hit_rays {st.hit_rays} global {st.global_triangles} "
                  f"kernel_ms {st.kernel_ms:.3f}")
            for x, y in zip(got[:3], ref[:3]):
                assert np.array_equal(bits(x), bits(y)), case
            assert st.hit_rays == ref[3].hit_rays and st.hits == ref[3].hits


# --------------------------------------------------------------------------- d. a moving general camera
def test_moving_general_camera(dragon):
    """One BINNED context over a sequence of general cameras of one image size
    (lists sized for an earlier camera are reused, re-sized when the camera
    stays put): every frame is bit-identical to a fresh BRUTE context's."""
    W, H = 160, 131
    base = oracle.camera_for_mesh(dragon, W, H)
    centre = ck.scene_centre([dragon])
    seq = [base, ck.case_camera("roll30", [dragon], W, H), ck.general_camera(base, centre, W, H, roll=31),
           ck.case_camera("roll45", [dragon], W, H)] + [ck.case_camera("roll90", [dragon], W, H)] * 3 + \
          [ck.case_camera("all", [dragon], W, H), base]
    with xrt.Context(0) as moving:
        moving.set_kernel(xrt.XRT_KERNEL_BINNED)
        moving.upload_mesh(dragon)
        for i, c13 in enumerate(seq):
            cam = ck.as_camera(c13, W, H)
            got = moving.render_rows(cam)
            with xrt.Context(0) as fresh:
                fresh.set_kernel(xrt.XRT_KERNEL_BRUTE)
                fresh.upload_mesh(dragon)
                ref = fresh.render_rows(cam)
            for x, y in zip(got[:3], ref[:3]):
                assert np.array_equal(bits(x), bits(y)), i
            for f in ("rays", "hit_rays", "odd_rays", "max_hits", "hits"):
                assert getattr(got[3], f) == getattr(ref[3], f), (i, f)
            assert got[3].hit_rays > 0


# --------------------------------------------------------------------------- e. strips
def test_multi_strips_general_camera(dragon):
    W, H = 160, 131
    cam = ck.as_camera(ck.case_camera("all", [dragon], W, H), W, H)
    with xrt.Context(0) as one:
        one.set_kernel(xrt.XRT_KERNEL_BINNED)
        one.upload_mesh(dragon)
        ref = one.render_rows(cam)
    assert ref[3].hit_rays > 0
    with xrt.MultiContext([0, 0]) as m:
        m.set_kernel(xrt.XRT_KERNEL_BINNED)
        m.upload_mesh(dragon)
        for _ in range(3):                              # the strip buffers rotate
            got = m.render(cam)
            for x, y in zip(got[:3], ref[:3]):
                assert np.array_equal(bits(x), bits(y))
            assert got[3].odd_rays == ref[3].odd_rays and got[3].hit_rays == ref[3].hit_rays
