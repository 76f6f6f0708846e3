"""CPU: general cameras (tests/camera_kit.py) -- rolled, pitched, skewed,
anisotropic, mirrored and off-centre, up and right mixing on one axis.  The
oracle against the reference's own compiled classes under them, the cull's
direction grid against a float32 restatement of
make_ray, and the footprints of the cull, compiled for the host, against every
hit the oracle reports.  No device."""
import ctypes

import numpy as np
import pytest

from simpleraytracing_amd import _abi
from oracle import oracle
from conftest import bits
import camera_kit as ck
from scene_kit import corner_soup, striped_sheets, synthetic_soup

W0, H0 = 67, 45
SIZES = [(64, 48), (67, 45), (512, 512)]


@pytest.fixture(scope="module")
def REF():
    """The reference's own compiled classes (oracle/_ref), mapped only by the
    CPU tests that use them; skipped where it has not been built."""
    r = oracle.ref_lib()
    if r is None:
        pytest.skip("oracle/_ref not built (needs the reference tree)")
    return r


@pytest.fixture(scope="module")
def scenes(dragon):
    return {"dragon": dragon, "soup": synthetic_soup(), "sheets": striped_sheets()}


# --------------------------------------------------------------------------- a. the oracle
@pytest.mark.parametrize("scene", ["dragon", "soup", "sheets"])
@pytest.mark.parametrize("case", ck.NAMES)
def test_oracle_equals_reference_classes(REF, scenes, case, scene):
    """oracle.render_rows under every general camera equals the same loop over
    the reference's compiled classes, image and L-buffer bit for bit; every
    case keeps the scene in view (and the open scenes' odd rays)."""
    tris = scenes[scene]
    cam = ck.case_camera(case, [tris], W0, H0)
    img, lb, u8, nh, odd = oracle.render_rows(tris, cam, W0, H0)
    r_img, r_lb, r_odd = oracle.ref_render_spans(tris, cam, W0, H0, range(H0), threads=4)
    assert np.array_equal(bits(r_img.ravel()), bits(img))
    assert np.array_equal(bits(r_lb.ravel()), bits(lb))
    assert r_odd == odd
    assert np.count_nonzero(nh) > 0
    if scene != "dragon":
        assert odd > 0


@pytest.mark.parametrize("case", ["roll30", "all"])
def test_signed_oracle_equals_reference_classes(REF, case):
    sheets = [striped_sheets()]
    cam = ck.case_camera(case, sheets, W0, H0)
    lb, nh, flagged = oracle.render_signed_rows(sheets, cam, W0, H0)
    lbr, flr = oracle.ref_render_signed_rows(sheets, cam, W0, H0)
    assert np.array_equal(bits(lb), bits(lbr))
    assert flagged == flr and flagged > 0


# --------------------------------------------------------------------------- b. the direction grid
def library_grid(c13, W, H):
    grids = (ctypes.c_int * 2)()
    cam = ck.as_camera(c13, W, H)
    assert _abi.load().xrt_debug_direction_grid(ctypes.byref(cam), grids) == 0
    return grids[0]


def test_make_ray_restatement_is_the_oracles(dragon):
    """The float32 restatement the grid is measured with sees the oracle's rays:
    a triangle placed on a pixel's ray is hit by that pixel."""
    cam = ck.case_camera("all", [dragon], W0, H0)
    d = ck.ray_directions(cam, W0, H0)
    assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=2) - 1.0) < 1e-6)
    o = cam[0:3].astype(np.float64)
    for row, col in [(0, 0), (7, 61), (44, 66), (22, 33)]:
        p = o + 50.0 * d[row, col].astype(np.float64)
        a, b = np.cross(d[row, col], [0.3, 0.5, 0.7]), np.cross(d[row, col], [0.9, -0.2, 0.1])
        tri = np.concatenate([p + 1e-3 * (a + b), p + 1e-3 * (-a + b), p - 2e-3 * b]).astype(np.float32)[None, :]
        px, _ = oracle.hit_pairs(tri, cam, W0, H0, np.arange(H0, dtype=np.uint32))
        assert row * W0 + col in px


@pytest.mark.parametrize("case", ck.NAMES)
def test_direction_grid_sound_under_general_cameras(dragon, case):
    """Every nonzero component of every ray direction of the image is a
    multiple of 2^dir_grid: the library's grid is not above the smallest
    lowest-set-bit exponent found over all pixels."""
    for W, H in SIZES:
        cam = ck.case_camera(case, [dragon], W, H)
        got, actual = library_grid(cam, W, H), ck.actual_direction_grid(cam, W, H)
        assert got <= actual, (W, H, got, actual)


def test_direction_grid_sound_on_random_mixed_cameras():
    """The same on 300 random cameras with every component of up and right
    nonzero (the mixed branch on all three axes)."""
    rng = np.random.default_rng(20251020)
    for i in range(300):
        cam, W, H = ck.random_general_camera(rng, 200)
        got, actual = library_grid(cam, W, H), ck.actual_direction_grid(cam, W, H)
        assert got <= actual, (i, list(cam), W, H, got, actual)


def never_culled_by_step0(tris, grid):
    """Triangles compute_footprint's step 0 gives up on: g1 + grid + g2 < -127."""
    t = np.asarray(tris, np.float32)
    g1 = ck.grid_exp(t[:, 3:6] - t[:, 0:3]).min(axis=1)
    g2 = ck.grid_exp(t[:, 6:9] - t[:, 0:3]).min(axis=1)
    return int(np.count_nonzero(g1 + grid + g2 < -127))


@pytest.mark.parametrize("case", ck.NAMES)
def test_direction_grid_tight_under_general_cameras(dragon, case):
    """The grid is tight enough for the cull to work: step 0 of
    compute_footprint gives up on no triangle of the dragon under any general
    camera (with the exact grid the count is 0 in every case)."""
    for W, H in SIZES:
        cam = ck.case_camera(case, [dragon], W, H)
        assert never_culled_by_step0(dragon, ck.actual_direction_grid(cam, W, H)) == 0, (W, H)
        grid = library_grid(cam, W, H)
        assert never_culled_by_step0(dragon, grid) == 0, (W, H, grid)


# --------------------------------------------------------------------------- c. the footprints, on the host
def host_footprints(c13, W, H, tris):
    tris = np.ascontiguousarray(tris, np.float32)
    fp = np.zeros((len(tris), 16), np.float32)
    cam = ck.as_camera(c13, W, H)
    assert _abi.load().xrt_host_footprints(ctypes.byref(cam), tris.ctypes.data_as(_abi._fp), len(tris),
                                           fp.ctypes.data_as(_abi._fp)) == 0
    return fp


def assert_footprints_contain_hits(fp, tris, c13, W, H):
    """test_footprints_contain_every_hit's assertions (f32, box and three
    edges) over every row; returns the number of hit pairs."""
    px, tri = oracle.hit_pairs(tris, c13, W, H, np.arange(H, dtype=np.uint32))
    row = (px // W).astype(np.float32)
    col = (px % W).astype(np.float32)
    f = fp[tri]
    box_miss = ~((f[:, 0] <= col) & (col <= f[:, 1]) & (f[:, 2] <= row) & (row <= f[:, 3]))
    assert not box_miss.any(), (int(box_miss.sum()), tri[box_miss][:8], px[box_miss][:8])
    with np.errstate(invalid="ignore"):
        for k in range(3):
            a, b, c = f[:, 4 + 4 * k], f[:, 5 + 4 * k], f[:, 6 + 4 * k]
            miss = ~(a * col + b * row + c >= 0)
            assert not miss.any(), (k, int(miss.sum()), tri[miss][:8], px[miss][:8])
    return len(px)


def never_cull(fp):
    """Footprints compute_footprint gave up on: an unbounded box and three
    edges that always pass."""
    return ((fp[:, 0] == -np.inf) & (fp[:, 1] == np.inf) & (fp[:, 2] == -np.inf) & (fp[:, 3] == np.inf) &
            (fp[:, 6] == np.inf) & (fp[:, 10] == np.inf) & (fp[:, 14] == np.inf))


def footprint_scene(name, dragon):
    """(triangles, W, H, base camera, centre of the turn)."""
    if name == "dragon":
        tris, W, H = dragon, W0, H0
    elif name == "soup":
        tris, W, H = synthetic_soup(), W0, H0
    elif name == "sheets":
        tris, W, H = striped_sheets(), W0, H0
    elif name == "corner":
        tris, W, H = corner_soup(), 33, 31
    else:                                       # the source inside the soup
        tris, W, H = synthetic_soup(), 64, 48
        return tris, W, H, ck.inside_source_camera(tris, W, H), ck.scene_centre([tris[:200]])
    return tris, W, H, oracle.camera_for_mesh(tris, W, H), ck.scene_centre([tris])


FOOTPRINT_SCENES = ["dragon", "soup", "sheets", "corner", "inside"]


@pytest.mark.parametrize("scene", FOOTPRINT_SCENES)
@pytest.mark.parametrize("case", ck.NAMES)
def test_host_footprints_contain_every_hit(dragon, case, scene):
    """Every (pixel, triangle) pair the oracle reports under a general camera
    lies inside the triangle's footprint box and passes its three relaxed
    edges; the dragon has no footprint the cull gave up on."""
    tris, W, H, base, centre = footprint_scene(scene, dragon)
    cam = ck.general_camera(base, centre, W, H, **ck.CASES[case])
    fp = host_footprints(cam, W, H, tris)
    assert assert_footprints_contain_hits(fp, tris, cam, W, H) > 0
    if scene == "dragon":
        assert not never_cull(fp).any()


def test_host_footprints_base_cameras(dragon):
    """The same under the scenes' own cameras (the device's footprints of these
    are checked by the GPU suite)."""
    for scene in FOOTPRINT_SCENES:
        tris, W, H, base, _ = footprint_scene(scene, dragon)
        fp = host_footprints(base, W, H, tris)
        assert assert_footprints_contain_hits(fp, tris, base, W, H) > 0, scene
    assert not never_cull(host_footprints(oracle.camera_for_mesh(dragon, 512, 512), 512, 512, dragon)).any()


def test_host_footprints_random_general_cameras():
    """60 random general cameras over a soup, 1 to 90 pixels a side."""
    tris = synthetic_soup(seed=9, n=800)
    centre = ck.scene_centre([tris])
    rng = np.random.default_rng(20251021)
    pairs = 0
    for i in range(60):
        W, H = (int(v) for v in rng.integers(1, 91, 2))
        params = dict(yaw=rng.uniform(-180, 180), pitch=rng.uniform(-90, 90), roll=rng.uniform(-180, 180),
                      skew=rng.uniform(-0.5, 0.5), su=rng.choice([-1, 1]) * rng.uniform(0.5, 2.0),
                      sv=rng.choice([-1, 1]) * rng.uniform(0.5, 2.0), shift_u=rng.uniform(-0.4, 0.4),
                      shift_v=rng.uniform(-0.4, 0.4), src_u=rng.uniform(-0.2, 0.2), src_v=rng.uniform(-0.2, 0.2))
        cam = ck.general_camera(oracle.camera_for_mesh(tris, W, H), centre, W, H, **params)
        pairs += assert_footprints_contain_hits(host_footprints(cam, W, H, tris), tris, cam, W, H)
    assert pairs > 1000
