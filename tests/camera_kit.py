"""General cameras (test-only): a base camera turned about the scene's centre
by yaw, pitch and roll, with a skewed, anisotropic, mirrored or off-centre
detector -- cameras whose up and right vectors mix on one axis, which
xrt_camera_from_bbox and orbit_camera never produce.  Shared by the CPU and
GPU suites; also a float32 restatement of make_ray for the direction grid."""
import numpy as np

import simpleraytracing_amd as xrt


def _rodrigues(v, axis, deg):
    """v turned about the unit axis by deg degrees (f64)."""
    k = axis / np.linalg.norm(axis)
    t = np.radians(deg)
    return v * np.cos(t) + np.cross(k, v) * np.sin(t) + k * np.dot(k, v) * (1.0 - np.cos(t))


def general_camera(base13, centre, W, H, yaw=0.0, pitch=0.0, roll=0.0, skew=0.0, su=1.0, sv=1.0,
                   shift_u=0.0, shift_v=0.0, src_u=0.0, src_v=0.0):
    """The 13 float32 values (origin, detector, up, right, spacing) of base13
    after, in f64 and in this order: a turn of origin, detector, up and right
    about centre by yaw about up, by pitch about the new right, by roll about
    the new detector - origin; the detector moved by (shift_u W, shift_v H)
    pixels and the source by (src_u W, src_v H) pixels along right and up;
    right = su (right + skew up), up = sv up."""
    b = np.asarray(base13, np.float64)
    centre = np.asarray(centre, np.float64)
    origin, detector, up, right, ps = b[0:3], b[3:6], b[6:9], b[9:12], b[12]
    for deg, axis_of in ((yaw, lambda: up), (pitch, lambda: right), (roll, lambda: detector - origin)):
        axis = np.array(axis_of())
        origin = centre + _rodrigues(origin - centre, axis, deg)
        detector = centre + _rodrigues(detector - centre, axis, deg)
        up = _rodrigues(up, axis, deg)
        right = _rodrigues(right, axis, deg)
    detector = detector + shift_u * W * ps * right + shift_v * H * ps * up
    origin = origin + src_u * W * ps * right + src_v * H * ps * up
    right = su * (right + skew * up)
    up = sv * up
    return np.concatenate([origin, detector, up, right, [ps]]).astype(np.float32)


CASES = {
    "roll30": dict(roll=30),
    "roll45": dict(roll=45),
    "roll90": dict(roll=90),
    "pitch25": dict(pitch=25),
    "pitch90": dict(pitch=90),
    "yaw33_pitch20_roll17": dict(yaw=33, pitch=20, roll=17),
    "skew": dict(skew=0.35, roll=10),
    "aniso": dict(su=1.5, sv=0.7, roll=-20),
    "mirror": dict(su=-1, pitch=12),
    "offaxis": dict(shift_u=0.3, shift_v=-0.2, src_u=-0.1, src_v=0.15, roll=7, pitch=5),
    "all": dict(yaw=-40, pitch=15, roll=63, skew=-0.2, su=1.2, sv=0.9, shift_u=0.1, shift_v=0.1),
}
NAMES = list(CASES)


def as_camera(c13, W, H):
    """xrt.Camera of 13 float32 values and an image size."""
    c13 = np.asarray(c13, np.float32)
    cam = xrt.Camera()
    cam.origin[:] = [float(x) for x in c13[0:3]]
    cam.detector[:] = [float(x) for x in c13[3:6]]
    cam.up[:] = [float(x) for x in c13[6:9]]
    cam.right[:] = [float(x) for x in c13[9:12]]
    cam.pixel_spacing = float(c13[12])
    cam.width, cam.height = int(W), int(H)
    return cam


def cam13(cam):
    return np.array(list(cam.origin) + list(cam.detector) + list(cam.up) + list(cam.right) +
                    [cam.pixel_spacing], np.float32)


def scene_centre(meshes):
    from oracle import oracle
    lo, hi = oracle.scene_bbox(meshes)
    return 0.5 * (np.asarray(lo, np.float64) + np.asarray(hi, np.float64))


def case_camera(name, meshes, W, H, base13=None):
    """CASES[name] applied to the scene's own camera (or base13) about the
    centre of the scene's bounding box: 13 float32 values."""
    from oracle import oracle
    if base13 is None:
        base13 = oracle.camera_for_scene(meshes, W, H)
    return general_camera(base13, scene_centre(meshes), W, H, **CASES[name])


def inside_source_camera(soup, W, H):
    """The camera fitted to the first 200 triangles of the soup: its source
    lies inside the whole soup."""
    from oracle import oracle
    return oracle.camera_for_mesh(soup[:200], W, H)


def random_general_camera(rng, max_side):
    """A camera with every component of up and right nonzero: scales 1e-3, 1
    and 100, spacing of either sign, 1..max_side pixels a side."""
    W, H = (int(v) for v in rng.integers(1, max_side + 1, 2))
    c = np.zeros(13, np.float32)
    for k in range(4):
        v = rng.normal(0.0, float(rng.choice([1e-3, 1.0, 100.0])), 3).astype(np.float32)
        if k >= 2:
            v[v == 0] = np.float32(1e-3)
        c[3 * k:3 * k + 3] = v
    c[12] = np.float32(rng.choice([1e-4, 0.01, 0.3, -0.05]))
    return c, W, H


# --------------------------------------------------------------------------- make_ray in float32
def pixel_offsets(ps, n):
    """make_ray's pixel offsets: f64 arithmetic narrowed to f32."""
    i = np.arange(n, dtype=np.float64)
    return (np.float64(np.float32(ps)) * ((0.5 + i) - np.float64(n) / 2.0)).astype(np.float32)


def ray_directions(c13, W, H):
    """Every pixel's ray direction as make_ray and the Ray constructor form it,
    (H, W, 3) float32: ((detector + up v) + right u) - origin with every f32
    operation rounded on its own, then normalised twice (the second time only
    where the length is not zero)."""
    c = np.asarray(c13, np.float32)
    v = pixel_offsets(c[12], H)[:, None]
    u = pixel_offsets(c[12], W)[None, :]
    with np.errstate(all="ignore"):
        d = np.empty((H, W, 3), np.float32)
        for k in range(3):
            d[:, :, k] = ((c[3 + k] + c[6 + k] * v) + c[9 + k] * u) - c[k]

        def length(a):
            return np.sqrt((a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2])
        d = d / length(d)[..., None]
        ln = length(d)
        d = np.where((ln == 0)[..., None], np.float32(0), d / ln[..., None])
    assert d.dtype == np.float32
    return d


def grid_exp(x):
    """Exponent of the lowest set bit of each float32 (x is a multiple of
    2^grid_exp(x)); 1000 for zero, NaN and infinities."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.int64)
    e = (u >> 23) & 0xFF
    m = (u & 0x7FFFFF) | np.where(e != 0, 0x800000, 0)
    low = m & -m
    tz = np.zeros(m.shape, np.int64)
    nz = low > 0
    tz[nz] = np.round(np.log2(low[nz])).astype(np.int64)
    g = np.where(e != 0, e - 150, -149) + tz
    return np.where((m == 0) | (e == 255), 1000, g)


def actual_direction_grid(c13, W, H):
    """The smallest grid_exp over every nonzero finite direction component of
    the image (1000 when there is none)."""
    return int(grid_exp(ray_directions(c13, W, H)).min())
