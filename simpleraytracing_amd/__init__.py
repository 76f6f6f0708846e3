"""simpleraytracing_amd -- MI355X-native X-ray attenuation render path.

A drop-in for the reference's per-pixel ``renderLoop`` (Brandagot/
SimpleRayTracing, src/main.cxx:626-743): ray generation -> brute-force
Moller-Trumbore over the whole mesh -> L-buffer path length -> Beer-Lambert
shade -> image store, bit-identical to the serial CPU program.

The product is native: HIP kernels for gfx950 behind the C ABI of
``include/xrt.h`` (``lib/libxrt.so``) and the C++ host API of
``csrc/host`` (``lib/libxrt_host.so``, ``lib/xrt_main``).  This Python module is
thin plumbing over that ABI for tests, ``bench.py`` and scripting; it never
computes pixels itself.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _abi
from ._abi import (Camera, Stats, XRT_KERNEL_AUTO, XRT_KERNEL_BINNED,  # noqa: F401
                   XRT_KERNEL_BRUTE, XRT_KERNEL_TILED, XRT_MISS_TRANSIT, XRT_MODEL_ATTENUATION,
                   XRT_MODEL_SIGNED, XRT_MODEL_MATERIALS, XRT_MAX_MESHES, XRT_MODEL_SPECTRUM, XRT_MAX_BINS, XRT_MODEL_PATHS, XRT_MAX_LSF_TAPS, XRT_ORDER_PROJECTIONS, XRT_ORDER_SINOGRAMS, XRT_NOISE_INTENSITY, XRT_NOISE_COUNTS, XRT_MAX_SOURCES, XRT_MAX_BIN, XRT_MAX_RAMP_WIDTH, XRT_RAMP_RAMLAK, XRT_RAMP_HANN, XRT_FP_PROJECT, XRT_FP_RESIDUAL, XRT_MAX_SUBSETS, XRT_GATHER_AUTO, XRT_GATHER_COPY, XRT_GATHER_RCCL, XRT_SPLIT_EQUAL,
                   XRT_SPLIT_BALANCED, XRT_TRANSIT_HITS, XRT_TRANSIT_PACKED, XRT_MAX_BASIS, XRT_DECOMPOSE_MASKED,
                   XRT_DECOMPOSE_FAILED, XRT_MAX_SCATTER_BIN, XRT_MAX_SCATTER_KERNELS)

__all__ = [
    "Camera", "Stats", "Context", "MultiContext", "XrtError", "load_ply", "mesh_bbox", "camera_from_bbox",
    "camera_for_mesh", "device_count", "XRT_KERNEL_AUTO", "XRT_KERNEL_BRUTE", "XRT_KERNEL_TILED",
    "XRT_KERNEL_BINNED", "XRT_MISS_TRANSIT", "load_meshes", "scene_bbox", "camera_for_scene",
    "XRT_MODEL_ATTENUATION", "XRT_MODEL_SIGNED", "XRT_GATHER_AUTO", "XRT_GATHER_COPY", "XRT_GATHER_RCCL",
    "XRT_SPLIT_EQUAL", "XRT_SPLIT_BALANCED", "XRT_TRANSIT_HITS", "XRT_TRANSIT_PACKED", "XRT_MODEL_MATERIALS",
    "XRT_MAX_MESHES", "XRT_MODEL_SPECTRUM", "XRT_MAX_BINS", "XRT_MODEL_PATHS", "pose_rotation", "pose_triangles",
    "XRT_MAX_LSF_TAPS", "lsf_gaussian", "host_lsf", "detector_response",
    "XRT_ORDER_PROJECTIONS", "XRT_ORDER_SINOGRAMS", "host_logf", "host_log_projection", "log_projection",
    "XRT_NOISE_INTENSITY", "XRT_NOISE_COUNTS", "host_philox4x32", "host_poisson", "host_photon_noise", "photon_noise",
    "XRT_MAX_CHANNELS", "XRT_DETECT_EXPECTED", "XRT_DETECT_NOISY", "XRT_DETECT_COUNTS", "XRT_DETECT_INTENSITY",
    "host_spectral_detector", "spectral_detector", "volume_bbox", "host_volume_paths", "load_volume",
    "XRT_MAX_SOURCES", "XRT_MAX_BIN", "supersampled_camera", "focal_spot", "host_area_integrate", "area_integrate",
    "ray_table_index", "XRT_MAX_RAMP_WIDTH", "XRT_RAMP_RAMLAK", "XRT_RAMP_HANN", "ramp_filter", "fdk_weights",
    "fdk_scale", "backprojection_matrix", "save_volume", "host_fdk_filter", "host_backproject",
    "XRT_FP_PROJECT", "XRT_FP_RESIDUAL", "XRT_MAX_SUBSETS", "ray_matrix", "host_forward_project", "host_volume_update",
    "host_sirt", "host_tv_gradient", "host_volume_sumsq", "host_tv_descend",
    "XRT_MAX_BASIS", "XRT_DECOMPOSE_MASKED", "XRT_DECOMPOSE_FAILED", "decompose_guess", "host_decompose", "decompose",
    "host_voxelize",
    "XRT_MAX_SCATTER_BIN", "XRT_MAX_SCATTER_KERNELS", "host_scatter_source", "host_scatter_add", "scatter_gaussian",
    "scatter",
]


class XrtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"xrt error {code}: {message}")
        self.code = code


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _u8ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _u16ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))


def _i32ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _scene_arrays(meshes):
    """A list of (T, 9) soups as xrt_upload_scene takes it: (soups one after another, counts)."""
    meshes = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 9) for m in meshes]
    counts = np.array([len(m) for m in meshes], np.uint64)
    tris = np.ascontiguousarray(np.concatenate(meshes) if meshes else np.zeros((0, 9), np.float32))
    return tris, counts


def _spectrum_arrays(weights, mu):
    """K weights and an (M, K) table as xrt_set_spectrum takes them: (weight[K], mu[M, K] mesh-major)."""
    w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    mu = np.ascontiguousarray(mu, dtype=np.float32)
    if mu.ndim != 2 or mu.shape[1] != w.size:
        raise ValueError(f"mu must have shape (meshes, {w.size}), got {mu.shape}")
    return w, mu


def device_count() -> int:
    return _abi.load().xrt_device_count()


def load_ply(path: str) -> np.ndarray:
    """Mesh 0 of a PLY file as a (T, 9) float32 triangle soup (p1, p2, p3)."""
    host = _abi.load_host()
    p = ctypes.POINTER(ctypes.c_float)()
    n = ctypes.c_uint64()
    rc = host.xrt_host_load_ply(str(path).encode(), ctypes.byref(p), ctypes.byref(n))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, f"cannot load {path}")
    try:
        count = n.value
        out = np.ctypeslib.as_array(p, shape=(max(count, 1) * 9,))[: count * 9].copy()
    finally:
        host.xrt_host_free(ctypes.cast(p, ctypes.c_void_p))
    return out.reshape(count, 9)


def load_meshes(path: str) -> list:
    """Every mesh of a PLY (one) or OBJ (one per object) file, as (T, 9) float32 soups."""
    host = _abi.load_host()
    p = ctypes.POINTER(ctypes.c_float)()
    c = ctypes.POINTER(ctypes.c_uint64)()
    m = ctypes.c_uint32()
    rc = host.xrt_host_load_meshes(str(path).encode(), ctypes.byref(p), ctypes.byref(c), ctypes.byref(m))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, f"cannot load {path}")
    try:
        counts = [int(c[i]) for i in range(m.value)]
        total = sum(counts)
        flat = np.ctypeslib.as_array(p, shape=(max(total, 1) * 9,))[: total * 9].copy().reshape(total, 9)
    finally:
        host.xrt_host_free(ctypes.cast(p, ctypes.c_void_p))
        host.xrt_host_free(ctypes.cast(c, ctypes.c_void_p))
    out, first = [], 0
    for n in counts:
        out.append(flat[first:first + n])
        first += n
    return out


def scene_bbox(meshes):
    """getBBox over several meshes (src/main.cxx:538-563)."""
    meshes = [np.ascontiguousarray(m, dtype=np.float32).reshape(-1, 9) for m in meshes]
    counts = np.array([len(m) for m in meshes], np.uint64)
    tris = np.ascontiguousarray(np.concatenate(meshes) if meshes else np.zeros((0, 9), np.float32))
    lo = np.zeros(3, np.float32)
    hi = np.zeros(3, np.float32)
    rc = _abi.load().xrt_scene_bbox(_fptr(tris), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                    len(counts), _fptr(lo), _fptr(hi))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_scene_bbox")
    return lo, hi


def camera_for_scene(meshes, width: int, height: int) -> Camera:
    """The camera of a scene: from the box of every mesh (main.cxx:634)."""
    lo, hi = scene_bbox(meshes)
    return camera_from_bbox(lo, hi, width, height)


def mesh_bbox(tris: np.ndarray):
    tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    lo = np.zeros(3, np.float32)
    hi = np.zeros(3, np.float32)
    rc = _abi.load().xrt_mesh_bbox(_fptr(tris), len(tris), _fptr(lo), _fptr(hi))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_mesh_bbox")
    return lo, hi


def camera_from_bbox(lower, upper, width: int, height: int) -> Camera:
    lo = np.ascontiguousarray(lower, dtype=np.float32)
    hi = np.ascontiguousarray(upper, dtype=np.float32)
    cam = Camera()
    rc = _abi.load().xrt_camera_from_bbox(_fptr(lo), _fptr(hi), width, height, ctypes.byref(cam))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_camera_from_bbox")
    return cam


def camera_for_mesh(tris: np.ndarray, width: int, height: int) -> Camera:
    lo, hi = mesh_bbox(tris)
    return camera_from_bbox(lo, hi, width, height)


def _pose_array(pose):
    """A pose as xrt_set_pose takes it: 12 f32, row-major 3x4 [R | t] (None: the identity, a NULL pointer)."""
    if pose is None:
        return None
    q = np.ascontiguousarray(pose, dtype=np.float32).reshape(-1)
    if q.size != 12:
        raise ValueError(f"a pose has 12 values (3x4, row-major), got {q.size}")
    return q


def pose_rotation(axis, degrees: float, centre=(0.0, 0.0, 0.0)) -> np.ndarray:
    """The pose (12 f32) turning a mesh by `degrees` about `axis` through `centre` (xrt_pose_rotation)."""
    a = np.ascontiguousarray(axis, dtype=np.float32).reshape(3)
    c = np.ascontiguousarray(centre, dtype=np.float32).reshape(3)
    out = np.empty(12, np.float32)
    rc = _abi.load().xrt_pose_rotation(_fptr(a), float(degrees), _fptr(c), _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_pose_rotation: the axis must be finite and not zero")
    return out


def pose_triangles(tris: np.ndarray, pose) -> np.ndarray:
    """A (T, 9) soup under a pose, in the device's arithmetic on the host (xrt_pose_triangles)."""
    t = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
    q = _pose_array(pose)
    if q is None:
        return t.copy()
    out = np.empty_like(t)
    rc = _abi.load().xrt_pose_triangles(_fptr(t), len(t), _fptr(q), _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_pose_triangles")
    return out


def _lsf_arrays(lsf_x, lsf_y):
    """The taps as xrt_detector_response takes them (lsf_y None: lsf_x on both axes)."""
    hx = np.ascontiguousarray(lsf_x, dtype=np.float32).reshape(-1)
    hy = hx if lsf_y is None else np.ascontiguousarray(lsf_y, dtype=np.float32).reshape(-1)
    return hx, hy


def _lsf_planes(image):
    """An (H, W) image or a (P, H, W) stack as contiguous f32: (array, P, H, W)."""
    a = np.ascontiguousarray(image, dtype=np.float32)
    if a.ndim not in (2, 3):
        raise ValueError(f"an image is (H, W) or (P, H, W), got shape {a.shape}")
    p = 1 if a.ndim == 2 else a.shape[0]
    return a, p, a.shape[-2], a.shape[-1]


def lsf_gaussian(sigma: float, taps: int) -> np.ndarray:
    """`taps` (odd) samples of a Gaussian line-spread function of `sigma` pixels, normalised (xrt_lsf_gaussian)."""
    out = np.empty(max(int(taps), 1), np.float32)
    rc = _abi.load().xrt_lsf_gaussian(float(sigma), int(taps), _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_lsf_gaussian: sigma must be finite and > 0, taps odd and in 1..XRT_MAX_LSF_TAPS")
    return out


def host_lsf(image, lsf_x, lsf_y=None, u8=True):
    """The detector response in the device's arithmetic on the host (xrt_host_lsf, a test hook): (out, u8)."""
    a, p, h, w = _lsf_planes(image)
    hx, hy = _lsf_arrays(lsf_x, lsf_y)
    out = np.empty_like(a)
    u = np.empty(a.shape, np.uint8) if u8 else None
    rc = _abi.load().xrt_host_lsf(w, h, p, _fptr(a), _fptr(hx), hx.size, _fptr(hy), hy.size, _fptr(out),
                                  _u8ptr(u) if u is not None else None)
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_lsf")
    return out, u


def detector_response(image, lsf_x, lsf_y=None, device: int = 0) -> np.ndarray:
    """The blurred f32 image(s) of Context.detector_response, on a context of its own on `device`."""
    with Context(device) as ctx:
        return ctx.detector_response(image, lsf_x, lsf_y, u8=False)[0]


def _scatter_planes(paths, open, num_meshes):
    """xrt_scatter_source's planes from (M, H, W) or (M, P, H, W) paths and (H, W) or (P, H, W) masks (or None):
    (paths, open, P, H, W, a plane stack's shape)."""
    p = np.ascontiguousarray(paths, dtype=np.float32)
    if p.ndim not in (3, 4) or p.shape[0] != num_meshes:
        raise ValueError(f"paths must be ({num_meshes}, H, W) or ({num_meshes}, P, H, W), got shape {p.shape}")
    o = None if open is None else np.ascontiguousarray(open, dtype=np.uint16)
    if o is not None and o.shape != p.shape[1:]:
        raise ValueError(f"open must have a plane stack's shape {p.shape[1:]}, got {o.shape}")
    return p, o, (1 if p.ndim == 3 else p.shape[1]), p.shape[-2], p.shape[-1], p.shape[1:]


def _scatter_tables(weights, mu, sigma):
    w, mu = _spectrum_arrays(weights, mu)
    sg = np.ascontiguousarray(sigma, dtype=np.float32)
    if sg.shape != mu.shape:
        raise ValueError(f"sigma must have mu's shape {mu.shape}, got {sg.shape}")
    return w, mu, sg


def _scatter_coarse(blurred, amp, shape, bin):
    """xrt_scatter_add's coarse planes for a fine (H, W) or (P, H, W) `shape`: (blurred (G, ...), amp (G,))."""
    a = np.ascontiguousarray(amp, dtype=np.float32).reshape(-1)
    d = max(int(bin), 1)
    want = (a.size,) + tuple(shape[:-2]) + ((shape[-2] + d - 1) // d, (shape[-1] + d - 1) // d)
    b = np.ascontiguousarray(blurred, dtype=np.float32)
    if b.shape != want:
        raise ValueError(f"blurred must have shape {want}, got {b.shape}")
    return b, a


def host_scatter_source(paths, open, weights, mu, sigma, bin, lbuffer=True):
    """Context.scatter_source in the device's arithmetic on the host (xrt_host_scatter_source, a test hook)."""
    w, mu, sg = _scatter_tables(weights, mu, sigma)
    p, o, planes, h, wd, shape = _scatter_planes(paths, open, mu.shape[0])
    d = max(int(bin), 1)
    src = np.empty(tuple(shape[:-2]) + ((h + d - 1) // d, (wd + d - 1) // d), np.float32)
    lb = np.empty(shape, np.float32) if lbuffer else None
    rc = _abi.load().xrt_host_scatter_source(wd, h, planes, mu.shape[0], _fptr(p), _u16ptr(o) if o is not None else None,
                                             _fptr(w), _fptr(mu), _fptr(sg), w.size, int(bin),
                                             _fptr(lb) if lb is not None else None, _fptr(src))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_scatter_source")
    return src, lb


def host_scatter_add(blurred, amp, bin, shape, primary=None, out=True, scatter=True, u8=True):
    """Context.scatter_add in the device's arithmetic on the host (xrt_host_scatter_add, a test hook)."""
    shape = tuple(int(v) for v in shape)
    b, a = _scatter_coarse(blurred, amp, shape, bin)
    pr = None if primary is None else np.ascontiguousarray(primary, dtype=np.float32).reshape(shape)
    o = np.empty(shape, np.float32) if out else None
    s = np.empty(shape, np.float32) if scatter else None
    u = np.empty(shape, np.uint8) if u8 else None
    planes = 1 if len(shape) == 2 else shape[0]
    rc = _abi.load().xrt_host_scatter_add(shape[-1], shape[-2], planes, int(bin), _fptr(b), a.size, _fptr(a),
                                          _fptr(pr) if pr is not None else None, _fptr(o) if o is not None else None,
                                          _fptr(s) if s is not None else None, _u8ptr(u) if u is not None else None)
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_scatter_add")
    return o, s, u


def scatter_gaussian(sigma_pixels: float, bin: int, taps: int | None = None) -> np.ndarray:
    """A Gaussian scatter kernel of `sigma_pixels` detector pixels as taps on the grid binned by `bin`:
    lsf_gaussian(sigma / bin, taps), taps by default 2 * ceil(4 * sigma / bin) + 1, at most XRT_MAX_LSF_TAPS."""
    s = float(sigma_pixels) / float(bin)
    if taps is None:
        if not (np.isfinite(s) and s > 0.0):
            raise XrtError(_abi.XRT_ERR_ARGUMENT, "scatter_gaussian: sigma and bin must be finite and > 0")
        taps = 2 * int(np.ceil(4.0 * s)) + 1
    if int(taps) > XRT_MAX_LSF_TAPS:
        raise XrtError(_abi.XRT_ERR_ARGUMENT, f"scatter_gaussian: {int(taps)} taps on the coarse grid, more than "
                                              f"XRT_MAX_LSF_TAPS = {XRT_MAX_LSF_TAPS}: bin further")
    return lsf_gaussian(s, int(taps))


def scatter(paths, open, weights, mu, sigma, kernels, bin, width, height, device: int = 0):
    """(total, scatter, primary) of Context.scatter, on a context of its own on `device`."""
    with Context(device) as ctx:
        return ctx.scatter(paths, open, weights, mu, sigma, kernels, bin, width, height)


def _projection_arrays(image, flat, dark, flat_value, sinograms):
    """xrt_log_projection's arguments from an (H, W) image or a (P, H, W) stack: the arrays, the sizes, the
    scalar flat (0 where a flat plane is given and none was named), the order and the output's shape."""
    a, p, h, w = _lsf_planes(image)
    planes = []
    for name, plane in (("flat", flat), ("dark", dark)):
        if plane is not None:
            plane = np.ascontiguousarray(plane, dtype=np.float32)
            if plane.shape != (h, w):
                raise ValueError(f"{name} is one (H, W) = ({h}, {w}) plane, got shape {plane.shape}")
        planes.append(plane)
    if flat_value is None:
        if flat is None:
            raise ValueError("log_projection needs a flat plane or a flat_value")
        flat_value = 0.0
    shape = ((h, p, w) if sinograms else a.shape) if a.ndim == 3 else ((h, 1, w) if sinograms else a.shape)
    order = _abi.XRT_ORDER_SINOGRAMS if sinograms else _abi.XRT_ORDER_PROJECTIONS
    return a, planes[0], planes[1], p, h, w, float(flat_value), order, shape


def host_logf(x) -> np.ndarray:
    """The device's logf restatement compiled for the host (xrt_host_logf_batch, a test hook)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    _abi.load().xrt_host_logf_batch(_fptr(x), _fptr(out), x.size)
    return out


def host_log_projection(image, flat=None, dark=None, flat_value=None, t_min=0.0, sinograms=False) -> np.ndarray:
    """Context.log_projection in the device's arithmetic on the host (xrt_host_log_projection, a test hook)."""
    a, f, d, p, h, w, fv, order, shape = _projection_arrays(image, flat, dark, flat_value, sinograms)
    out = np.empty(shape, np.float32)
    rc = _abi.load().xrt_host_log_projection(w, h, p, _fptr(a), _fptr(f) if f is not None else None,
                                             _fptr(d) if d is not None else None, fv, float(t_min), order, _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_log_projection")
    return out


def log_projection(image, flat=None, dark=None, flat_value=None, t_min=0.0, sinograms=False, device: int = 0) -> np.ndarray:
    """The line integrals of Context.log_projection, on a context of its own on `device`."""
    with Context(device) as ctx:
        return ctx.log_projection(image, flat, dark, flat_value, t_min, sinograms)


def _u32ptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _noise_mode(counts):
    return _abi.XRT_NOISE_COUNTS if counts else _abi.XRT_NOISE_INTENSITY


def _poisson_arrays(lam, words):
    """Means and words as the sampler's hooks take them: f64 and u32 of one shape."""
    lam, words = np.broadcast_arrays(np.asarray(lam, np.float64), np.asarray(words, np.uint32))
    return np.ascontiguousarray(lam), np.ascontiguousarray(words)


def host_philox4x32(counter, key) -> np.ndarray:
    """Philox4x32-10's four words for a counter of four u32 and a key of two (xrt_host_philox4x32, a test hook)."""
    c = np.ascontiguousarray(counter, dtype=np.uint32).reshape(4)
    k = np.ascontiguousarray(key, dtype=np.uint32).reshape(2)
    out = np.empty(4, np.uint32)
    _abi.load().xrt_host_philox4x32(_u32ptr(c), _u32ptr(k), _u32ptr(out))
    return out


def host_poisson(lam, words) -> np.ndarray:
    """The device's Poisson sampler compiled for the host: the counts (f64) of the means `lam` under the random
    words `words` (xrt_host_poisson_batch, a test hook)."""
    lam, words = _poisson_arrays(lam, words)
    out = np.empty(lam.shape, np.float64)
    _abi.load().xrt_host_poisson_batch(_dptr(lam), _u32ptr(words), lam.size, _dptr(out))
    return out


def host_photon_noise(image, gain, seed, counts=False, first_index=0) -> np.ndarray:
    """Context.photon_noise in the device's arithmetic on the host (xrt_host_photon_noise, a test hook)."""
    a, p, h, w = _lsf_planes(image)
    out = np.empty_like(a)
    rc = _abi.load().xrt_host_photon_noise(w, h, p, _fptr(a), float(gain), int(seed), int(first_index),
                                           _noise_mode(counts), _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_photon_noise")
    return out


def photon_noise(image, gain, seed, counts=False, first_index=0, device: int = 0) -> np.ndarray:
    """The noisy image(s) of Context.photon_noise, on a context of its own on `device`."""
    with Context(device) as ctx:
        return ctx.photon_noise(image, gain, seed, counts, first_index)


def ray_table_index(width: int, height: int, row_begin: int, row_end: int, row: int, col: int):
    """(index, floats): where the ray table of the strip [row_begin, row_end) of a width x height image keeps
    dx of pixel (row, col) -- dy and dz lie 64 and 128 floats on -- and the table's size in floats
    (xrt_debug_ray_table_index: host code, the kernels' own function)."""
    index, floats = ctypes.c_uint64(), ctypes.c_uint64()
    rc = _abi.load().xrt_debug_ray_table_index(int(width), int(height), int(row_begin), int(row_end), int(row),
                                               int(col), ctypes.byref(index), ctypes.byref(floats))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_debug_ray_table_index: the pixel must lie in the strip and the strip in the image")
    return int(index.value), int(floats.value)


def supersampled_camera(cam: Camera, bin: int) -> Camera:
    """The camera whose pixels tile `cam`'s, bin x bin to each (xrt_camera_supersample)."""
    out = Camera()
    rc = _abi.load().xrt_camera_supersample(ctypes.byref(cam), int(bin), ctypes.byref(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_camera_supersample: bin must be in 1..XRT_MAX_BIN and the size stay below 2^31")
    return out


def focal_spot(cam: Camera, size_u: float, size_v: float, nu: int, nv: int):
    """A uniform rectangular focal spot of size_u x size_v along `right` and `up`, sampled at the centres of an
    nu x nv grid (xrt_focal_spot): (the nu * nv sub-source cameras, their weights)."""
    n = max(int(nu) * int(nv), 1)
    cams = (Camera * n)()
    weights = np.empty(n, np.float32)
    rc = _abi.load().xrt_focal_spot(ctypes.byref(cam), float(size_u), float(size_v), int(nu), int(nv), cams, _fptr(weights))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_focal_spot: sizes must be finite and >= 0, counts > 0 and nu * nv <= XRT_MAX_SOURCES")
    out = []
    for c in cams:                                          # copies that do not live in the ctypes array
        one = Camera()
        ctypes.memmove(ctypes.byref(one), ctypes.byref(c), ctypes.sizeof(Camera))
        out.append(one)
    return out, weights


def _area_bins(bin):
    """`bin` as (bin_y, bin_x): an int for both, or the pair."""
    if isinstance(bin, (tuple, list)):
        by, bx = bin
        return int(by), int(bx)
    return int(bin), int(bin)


def _area_arrays(image, bin, weights):
    """xrt_area_integrate's arguments from an (Hb, Wb), (S, Hb, Wb) or (P, S, Hb, Wb) image: the array, the weights,
    P, S, H, W, bin_y, bin_x and the output's shape."""
    a = np.ascontiguousarray(image, dtype=np.float32)
    if a.ndim not in (2, 3, 4):
        raise ValueError(f"an image is (Hb, Wb), (S, Hb, Wb) or (P, S, Hb, Wb), got shape {a.shape}")
    by, bx = _area_bins(bin)
    p = a.shape[0] if a.ndim == 4 else 1
    s = a.shape[-3] if a.ndim >= 3 else 1
    hb, wb = a.shape[-2], a.shape[-1]
    if by < 1 or bx < 1 or hb % by or wb % bx:
        raise ValueError(f"the planes' size ({hb}, {wb}) is no multiple of the bin ({by}, {bx})")
    w = np.ones(s, np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if w.size != s:
        raise ValueError(f"{s} sub-sources need {s} weights, got {w.size}")
    h, wd = hb // by, wb // bx
    return a, w, p, s, h, wd, by, bx, ((p, h, wd) if a.ndim == 4 else (h, wd))


def host_area_integrate(image, bin=1, weights=None, u8=False):
    """Context.area_integrate in the device's arithmetic on the host (xrt_host_area_integrate, a test hook)."""
    a, w, p, s, h, wd, by, bx, shape = _area_arrays(image, bin, weights)
    out = np.empty(shape, np.float32)
    u = np.empty(shape, np.uint8) if u8 else None
    rc = _abi.load().xrt_host_area_integrate(wd, h, bx, by, s, p, _fptr(w), _fptr(a), _fptr(out),
                                             _u8ptr(u) if u is not None else None)
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_area_integrate")
    return (out, u) if u8 else out


def area_integrate(image, bin=1, weights=None, u8=False, device: int = 0):
    """The integrated image(s) of Context.area_integrate, on a context of its own on `device`."""
    with Context(device) as ctx:
        return ctx.area_integrate(image, bin, weights, u8)


def _detector_arrays(paths, open, weights, mu, response):
    """The spectral detector's host arguments: (paths (M, ...) f32, open uint16 of a plane's shape or None,
    weights (K,), mu (M, K), response (C, K))."""
    w, mu = _spectrum_arrays(weights, mu)
    p = np.ascontiguousarray(paths, dtype=np.float32)
    if p.ndim < 1 or p.shape[0] != mu.shape[0]:
        raise ValueError(f"paths must hold {mu.shape[0]} planes, got shape {p.shape}")
    o = None if open is None else np.ascontiguousarray(open, dtype=np.uint16)
    if o is not None and o.shape != p.shape[1:]:
        raise ValueError(f"open must have a plane's shape {p.shape[1:]}, got {o.shape}")
    r = _detector_response_rows(response, w.size)
    return p, o, w, mu, r


def _detector_response_rows(response, num_bins):
    r = np.ascontiguousarray(response, dtype=np.float32)
    if r.ndim == 1:
        r = r.reshape(1, -1)
    if r.ndim != 2 or r.shape[1] != num_bins:
        raise ValueError(f"response must be (channels, {num_bins}), got shape {r.shape}")
    return r


def _detector_modes(noisy, counts):
    return (_abi.XRT_DETECT_NOISY if noisy else _abi.XRT_DETECT_EXPECTED,
            _abi.XRT_DETECT_COUNTS if counts else _abi.XRT_DETECT_INTENSITY)


def host_spectral_detector(paths, open, weights, mu, response, gain=1.0, seed=0, noisy=True, counts=True,
                           read_noise=0.0, first_index=0) -> np.ndarray:
    """Context.spectral_detector in the device's arithmetic on the host (xrt_host_spectral_detector, a test
    hook)."""
    p, o, w, mu, r = _detector_arrays(paths, open, weights, mu, response)
    out = np.empty((r.shape[0],) + p.shape[1:], np.float32)
    draw, mode = _detector_modes(noisy, counts)
    rc = _abi.load().xrt_host_spectral_detector(
        out[0].size, mu.shape[0], _fptr(p), _u16ptr(o) if o is not None else None, _fptr(w), _fptr(mu), w.size,
        _fptr(r), r.shape[0], float(gain), float(read_noise), int(seed), int(first_index), draw, mode, _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_spectral_detector")
    return out


def spectral_detector(paths, open, weights, mu, response, gain=1.0, seed=0, noisy=True, counts=True,
                      read_noise=0.0, first_index=0, device: int = 0) -> np.ndarray:
    """The channel planes of Context.spectral_detector, on a context of its own on `device`."""
    with Context(device) as ctx:
        return ctx.spectral_detector(paths, open, weights, mu, response, gain, seed, noisy, counts, read_noise,
                                     first_index)


def _decompose_tables(weights, mu, response):
    """Material decomposition's tables: (weights (K,), mu (B, K), response (C, K))."""
    w, mu = _spectrum_arrays(weights, mu)
    return w, mu, _detector_response_rows(response, w.size)


def decompose_guess(weights, mu, response) -> np.ndarray:
    """xrt_decompose_guess: the (B, C) f64 matrix that turns the channels' -ln(y / y0) into the iteration's
    starting line integrals, for the basis table (weights[K], mu[B, K]) under the response (C, K).  Host
    arithmetic; no device."""
    w, mu, r = _decompose_tables(weights, mu, response)
    out = np.zeros((mu.shape[0], r.shape[0]), np.float64)
    lib = _abi.load()
    rc = lib.xrt_decompose_guess(_fptr(w), _fptr(mu), mu.shape[0], w.size, _fptr(r), r.shape[0],
                                 out.ctypes.data_as(_abi._dp))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, (lib.xrt_last_error(None) or b"").decode() or "xrt_decompose_guess")
    return out


def _decompose_guess_arg(guess, w, mu, r):
    """guess="auto": decompose_guess of the tables; None: none; an array: (B, C) f64."""
    if guess is None:
        return None
    if isinstance(guess, str):
        if guess != "auto":
            raise ValueError(f"guess must be 'auto', None or a ({mu.shape[0]}, {r.shape[0]}) array, got {guess!r}")
        return decompose_guess(w, mu, r)
    g = np.ascontiguousarray(guess, dtype=np.float64)
    if g.shape != (mu.shape[0], r.shape[0]):
        raise ValueError(f"guess must have shape {(mu.shape[0], r.shape[0])}, got {g.shape}")
    return g


def _decompose_arrays(channels, open, weights, mu, response, guess):
    """xrt_decompose's host arguments: (channels (C, ...) f32, open uint16 of a plane's shape or None, weights
    (K,), mu (B, K), response (C, K), guess (B, C) f64 or None)."""
    w, mu, r = _decompose_tables(weights, mu, response)
    ch = np.ascontiguousarray(channels, dtype=np.float32)
    if ch.ndim < 1 or ch.shape[0] != r.shape[0]:
        raise ValueError(f"channels must hold {r.shape[0]} planes, got shape {ch.shape}")
    o = None if open is None else np.ascontiguousarray(open, dtype=np.uint16)
    if o is not None and o.shape != ch.shape[1:]:
        raise ValueError(f"open must have a plane's shape {ch.shape[1:]}, got {o.shape}")
    return ch, o, w, mu, r, _decompose_guess_arg(guess, w, mu, r)


def _dptr(a):
    return None if a is None else a.ctypes.data_as(_abi._dp)


def host_decompose(channels, open, weights, mu, response, gain=1.0, counts=True, guess="auto", max_iter=32, tol=1e-6,
                   damping=0.0, return_iters=False):
    """Context.decompose in the device's arithmetic on the host (xrt_host_decompose, a test hook)."""
    ch, o, w, mu, r, g = _decompose_arrays(channels, open, weights, mu, response, guess)
    out = np.empty((mu.shape[0],) + ch.shape[1:], np.float32)
    iters = np.empty(ch.shape[1:], np.uint8)
    rc = _abi.load().xrt_host_decompose(
        out[0].size, _fptr(ch), _u16ptr(o) if o is not None else None, _fptr(w), _fptr(mu), mu.shape[0], w.size, _fptr(r),
        r.shape[0], float(gain), _detector_modes(False, counts)[1], _dptr(g), int(max_iter), float(tol), float(damping),
        _fptr(out), _u8ptr(iters))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_decompose")
    return (out, iters) if return_iters else out


def decompose(channels, open, weights, mu, response, gain=1.0, counts=True, guess="auto", max_iter=32, tol=1e-6,
              damping=0.0, return_iters=False, device: int = 0):
    """The basis planes of Context.decompose, on a context of its own on `device`."""
    with Context(device) as ctx:
        return ctx.decompose(channels, open, weights, mu, response, gain, counts, guess, max_iter, tol, damping,
                             return_iters)


def _volume_arrays(labels, spacing, origin, density, num_labels):
    """A voxel volume as xrt_upload_volume takes it: (labels (nz, ny, nx) uint8, density f32 of that shape or
    None, dims (nx, ny, nz) uint32, origin f32[3], spacing f32[3], num_labels)."""
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    if lab.ndim != 3:
        raise ValueError(f"labels must have shape (nz, ny, nx), got {lab.shape}")
    den = None if density is None else np.ascontiguousarray(density, dtype=np.float32)
    if den is not None and den.shape != lab.shape:
        raise ValueError(f"density must have the labels' shape {lab.shape}, got {den.shape}")
    dims = np.array(lab.shape[::-1], np.uint32)
    org = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1)
    spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
    if org.size != 3:
        raise ValueError("origin must hold 3 values (x, y, z)")
    m = int(lab.max()) if num_labels is None and lab.size else int(num_labels or 0)
    return lab, den, dims, org, spc, m


def load_volume(path: str):
    """A MetaImage volume (xrt_host_load_volume): (data (nz, ny, nx) uint8 -- MET_UCHAR labels -- or float32 --
    a MET_FLOAT density --, spacing f32[3], origin f32[3]), both in x, y, z order, as upload_volume takes them."""
    host = _abi.load_host()
    data, kind = ctypes.c_void_p(), ctypes.c_int()
    dims, org, spc = np.zeros(3, np.uint32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    rc = host.xrt_host_load_volume(path.encode(), ctypes.byref(data), ctypes.byref(kind), _u32ptr(dims), _fptr(org),
                                   _fptr(spc))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, f"xrt_host_load_volume({path}): {host.xrt_host_last_error().decode()}")
    try:
        n = int(dims[0]) * int(dims[1]) * int(dims[2])
        ctype, dtype = (ctypes.c_uint8, np.uint8) if kind.value == _abi.XRT_VOLUME_U8 else (ctypes.c_float, np.float32)
        arr = np.ctypeslib.as_array(ctypes.cast(data, ctypes.POINTER(ctype)), shape=(n,)).astype(dtype, copy=True)
    finally:
        host.xrt_host_free(data)
    return arr.reshape(int(dims[2]), int(dims[1]), int(dims[0])), spc, org


def save_volume(path: str, data, spacing, origin=(0.0, 0.0, 0.0)):
    """A (nz, ny, nx) f32 volume as a MetaImage (xrt_host_save_volume): `path` (NAME.mhd) and NAME.raw beside it;
    load_volume reads it back bit for bit."""
    host = _abi.load_host()
    a = np.ascontiguousarray(data, dtype=np.float32)
    if a.ndim != 3:
        raise ValueError(f"a volume is (nz, ny, nx), got shape {a.shape}")
    dims = np.array(a.shape[::-1], np.uint32)
    org = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
    spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
    rc = host.xrt_host_save_volume(str(path).encode(), _fptr(a), _u32ptr(dims), _fptr(org), _fptr(spc))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, f"xrt_host_save_volume({path}): {host.xrt_host_last_error().decode()}")


def volume_bbox(dims, spacing, origin=(0.0, 0.0, 0.0)):
    """(lower, upper) of a volume of dims (nx, ny, nz) voxels of `spacing` whose minimum corner is `origin`
    (xrt_volume_bbox)."""
    d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(-1)
    org = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1)
    spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
    if d.size != 3 or org.size != 3:
        raise ValueError("dims and origin must hold 3 values (x, y, z)")
    lo, hi = np.empty(3, np.float32), np.empty(3, np.float32)
    rc = _abi.load().xrt_volume_bbox(_u32ptr(d), _fptr(org), _fptr(spc), _fptr(lo), _fptr(hi))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_volume_bbox")
    return lo, hi


def host_volume_paths(cam: Camera, labels, spacing, origin=(0.0, 0.0, 0.0), density=None, num_labels=None,
                      row_begin: int = 0, row_end: int | None = None) -> np.ndarray:
    """Context.volume_paths in the device's arithmetic on the host (xrt_host_volume_paths, a test hook)."""
    lab, den, dims, org, spc, m = _volume_arrays(labels, spacing, origin, density, num_labels)
    if row_end is None:
        row_end = cam.height
    out = np.empty((max(m, 1), max(row_end - row_begin, 0), cam.width), np.float32)
    rc = _abi.load().xrt_host_volume_paths(ctypes.byref(cam), row_begin, row_end, _u8ptr(lab),
                                           _fptr(den) if den is not None else None, _u32ptr(dims), _fptr(org),
                                           _fptr(spc), m, _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_volume_paths")
    return out


def _voxel_grid_arrays(dims, spacing, origin):
    """A voxeliser's grid as xrt_voxelize takes it: (dims (nx, ny, nz) uint32, origin f32[3], spacing f32[3])."""
    d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(-1)
    org = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1)
    spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
    if d.size != 3 or org.size != 3:
        raise ValueError("dims and origin must hold 3 values (x, y, z)")
    return d, org, spc


def _voxel_outputs(dims, num_meshes, value, mask, labels, volume, odd_columns):
    """The host buffers of the outputs asked for (None: not asked for), and value as f32 per mesh."""
    shape = (int(dims[2]), int(dims[1]), int(dims[0])) if dims.size == 3 else (0, 0, 0)
    val = None
    if value is not None:
        val = np.ascontiguousarray(value, dtype=np.float32).reshape(-1)
        if val.size != num_meshes:
            raise ValueError(f"value must hold one entry per mesh ({num_meshes}), got {val.size}")
    return (val, np.empty(shape, np.uint16) if mask else None, np.empty(shape, np.uint8) if labels else None,
            np.empty(shape, np.float32) if volume else None, np.zeros(_abi.XRT_MAX_MESHES, np.uint64) if odd_columns else None)


def _voxel_result(mask, labels, volume, odd, num_meshes):
    out = {}
    if mask is not None:
        out["mask"] = mask
    if labels is not None:
        out["labels"] = labels
    if volume is not None:
        out["volume"] = volume
    if odd is not None:
        out["odd_columns"] = odd[:num_meshes].copy()
    return out


def host_voxelize(meshes, dims, spacing, origin=(0.0, 0.0, 0.0), value=None, mask=True, labels=True, volume=None,
                  odd_columns=True) -> dict:
    """Context.voxelize in the device's arithmetic on the host (xrt_host_voxelize, a test hook): `meshes` is the
    list of (T, 9) soups as posed."""
    tris, counts = _scene_arrays(meshes)
    d, org, spc = _voxel_grid_arrays(dims, spacing, origin)
    volume = value is not None if volume is None else volume
    val, m, lab, vol, odd = _voxel_outputs(d, len(counts), value, mask, labels, volume, odd_columns)
    rc = _abi.load().xrt_host_voxelize(_fptr(tris), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(counts),
                                       _u32ptr(d), _fptr(org), _fptr(spc), _fptr(val) if val is not None else None,
                                       _u16ptr(m) if m is not None else None, _u8ptr(lab) if lab is not None else None,
                                       _fptr(vol) if vol is not None else None,
                                       odd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if odd is not None else None)
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_voxelize")
    return _voxel_result(m, lab, vol, odd, len(counts))


def ramp_filter(num_taps: int, window: int = _abi.XRT_RAMP_RAMLAK) -> np.ndarray:
    """`num_taps` (odd) samples of the band-limited ramp at unit sample distance, plain (XRT_RAMP_RAMLAK) or
    under a Hann window (XRT_RAMP_HANN), as f32 (xrt_ramp_filter)."""
    out = np.empty(max(int(num_taps), 1), np.float32)
    rc = _abi.load().xrt_ramp_filter(int(num_taps), int(window), _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_ramp_filter: num_taps odd and in 1..2*XRT_MAX_RAMP_WIDTH-1, window RAMLAK or HANN")
    return out


def fdk_weights(cam: Camera) -> np.ndarray:
    """The (H, W) f32 cosine weights of FDK for a camera (xrt_fdk_weights)."""
    out = np.empty((cam.height, cam.width), np.float32)
    rc = _abi.load().xrt_fdk_weights(ctypes.byref(cam), _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_fdk_weights")
    return out


def fdk_scale(cam: Camera, axis_point, num_projections: int) -> float:
    """The full-turn FDK constant of a scan of `num_projections` about an axis through `axis_point`
    (xrt_fdk_scale)."""
    q = np.ascontiguousarray(axis_point, dtype=np.float32).reshape(3)
    out = ctypes.c_double(0.0)
    rc = _abi.load().xrt_fdk_scale(ctypes.byref(cam), _fptr(q), int(num_projections), ctypes.byref(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_fdk_scale")
    return out.value


def backprojection_matrix(cam: Camera, origin, spacing, pose=None) -> np.ndarray:
    """The (3, 4) f64 matrix taking a voxel index (i, j, k) of the grid whose voxel (0, 0, 0) has its minimum
    corner at `origin` (voxels of `spacing`, one value or (x, y, z)), posed by `pose` (None: the identity), to the
    camera's homogeneous (col, row, 1) * c (xrt_backprojection_matrix)."""
    org = np.ascontiguousarray(origin, dtype=np.float32).reshape(3)
    spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
    q = _pose_array(pose)
    out = np.empty(12, np.float64)
    rc = _abi.load().xrt_backprojection_matrix(ctypes.byref(cam), _fptr(q) if q is not None else None, _fptr(org),
                                               _fptr(spc), _dptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_backprojection_matrix: the camera's axes must be finite and independent")
    return out.reshape(3, 4)


def _fdk_filter_arrays(image, weight, taps):
    """xrt_fdk_filter's arguments from an (H, W) image or a (P, H, W) stack: (image, weight or None, taps, P, H, W)."""
    a, p, h, w = _lsf_planes(image)
    if weight is not None:
        weight = np.ascontiguousarray(weight, dtype=np.float32)
        if weight.shape != (h, w):
            raise ValueError(f"weight is one (H, W) = ({h}, {w}) plane, got shape {weight.shape}")
    return a, weight, np.ascontiguousarray(taps, dtype=np.float32).reshape(-1), p, h, w


def _backproject_arrays(proj, matrices, dims, slabs, volume, accumulate):
    """xrt_backproject's arguments: (projections, matrices (P, 12) f64, dims u32[3], slab range, volume)."""
    a, p, h, w = _lsf_planes(proj)
    m = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 12)
    if m.shape[0] != p:
        raise ValueError(f"{p} projections need {p} matrices, got {m.shape[0]}")
    d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
    lo, hi = (0, int(d[2])) if slabs is None else (int(slabs[0]), int(slabs[1]))
    shape = (max(hi - lo, 0), int(d[1]), int(d[0]))
    if accumulate:
        if volume is None:
            raise ValueError("accumulate needs the volume to add to")
        volume = np.array(volume, dtype=np.float32, order="C")
        if volume.shape != shape:
            raise ValueError(f"the volume to add to must have shape {shape}, got {volume.shape}")
    else:
        volume = np.empty(shape, np.float32)
    return a, m, d, lo, hi, volume, p, h, w


def host_fdk_filter(image, taps, weight=None) -> np.ndarray:
    """Context.fdk_filter's contract on the host (xrt_host_fdk_filter, a test hook)."""
    a, wt, t, p, h, w = _fdk_filter_arrays(image, weight, taps)
    out = np.empty_like(a)
    rc = _abi.load().xrt_host_fdk_filter(w, h, p, _fptr(a), _fptr(wt) if wt is not None else None, _fptr(t), t.size,
                                         _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_fdk_filter")
    return out


def host_backproject(proj, matrices, dims, scale=1.0, slabs=None, volume=None, accumulate=False) -> np.ndarray:
    """Context.backproject in the device's arithmetic on the host (xrt_host_backproject, a test hook)."""
    a, m, d, lo, hi, vol, p, h, w = _backproject_arrays(proj, matrices, dims, slabs, volume, accumulate)
    rc = _abi.load().xrt_host_backproject(w, h, p, _fptr(a), _dptr(m), _u32ptr(d), lo, hi, float(scale),
                                          int(bool(accumulate)), _fptr(vol))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_backproject")
    return vol


def ray_matrix(A) -> np.ndarray:
    """The (3, 4) f64 ray matrix R = [A3^-1 | -A3^-1 a4] of a backprojection matrix A = [A3 | a4]: column 3 is the
    source in centre-index coordinates and pixel (row, col)'s ray direction is R[:, 0] * col + (R[:, 1] * row +
    R[:, 2]) (xrt_ray_matrix)."""
    a = np.ascontiguousarray(A, dtype=np.float64).reshape(12)
    out = np.empty(12, np.float64)
    rc = _abi.load().xrt_ray_matrix(_dptr(a), _dptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_ray_matrix: the matrix must be finite and its left 3 x 3 block invertible")
    return out.reshape(3, 4)


def _forward_arrays(volume, spacing, rays, mode, meas, shape):
    """xrt_forward_project's arguments: (volume, dims u32[3], spacing f32[3], rays (P, 12) f64, meas or None, P, H,
    W); shape = (H, W) of a plane."""
    v = np.ascontiguousarray(volume, dtype=np.float32)
    if v.ndim != 3:
        raise ValueError(f"a volume is (nz, ny, nx), got shape {v.shape}")
    d = np.array(v.shape[::-1], np.uint32)
    spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
    r = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 12)
    p = r.shape[0]
    if meas is not None:
        meas, mp, h, w = _lsf_planes(meas)
        if mp != p:
            raise ValueError(f"{p} ray matrices need {p} measured planes, got {mp}")
    else:
        if mode == _abi.XRT_FP_RESIDUAL:
            raise ValueError("the residual mode needs meas")
        h, w = (int(x) for x in shape)
    return v, d, spc, r, meas, p, h, w


def host_forward_project(volume, spacing, rays, shape=None, mode=_abi.XRT_FP_PROJECT, meas=None) -> np.ndarray:
    """Context.forward_project in the device's arithmetic on the host (xrt_host_forward_project, a test hook)."""
    v, d, spc, r, m, p, h, w = _forward_arrays(volume, spacing, rays, mode, meas, shape)
    out = np.empty((p, h, w), np.float32)
    rc = _abi.load().xrt_host_forward_project(w, h, p, _fptr(v), _u32ptr(d), _fptr(spc), _dptr(r), int(mode),
                                              _fptr(m) if m is not None else None, _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_forward_project")
    return out


def _update_arrays(x, corr, norm):
    x = np.array(x, dtype=np.float32, order="C")
    c, n = np.ascontiguousarray(corr, dtype=np.float32), np.ascontiguousarray(norm, dtype=np.float32)
    if c.shape != x.shape or n.shape != x.shape:
        raise ValueError(f"x, corr and norm must share a shape, got {x.shape}, {c.shape}, {n.shape}")
    return x, c, n


def host_volume_update(x, corr, norm, relax=1.0, lo=-np.inf, hi=np.inf) -> np.ndarray:
    """Context.volume_update on the host (xrt_host_volume_update, a test hook): the updated copy of x."""
    x, c, n = _update_arrays(x, corr, norm)
    rc = _abi.load().xrt_host_volume_update(x.size, _fptr(x), _fptr(c), _fptr(n), float(relax), float(lo), float(hi))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_volume_update")
    return x


def _sirt_arrays(proj, matrices, dims, spacing, start):
    a, p, h, w = _lsf_planes(proj)
    m = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 12)
    if m.shape[0] != p:
        raise ValueError(f"{p} projections need {p} matrices, got {m.shape[0]}")
    d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
    spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
    shape = (int(d[2]), int(d[1]), int(d[0]))
    vol = np.zeros(shape, np.float32) if start is None else np.array(start, dtype=np.float32, order="C")
    if vol.shape != shape:
        raise ValueError(f"the start must have shape {shape}, got {vol.shape}")
    return a, m, d, spc, vol, p, h, w


def _tv_params(tv):
    """xrt_tv_params from a (steps, alpha, reduction, eps) tuple; None stays None."""
    if tv is None:
        return None
    steps, alpha, reduction, eps = tv
    return _abi.TvParams(int(steps), float(alpha), float(reduction), float(eps))


def host_sirt(proj, matrices, dims, spacing, iterations, subsets=1, relax=1.0, lo=0.0, hi=np.inf, start=None,
              tv=None) -> np.ndarray:
    """Context.sirt_matrices in the device's arithmetic on the host (xrt_host_sirt, or with tv xrt_host_sirt_tv; test
    hooks)."""
    a, m, d, spc, vol, p, h, w = _sirt_arrays(proj, matrices, dims, spacing, start)
    if tv is None:
        rc = _abi.load().xrt_host_sirt(w, h, p, _fptr(a), _dptr(m), _u32ptr(d), _fptr(spc), int(iterations), int(subsets),
                                       float(relax), float(lo), float(hi), _fptr(vol))
    else:
        params = _tv_params(tv)
        rc = _abi.load().xrt_host_sirt_tv(w, h, p, _fptr(a), _dptr(m), _u32ptr(d), _fptr(spc), int(iterations),
                                          int(subsets), float(relax), float(lo), float(hi), ctypes.byref(params), _fptr(vol))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_sirt")
    return vol


def _poisson_project_arrays(volume, spacing, rays, counts, flat, background):
    """xrt_poisson_project's arguments: (volume, dims, spacing, rays, counts, flat, background or None, P, H, W)."""
    v, d, spc, r, y, p, h, w = _forward_arrays(volume, spacing, rays, _abi.XRT_FP_RESIDUAL, counts, None)
    f = np.ascontiguousarray(flat, dtype=np.float32)
    if f.shape != (h, w):
        raise ValueError(f"flat is one (H, W) = ({h}, {w}) plane, got shape {f.shape}")
    if background is not None:
        background = np.ascontiguousarray(background, dtype=np.float32)
        if background.size != y.size:
            raise ValueError(f"the background has the counts' shape {y.shape}, got {background.shape}")
    return v, d, spc, r, y, f, background, p, h, w


def _pairs_arrays(pairs, matrices, dims, volume):
    """xrt_backproject_update's arguments: (pairs (P, H, W, 2) f32, matrices (P, 12) f64, dims u32[3], a copy of the
    volume, P, H, W)."""
    a = np.ascontiguousarray(pairs, dtype=np.float32)
    if a.ndim == 3:
        a = a[None]
    if a.ndim != 4 or a.shape[-1] != 2:
        raise ValueError(f"pairs are (P, H, W, 2), got shape {a.shape}")
    p, h, w = a.shape[:3]
    m = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 12)
    if m.shape[0] != p:
        raise ValueError(f"{p} planes of pairs need {p} matrices, got {m.shape[0]}")
    d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
    shape = (int(d[2]), int(d[1]), int(d[0]))
    vol = np.array(volume, dtype=np.float32, order="C")
    if vol.shape != shape:
        raise ValueError(f"the volume must have shape {shape}, got {vol.shape}")
    return a, m, d, vol, p, h, w


def _mltr_arrays(counts, flat, background, matrices, dims, spacing, start):
    y, m, d, spc, vol, p, h, w = _sirt_arrays(counts, matrices, dims, spacing, start)
    f = np.ascontiguousarray(np.broadcast_to(np.asarray(flat, np.float32), (h, w)))
    if background is not None:
        background = np.ascontiguousarray(np.broadcast_to(np.asarray(background, np.float32), y.shape))
    return y, f, background, m, d, spc, vol, p, h, w


def host_poisson_project(volume, spacing, rays, counts, flat, background=None) -> np.ndarray:
    """Context.poisson_project in the device's arithmetic on the host (xrt_host_poisson_project, a test hook)."""
    v, d, spc, r, y, f, b, p, h, w = _poisson_project_arrays(volume, spacing, rays, counts, flat, background)
    out = np.empty((p, h, w, 2), np.float32)
    rc = _abi.load().xrt_host_poisson_project(w, h, p, _fptr(v), _u32ptr(d), _fptr(spc), _dptr(r), _fptr(y), _fptr(f),
                                              _fptr(b) if b is not None else None, _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_poisson_project")
    return out


def host_backproject_update(pairs, matrices, dims, volume, relax=1.0, lo=-np.inf, hi=np.inf) -> np.ndarray:
    """Context.backproject_update on the host (xrt_host_backproject_update, a test hook): the updated copy."""
    a, m, d, vol, p, h, w = _pairs_arrays(pairs, matrices, dims, volume)
    rc = _abi.load().xrt_host_backproject_update(w, h, p, _fptr(a), _dptr(m), _u32ptr(d), float(relax), float(lo), float(hi),
                                                 _fptr(vol))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_backproject_update")
    return vol


def host_mltr(counts, flat, matrices, dims, spacing, iterations, subsets=1, relax=1.0, lo=0.0, hi=np.inf, start=None,
              tv=None, background=None) -> np.ndarray:
    """Context.mltr_matrices in the device's arithmetic on the host (xrt_host_mltr, a test hook)."""
    y, f, b, m, d, spc, vol, p, h, w = _mltr_arrays(counts, flat, background, matrices, dims, spacing, start)
    params = _tv_params(tv)
    rc = _abi.load().xrt_host_mltr(w, h, p, _fptr(y), _fptr(f), _fptr(b) if b is not None else None, _dptr(m), _u32ptr(d),
                                   _fptr(spc), int(iterations), int(subsets), float(relax), float(lo), float(hi),
                                   ctypes.byref(params) if params is not None else None, _fptr(vol))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_mltr")
    return vol


def _tv_volume(volume, copy=False):
    """(volume f32 (nz, ny, nx), dims u32[3]) of xrt_tv_gradient and xrt_tv_descend."""
    v = np.array(volume, dtype=np.float32, order="C") if copy else np.ascontiguousarray(volume, dtype=np.float32)
    if v.ndim != 3:
        raise ValueError(f"a volume is (nz, ny, nx), got shape {v.shape}")
    return v, np.array(v.shape[::-1], np.uint32)


def _sumsq_arrays(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float32)
        if b.shape != a.shape:
            raise ValueError(f"a and b must share a shape, got {a.shape} and {b.shape}")
    return a, b


def host_tv_gradient(volume, eps=1e-8) -> np.ndarray:
    """Context.tv_gradient on the host (xrt_host_tv_gradient, a test hook)."""
    v, d = _tv_volume(volume)
    out = np.empty_like(v)
    rc = _abi.load().xrt_host_tv_gradient(_fptr(v), _u32ptr(d), float(eps), _fptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_tv_gradient")
    return out


def host_volume_sumsq(a, b=None) -> float:
    """Context.volume_sumsq on the host (xrt_host_volume_sumsq, a test hook)."""
    a, b = _sumsq_arrays(a, b)
    out = np.zeros(1, np.float64)
    rc = _abi.load().xrt_host_volume_sumsq(a.size, _fptr(a), _fptr(b) if b is not None else None, _dptr(out))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_volume_sumsq")
    return float(out[0])


def host_tv_descend(volume, steps, length, eps=1e-8, lo=-np.inf, hi=np.inf) -> np.ndarray:
    """Context.tv_descend on the host (xrt_host_tv_descend, a test hook): the descended copy of the volume."""
    v, d = _tv_volume(volume, copy=True)
    rc = _abi.load().xrt_host_tv_descend(_fptr(v), _u32ptr(d), float(eps), int(steps), float(length), float(lo), float(hi))
    if rc != _abi.XRT_OK:
        raise XrtError(rc, "xrt_host_tv_descend")
    return v


class Context:
    """One xrt_context (one device).  Not thread-safe."""

    def __init__(self, device: int = 0):
        self._lib = _abi.load()
        self._ctx = _abi._CtxP()
        self._num_meshes = 0               # of the uploaded scene (render_paths' planes)
        self._num_labels = 0               # of the uploaded volume (volume_paths' planes)
        rc = self._lib.xrt_create(device, ctypes.byref(self._ctx))
        if rc != _abi.XRT_OK:
            raise XrtError(rc, self._lib.xrt_last_error(None).decode())
        self.device = device

    def close(self):
        if self._ctx:
            self._lib.xrt_destroy(self._ctx)
            self._ctx = _abi._CtxP()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != _abi.XRT_OK:
            raise XrtError(rc, f"{what}: {self._lib.xrt_last_error(self._ctx).decode()}")

    def upload_mesh(self, tris: np.ndarray):
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        self._check(self._lib.xrt_upload_mesh(self._ctx, _fptr(tris), len(tris)), "xrt_upload_mesh")
        self._num_meshes = 1

    def set_kernel(self, kernel: int):
        self._check(self._lib.xrt_set_kernel(self._ctx, int(kernel)), "xrt_set_kernel")

    def set_model(self, model: int, mu: float = 0.1037):
        """XRT_MODEL_ATTENUATION (main.cxx) or XRT_MODEL_SIGNED (the L-buffer fork, mesh-0 mu)."""
        self._check(self._lib.xrt_set_model(self._ctx, int(model), float(np.float32(mu))), "xrt_set_model")

    def upload_scene(self, meshes):
        """A scene of several meshes ((T, 9) soups, any of them empty); upload_mesh is a one-mesh scene."""
        tris, counts = _scene_arrays(meshes)
        self._check(self._lib.xrt_upload_scene(self._ctx, _fptr(tris),
                                               counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(counts)),
                    "xrt_upload_scene")
        self._num_meshes = len(counts)

    def set_pose(self, mesh: int, pose=None):
        """Mesh `mesh` of the scene under a pose (12 f32, row-major 3x4 [R | t]; None: the identity), on the device."""
        q = _pose_array(pose)
        self._check(self._lib.xrt_set_pose(self._ctx, int(mesh), _fptr(q) if q is not None else None), "xrt_set_pose")

    def reset_poses(self):
        """Every mesh back at rest."""
        self._check(self._lib.xrt_reset_poses(self._ctx), "xrt_reset_poses")

    def posed_triangles(self) -> np.ndarray:
        """The (T, 9) soup the next render would read (xrt_debug_posed_triangles)."""
        n = ctypes.c_uint64()
        self._check(self._lib.xrt_debug_posed_triangles(self._ctx, None, 0, ctypes.byref(n)),
                    "xrt_debug_posed_triangles")
        out = np.empty(n.value, np.float32)
        self._check(self._lib.xrt_debug_posed_triangles(self._ctx, _fptr(out), out.size, ctypes.byref(n)),
                    "xrt_debug_posed_triangles")
        return out.reshape(-1, 9)

    def pose_span(self, launches: int = 200) -> float:
        """Microseconds k_pose takes to write the whole posed soup, by device events over `launches` writings."""
        us = ctypes.c_double()
        self._check(self._lib.xrt_debug_pose_span(self._ctx, int(launches), ctypes.byref(us)), "xrt_debug_pose_span")
        return us.value

    def pose_counters(self) -> dict:
        """k_pose launches so far and the triangles they wrote (xrt_debug_pose_counters)."""
        c = (ctypes.c_uint64 * 2)()
        self._check(self._lib.xrt_debug_pose_counters(self._ctx, c), "xrt_debug_pose_counters")
        return {"launches": int(c[0]), "triangles": int(c[1])}

    def _render_model(self, entry, name, cam):
        """A whole-frame render and hole fill through `entry` (xrt_render_signed and its kin)."""
        n = cam.width * cam.height
        img = np.empty(n, np.float32)
        lb = np.empty(n, np.float32)
        u8 = np.empty(n, np.uint8)
        st = Stats()
        self._check(entry(self._ctx, ctypes.byref(cam), _fptr(img), _fptr(lb), _u8ptr(u8), ctypes.byref(st)), name)
        return img, lb, u8, st

    def set_materials(self, mu):
        """XRT_MODEL_MATERIALS with one attenuation coefficient per mesh of the scene."""
        mu = np.ascontiguousarray(mu, dtype=np.float32).reshape(-1)
        self._check(self._lib.xrt_set_materials(self._ctx, _fptr(mu), mu.size), "xrt_set_materials")

    def render_materials(self, cam: Camera):
        """The materials model end to end: (hole-filled image f32, lbuffer f32 with -1 flags, u8, Stats)."""
        return self._render_model(self._lib.xrt_render_materials, "xrt_render_materials", cam)

    def probe_materials(self, distance: np.ndarray, sign_sum, mu):
        """The device's chained L of rays with given per-mesh sums ((n, M) arrays; sign_sum may be None)."""
        d = np.ascontiguousarray(distance, dtype=np.float32)
        mu = np.ascontiguousarray(mu, dtype=np.float32).reshape(-1)
        d = d.reshape(-1, mu.size)
        s = None if sign_sum is None else np.ascontiguousarray(sign_sum, dtype=np.int32).reshape(d.shape)
        out = np.empty(len(d), np.float32)
        self._check(self._lib.xrt_probe_materials(
            self._ctx, _fptr(d), _i32ptr(s) if s is not None else None,
            _fptr(mu), mu.size, _fptr(out), len(d)), "xrt_probe_materials")
        return out

    def set_spectrum(self, weights, mu):
        """XRT_MODEL_SPECTRUM: K bin weights and mu of shape (M, K), mesh m's coefficient in bin e at mu[m, e]."""
        w, mu = _spectrum_arrays(weights, mu)
        self._check(self._lib.xrt_set_spectrum(self._ctx, _fptr(w), _fptr(mu), mu.shape[0], w.size), "xrt_set_spectrum")

    def render_spectrum(self, cam: Camera):
        """The spectrum model end to end: (hole-filled image f32, lbuffer f32 with -1 flags, u8, Stats)."""
        return self._render_model(self._lib.xrt_render_spectrum, "xrt_render_spectrum", cam)

    def probe_spectrum(self, distance: np.ndarray, sign_sum, weights, mu):
        """The device's spectrum L of rays with given per-mesh sums ((n, M) arrays; sign_sum may be None)."""
        w, mu = _spectrum_arrays(weights, mu)
        d = np.ascontiguousarray(distance, dtype=np.float32).reshape(-1, mu.shape[0])
        s = None if sign_sum is None else np.ascontiguousarray(sign_sum, dtype=np.int32).reshape(d.shape)
        out = np.empty(len(d), np.float32)
        self._check(self._lib.xrt_probe_spectrum(
            self._ctx, _fptr(d), _i32ptr(s) if s is not None else None,
            _fptr(w), _fptr(mu), mu.shape[0], w.size, _fptr(out), len(d)), "xrt_probe_spectrum")
        return out

    def set_paths(self):
        """XRT_MODEL_PATHS: renders store the per-mesh path lengths of the uploaded scene (render_paths)."""
        self._check(self._lib.xrt_set_paths(self._ctx), "xrt_set_paths")

    def render_paths(self, cam: Camera, row_begin: int = 0, row_end: int | None = None, num_meshes: int | None = None):
        """The paths model's strip: (paths (M, rows, W) f32, open (rows, W) uint16 -- bit m set where mesh m's
        signs do not cancel --, Stats).  M is the uploaded scene's mesh count (num_meshes overrides the
        buffers' size as stated to the library, which checks it against the scene)."""
        if row_end is None:
            row_end = cam.height
        m = self._num_meshes if num_meshes is None else int(num_meshes)
        rows = max(row_end - row_begin, 0)
        paths = np.empty((max(m, 1), rows, cam.width), np.float32)
        opn = np.empty((rows, cam.width), np.uint16)
        st = Stats()
        self._check(self._lib.xrt_render_paths(self._ctx, ctypes.byref(cam), row_begin, row_end, m, _fptr(paths),
                                               _u16ptr(opn), ctypes.byref(st)),
                    "xrt_render_paths")
        return paths, opn, st

    def render_paths_device(self, cam: Camera, row_begin: int, row_end: int, num_meshes: int, d_paths: int,
                            d_open: int = 0, stream: int = 0):
        """Device-buffer paths render (raw device pointers: num_meshes f32 planes of the strip, one after
        another, and its uint16 mask plane or 0); asynchronous on `stream`."""
        rc = self._lib.xrt_render_paths_device(self._ctx, ctypes.byref(cam), row_begin, row_end, int(num_meshes),
                                               d_paths or None, d_open or None, stream or None)
        self._check(rc, "xrt_render_paths_device")

    def apply_spectrum(self, paths, open, weights, mu):
        """The spectrum model's lbuffer from render_paths' planes ((M, ...) f32 and the masks, or None) under
        the table (weights[K], mu[M, K]): what render_spectrum stores, shaped like one plane."""
        w, mu = _spectrum_arrays(weights, mu)
        p = np.ascontiguousarray(paths, dtype=np.float32)
        if p.ndim < 1 or p.shape[0] != mu.shape[0]:
            raise ValueError(f"paths must hold {mu.shape[0]} planes, got shape {p.shape}")
        o = None if open is None else np.ascontiguousarray(open, dtype=np.uint16)
        if o is not None and o.shape != p.shape[1:]:
            raise ValueError(f"open must have a plane's shape {p.shape[1:]}, got {o.shape}")
        out = np.empty(p.shape[1:], np.float32)
        self._check(self._lib.xrt_apply_spectrum(
            self._ctx, out.size, mu.shape[0], _fptr(p), _u16ptr(o) if o is not None else None, _fptr(w), _fptr(mu),
            w.size, _fptr(out)), "xrt_apply_spectrum")
        return out

    def apply_spectrum_device(self, num_pixels: int, d_paths: int, d_open: int, weights, mu, d_lbuffer: int,
                              stream: int = 0):
        """apply_spectrum over device buffers (raw pointers; the table is host data and travels with the
        launch); asynchronous on `stream`."""
        w, mu = _spectrum_arrays(weights, mu)
        rc = self._lib.xrt_apply_spectrum_device(self._ctx, int(num_pixels), mu.shape[0], d_paths or None,
                                                 d_open or None, _fptr(w), _fptr(mu), w.size, d_lbuffer or None,
                                                 stream or None)
        self._check(rc, "xrt_apply_spectrum_device")

    def spectral_detector(self, paths, open, weights, mu, response, gain=1.0, seed=0, noisy=True, counts=True,
                          read_noise=0.0, first_index=0):
        """The spectral detector over render_paths' planes ((M, ...) f32 and the masks, or None) under the table
        (weights[K], mu[M, K]) and the response (C, K): per pixel and bin a Poisson count of mean gain *
        weight * exp(-x) -- noisy=False: the mean itself --, drawn from (seed, first_index + the pixel's flat
        index, the bin) alone, summed into C channels under the response, plus read_noise (counts, Gaussian)
        a channel; as counts or -- counts=False -- divided by gain.  -1 where the mask is set.  (C, ...)."""
        p, o, w, mu, r = _detector_arrays(paths, open, weights, mu, response)
        out = np.empty((r.shape[0],) + p.shape[1:], np.float32)
        draw, mode = _detector_modes(noisy, counts)
        self._check(self._lib.xrt_spectral_detector(
            self._ctx, out[0].size, mu.shape[0], _fptr(p), _u16ptr(o) if o is not None else None, _fptr(w), _fptr(mu),
            w.size, _fptr(r), r.shape[0], float(gain), float(read_noise), int(seed), int(first_index), draw, mode,
            _fptr(out)), "xrt_spectral_detector")
        return out

    def spectral_detector_device(self, num_pixels: int, d_paths: int, d_open: int, weights, mu, response, d_out: int,
                                 gain: float = 1.0, seed: int = 0, noisy: bool = True, counts: bool = True,
                                 read_noise: float = 0.0, first_index: int = 0, stream: int = 0):
        """spectral_detector over device buffers (raw pointers; d_out holds C planes of num_pixels; the table
        and the response are host data and travel with the launch); asynchronous on `stream`."""
        w, mu = _spectrum_arrays(weights, mu)
        r = _detector_response_rows(response, w.size)
        draw, mode = _detector_modes(noisy, counts)
        rc = self._lib.xrt_spectral_detector_device(
            self._ctx, int(num_pixels), mu.shape[0], d_paths or None, d_open or None, _fptr(w), _fptr(mu), w.size,
            _fptr(r), r.shape[0], float(gain), float(read_noise), int(seed), int(first_index), draw, mode,
            d_out or None, stream or None)
        self._check(rc, "xrt_spectral_detector_device")

    def decompose(self, channels, open, weights, mu, response, gain=1.0, counts=True, guess="auto", max_iter=32,
                  tol=1e-6, damping=0.0, return_iters=False):
        """Projection-domain material decomposition, the inverse of spectral_detector(noisy=False): from the
        channel planes ((C, ...) f32, as counts or -- counts=False -- as intensities) and the masks (or None)
        the line integrals of the B basis materials of the table (weights[K], mu[B, K]) under the response
        (C, K) and gain: (B, ...) f32 path planes, +0 where the mask is set.  Per pixel at most max_iter steps
        of Fisher scoring, until no line integral moves by more than tol; damping scales the normal matrix's
        diagonal by 1 + damping.  guess="auto" starts from decompose_guess' matrix, None from zero, an array is
        the (B, C) matrix itself.  return_iters=True: also the uint8 plane of each pixel's iterations,
        XRT_DECOMPOSE_MASKED or XRT_DECOMPOSE_FAILED."""
        ch, o, w, mu, r, g = _decompose_arrays(channels, open, weights, mu, response, guess)
        out = np.empty((mu.shape[0],) + ch.shape[1:], np.float32)
        iters = np.empty(ch.shape[1:], np.uint8) if return_iters else None
        self._check(self._lib.xrt_decompose(
            self._ctx, out[0].size, _fptr(ch), _u16ptr(o) if o is not None else None, _fptr(w), _fptr(mu), mu.shape[0],
            w.size, _fptr(r), r.shape[0], float(gain), _detector_modes(False, counts)[1], _dptr(g), int(max_iter),
            float(tol), float(damping), _fptr(out), _u8ptr(iters) if iters is not None else None), "xrt_decompose")
        return (out, iters) if return_iters else out

    def decompose_device(self, num_pixels: int, d_channels: int, d_open: int, weights, mu, response, d_out: int,
                         d_iters: int = 0, gain: float = 1.0, counts: bool = True, guess="auto", max_iter: int = 32,
                         tol: float = 1e-6, damping: float = 0.0, stream: int = 0):
        """decompose over device buffers (raw pointers; d_channels holds C planes of num_pixels, d_out B planes,
        d_iters a uint8 plane or 0; the tables and the guess are host data and travel with the launch);
        asynchronous on `stream`."""
        w, mu, r = _decompose_tables(weights, mu, response)
        g = _decompose_guess_arg(guess, w, mu, r)
        rc = self._lib.xrt_decompose_device(
            self._ctx, int(num_pixels), d_channels or None, d_open or None, _fptr(w), _fptr(mu), mu.shape[0], w.size,
            _fptr(r), r.shape[0], float(gain), _detector_modes(False, counts)[1], _dptr(g), int(max_iter), float(tol),
            float(damping), d_out or None, d_iters or None, stream or None)
        self._check(rc, "xrt_decompose_device")

    def upload_volume(self, labels, spacing, origin=(0.0, 0.0, 0.0), density=None, num_labels=None):
        """A voxel volume: labels (nz, ny, nx) uint8 (0: empty, L into plane L - 1), voxels of `spacing` (one
        value or (x, y, z)), the minimum corner at `origin`, an optional f32 density of the labels' shape.
        num_labels defaults to labels.max().  Replaces any earlier volume; labels=None frees it."""
        if labels is None:
            self._check(self._lib.xrt_upload_volume(self._ctx, None, None, None, None, None, 0), "xrt_upload_volume")
            self._num_labels = 0
            return
        lab, den, dims, org, spc, m = _volume_arrays(labels, spacing, origin, density, num_labels)
        if m == 0:                         # (num_labels = 0 would free the volume)
            raise ValueError("the volume has no label above 0: give num_labels")
        self._check(self._lib.xrt_upload_volume(self._ctx, _u8ptr(lab), _fptr(den) if den is not None else None,
                                                _u32ptr(dims), _fptr(org), _fptr(spc), m), "xrt_upload_volume")
        self._num_labels = m

    def volume_paths(self, cam: Camera, row_begin: int = 0, row_end: int | None = None, num_labels: int | None = None):
        """The uploaded volume's planes over the strip: (M, rows, W) f32, plane m the length of each ray inside
        label m + 1 (times the voxels' density).  M is the uploaded volume's label count (num_labels overrides
        the buffer's size as stated to the library, which checks it against the volume)."""
        if row_end is None:
            row_end = cam.height
        m = self._num_labels if num_labels is None else int(num_labels)
        paths = np.empty((max(m, 1), max(row_end - row_begin, 0), cam.width), np.float32)
        self._check(self._lib.xrt_volume_paths(self._ctx, ctypes.byref(cam), row_begin, row_end, m, _fptr(paths)),
                    "xrt_volume_paths")
        return paths

    def volume_paths_device(self, cam: Camera, row_begin: int, row_end: int, num_labels: int, d_paths: int,
                            stream: int = 0):
        """Device-buffer volume trace (a raw device pointer: num_labels f32 planes of the strip, one after
        another); asynchronous on `stream`."""
        rc = self._lib.xrt_volume_paths_device(self._ctx, ctypes.byref(cam), row_begin, row_end, int(num_labels),
                                               d_paths or None, stream or None)
        self._check(rc, "xrt_volume_paths_device")

    def volume_wave_shape(self, rows: bool):
        """k_volume_paths' waves as 64 x 1 row segments (rows=True) or 8 x 8 tiles (the default): a timing A/B,
        the planes are the same (xrt_debug_volume_wave_shape)."""
        self._check(self._lib.xrt_debug_volume_wave_shape(self._ctx, int(bool(rows))), "xrt_debug_volume_wave_shape")

    def voxelize(self, dims, spacing, origin=(0.0, 0.0, 0.0), value=None, mask=True, labels=True, volume=None,
                 odd_columns=True, upload=False) -> dict:
        """The uploaded scene under its poses on a grid of dims (nx, ny, nz) voxels of `spacing` (one value or
        (x, y, z)) whose minimum corner is `origin` (xrt_voxelize): a dict of the outputs asked for -- mask
        (nz, ny, nx) uint16 (bit m: inside mesh m), labels uint8 (0, else 1 + the highest mesh), volume f32 (the
        sum of value[m] over the meshes a voxel lies in; asked for by default when `value`, one entry per mesh,
        is given) and odd_columns (one count per mesh: the columns over which it does not close).
        upload=True hands the labels to upload_volume on the same grid, one label per mesh."""
        d, org, spc = _voxel_grid_arrays(dims, spacing, origin)
        volume = value is not None if volume is None else volume
        val, m, lab, vol, odd = _voxel_outputs(d, self._num_meshes, value, mask, labels or upload, volume, odd_columns)
        rc = self._lib.xrt_voxelize(self._ctx, _u32ptr(d), _fptr(org), _fptr(spc), _fptr(val) if val is not None else None,
                                    _u16ptr(m) if m is not None else None, _u8ptr(lab) if lab is not None else None,
                                    _fptr(vol) if vol is not None else None,
                                    odd.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if odd is not None else None)
        self._check(rc, "xrt_voxelize")
        if upload:
            self.upload_volume(lab, spc, org, num_labels=self._num_meshes)
        return _voxel_result(m, lab if labels else None, vol, odd, self._num_meshes)

    def voxelize_device(self, dims, spacing, origin=(0.0, 0.0, 0.0), value=None, d_mask: int = 0, d_labels: int = 0,
                        d_volume: int = 0, d_odd_columns: int = 0, stream: int = 0):
        """Device-buffer voxelisation (raw device pointers, 0: not asked for: d_mask u16, d_labels u8 and d_volume
        f32 of nz * ny * nx entries, d_odd_columns XRT_MAX_MESHES u64); asynchronous on `stream`."""
        d, org, spc = _voxel_grid_arrays(dims, spacing, origin)
        val = None if value is None else np.ascontiguousarray(value, dtype=np.float32).reshape(-1)
        if val is not None and val.size != self._num_meshes:
            raise ValueError(f"value must hold one entry per mesh ({self._num_meshes}), got {val.size}")
        rc = self._lib.xrt_voxelize_device(self._ctx, _u32ptr(d), _fptr(org), _fptr(spc),
                                           _fptr(val) if val is not None else None, d_mask or None, d_labels or None,
                                           d_volume or None, d_odd_columns or None, stream or None)
        self._check(rc, "xrt_voxelize_device")

    def voxelize_threshold(self, columns: int = 0):
        """The footprint, in grid columns, from which the scatter queues a triangle for the tile waves (0: the
        default; 0xFFFFFFFF: a lane per triangle only): a timing A/B, the outputs are the same
        (xrt_debug_voxelize_threshold)."""
        self._check(self._lib.xrt_debug_voxelize_threshold(self._ctx, int(columns)), "xrt_debug_voxelize_threshold")

    def voxelize_stages(self, stages: int = 7):
        """The steps the next voxelisations enqueue, for timing them apart: 1 scatter + 2 scan + 4 clear
        (xrt_debug_voxelize_stages)."""
        self._check(self._lib.xrt_debug_voxelize_stages(self._ctx, int(stages)), "xrt_debug_voxelize_stages")

    def voxelize_counters(self) -> dict:
        """The last voxelisation's triangles by path (xrt_debug_voxelize_counters)."""
        c = (ctypes.c_uint64 * 4)()
        self._check(self._lib.xrt_debug_voxelize_counters(self._ctx, c), "xrt_debug_voxelize_counters")
        return {"direct": int(c[0]), "queued": int(c[1]), "entries": int(c[2]), "overflowed": int(c[3])}

    def fdk_filter(self, image, taps, weight=None) -> np.ndarray:
        """The row filter of FDK over an (H, W) image or a (P, H, W) stack: every row of image * weight (one
        (H, W) plane or None) correlated with `taps` (odd count) in f64, pixels outside the row skipped.  The
        image's shape."""
        a, wt, t, p, h, w = _fdk_filter_arrays(image, weight, taps)
        out = np.empty_like(a)
        self._check(self._lib.xrt_fdk_filter(self._ctx, w, h, p, _fptr(a), _fptr(wt) if wt is not None else None,
                                             _fptr(t), t.size, _fptr(out)), "xrt_fdk_filter")
        return out

    def fdk_filter_device(self, width: int, height: int, num_planes: int, d_image: int, d_taps: int, num_taps: int,
                          d_out: int, d_weight: int = 0, stream: int = 0):
        """fdk_filter over device buffers (raw pointers, the taps and the weight plane too); asynchronous on
        `stream`."""
        rc = self._lib.xrt_fdk_filter_device(self._ctx, int(width), int(height), int(num_planes), d_image or None,
                                             d_weight or None, d_taps or None, int(num_taps), d_out or None,
                                             stream or None)
        self._check(rc, "xrt_fdk_filter_device")

    def backproject(self, proj, matrices, dims, scale=1.0, slabs=None, volume=None, accumulate=False) -> np.ndarray:
        """The cone-beam backprojection of a (P, H, W) stack (or one (H, W) plane) under P (3, 4) f64 matrices
        into the slabs [slabs[0], slabs[1]) (None: all) of a grid of dims = (nx, ny, nz): (slabs, ny, nx) f32,
        each voxel's sum times `scale`; accumulate=True adds it to `volume` (a copy is returned)."""
        a, m, d, lo, hi, vol, p, h, w = _backproject_arrays(proj, matrices, dims, slabs, volume, accumulate)
        self._check(self._lib.xrt_backproject(self._ctx, w, h, p, _fptr(a), _dptr(m), _u32ptr(d), lo, hi, float(scale),
                                              int(bool(accumulate)), _fptr(vol)), "xrt_backproject")
        return vol

    def backproject_device(self, width: int, height: int, num_planes: int, d_proj: int, d_matrices: int, dims,
                           slab_begin: int, slab_end: int, scale: float, accumulate: bool, d_volume: int,
                           stream: int = 0):
        """backproject over device buffers (raw pointers: f32 planes, f64 matrices, the f32 slabs); asynchronous
        on `stream`."""
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        rc = self._lib.xrt_backproject_device(self._ctx, int(width), int(height), int(num_planes), d_proj or None,
                                              d_matrices or None, _u32ptr(d), int(slab_begin), int(slab_end),
                                              float(scale), int(bool(accumulate)), d_volume or None, stream or None)
        self._check(rc, "xrt_backproject_device")

    def fdk(self, projections, camera: Camera, poses, dims, origin, spacing, axis_point,
            window: int = _abi.XRT_RAMP_RAMLAK) -> np.ndarray:
        """FDK over a full turn: the (P, H, W) line integrals `projections`, taken by `camera` -- one Camera, or
        P of them for a turning source -- of an object under `poses` (P poses, or None: at rest), into the grid of
        dims = (nx, ny, nz) voxels of `spacing` with its minimum corner at `origin`, about the axis through
        `axis_point` parallel to the detector's up.  Weights, the ramp (2 W - 1 taps under `window`), the
        matrices and the backprojection: (nz, ny, nx) f32."""
        a, p, h, w = _lsf_planes(projections)
        cams = [camera] * p if isinstance(camera, Camera) else list(camera)
        poses = [None] * p if poses is None else list(poses)
        if len(cams) != p or len(poses) != p:
            raise ValueError(f"{p} projections need one camera or {p}, and {p} poses or None")
        taps = ramp_filter(2 * w - 1, window)
        mats = np.stack([backprojection_matrix(c, origin, spacing, q) for c, q in zip(cams, poses)])
        same = all(bytes(c) == bytes(cams[0]) for c in cams)
        if same:
            filtered = self.fdk_filter(a, taps, fdk_weights(cams[0]))
        else:
            filtered = np.stack([self.fdk_filter(a.reshape(p, h, w)[i], taps, fdk_weights(c))
                                 for i, c in enumerate(cams)])
        return self.backproject(filtered.reshape(p, h, w), mats, dims, fdk_scale(cams[0], axis_point, p))

    def forward_project(self, volume, spacing, rays, shape=None, mode=_abi.XRT_FP_PROJECT, meas=None) -> np.ndarray:
        """The line integrals of a (nz, ny, nx) f32 volume of voxels of `spacing` along the rays of P (3, 4) f64 ray
        matrices (ray_matrix), one (H, W) = `shape` plane each: (P, H, W) f32.  mode XRT_FP_RESIDUAL: (meas -
        integral) / the ray's length inside the grid, with `meas` a (P, H, W) stack that gives the shape."""
        v, d, spc, r, m, p, h, w = _forward_arrays(volume, spacing, rays, mode, meas, shape)
        out = np.empty((p, h, w), np.float32)
        self._check(self._lib.xrt_forward_project(self._ctx, w, h, p, _fptr(v), _u32ptr(d), _fptr(spc), _dptr(r), int(mode),
                                                  _fptr(m) if m is not None else None, _fptr(out)), "xrt_forward_project")
        return out

    def forward_project_device(self, width: int, height: int, num_planes: int, d_volume: int, dims, spacing,
                               d_rays: int, d_out: int, mode: int = _abi.XRT_FP_PROJECT, d_meas: int = 0,
                               stream: int = 0):
        """forward_project over device buffers (raw pointers: the f32 volume, f64 ray matrices, f32 planes);
        asynchronous on `stream`."""
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
        rc = self._lib.xrt_forward_project_device(self._ctx, int(width), int(height), int(num_planes), d_volume or None,
                                                  _u32ptr(d), _fptr(spc), d_rays or None, int(mode), d_meas or None,
                                                  d_out or None, stream or None)
        self._check(rc, "xrt_forward_project_device")

    def volume_update(self, x, corr, norm, relax=1.0, lo=-np.inf, hi=np.inf) -> np.ndarray:
        """x + relax * corr / norm where norm > 0, clamped to [lo, hi]; elsewhere x: the updated copy of x."""
        x, c, n = _update_arrays(x, corr, norm)
        self._check(self._lib.xrt_volume_update(self._ctx, x.size, _fptr(x), _fptr(c), _fptr(n), float(relax), float(lo),
                                                float(hi)), "xrt_volume_update")
        return x

    def volume_update_device(self, n: int, d_x: int, d_corr: int, d_norm: int, relax: float = 1.0, lo: float = -np.inf,
                             hi: float = np.inf, stream: int = 0):
        """volume_update over device buffers (raw pointers), in place in d_x; asynchronous on `stream`."""
        rc = self._lib.xrt_volume_update_device(self._ctx, int(n), d_x or None, d_corr or None, d_norm or None,
                                                float(relax), float(lo), float(hi), stream or None)
        self._check(rc, "xrt_volume_update_device")

    def tv_gradient(self, volume, eps: float = 1e-8) -> np.ndarray:
        """The gradient of the smoothed isotropic total variation sum sqrt(dx^2 + dy^2 + dz^2 + eps) (forward
        differences, none across the border) of a (nz, ny, nx) f32 volume: (nz, ny, nx) f32."""
        v, d = _tv_volume(volume)
        out = np.empty_like(v)
        self._check(self._lib.xrt_tv_gradient(self._ctx, _fptr(v), _u32ptr(d), float(eps), _fptr(out)), "xrt_tv_gradient")
        return out

    def tv_gradient_device(self, d_volume: int, dims, d_out: int, eps: float = 1e-8, stream: int = 0):
        """tv_gradient over device buffers (raw pointers to f32 volumes); asynchronous on `stream`."""
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        self._check(self._lib.xrt_tv_gradient_device(self._ctx, d_volume or None, _u32ptr(d), float(eps), d_out or None,
                                                     stream or None), "xrt_tv_gradient_device")

    def volume_sumsq(self, a, b=None) -> float:
        """The sum of the squares of a's entries, or of a - b's, in f64 in the fixed order of xrt_volume_sumsq."""
        a, b = _sumsq_arrays(a, b)
        out = np.zeros(1, np.float64)
        self._check(self._lib.xrt_volume_sumsq(self._ctx, a.size, _fptr(a), _fptr(b) if b is not None else None,
                                               _dptr(out)), "xrt_volume_sumsq")
        return float(out[0])

    def volume_sumsq_device(self, n: int, d_a: int, d_b: int, d_out: int, stream: int = 0):
        """volume_sumsq over device buffers (raw pointers; d_b 0: none); one f64 is written at d_out.  Asynchronous on
        `stream`."""
        self._check(self._lib.xrt_volume_sumsq_device(self._ctx, int(n), d_a or None, d_b or None, d_out or None,
                                                      stream or None), "xrt_volume_sumsq_device")

    def tv_descend(self, volume, steps: int, length: float, eps: float = 1e-8, lo: float = -np.inf,
                   hi: float = np.inf) -> np.ndarray:
        """`steps` steepest-descent steps of `length` each on the volume's total variation (tv_gradient, normalised),
        clamped to [lo, hi]: the descended copy of the volume."""
        v, d = _tv_volume(volume, copy=True)
        self._check(self._lib.xrt_tv_descend(self._ctx, _fptr(v), _u32ptr(d), float(eps), int(steps), float(length),
                                             float(lo), float(hi)), "xrt_tv_descend")
        return v

    def tv_descend_device(self, d_volume: int, dims, steps: int, length: float, eps: float = 1e-8, lo: float = -np.inf,
                          hi: float = np.inf, stream: int = 0):
        """tv_descend over a device volume (a raw pointer), in place; asynchronous on `stream`."""
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        self._check(self._lib.xrt_tv_descend_device(self._ctx, d_volume or None, _u32ptr(d), float(eps), int(steps),
                                                    float(length), float(lo), float(hi), stream or None),
                    "xrt_tv_descend_device")

    def sirt_matrices(self, projections, matrices, dims, spacing, iterations: int, subsets: int = 1, relax: float = 1.0,
                      lo: float = 0.0, hi: float = np.inf, start=None, tv=None) -> np.ndarray:
        """sirt under P given (3, 4) f64 backprojection matrices in place of cameras and poses."""
        a, m, d, spc, vol, p, h, w = _sirt_arrays(projections, matrices, dims, spacing, start)
        if tv is None:
            self._check(self._lib.xrt_sirt(self._ctx, w, h, p, _fptr(a), _dptr(m), _u32ptr(d), _fptr(spc), int(iterations),
                                           int(subsets), float(relax), float(lo), float(hi), _fptr(vol)), "xrt_sirt")
        else:
            params = _tv_params(tv)
            self._check(self._lib.xrt_sirt_tv(self._ctx, w, h, p, _fptr(a), _dptr(m), _u32ptr(d), _fptr(spc),
                                              int(iterations), int(subsets), float(relax), float(lo), float(hi),
                                              ctypes.byref(params), _fptr(vol)), "xrt_sirt_tv")
        return vol

    def sirt(self, projections, camera: Camera, poses, dims, origin, spacing, iterations: int, subsets: int = 1,
             relax: float = 1.0, lo: float = 0.0, hi: float = np.inf, start=None, tv=None) -> np.ndarray:
        """SIRT (subsets = 1) or OS-SART (subsets > 1; subset s holds the projections p with p mod subsets == s) of
        the (P, H, W) line integrals `projections`, taken by `camera` -- one Camera, or P of them -- of an object
        under `poses` (P poses, or None: at rest), into the grid of dims = (nx, ny, nz) voxels of `spacing` with its
        minimum corner at `origin`: `iterations` passes over every subset from `start` (None: zeros), each update
        relaxed by `relax` and clamped to [lo, hi].  tv = (steps, alpha, reduction, eps): after every iteration `steps`
        descent steps on the volume's total variation (tv_gradient with `eps`), each as long as alpha times the
        distance the iteration moved the volume, alpha multiplied by `reduction` from one iteration to the next
        (xrt_sirt_tv; alpha above about 0.5 flattens the object's level).  (nz, ny, nx) f32."""
        a, p, h, w = _lsf_planes(projections)
        cams = [camera] * p if isinstance(camera, Camera) else list(camera)
        poses = [None] * p if poses is None else list(poses)
        if len(cams) != p or len(poses) != p:
            raise ValueError(f"{p} projections need one camera or {p}, and {p} poses or None")
        mats = np.stack([backprojection_matrix(c, origin, spacing, q) for c, q in zip(cams, poses)])
        return self.sirt_matrices(a, mats, dims, spacing, iterations, subsets, relax, lo, hi, start, tv)

    def sirt_device(self, width: int, height: int, num_planes: int, d_proj: int, matrices, dims, spacing,
                    iterations: int, d_volume: int, subsets: int = 1, relax: float = 1.0, lo: float = 0.0,
                    hi: float = np.inf, stream: int = 0, tv=None):
        """sirt over device buffers (raw pointers: the f32 projections and the f32 volume, start and result);
        `matrices` is a host (P, 12) f64 array.  Asynchronous on `stream`."""
        m = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 12)
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
        if tv is not None:
            params = _tv_params(tv)
            rc = self._lib.xrt_sirt_tv_device(self._ctx, int(width), int(height), int(num_planes), d_proj or None, _dptr(m),
                                              _u32ptr(d), _fptr(spc), int(iterations), int(subsets), float(relax), float(lo),
                                              float(hi), ctypes.byref(params), d_volume or None, stream or None)
            self._check(rc, "xrt_sirt_tv_device")
            return
        rc = self._lib.xrt_sirt_device(self._ctx, int(width), int(height), int(num_planes), d_proj or None, _dptr(m),
                                       _u32ptr(d), _fptr(spc), int(iterations), int(subsets), float(relax), float(lo),
                                       float(hi), d_volume or None, stream or None)
        self._check(rc, "xrt_sirt_device")

    def poisson_project(self, volume, spacing, rays, counts, flat, background=None) -> np.ndarray:
        """The pixel stage of mltr: under P ray matrices, from the (P, H, W) measured `counts`, the (H, W) `flat`
        field and the (P, H, W) `background` (None: none), the expected counts psi = flat * exp(-line integral) and
        per pixel (psi - y psi / (psi + r), L psi psi / (psi + r)) with L the ray's length inside the grid:
        (P, H, W, 2) f32, (num, den) interleaved."""
        v, d, spc, r, y, f, b, p, h, w = _poisson_project_arrays(volume, spacing, rays, counts, flat, background)
        out = np.empty((p, h, w, 2), np.float32)
        self._check(self._lib.xrt_poisson_project(self._ctx, w, h, p, _fptr(v), _u32ptr(d), _fptr(spc), _dptr(r), _fptr(y),
                                                  _fptr(f), _fptr(b) if b is not None else None, _fptr(out)),
                    "xrt_poisson_project")
        return out

    def poisson_project_device(self, width: int, height: int, num_planes: int, d_volume: int, dims, spacing,
                               d_rays: int, d_counts: int, d_flat: int, d_pairs: int, d_background: int = 0,
                               stream: int = 0):
        """poisson_project over device buffers (raw pointers: the f32 volume, f64 ray matrices, f32 planes and
        pairs); asynchronous on `stream`."""
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
        rc = self._lib.xrt_poisson_project_device(self._ctx, int(width), int(height), int(num_planes), d_volume or None,
                                                  _u32ptr(d), _fptr(spc), d_rays or None, d_counts or None, d_flat or None,
                                                  d_background or None, d_pairs or None, stream or None)
        self._check(rc, "xrt_poisson_project_device")

    def backproject_update(self, pairs, matrices, dims, volume, relax=1.0, lo=-np.inf, hi=np.inf) -> np.ndarray:
        """The backprojections of both components of (P, H, W, 2) `pairs` under P (3, 4) f64 matrices and the update
        x + relax * num / den where den > 0, clamped to [lo, hi], in one pass: the updated copy of `volume`."""
        a, m, d, vol, p, h, w = _pairs_arrays(pairs, matrices, dims, volume)
        self._check(self._lib.xrt_backproject_update(self._ctx, w, h, p, _fptr(a), _dptr(m), _u32ptr(d), float(relax),
                                                     float(lo), float(hi), _fptr(vol)), "xrt_backproject_update")
        return vol

    def backproject_update_device(self, width: int, height: int, num_planes: int, d_pairs: int, d_matrices: int, dims,
                                  d_volume: int, relax: float = 1.0, lo: float = -np.inf, hi: float = np.inf,
                                  stream: int = 0):
        """backproject_update over device buffers (raw pointers), in place in d_volume; asynchronous on `stream`."""
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        rc = self._lib.xrt_backproject_update_device(self._ctx, int(width), int(height), int(num_planes), d_pairs or None,
                                                     d_matrices or None, _u32ptr(d), float(relax), float(lo), float(hi),
                                                     d_volume or None, stream or None)
        self._check(rc, "xrt_backproject_update_device")

    def mltr_matrices(self, counts, flat, matrices, dims, spacing, iterations: int, subsets: int = 1, relax: float = 1.0,
                      lo: float = 0.0, hi: float = np.inf, start=None, tv=None, background=None) -> np.ndarray:
        """mltr under P given (3, 4) f64 backprojection matrices in place of cameras and poses."""
        y, f, b, m, d, spc, vol, p, h, w = _mltr_arrays(counts, flat, background, matrices, dims, spacing, start)
        params = _tv_params(tv)
        self._check(self._lib.xrt_mltr(self._ctx, w, h, p, _fptr(y), _fptr(f), _fptr(b) if b is not None else None,
                                       _dptr(m), _u32ptr(d), _fptr(spc), int(iterations), int(subsets), float(relax),
                                       float(lo), float(hi), ctypes.byref(params) if params is not None else None,
                                       _fptr(vol)), "xrt_mltr")
        return vol

    def mltr(self, counts, flat, camera: Camera, poses, dims, origin, spacing, iterations: int, subsets: int = 1,
             relax: float = 1.0, lo: float = 0.0, hi: float = np.inf, start=None, tv=None, background=None) -> np.ndarray:
        """OS-MLTR: the maximum-likelihood reconstruction of the (P, H, W) transmission `counts` -- the measurement
        itself, no logarithm; zero counts are fine -- under the Poisson model counts ~ flat * exp(-line integral) +
        background, with `flat` an (H, W) plane (or a scalar) of the expected counts without the object and
        `background` (P, H, W) expected counts that did not come through it (scatter, dark current; None: none).
        Cameras, poses, grid, subsets, relax, the clamp, start and tv as sirt's.  (nz, ny, nx) f32."""
        a, p, h, w = _lsf_planes(counts)
        cams = [camera] * p if isinstance(camera, Camera) else list(camera)
        poses = [None] * p if poses is None else list(poses)
        if len(cams) != p or len(poses) != p:
            raise ValueError(f"{p} projections need one camera or {p}, and {p} poses or None")
        mats = np.stack([backprojection_matrix(c, origin, spacing, q) for c, q in zip(cams, poses)])
        return self.mltr_matrices(a, flat, mats, dims, spacing, iterations, subsets, relax, lo, hi, start, tv, background)

    def mltr_device(self, width: int, height: int, num_planes: int, d_counts: int, d_flat: int, matrices, dims, spacing,
                    iterations: int, d_volume: int, subsets: int = 1, relax: float = 1.0, lo: float = 0.0,
                    hi: float = np.inf, stream: int = 0, tv=None, d_background: int = 0):
        """mltr over device buffers (raw pointers: the f32 counts, flat plane, background or 0, and the f32 volume,
        start and result); `matrices` is a host (P, 12) f64 array.  Asynchronous on `stream`."""
        m = np.ascontiguousarray(matrices, dtype=np.float64).reshape(-1, 12)
        d = np.ascontiguousarray(dims, dtype=np.uint32).reshape(3)
        spc = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float32), (3,)))
        params = _tv_params(tv)
        rc = self._lib.xrt_mltr_device(self._ctx, int(width), int(height), int(num_planes), d_counts or None,
                                       d_flat or None, d_background or None, _dptr(m), _u32ptr(d), _fptr(spc),
                                       int(iterations), int(subsets), float(relax), float(lo), float(hi),
                                       ctypes.byref(params) if params is not None else None, d_volume or None,
                                       stream or None)
        self._check(rc, "xrt_mltr_device")

    def detector_response(self, image, lsf_x, lsf_y=None, out=True, u8=True):
        """The detector's line-spread function over an (H, W) image or a (P, H, W) stack of them (taps as
        written -- a correlation --, edges replicated, lsf_y None: lsf_x on both axes): (out f32, u8), of the
        image's shape; out=False or u8=False leaves that plane out (None)."""
        a, p, h, w = _lsf_planes(image)
        hx, hy = _lsf_arrays(lsf_x, lsf_y)
        o = np.empty_like(a) if out else None
        u = np.empty(a.shape, np.uint8) if u8 else None
        self._check(self._lib.xrt_detector_response(
            self._ctx, w, h, p, _fptr(a), _fptr(hx), hx.size, _fptr(hy), hy.size,
            _fptr(o) if o is not None else None, _u8ptr(u) if u is not None else None), "xrt_detector_response")
        return o, u

    def detector_response_device(self, width: int, height: int, num_planes: int, d_image: int, lsf_x, lsf_y,
                                 d_out: int, d_u8: int = 0, stream: int = 0):
        """detector_response over device buffers (raw pointers; the taps are host data and travel with the
        launch); asynchronous on `stream`."""
        hx, hy = _lsf_arrays(lsf_x, lsf_y)
        rc = self._lib.xrt_detector_response_device(self._ctx, int(width), int(height), int(num_planes),
                                                    d_image or None, _fptr(hx), hx.size, _fptr(hy), hy.size,
                                                    d_out or None, d_u8 or None, stream or None)
        self._check(rc, "xrt_detector_response_device")

    def scatter_source(self, paths, open, weights, mu, sigma, bin, lbuffer=True):
        """The scatter model's source (xrt_scatter_source) from render_paths' planes ((M, H, W) or (M, P, H, W) f32
        and the masks, or None) under the table (weights[K], mu[M, K], sigma[M, K]), binned by `bin`: (source
        (..., Hc, Wc), lbuffer of a plane stack's shape -- apply_spectrum's -- or None with lbuffer=False)."""
        w, mu, sg = _scatter_tables(weights, mu, sigma)
        p, o, planes, h, wd, shape = _scatter_planes(paths, open, mu.shape[0])
        d = max(int(bin), 1)
        src = np.empty(tuple(shape[:-2]) + ((h + d - 1) // d, (wd + d - 1) // d), np.float32)
        lb = np.empty(shape, np.float32) if lbuffer else None
        self._check(self._lib.xrt_scatter_source(
            self._ctx, wd, h, planes, mu.shape[0], _fptr(p), _u16ptr(o) if o is not None else None, _fptr(w), _fptr(mu),
            _fptr(sg), w.size, int(bin), _fptr(lb) if lb is not None else None, _fptr(src)), "xrt_scatter_source")
        return src, lb

    def scatter_source_device(self, width: int, height: int, num_planes: int, d_paths: int, d_open: int, weights, mu,
                              sigma, bin: int, d_lbuffer: int, d_source: int, stream: int = 0):
        """scatter_source over device buffers (raw pointers; the tables are host data and travel with the launch);
        asynchronous on `stream`."""
        w, mu, sg = _scatter_tables(weights, mu, sigma)
        rc = self._lib.xrt_scatter_source_device(self._ctx, int(width), int(height), int(num_planes), mu.shape[0],
                                                 d_paths or None, d_open or None, _fptr(w), _fptr(mu), _fptr(sg), w.size,
                                                 int(bin), d_lbuffer or None, d_source or None, stream or None)
        self._check(rc, "xrt_scatter_source_device")

    def scatter_add(self, blurred, amp, bin, shape, primary=None, out=True, scatter=True, u8=True):
        """The scatter model's last step (xrt_scatter_add): the G blurred coarse stacks (G, [P,] Hc, Wc) sampled on
        the fine (H, W) or (P, H, W) `shape`, weighed by amp[G], summed and added to `primary` (or None):
        (out, scatter, u8), any of them None when left out."""
        shape = tuple(int(v) for v in shape)
        b, a = _scatter_coarse(blurred, amp, shape, bin)
        pr = None if primary is None else np.ascontiguousarray(primary, dtype=np.float32).reshape(shape)
        o = np.empty(shape, np.float32) if out else None
        s = np.empty(shape, np.float32) if scatter else None
        u = np.empty(shape, np.uint8) if u8 else None
        planes = 1 if len(shape) == 2 else shape[0]
        self._check(self._lib.xrt_scatter_add(
            self._ctx, shape[-1], shape[-2], planes, int(bin), _fptr(b), a.size, _fptr(a),
            _fptr(pr) if pr is not None else None, _fptr(o) if o is not None else None,
            _fptr(s) if s is not None else None, _u8ptr(u) if u is not None else None), "xrt_scatter_add")
        return o, s, u

    def scatter_add_device(self, width: int, height: int, num_planes: int, bin: int, d_blurred: int, amp, d_primary: int,
                           d_out: int, d_out_scatter: int = 0, d_out_u8: int = 0, stream: int = 0):
        """scatter_add over device buffers (raw pointers; the amplitudes are host data and travel with the launch);
        asynchronous on `stream`."""
        a = np.ascontiguousarray(amp, dtype=np.float32).reshape(-1)
        rc = self._lib.xrt_scatter_add_device(self._ctx, int(width), int(height), int(num_planes), int(bin),
                                              d_blurred or None, a.size, _fptr(a), d_primary or None, d_out or None,
                                              d_out_scatter or None, d_out_u8 or None, stream or None)
        self._check(rc, "xrt_scatter_add_device")

    def scatter(self, paths, open, weights, mu, sigma, kernels, bin, width, height):
        """The scatter estimate end to end over render_paths' planes of `width` x `height` projections: the source
        and the L-buffer in one pass, the fork's hole fill of the L-buffer (the primary), one detector_response
        per scatter kernel -- `kernels` a list of (amp, taps_x, taps_y) on the grid binned by `bin` -- and the
        sum.  (total, scatter, primary), each of a plane stack's shape."""
        kernels = list(kernels)
        if not 1 <= len(kernels) <= _abi.XRT_MAX_SCATTER_KERNELS:
            raise ValueError(f"1 to {_abi.XRT_MAX_SCATTER_KERNELS} scatter kernels, got {len(kernels)}")
        src, lb = self.scatter_source(paths, open, weights, mu, sigma, bin)
        if lb.shape[-2:] != (int(height), int(width)):
            raise ValueError(f"the planes are {lb.shape[-2:]}, not ({height}, {width})")
        frames = lb.reshape(-1, int(height), int(width))
        primary = np.stack([self.hole_fill(f, int(width), int(height))[0].reshape(int(height), int(width))
                            for f in frames]).reshape(lb.shape)
        blurred = np.stack([self.detector_response(src, hx, hy, u8=False)[0] for _, hx, hy in kernels])
        total, sc, _ = self.scatter_add(blurred, [k[0] for k in kernels], bin, lb.shape, primary, u8=False)
        return total, sc, primary

    def log_projection(self, image, flat=None, dark=None, flat_value=None, t_min=0.0, sinograms=False):
        """Line integrals -ln((I - dark) / (flat - dark)) of an (H, W) image or a (P, H, W) stack of projections;
        flat and dark are one (H, W) plane each or None (flat None: the scalar flat_value); a transmission below
        t_min > 0 is raised to it.  Returns the image's shape, or (H, P, W) -- one sinogram per detector row --
        with sinograms=True."""
        a, f, d, p, h, w, fv, order, shape = _projection_arrays(image, flat, dark, flat_value, sinograms)
        out = np.empty(shape, np.float32)
        self._check(self._lib.xrt_log_projection(
            self._ctx, w, h, p, _fptr(a), _fptr(f) if f is not None else None, _fptr(d) if d is not None else None,
            fv, float(t_min), order, _fptr(out)), "xrt_log_projection")
        return out

    def log_projection_device(self, width: int, height: int, num_planes: int, d_image: int, d_out: int,
                              d_flat: int = 0, d_dark: int = 0, flat_value: float = 0.0, t_min: float = 0.0,
                              sinograms: bool = False, stream: int = 0):
        """log_projection over device buffers (raw pointers; d_out == d_image is in place, projection order
        only); asynchronous on `stream`."""
        order = _abi.XRT_ORDER_SINOGRAMS if sinograms else _abi.XRT_ORDER_PROJECTIONS
        rc = self._lib.xrt_log_projection_device(self._ctx, int(width), int(height), int(num_planes), d_image or None,
                                                 d_flat or None, d_dark or None, float(flat_value), float(t_min), order,
                                                 d_out or None, stream or None)
        self._check(rc, "xrt_log_projection_device")

    def photon_noise(self, image, gain, seed, counts=False, first_index=0):
        """Photon noise over an (H, W) image or a (P, H, W) stack: each pixel a Poisson count of mean
        image * gain, drawn from (seed, first_index + the pixel's flat index) alone, returned as counts or --
        counts=False -- divided by gain again.  The image's shape."""
        a, p, h, w = _lsf_planes(image)
        out = np.empty_like(a)
        self._check(self._lib.xrt_photon_noise(self._ctx, w, h, p, _fptr(a), float(gain), int(seed), int(first_index),
                                               _noise_mode(counts), _fptr(out)), "xrt_photon_noise")
        return out

    def photon_noise_device(self, width: int, height: int, num_planes: int, d_image: int, d_out: int, gain: float,
                            seed: int, counts: bool = False, first_index: int = 0, stream: int = 0):
        """photon_noise over device buffers (raw pointers; d_out == d_image is in place); asynchronous on
        `stream`."""
        rc = self._lib.xrt_photon_noise_device(self._ctx, int(width), int(height), int(num_planes), d_image or None,
                                               float(gain), int(seed), int(first_index), _noise_mode(counts),
                                               d_out or None, stream or None)
        self._check(rc, "xrt_photon_noise_device")

    def debug_poisson(self, lam, words) -> np.ndarray:
        """host_poisson on the device (xrt_debug_poisson_batch, a probe)."""
        lam, words = _poisson_arrays(lam, words)
        out = np.empty(lam.shape, np.float64)
        self._check(self._lib.xrt_debug_poisson_batch(self._ctx, _dptr(lam), _u32ptr(words), lam.size, _dptr(out)),
                    "xrt_debug_poisson_batch")
        return out

    def area_integrate(self, image, bin=1, weights=None, u8=False):
        """Area sampling: the weighted mean over S sub-sources and over each pixel's bin_y x bin_x block of finer
        samples, in f64, rounded once.  `image` is (Hb, Wb), (S, Hb, Wb) or (P, S, Hb, Wb); `bin` an int or
        (bin_y, bin_x); `weights` S values, ones by default.  The (H, W) or (P, H, W) image -- with u8=True
        (image, u8)."""
        a, w, p, s, h, wd, by, bx, shape = _area_arrays(image, bin, weights)
        out = np.empty(shape, np.float32)
        u = np.empty(shape, np.uint8) if u8 else None
        self._check(self._lib.xrt_area_integrate(self._ctx, wd, h, bx, by, s, p, _fptr(w), _fptr(a), _fptr(out),
                                                 _u8ptr(u) if u is not None else None), "xrt_area_integrate")
        return (out, u) if u8 else out

    def area_integrate_device(self, width: int, height: int, num_planes: int, d_image: int, d_out: int, d_out_u8: int = 0,
                              bin=1, weights=None, num_sources: int | None = None, stream: int = 0):
        """area_integrate over device buffers (raw pointers; width and height are the OUTPUT's; the weights are host
        values that travel with the launch); asynchronous on `stream`."""
        by, bx = _area_bins(bin)
        if weights is None:
            weights = np.ones(1 if num_sources is None else int(num_sources), np.float32)
        w = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        s = w.size if num_sources is None else int(num_sources)
        if w.size != s:
            raise ValueError(f"{s} sub-sources need {s} weights, got {w.size}")
        rc = self._lib.xrt_area_integrate_device(self._ctx, int(width), int(height), bx, by, s, int(num_planes), _fptr(w),
                                                 d_image or None, d_out or None, d_out_u8 or None, stream or None)
        self._check(rc, "xrt_area_integrate_device")

    def render_area(self, cam: Camera, bin: int = 1, spot=None):
        """The attenuation model's image of `cam` under area sampling: every pixel the mean of bin x bin samples of
        its area, seen from each sub-source of the focal spot `spot` = (size_u, size_v, nu, nv) (None: the point
        source).  The sub-cameras' renders stay in one device buffer and are integrated there.  (H, W) f32."""
        import torch
        cams, weights = focal_spot(cam, *spot) if spot is not None else ([cam], np.ones(1, np.float32))
        fine = [supersampled_camera(c, bin) for c in cams]
        hb, wb = fine[0].height, fine[0].width
        dev = torch.device("cuda", self.device)
        samples = torch.empty((len(fine), hb, wb), dtype=torch.float32, device=dev)
        out = torch.empty((cam.height, cam.width), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        for k, c in enumerate(fine):
            self.render_rows_device(c, 0, hb, samples[k].data_ptr(), 0, 0)
        self.area_integrate_device(cam.width, cam.height, 1, samples.data_ptr(), out.data_ptr(), 0, int(bin), weights)
        self.read_stats()                                   # (synchronises the renders' stream)
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()

    def render_signed(self, cam: Camera):
        """The L-buffer fork end to end: (image f32, lbuffer f32 with -1 flags, u8, Stats)."""
        return self._render_model(self._lib.xrt_render_signed, "xrt_render_signed", cam)

    def hole_fill(self, lbuffer: np.ndarray, width: int, height: int):
        """The fork's hole fill of a whole-frame L-buffer: (image f32, u8)."""
        lb = np.ascontiguousarray(lbuffer, dtype=np.float32).reshape(-1)
        if lb.size != width * height:
            raise ValueError("L-buffer size does not match width x height")
        img = np.empty_like(lb)
        u8 = np.empty(lb.size, np.uint8)
        self._check(self._lib.xrt_hole_fill(self._ctx, width, height, _fptr(lb), _fptr(img), _u8ptr(u8)),
                    "xrt_hole_fill")
        return img, u8

    def hole_fill_device(self, width: int, height: int, d_lbuffer: int, d_image: int, d_u8: int, stream: int = 0):
        self._check(self._lib.xrt_hole_fill_device(self._ctx, width, height, d_lbuffer, d_image, d_u8, stream),
                    "xrt_hole_fill_device")

    def set_hit_capacity(self, capacity: int):
        self._check(self._lib.xrt_set_hit_capacity(self._ctx, int(capacity)), "xrt_set_hit_capacity")

    def set_bin_capacity(self, entries: int):
        self._check(self._lib.xrt_set_bin_capacity(self._ctx, int(entries)), "xrt_set_bin_capacity")

    def set_fill_plan(self, mode: int):
        """BINNED fill plan: 1 on (default), 0 off, 2 every region planned empty (test hook)."""
        self._check(self._lib.xrt_set_fill_plan(self._ctx, int(mode)), "xrt_set_fill_plan")

    def fill_regions(self) -> int:
        """Regions the last enqueued BINNED frame rendered through the fill plan."""
        n = ctypes.c_uint32()
        self._check(self._lib.xrt_debug_fill_regions(self._ctx, ctypes.byref(n)), "xrt_debug_fill_regions")
        return n.value

    def geometry_counters(self) -> dict:
        """BINNED frames by geometry path: sized, reused (moving camera), plan misses, list overflows."""
        c = (ctypes.c_uint64 * 4)()
        self._check(self._lib.xrt_debug_geometry_counters(self._ctx, c), "xrt_debug_geometry_counters")
        return dict(zip(("sizings", "reused", "plan_misses", "overflows"), (int(v) for v in c)))

    def first_frames(self) -> dict:
        """Frames of a new geometry sized on the device, and those whose pool was regrown (xrt_debug_first_frames)."""
        c = (ctypes.c_uint64 * 4)()
        self._check(self._lib.xrt_debug_first_frames(self._ctx, c), "xrt_debug_first_frames")
        return {"device_sized": int(c[0]), "recounted": int(c[1]), "last_pairs": int(c[2]), "last_pool": int(c[3])}

    def wave_times(self, frames_back: int = 0) -> np.ndarray:
        """Timing records of the render frames_back frames before the last (xrt_debug_wave_times):
        (n, 2) u32 s_memrealtime start / end (100 MHz, low 32 bits), one per statistics record."""
        n = ctypes.c_uint64()
        self._check(self._lib.xrt_debug_wave_times(self._ctx, frames_back, None, 0, ctypes.byref(n)),
                    "xrt_debug_wave_times")
        out = np.zeros((n.value, 2), np.uint32)
        self._check(self._lib.xrt_debug_wave_times(self._ctx, frames_back,
                                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                   n.value, ctypes.byref(n)), "xrt_debug_wave_times")
        return out

    def block_records(self) -> np.ndarray:
        """The last render's statistics records (xrt_debug_block_records): (n, 8) u32 -- rays,
        hit rays, odd rays, overflow rays, hits, tile tests, candidates, max hits."""
        n = ctypes.c_uint64()
        self._check(self._lib.xrt_debug_block_records(self._ctx, None, 0, ctypes.byref(n)),
                    "xrt_debug_block_records")
        out = np.zeros((n.value, 8), np.uint32)
        self._check(self._lib.xrt_debug_block_records(self._ctx, out.ctypes.data, out.nbytes, ctypes.byref(n)),
                    "xrt_debug_block_records")
        return out

    def tile_plan_counters(self) -> dict:
        """Binned frames rendered with a tile plan, tile plans taken (xrt_debug_tile_plan)."""
        c = (ctypes.c_uint64 * 2)()
        self._check(self._lib.xrt_debug_tile_plan(self._ctx, c), "xrt_debug_tile_plan")
        return {"frames": int(c[0]), "plans": int(c[1])}

    def prep_times(self, enable=None) -> np.ndarray:
        """k_prep's per-wave timestamps of the last recorded launch (xrt_debug_prep_times):
        (n, 8) u32 stamps (xrt_debug.h); enable turns recording on / off."""
        n = ctypes.c_uint64()
        en = -1 if enable is None else int(bool(enable))
        self._check(self._lib.xrt_debug_prep_times(self._ctx, en, None, 0, ctypes.byref(n)), "xrt_debug_prep_times")
        out = np.zeros((n.value, 8), np.uint32)
        if n.value and enable is None:
            self._check(self._lib.xrt_debug_prep_times(self._ctx, -1, out.ctypes.data, n.value, ctypes.byref(n)),
                        "xrt_debug_prep_times")
        return out

    def set_tile_plan(self, on: bool):
        """The tile plan on / off for later frames (off by default: xrt_debug_set_tile_plan)."""
        self._check(self._lib.xrt_debug_set_tile_plan(self._ctx, 1 if on else 0), "xrt_debug_set_tile_plan")

    def set_ray_table(self, on: bool):
        """The ray table on / off for later frames (on by default: xrt_debug_set_ray_table)."""
        self._check(self._lib.xrt_debug_set_ray_table(self._ctx, 1 if on else 0), "xrt_debug_set_ray_table")

    def ray_table_counters(self) -> dict:
        """Fills launched, frames rendered from the ray table, frames in its scope that
        computed their rays, bytes held (xrt_debug_ray_table_counters)."""
        c = (ctypes.c_uint64 * 4)()
        self._check(self._lib.xrt_debug_ray_table_counters(self._ctx, c), "xrt_debug_ray_table_counters")
        return dict(zip(("fills", "frames", "computed", "bytes"), (int(v) for v in c)))

    def read_ray_table(self):
        """(table, (width, height, row_begin, row_end)): the valid ray table's floats, padding included, in
        ray_table_index's layout, and its key's sizes (xrt_debug_ray_table_read; XrtError while none is valid)."""
        cap = max(self.ray_table_counters()["bytes"] // 4, 1)
        out = np.zeros(cap, np.float32)
        dims = (ctypes.c_uint32 * 4)()
        self._check(self._lib.xrt_debug_ray_table_read(self._ctx, out.ctypes.data, cap, dims),
                    "xrt_debug_ray_table_read")
        W, H, r0, r1 = (int(v) for v in dims)
        return out[:ray_table_index(W, H, r0, r1, r0, 0)[1]].copy(), (W, H, r0, r1)

    def pipeline_counters(self) -> dict:
        """Frames rendered from a preparation made ahead, preparations dropped, renders
        launched with no wait, renders launched after a host wait (xrt_debug_pipeline_counters)."""
        c = (ctypes.c_uint64 * 4)()
        self._check(self._lib.xrt_debug_pipeline_counters(self._ctx, c), "xrt_debug_pipeline_counters")
        return dict(zip(("ahead_used", "ahead_dropped", "no_wait", "host_waits"), (int(v) for v in c)))

    def host_call_ms(self) -> dict:
        """Host time of the last render_rows call, ms (xrt_debug_host_call_ms)."""
        ms = (ctypes.c_double * 16)()
        self._check(self._lib.xrt_debug_host_call_ms(self._ctx, ms), "xrt_debug_host_call_ms")
        keys = ("device_planes", "enqueue", "render_wait", "d2h", "d2h_copy_threads", "d2h_mb", "stats", "total",
                "of_which_hipmalloc", "of_which_list_sizing", "of_which_device_sync", "of_which_prep_wait",
                "of_which_launches", "device_sync_prep_stream", "device_sync_set_events",
                "device_sync_last_stream")
        return dict(zip(keys, (float(v) for v in ms)))

    @staticmethod
    def last_destroy_ms() -> dict:
        """Phases of the last xrt_destroy in this process, ms (xrt_debug_destroy_ms)."""
        ms = (ctypes.c_double * 4)()
        _abi.load().xrt_debug_destroy_ms(ms)
        return dict(zip(("wait_for_work", "device_frees", "pinned_host_frees", "streams_events"),
                        (float(v) for v in ms)))

    def render_rows(self, cam: Camera, row_begin: int = 0, row_end: int | None = None,
                    image=True, lbuffer=True, u8=True, out=None):
        """Host-buffer render of rows [row_begin, row_end); returns (image, lbuffer, u8, stats).
        `out`: (image, lbuffer, u8) arrays to render into instead of new ones."""
        if row_end is None:
            row_end = cam.height
        n = max(row_end - row_begin, 0) * cam.width
        if out is not None:
            img, lb, u = out
            for a, dt in ((img, np.float32), (lb, np.float32), (u, np.uint8)):
                if a is not None and (a.dtype != dt or a.size != n or not a.flags.c_contiguous):
                    raise ValueError("out arrays must be contiguous, of the strip's size and dtype")
        else:
            img = np.empty(n, np.float32) if image else None
            lb = np.empty(n, np.float32) if lbuffer else None
            u = np.empty(n, np.uint8) if u8 else None
        st = Stats()
        rc = self._lib.xrt_render_rows(
            self._ctx, ctypes.byref(cam), row_begin, row_end,
            _fptr(img) if img is not None else None,
            _fptr(lb) if lb is not None else None,
            _u8ptr(u) if u is not None else None, ctypes.byref(st))
        self._check(rc, "xrt_render_rows")
        return img, lb, u, st

    def render_rows_device(self, cam: Camera, row_begin: int, row_end: int, d_image: int,
                           d_lbuffer: int, d_u8: int, stream: int = 0):
        """Device-buffer render (raw device pointers, hipStream_t as int); asynchronous."""
        rc = self._lib.xrt_render_rows_device(self._ctx, ctypes.byref(cam), row_begin, row_end,
                                              d_image or None, d_lbuffer or None, d_u8 or None,
                                              stream or None)
        self._check(rc, "xrt_render_rows_device")

    def read_stats(self) -> Stats:
        st = Stats()
        self._check(self._lib.xrt_read_stats(self._ctx, ctypes.byref(st)), "xrt_read_stats")
        return st

    def render_frames_device(self, cam: Camera, row_begin: int, row_end: int, n_frames: int, sets):
        """n_frames frames of one geometry in one call (xrt_render_frames_device); frame k into
        sets[k % len(sets)] = (d_image, d_lbuffer, d_u8, stream) raw pointers (0 = none / default)."""
        ns = len(sets)
        arrs = [(ctypes.c_void_p * ns)(*[(s[i] or None) for s in sets]) for i in range(4)]
        rc = self._lib.xrt_render_frames_device(self._ctx, ctypes.byref(cam), row_begin, row_end, int(n_frames), ns,
                                                *arrs)
        self._check(rc, "xrt_render_frames_device")

    def render_frames(self, cam: Camera, n_frames: int, row_begin: int = 0, row_end: int | None = None):
        """n_frames frames back to back, the last one's host planes: (image, lbuffer, u8, stats, ms_per_frame)."""
        if row_end is None:
            row_end = cam.height
        n = max(row_end - row_begin, 0) * cam.width
        img, lb, u = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.uint8)
        st = Stats()
        ms = ctypes.c_double()
        self._check(self._lib.xrt_render_frames(self._ctx, ctypes.byref(cam), row_begin, row_end, int(n_frames),
                                                _fptr(img), _fptr(lb), _u8ptr(u), ctypes.byref(st), ctypes.byref(ms)),
                    "xrt_render_frames")
        return img, lb, u, st, ms.value

    def set_miss_code(self, bits: int):
        """L-buffer bits of a miss in later renders: 0 (+inf) or XRT_MISS_TRANSIT."""
        self._check(self._lib.xrt_set_miss_code(self._ctx, int(bits)), "xrt_set_miss_code")

    def expand_rows_device(self, num_pixels: int, d_lbuffer: int, d_image: int, d_u8: int, stream: int = 0):
        """A received transit L-buffer into image / u8 planes, in place (device pointers)."""
        rc = self._lib.xrt_expand_rows_device(self._ctx, int(num_pixels), d_lbuffer or None, d_image or None,
                                              d_u8 or None, stream or None)
        self._check(rc, "xrt_expand_rows_device")

    def plan_region_map(self, width: int, rows: int):
        """(map, n_packed) of the last frame's strip: map[r] = packed index of region r
        (row-major 32x32 regions), 0xFFFFFFFF for a region its fill plan filled."""
        n = -(-width // 32) * -(-rows // 32)
        m = np.zeros(n, np.uint32)
        k = ctypes.c_uint32()
        self._check(self._lib.xrt_plan_region_map(self._ctx, width, rows,
                                                  m.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n,
                                                  ctypes.byref(k)), "xrt_plan_region_map")
        return m, k.value

    def pack_regions_device(self, width: int, rows: int, d_map: int, d_lbuffer: int, d_packed: int, stream: int = 0):
        """A transit L-buffer strip into its packed regions (device pointers)."""
        self._check(self._lib.xrt_pack_regions_device(self._ctx, width, rows, d_map, d_lbuffer, d_packed,
                                                      stream or None), "xrt_pack_regions_device")

    def unpack_regions_device(self, width: int, rows: int, d_map: int, d_packed: int, d_lbuffer: int, d_image: int,
                              d_u8: int, stream: int = 0):
        """Packed regions into a strip's L / image / u8 planes (device pointers; 0 skips a plane)."""
        self._check(self._lib.xrt_unpack_regions_device(self._ctx, width, rows, d_map, d_packed, d_lbuffer or None,
                                                        d_image or None, d_u8 or None, stream or None),
                    "xrt_unpack_regions_device")

    def set_transit_layout(self, packed_floats: int):
        """Render L-buffers in the packed layout (capacity in floats; 0: row-major)."""
        self._check(self._lib.xrt_set_transit_layout(self._ctx, int(packed_floats)), "xrt_set_transit_layout")

    def unpack_blocks_device(self, width: int, n_blocks: int, d_desc: int, d_packed: int, d_lbuffer: int,
                             d_image: int, d_u8: int, stream: int = 0):
        """Many strips' packed regions into whole-frame planes in one launch (see xrt.h)."""
        self._check(self._lib.xrt_unpack_blocks_device(self._ctx, width, n_blocks, d_desc, d_packed,
                                                       d_lbuffer or None, d_image or None, d_u8 or None,
                                                       stream or None), "xrt_unpack_blocks_device")

    def plan_hit_layout(self):
        """(tile_hits, words) of the last frame's geometry (xrt_plan_hit_layout): the
        hit count of each tile of its fill plan (16 per tile slot) and the words of
        its hit-layout message."""
        n, w = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.xrt_plan_hit_layout(self._ctx, None, 0, ctypes.byref(n), ctypes.byref(w)),
                    "xrt_plan_hit_layout")
        hits = np.zeros(n.value, np.uint32)
        self._check(self._lib.xrt_plan_hit_layout(self._ctx, hits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                  n.value, ctypes.byref(n), ctypes.byref(w)), "xrt_plan_hit_layout")
        return hits, w.value

    def set_transit_hits(self, capacity_words: int):
        """Render L-buffers in the hit layout (message capacity in 32-bit words; 0: off)."""
        self._check(self._lib.xrt_set_transit_hits(self._ctx, int(capacity_words)), "xrt_set_transit_hits")

    def unpack_hits_device(self, width: int, n_blocks: int, d_desc: int, d_tdesc: int, d_msg: int, d_lbuffer: int,
                           d_image: int, d_u8: int, d_bad: int = 0, stream: int = 0):
        """Many strips' hit-layout messages into whole-frame planes in one launch (see xrt.h)."""
        self._check(self._lib.xrt_unpack_hits_device(self._ctx, width, n_blocks, d_desc, d_tdesc, d_msg,
                                                     d_lbuffer or None, d_image or None, d_u8 or None,
                                                     d_bad or None, stream or None), "xrt_unpack_hits_device")

    def timing_begin(self):
        self._check(self._lib.xrt_timing_begin(self._ctx), "xrt_timing_begin")

    def timing_end(self):
        """(summed kernel spans in ms, sampled launches) of the render kernel since
        timing_begin: every render's in-kernel span (its waves' s_memrealtime
        records, first start to last end)."""
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        self._check(self._lib.xrt_timing_end(self._ctx, ctypes.byref(ms), ctypes.byref(n)),
                    "xrt_timing_end")
        return ms.value, n.value

    def timing_events(self):
        """(summed ms, launches) of the HIP start/stop event pairs on every 16th render
        dispatch of the last timed region (a cross-check of timing_end)."""
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        self._check(self._lib.xrt_timing_events(self._ctx, ctypes.byref(ms), ctypes.byref(n)),
                    "xrt_timing_events")
        return ms.value, n.value

    def probe_intersect(self, rays: np.ndarray, tris: np.ndarray):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        n = len(rays)
        hit = np.zeros(n, np.uint8)
        t = np.zeros(n, np.float32)
        self._check(self._lib.xrt_probe_intersect(self._ctx, _fptr(rays), _fptr(tris), n,
                                                  _u8ptr(hit), _fptr(t)), "xrt_probe_intersect")
        return hit, t

    def probe_prep(self, cam: Camera, n: int):
        """(records (n,16), footprint (n,16)) of the uploaded mesh (n triangles) for `cam`."""
        rec = np.zeros((n, 16), np.float32)
        fp = np.zeros((n, 16), np.float32)
        self._check(self._lib.xrt_probe_prep(self._ctx, ctypes.byref(cam), _fptr(rec), _fptr(fp)),
                    "xrt_probe_prep")
        return rec, fp

    def probe_math(self, op: int, x: np.ndarray):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        self._check(self._lib.xrt_probe_math(self._ctx, int(op), _fptr(x), _fptr(out), x.size),
                    "xrt_probe_math")
        return out


class MultiContext:
    """xrt_multi: row strips over several devices, gathered into device 0's
    frame with RCCL (include/xrt.h, "multi-GPU").  A device listed twice
    rehearses the strip logic on one GPU (device-copy gather)."""

    def __init__(self, devices):
        self._lib = _abi.load()
        self._m = _abi._MultiP()
        arr = (ctypes.c_int * len(devices))(*devices)
        rc = self._lib.xrt_multi_create(arr, len(devices), ctypes.byref(self._m))
        if rc != _abi.XRT_OK:
            raise XrtError(rc, self._lib.xrt_multi_last_error(None).decode())
        self.devices = list(devices)

    def close(self):
        if self._m:
            self._lib.xrt_multi_destroy(self._m)
            self._m = _abi._MultiP()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != _abi.XRT_OK:
            raise XrtError(rc, f"{what}: {self._lib.xrt_multi_last_error(self._m).decode()}")

    def upload_mesh(self, tris: np.ndarray):
        tris = np.ascontiguousarray(tris, dtype=np.float32).reshape(-1, 9)
        self._check(self._lib.xrt_multi_upload_mesh(self._m, _fptr(tris), len(tris)), "xrt_multi_upload_mesh")

    def set_kernel(self, kernel: int):
        self._check(self._lib.xrt_multi_set_kernel(self._m, int(kernel)), "xrt_multi_set_kernel")

    def set_gather(self, mode: int):
        """XRT_GATHER_AUTO / _COPY / _RCCL (a one-rank RCCL communicator when one
        device is listed n times)."""
        self._check(self._lib.xrt_multi_set_gather(self._m, int(mode)), "xrt_multi_set_gather")

    def set_model(self, model: int, mu: float = 0.1037):
        self._check(self._lib.xrt_multi_set_model(self._m, int(model), float(np.float32(mu))), "xrt_multi_set_model")

    def upload_scene(self, meshes):
        tris, counts = _scene_arrays(meshes)
        self._check(self._lib.xrt_multi_upload_scene(self._m, _fptr(tris),
                                                     counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                     len(counts)), "xrt_multi_upload_scene")

    def set_pose(self, mesh: int, pose=None):
        """Context.set_pose on every device."""
        q = _pose_array(pose)
        self._check(self._lib.xrt_multi_set_pose(self._m, int(mesh), _fptr(q) if q is not None else None),
                    "xrt_multi_set_pose")

    def reset_poses(self):
        self._check(self._lib.xrt_multi_reset_poses(self._m), "xrt_multi_reset_poses")

    def set_materials(self, mu):
        mu = np.ascontiguousarray(mu, dtype=np.float32).reshape(-1)
        self._check(self._lib.xrt_multi_set_materials(self._m, _fptr(mu), mu.size), "xrt_multi_set_materials")

    def render_materials(self, cam: Camera):
        """The materials model's frame: (hole-filled image, lbuffer with -1 flags, u8, stats)."""
        return self.render(cam)

    def set_spectrum(self, weights, mu):
        w, mu = _spectrum_arrays(weights, mu)
        self._check(self._lib.xrt_multi_set_spectrum(self._m, _fptr(w), _fptr(mu), mu.shape[0], w.size),
                    "xrt_multi_set_spectrum")

    def render_spectrum(self, cam: Camera):
        """The spectrum model's frame: (hole-filled image, lbuffer with -1 flags, u8, stats)."""
        return self.render(cam)

    def set_split(self, mode: int, link_bytes_per_us: float = 0.0):
        """XRT_SPLIT_EQUAL (the reference's H/N rows) or XRT_SPLIT_BALANCED (the default;
        link rate in bytes/us, 0 = measured once)."""
        self._check(self._lib.xrt_multi_set_split(self._m, int(mode), float(link_bytes_per_us)), "xrt_multi_set_split")

    def set_transit(self, mode: int):
        """XRT_TRANSIT_HITS (the default: hit masks and hit values once a strip geometry
        repeats) or XRT_TRANSIT_PACKED (the fill plan's 32x32 blocks)."""
        self._check(self._lib.xrt_multi_set_transit(self._m, int(mode)), "xrt_multi_set_transit")

    def transit_stats(self):
        """{frames_hits, frames_packed, last_bytes, bad} (xrt_multi_transit_stats)."""
        out = (ctypes.c_uint64 * 4)()
        self._check(self._lib.xrt_multi_transit_stats(self._m, out), "xrt_multi_transit_stats")
        return {"frames_hits": int(out[0]), "frames_packed": int(out[1]), "last_bytes": int(out[2]),
                "bad": int(out[3])}

    def plan_stats(self):
        """{plans, equal_no_model, link_probes, models} (xrt_multi_plan_stats)."""
        out = (ctypes.c_uint64 * 4)()
        self._check(self._lib.xrt_multi_plan_stats(self._m, out), "xrt_multi_plan_stats")
        return dict(zip(("plans", "equal_no_model", "link_probes", "models"), (int(v) for v in out)))

    def corrupt_hit_plan(self):
        """Test hook: the next hit frame's receive disagrees with its plan (xrt_multi_debug_corrupt_hit_plan)."""
        self._check(self._lib.xrt_multi_debug_corrupt_hit_plan(self._m), "xrt_multi_debug_corrupt_hit_plan")

    def plan(self, cam: Camera):
        """The strips of cam's frame: ([(begin, end) per device], {link, span_us, step_us})."""
        n = len(self.devices)
        b = (ctypes.c_uint32 * (2 * n))()
        info = (ctypes.c_double * 3)()
        self._check(self._lib.xrt_multi_plan(self._m, ctypes.byref(cam), b, info), "xrt_multi_plan")
        return ([(int(b[2 * g]), int(b[2 * g + 1])) for g in range(n)],
                {"link_bytes_per_us": info[0], "frame_span_us": info[1], "predicted_step_us": info[2]})

    def render(self, cam: Camera, image=True, lbuffer=True, u8=True):
        """The whole frame, gathered to the host: (image, lbuffer, u8, stats)."""
        n = cam.width * cam.height
        img = np.empty(n, np.float32) if image else None
        lb = np.empty(n, np.float32) if lbuffer else None
        u = np.empty(n, np.uint8) if u8 else None
        st = Stats()
        rc = self._lib.xrt_render_rows_multi(self._m, ctypes.byref(cam),
                                             _fptr(img) if img is not None else None,
                                             _fptr(lb) if lb is not None else None,
                                             _u8ptr(u) if u is not None else None, ctypes.byref(st))
        self._check(rc, "xrt_render_rows_multi")
        return img, lb, u, st

    def render_device(self, cam: Camera, d_image: int, d_lbuffer: int, d_u8: int, stream: int = 0):
        """Into device-0 planes (raw pointers), ordered on device 0's stream; asynchronous."""
        rc = self._lib.xrt_render_rows_multi_device(self._m, ctypes.byref(cam), d_image or None,
                                                    d_lbuffer or None, d_u8 or None, stream or None)
        self._check(rc, "xrt_render_rows_multi_device")

    def read_stats(self) -> Stats:
        st = Stats()
        self._check(self._lib.xrt_multi_read_stats(self._m, ctypes.byref(st)), "xrt_multi_read_stats")
        return st
