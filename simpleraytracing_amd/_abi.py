"""ctypes bindings of the C ABI (include/xrt.h, include/xrt_host.h).

The shared libraries are built in-tree by ``simpleraytracing_amd/csrc/Makefile``
into ``simpleraytracing_amd/lib/``.  Loading fails loudly when they are
missing: there is no Python or CPU fallback for the render path.
"""
from __future__ import annotations

import ctypes
import os

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")

XRT_OK = 0
XRT_ERR_ARGUMENT = 1
XRT_ERR_DEVICE = 2
XRT_ERR_NO_MESH = 3
XRT_ERR_OVERFLOW = 4
XRT_ERR_IO = 5
XRT_ERR_FORMAT = 6
XRT_ERR_MEMORY = 7

XRT_KERNEL_AUTO = 0
XRT_KERNEL_BRUTE = 1
XRT_KERNEL_TILED = 2
XRT_KERNEL_BINNED = 3

XRT_MISS_TRANSIT = 0x7F800001

XRT_PROBE_EXPF = 0
XRT_PROBE_SQRTF = 1
XRT_PROBE_RCP = 2
XRT_PROBE_LUT_U8 = 3
XRT_PROBE_RCP_FAST = 4
XRT_PROBE_SIGNED_L = 5
XRT_PROBE_LOGF = 6

XRT_MODEL_ATTENUATION = 0
XRT_MODEL_SIGNED = 1
XRT_MODEL_MATERIALS = 2
XRT_MAX_MESHES = 16
XRT_MODEL_SPECTRUM = 3
XRT_MAX_BINS = 32
XRT_MODEL_PATHS = 4
XRT_MAX_LSF_TAPS = 129
XRT_ORDER_PROJECTIONS = 0
XRT_ORDER_SINOGRAMS = 1
XRT_NOISE_INTENSITY = 0
XRT_NOISE_COUNTS = 1
XRT_MAX_CHANNELS = 8
XRT_DETECT_EXPECTED = 0
XRT_DETECT_NOISY = 1
XRT_DETECT_COUNTS = 0
XRT_DETECT_INTENSITY = 1
XRT_MAX_SOURCES = 64
XRT_MAX_BIN = 8
XRT_MAX_SCATTER_BIN = 64
XRT_MAX_SCATTER_KERNELS = 4
XRT_MAX_RAMP_WIDTH = 4096
XRT_RAMP_RAMLAK = 0
XRT_RAMP_HANN = 1
XRT_FP_PROJECT = 0
XRT_FP_RESIDUAL = 1
XRT_MAX_SUBSETS = 64
XRT_MAX_BASIS = 3
XRT_DECOMPOSE_MASKED = 254
XRT_DECOMPOSE_FAILED = 255

XRT_GATHER_AUTO = 0
XRT_GATHER_COPY = 1
XRT_GATHER_RCCL = 2

XRT_SPLIT_EQUAL = 0
XRT_SPLIT_BALANCED = 1

XRT_TRANSIT_PACKED = 0
XRT_TRANSIT_HITS = 1

XRT_IMAGE_TEXT = 0
XRT_IMAGE_TGA = 1
XRT_IMAGE_PGM = 2
XRT_IMAGE_JPEG = 3

XRT_VOLUME_U8 = 0
XRT_VOLUME_F32 = 1

_f = ctypes.c_float
_fp = ctypes.POINTER(ctypes.c_float)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_u16p = ctypes.POINTER(ctypes.c_uint16)
_u32 = ctypes.c_uint32
_u64 = ctypes.c_uint64
_vp = ctypes.c_void_p
_dp = ctypes.POINTER(ctypes.c_double)
_i32p = ctypes.POINTER(ctypes.c_int32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)


class Camera(ctypes.Structure):
    """xrt_camera: RayTracerInfo (src/main.cxx:111-121) + pixel spacing + size."""

    _fields_ = [
        ("origin", _f * 3),
        ("detector", _f * 3),
        ("up", _f * 3),
        ("right", _f * 3),
        ("pixel_spacing", _f),
        ("width", _u32),
        ("height", _u32),
    ]


class TvParams(ctypes.Structure):
    """xrt_tv_params: the TV descent of xrt_sirt_tv."""

    _fields_ = [
        ("steps", _u32),
        ("alpha", ctypes.c_double),
        ("reduction", ctypes.c_double),
        ("eps", ctypes.c_double),
    ]


_TvP = ctypes.POINTER(TvParams)


class Stats(ctypes.Structure):
    _fields_ = [
        ("rays", _u64),
        ("hit_rays", _u64),
        ("odd_rays", _u64),
        ("overflow_rays", _u64),
        ("hits", _u64),
        ("max_hits", _u32),
        ("kernel", _u32),
        ("kernel_ms", ctypes.c_double),
        ("candidates", _u64),
        ("tile_tests", _u64),
        ("global_triangles", _u64),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class _Context(ctypes.Structure):
    pass


class _Multi(ctypes.Structure):
    pass


_CtxP = ctypes.POINTER(_Context)
_MultiP = ctypes.POINTER(_Multi)

# name -> (restype, argtypes); every symbol declared in include/xrt.h
XRT_SYMBOLS = {
    "xrt_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_CtxP)]),
    "xrt_destroy": (None, [_CtxP]),
    "xrt_last_error": (ctypes.c_char_p, [_CtxP]),
    "xrt_abi_version": (ctypes.c_int, []),
    "xrt_device_count": (ctypes.c_int, []),
    "xrt_upload_mesh": (ctypes.c_int, [_CtxP, _fp, _u64]),
    "xrt_mesh_bbox": (ctypes.c_int, [_fp, _u64, _fp, _fp]),
    "xrt_scene_bbox": (ctypes.c_int, [_fp, _u64p, _u32, _fp, _fp]),
    "xrt_camera_from_bbox": (ctypes.c_int, [_fp, _fp, _u32, _u32, ctypes.POINTER(Camera)]),
    "xrt_set_kernel": (ctypes.c_int, [_CtxP, ctypes.c_int]),
    "xrt_render_rows": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _fp, _fp, _u8p,
                                       ctypes.POINTER(Stats)]),
    "xrt_render_rows_device": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _vp, _vp,
                                              _vp, _vp]),
    "xrt_read_stats": (ctypes.c_int, [_CtxP, ctypes.POINTER(Stats)]),
    "xrt_render_frames_device": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _u32, _u32,
                                                ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                                ctypes.POINTER(_vp)]),
    "xrt_render_frames": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _u32, _fp, _fp, _u8p,
                                         ctypes.POINTER(Stats), _dp]),
    "xrt_timing_begin": (ctypes.c_int, [_CtxP]),
    "xrt_timing_end": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_u64)]),
    "xrt_timing_events": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_u64)]),
    "xrt_probe_intersect": (ctypes.c_int, [_CtxP, _fp, _fp, _u64, _u8p, _fp]),
    "xrt_probe_math": (ctypes.c_int, [_CtxP, ctypes.c_int, _fp, _fp, _u64]),
    "xrt_probe_prep": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _fp, _fp]),
    "xrt_host_expf_batch": (None, [_fp, _fp, _u64]),
    "xrt_host_exp_batch": (None, [_dp, _dp, _u64]),
    "xrt_host_signed_lbuffer_batch": (None, [_fp, _i32p, _f, _fp, _u64]),
    "xrt_set_model": (ctypes.c_int, [_CtxP, ctypes.c_int, _f]),
    "xrt_hole_fill": (ctypes.c_int, [_CtxP, _u32, _u32, _fp, _fp, _u8p]),
    "xrt_hole_fill_device": (ctypes.c_int, [_CtxP, _u32, _u32, _vp, _vp, _vp, _vp]),
    "xrt_render_signed": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _fp, _fp, _u8p, ctypes.POINTER(Stats)]),
    "xrt_upload_scene": (ctypes.c_int, [_CtxP, _fp, _u64p, _u32]),
    "xrt_set_materials": (ctypes.c_int, [_CtxP, _fp, _u32]),
    "xrt_render_materials": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _fp, _fp, _u8p, ctypes.POINTER(Stats)]),
    "xrt_host_materials_lbuffer_batch": (None, [_fp, _i32p, _fp, _u32, _fp, _u64]),
    "xrt_probe_materials": (ctypes.c_int, [_CtxP, _fp, _i32p, _fp, _u32, _fp, _u64]),
    "xrt_set_spectrum": (ctypes.c_int, [_CtxP, _fp, _fp, _u32, _u32]),
    "xrt_render_spectrum": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _fp, _fp, _u8p, ctypes.POINTER(Stats)]),
    "xrt_set_paths": (ctypes.c_int, [_CtxP]),
    "xrt_render_paths": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _u32, _fp, _u16p,
                                        ctypes.POINTER(Stats)]),
    "xrt_render_paths_device": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _u32, _vp, _vp, _vp]),
    "xrt_apply_spectrum": (ctypes.c_int, [_CtxP, _u64, _u32, _fp, _u16p, _fp, _fp, _u32, _fp]),
    "xrt_apply_spectrum_device": (ctypes.c_int, [_CtxP, _u64, _u32, _vp, _vp, _fp, _fp, _u32, _vp, _vp]),
    "xrt_host_spectrum_lbuffer_batch": (None, [_fp, _i32p, _fp, _fp, _u32, _u32, _fp, _u64]),
    "xrt_host_spectrum_miss": (_f, [_fp, _u32]),
    "xrt_probe_spectrum": (ctypes.c_int, [_CtxP, _fp, _i32p, _fp, _fp, _u32, _u32, _fp, _u64]),
    "xrt_set_pose": (ctypes.c_int, [_CtxP, _u32, _fp]),
    "xrt_reset_poses": (ctypes.c_int, [_CtxP]),
    "xrt_pose_rotation": (ctypes.c_int, [_fp, ctypes.c_double, _fp, _fp]),
    "xrt_pose_triangles": (ctypes.c_int, [_fp, _u64, _fp, _fp]),
    "xrt_debug_posed_triangles": (ctypes.c_int, [_CtxP, _fp, _u64, ctypes.POINTER(_u64)]),
    "xrt_debug_pose_span": (ctypes.c_int, [_CtxP, _u32, _dp]),
    "xrt_debug_pose_counters": (ctypes.c_int, [_CtxP, ctypes.POINTER(_u64)]),
    "xrt_detector_response": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _fp, _u32, _fp, _u32, _fp, _u8p]),
    "xrt_detector_response_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _fp, _u32, _fp, _u32, _vp, _vp, _vp]),
    "xrt_lsf_gaussian": (ctypes.c_int, [ctypes.c_double, _u32, _fp]),
    "xrt_host_lsf": (ctypes.c_int, [_u32, _u32, _u32, _fp, _fp, _u32, _fp, _u32, _fp, _u8p]),
    "xrt_log_projection": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _fp, _fp, ctypes.c_float, ctypes.c_float,
                                          ctypes.c_int, _fp]),
    "xrt_log_projection_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _vp, _vp, ctypes.c_float, ctypes.c_float,
                                                 ctypes.c_int, _vp, _vp]),
    "xrt_host_logf_batch": (None, [_fp, _fp, _u64]),
    "xrt_host_log_projection": (ctypes.c_int, [_u32, _u32, _u32, _fp, _fp, _fp, ctypes.c_float, ctypes.c_float,
                                               ctypes.c_int, _fp]),
    "xrt_photon_noise": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, ctypes.c_float, _u64, _u64, ctypes.c_int, _fp]),
    "xrt_photon_noise_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, ctypes.c_float, _u64, _u64, ctypes.c_int, _vp,
                                               _vp]),
    "xrt_spectral_detector": (ctypes.c_int, [_CtxP, _u64, _u32, _fp, _u16p, _fp, _fp, _u32, _fp, _u32, ctypes.c_float,
                                             ctypes.c_float, _u64, _u64, ctypes.c_int, ctypes.c_int, _fp]),
    "xrt_spectral_detector_device": (ctypes.c_int, [_CtxP, _u64, _u32, _vp, _vp, _fp, _fp, _u32, _fp, _u32,
                                                    ctypes.c_float, ctypes.c_float, _u64, _u64, ctypes.c_int,
                                                    ctypes.c_int, _vp, _vp]),
    "xrt_host_spectral_detector": (ctypes.c_int, [_u64, _u32, _fp, _u16p, _fp, _fp, _u32, _fp, _u32, ctypes.c_float,
                                                  ctypes.c_float, _u64, _u64, ctypes.c_int, ctypes.c_int, _fp]),
    "xrt_upload_volume": (ctypes.c_int, [_CtxP, _u8p, _fp, _u32p, _fp, _fp, _u32]),
    "xrt_volume_bbox": (ctypes.c_int, [_u32p, _fp, _fp, _fp, _fp]),
    "xrt_volume_paths": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _u32, _fp]),
    "xrt_volume_paths_device": (ctypes.c_int, [_CtxP, ctypes.POINTER(Camera), _u32, _u32, _u32, _vp, _vp]),
    "xrt_host_volume_paths": (ctypes.c_int, [ctypes.POINTER(Camera), _u32, _u32, _u8p, _fp, _u32p, _fp, _fp, _u32,
                                             _fp]),
    "xrt_debug_volume_wave_shape": (ctypes.c_int, [_CtxP, ctypes.c_int]),
    "xrt_fdk_filter": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _fp, _fp, _u32, _fp]),
    "xrt_fdk_filter_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _vp]),
    "xrt_backproject": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _dp, _u32p, _u32, _u32, ctypes.c_double,
                                       ctypes.c_int, _fp]),
    "xrt_backproject_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _vp, _u32p, _u32, _u32, ctypes.c_double,
                                              ctypes.c_int, _vp, _vp]),
    "xrt_backprojection_matrix": (ctypes.c_int, [ctypes.POINTER(Camera), _fp, _fp, _fp, _dp]),
    "xrt_fdk_weights": (ctypes.c_int, [ctypes.POINTER(Camera), _fp]),
    "xrt_ramp_filter": (ctypes.c_int, [_u32, ctypes.c_int, _fp]),
    "xrt_fdk_scale": (ctypes.c_int, [ctypes.POINTER(Camera), _fp, _u32, _dp]),
    "xrt_host_fdk_filter": (ctypes.c_int, [_u32, _u32, _u32, _fp, _fp, _fp, _u32, _fp]),
    "xrt_host_backproject": (ctypes.c_int, [_u32, _u32, _u32, _fp, _dp, _u32p, _u32, _u32, ctypes.c_double, ctypes.c_int,
                                            _fp]),
    "xrt_ray_matrix": (ctypes.c_int, [_dp, _dp]),
    "xrt_forward_project": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _u32p, _fp, _dp, ctypes.c_int, _fp, _fp]),
    "xrt_forward_project_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _u32p, _fp, _vp, ctypes.c_int, _vp, _vp,
                                                  _vp]),
    "xrt_volume_update": (ctypes.c_int, [_CtxP, _u64, _fp, _fp, _fp, ctypes.c_double, _f, _f]),
    "xrt_volume_update_device": (ctypes.c_int, [_CtxP, _u64, _vp, _vp, _vp, ctypes.c_double, _f, _f, _vp]),
    "xrt_sirt": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f, _fp]),
    "xrt_sirt_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f,
                                       _vp, _vp]),
    "xrt_host_forward_project": (ctypes.c_int, [_u32, _u32, _u32, _fp, _u32p, _fp, _dp, ctypes.c_int, _fp, _fp]),
    "xrt_host_volume_update": (ctypes.c_int, [_u64, _fp, _fp, _fp, ctypes.c_double, _f, _f]),
    "xrt_host_sirt": (ctypes.c_int, [_u32, _u32, _u32, _fp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f, _fp]),
    "xrt_tv_gradient": (ctypes.c_int, [_CtxP, _fp, _u32p, ctypes.c_double, _fp]),
    "xrt_tv_gradient_device": (ctypes.c_int, [_CtxP, _vp, _u32p, ctypes.c_double, _vp, _vp]),
    "xrt_volume_sumsq": (ctypes.c_int, [_CtxP, _u64, _fp, _fp, _dp]),
    "xrt_volume_sumsq_device": (ctypes.c_int, [_CtxP, _u64, _vp, _vp, _vp, _vp]),
    "xrt_tv_descend": (ctypes.c_int, [_CtxP, _fp, _u32p, ctypes.c_double, _u32, ctypes.c_double, _f, _f]),
    "xrt_tv_descend_device": (ctypes.c_int, [_CtxP, _vp, _u32p, ctypes.c_double, _u32, ctypes.c_double, _f, _f, _vp]),
    "xrt_sirt_tv": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f, _TvP,
                                   _fp]),
    "xrt_sirt_tv_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f,
                                          _TvP, _vp, _vp]),
    "xrt_host_tv_gradient": (ctypes.c_int, [_fp, _u32p, ctypes.c_double, _fp]),
    "xrt_host_volume_sumsq": (ctypes.c_int, [_u64, _fp, _fp, _dp]),
    "xrt_host_tv_descend": (ctypes.c_int, [_fp, _u32p, ctypes.c_double, _u32, ctypes.c_double, _f, _f]),
    "xrt_host_sirt_tv": (ctypes.c_int, [_u32, _u32, _u32, _fp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f, _TvP,
                                        _fp]),
    "xrt_poisson_project": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _u32p, _fp, _dp, _fp, _fp, _fp, _fp]),
    "xrt_poisson_project_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _u32p, _fp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xrt_backproject_update": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _dp, _u32p, ctypes.c_double, _f, _f, _fp]),
    "xrt_backproject_update_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _vp, _u32p, ctypes.c_double, _f, _f, _vp,
                                                     _vp]),
    "xrt_mltr": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _fp, _fp, _fp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f,
                                _TvP, _fp]),
    "xrt_mltr_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _vp, _vp, _vp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double,
                                       _f, _f, _TvP, _vp, _vp]),
    "xrt_host_poisson_project": (ctypes.c_int, [_u32, _u32, _u32, _fp, _u32p, _fp, _dp, _fp, _fp, _fp, _fp]),
    "xrt_host_backproject_update": (ctypes.c_int, [_u32, _u32, _u32, _fp, _dp, _u32p, ctypes.c_double, _f, _f, _fp]),
    "xrt_host_mltr": (ctypes.c_int, [_u32, _u32, _u32, _fp, _fp, _fp, _dp, _u32p, _fp, _u32, _u32, ctypes.c_double, _f, _f,
                                     _TvP, _fp]),
    "xrt_decompose": (ctypes.c_int, [_CtxP, _u64, _fp, _u16p, _fp, _fp, _u32, _u32, _fp, _u32, ctypes.c_float, ctypes.c_int, _dp,
                                     _u32, ctypes.c_double, ctypes.c_double, _fp, _u8p]),
    "xrt_decompose_device": (ctypes.c_int, [_CtxP, _u64, _vp, _vp, _fp, _fp, _u32, _u32, _fp, _u32, ctypes.c_float,
                                            ctypes.c_int, _dp, _u32, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]),
    "xrt_decompose_guess": (ctypes.c_int, [_fp, _fp, _u32, _u32, _fp, _u32, _dp]),
    "xrt_host_decompose": (ctypes.c_int, [_u64, _fp, _u16p, _fp, _fp, _u32, _u32, _fp, _u32, ctypes.c_float, ctypes.c_int, _dp,
                                          _u32, ctypes.c_double, ctypes.c_double, _fp, _u8p]),
    "xrt_voxelize": (ctypes.c_int, [_CtxP, _u32p, _fp, _fp, _fp, _u16p, _u8p, _fp, _u64p]),
    "xrt_voxelize_device": (ctypes.c_int, [_CtxP, _u32p, _fp, _fp, _fp, _vp, _vp, _vp, _vp, _vp]),
    "xrt_host_voxelize": (ctypes.c_int, [_fp, _u64p, _u32, _u32p, _fp, _fp, _fp, _u16p, _u8p, _fp, _u64p]),
    "xrt_debug_voxelize_threshold": (ctypes.c_int, [_CtxP, _u32]),
    "xrt_debug_voxelize_stages": (ctypes.c_int, [_CtxP, _u32]),
    "xrt_debug_voxelize_counters": (ctypes.c_int, [_CtxP, _u64p]),
    "xrt_host_philox4x32": (None, [_u32p, _u32p, _u32p]),
    "xrt_host_poisson_batch": (None, [_dp, _u32p, _u64, _dp]),
    "xrt_host_photon_noise": (ctypes.c_int, [_u32, _u32, _u32, _fp, ctypes.c_float, _u64, _u64, ctypes.c_int, _fp]),
    "xrt_debug_poisson_batch": (ctypes.c_int, [_CtxP, _dp, _u32p, _u64, _dp]),
    "xrt_area_integrate": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _u32, _u32, _u32, _fp, _fp, _fp,
                                          ctypes.POINTER(ctypes.c_uint8)]),
    "xrt_area_integrate_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _u32, _u32, _u32, _fp, _vp, _vp, _vp, _vp]),
    "xrt_host_area_integrate": (ctypes.c_int, [_u32, _u32, _u32, _u32, _u32, _u32, _fp, _fp, _fp,
                                               ctypes.POINTER(ctypes.c_uint8)]),
    "xrt_scatter_source": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _u32, _fp, _u16p, _fp, _fp, _fp, _u32, _u32, _fp, _fp]),
    "xrt_scatter_source_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _u32, _vp, _vp, _fp, _fp, _fp, _u32, _u32, _vp,
                                                 _vp, _vp]),
    "xrt_scatter_add": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _u32, _fp, _u32, _fp, _fp, _fp, _fp, _u8p]),
    "xrt_scatter_add_device": (ctypes.c_int, [_CtxP, _u32, _u32, _u32, _u32, _vp, _u32, _fp, _vp, _vp, _vp, _vp, _vp]),
    "xrt_host_scatter_source": (ctypes.c_int, [_u32, _u32, _u32, _u32, _fp, _u16p, _fp, _fp, _fp, _u32, _u32, _fp, _fp]),
    "xrt_host_scatter_add": (ctypes.c_int, [_u32, _u32, _u32, _u32, _fp, _u32, _fp, _fp, _fp, _fp, _u8p]),
    "xrt_camera_supersample": (ctypes.c_int, [ctypes.POINTER(Camera), _u32, ctypes.POINTER(Camera)]),
    "xrt_focal_spot": (ctypes.c_int, [ctypes.POINTER(Camera), ctypes.c_float, ctypes.c_float, _u32, _u32,
                                      ctypes.POINTER(Camera), _fp]),
    "xrt_multi_set_pose": (ctypes.c_int, [_MultiP, _u32, _fp]),
    "xrt_multi_reset_poses": (ctypes.c_int, [_MultiP]),
    "xrt_host_mt_check": (None, [_fp, _fp, _fp, _fp, _u64, ctypes.POINTER(ctypes.c_uint8),
                                 ctypes.POINTER(ctypes.c_uint8), _fp]),
    "xrt_set_hit_capacity": (ctypes.c_int, [_CtxP, _u32]),
    "xrt_set_bin_capacity": (ctypes.c_int, [_CtxP, _u64]),
    "xrt_set_fill_plan": (ctypes.c_int, [_CtxP, ctypes.c_int]),
    "xrt_debug_fill_regions": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_uint32)]),
    "xrt_debug_geometry_counters": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_uint64)]),
    "xrt_debug_first_frames": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_uint64)]),
    "xrt_debug_pipeline_counters": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_uint64)]),
    "xrt_debug_host_call_ms": (ctypes.c_int, [_CtxP, _dp]),
    "xrt_debug_destroy_ms": (ctypes.c_int, [_dp]),
    "xrt_debug_tile_plan": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_uint64)]),
    "xrt_debug_set_tile_plan": (ctypes.c_int, [_CtxP, ctypes.c_int]),
    "xrt_debug_set_ray_table": (ctypes.c_int, [_CtxP, ctypes.c_int]),
    "xrt_debug_ray_table_counters": (ctypes.c_int, [_CtxP, ctypes.POINTER(ctypes.c_uint64)]),
    "xrt_debug_ray_table_index": (ctypes.c_int, [_u32, _u32, _u32, _u32, _u32, _u32, _u64p, _u64p]),
    "xrt_debug_ray_table_read": (ctypes.c_int, [_CtxP, _vp, _u64, ctypes.POINTER(_u32)]),
    "xrt_debug_direction_grid": (ctypes.c_int, [ctypes.POINTER(Camera), ctypes.POINTER(ctypes.c_int)]),
    "xrt_host_footprints": (ctypes.c_int, [ctypes.POINTER(Camera), _fp, _u64, _fp]),
    "xrt_debug_prep_times": (ctypes.c_int, [_CtxP, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.POINTER(ctypes.c_uint64)]),
    "xrt_debug_block_records": (ctypes.c_int, [_CtxP, _vp, _u64, ctypes.POINTER(_u64)]),
    "xrt_debug_wave_times": (ctypes.c_int, [_CtxP, _u32, ctypes.POINTER(_u32), _u64, ctypes.POINTER(_u64)]),
    "xrt_set_miss_code": (ctypes.c_int, [_CtxP, _u32]),
    "xrt_expand_rows_device": (ctypes.c_int, [_CtxP, _u64, _vp, _vp, _vp, _vp]),
    "xrt_plan_region_map": (ctypes.c_int, [_CtxP, ctypes.c_uint32, ctypes.c_uint32,
                                           ctypes.POINTER(ctypes.c_uint32), _u64, ctypes.POINTER(ctypes.c_uint32)]),
    "xrt_pack_regions_device": (ctypes.c_int, [_CtxP, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "xrt_unpack_regions_device": (ctypes.c_int, [_CtxP, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                                 _vp]),
    "xrt_set_transit_layout": (ctypes.c_int, [_CtxP, _u64]),
    "xrt_unpack_blocks_device": (ctypes.c_int, [_CtxP, ctypes.c_uint32, _u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "xrt_plan_hit_layout": (ctypes.c_int, [_CtxP, ctypes.POINTER(_u32), _u64, ctypes.POINTER(_u64),
                                           ctypes.POINTER(_u64)]),
    "xrt_set_transit_hits": (ctypes.c_int, [_CtxP, _u64]),
    "xrt_unpack_hits_device": (ctypes.c_int, [_CtxP, ctypes.c_uint32, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                              _vp]),
    "xrt_multi_create": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_MultiP)]),
    "xrt_multi_destroy": (None, [_MultiP]),
    "xrt_multi_last_error": (ctypes.c_char_p, [_MultiP]),
    "xrt_multi_num_devices": (ctypes.c_int, [_MultiP]),
    "xrt_multi_upload_mesh": (ctypes.c_int, [_MultiP, _fp, _u64]),
    "xrt_multi_set_kernel": (ctypes.c_int, [_MultiP, ctypes.c_int]),
    "xrt_multi_set_model": (ctypes.c_int, [_MultiP, ctypes.c_int, _f]),
    "xrt_multi_upload_scene": (ctypes.c_int, [_MultiP, _fp, _u64p, _u32]),
    "xrt_multi_set_materials": (ctypes.c_int, [_MultiP, _fp, _u32]),
    "xrt_multi_set_spectrum": (ctypes.c_int, [_MultiP, _fp, _fp, _u32, _u32]),
    "xrt_render_rows_multi": (ctypes.c_int, [_MultiP, ctypes.POINTER(Camera), _fp, _fp, _u8p,
                                             ctypes.POINTER(Stats)]),
    "xrt_render_rows_multi_device": (ctypes.c_int, [_MultiP, ctypes.POINTER(Camera), _vp, _vp, _vp, _vp]),
    "xrt_multi_read_stats": (ctypes.c_int, [_MultiP, ctypes.POINTER(Stats)]),
    "xrt_multi_set_gather": (ctypes.c_int, [_MultiP, ctypes.c_int]),
    "xrt_multi_set_split": (ctypes.c_int, [_MultiP, ctypes.c_int, ctypes.c_double]),
    "xrt_multi_set_transit": (ctypes.c_int, [_MultiP, ctypes.c_int]),
    "xrt_multi_transit_stats": (ctypes.c_int, [_MultiP, ctypes.POINTER(_u64)]),
    "xrt_multi_plan_stats": (ctypes.c_int, [_MultiP, ctypes.POINTER(_u64)]),
    "xrt_multi_debug_corrupt_hit_plan": (ctypes.c_int, [_MultiP]),
    "xrt_multi_plan": (ctypes.c_int, [_MultiP, ctypes.POINTER(Camera), ctypes.POINTER(_u32), _dp]),
    "xrt_balanced_bounds": (ctypes.c_int, [_dp, _dp, _u32, _u32, ctypes.c_double, _u32, _u32, ctypes.c_double,
                                           ctypes.POINTER(_u32), _dp]),
}

# every C symbol declared in include/xrt_host.h
XRT_HOST_SYMBOLS = {
    "xrt_host_load_ply": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_fp), ctypes.POINTER(_u64)]),
    "xrt_host_load_meshes": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_fp), ctypes.POINTER(_u64p),
                                            ctypes.POINTER(_u32)]),
    "xrt_host_free": (None, [_vp]),
    "xrt_host_load_volume": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_vp), ctypes.POINTER(ctypes.c_int), _u32p, _fp,
                                            _fp]),
    "xrt_host_last_error": (ctypes.c_char_p, []),
    "xrt_host_save_volume": (ctypes.c_int, [ctypes.c_char_p, _fp, _u32p, _fp, _fp]),
    "xrt_host_intersect_batch": (None, [_fp, _fp, _u64, _u8p, _fp]),
    "xrt_host_save_image": (ctypes.c_int, [_fp, _u32, _u32, ctypes.c_char_p, ctypes.c_int, _f, _f]),
}

_lib = None
_host = None


def _bind(lib, table):
    variant = bool(os.environ.get("XRT_LIB"))
    for name, (res, args) in table.items():
        if variant and not hasattr(lib, name):     # an A/B build of an older ABI: its entry points only
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def lib_path(name="libxrt.so"):
    return os.path.join(LIB_DIR, name)


def load():
    """Returns the bound libxrt.so; raises if it has not been built."""
    global _lib
    if _lib is None:
        # XRT_LIB: a variant build (tools/build_variants.sh) for A/B timing only
        path = os.environ.get("XRT_LIB") or lib_path("libxrt.so")
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C simpleraytracing_amd/csrc` (there is no CPU fallback)")
        # torch's ROCm libraries first: they are NEEDED by unversioned names
        # (libamdhip64.so, librccl.so), so a torch imported after libxrt.so
        # (which needs libamdhip64.so.7, librccl.so.1) would load a second HIP
        # and HSA runtime into the process -- two runtimes that corrupt the heap
        # at exit.  Imported first, torch's copies carry the versioned sonames
        # and libxrt.so binds to them.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = _bind(ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL), XRT_SYMBOLS)
    return _lib


def load_host():
    """Returns the bound libxrt_host.so (C++ host API's C entry points)."""
    global _host
    if _host is None:
        load()
        # XRT_HOST_LIB: a sanitizer build (make -C simpleraytracing_amd/csrc SAN=1, tools/san_check.sh)
        path = os.environ.get("XRT_HOST_LIB") or lib_path("libxrt_host.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build simpleraytracing_amd/csrc first")
        _host = _bind(ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL), XRT_HOST_SYMBOLS)
    return _host
