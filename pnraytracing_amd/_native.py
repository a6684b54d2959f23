"""Loading of the in-tree native libraries (ctypes; no torch types cross the ABI).

* ``libpnrt.so``      -- HIP device library, C ABI in ``include/pnrt.h``
* ``libpnrt_host.so`` -- host scene library, C ABI in ``include/pnrt_host.h``

Both are built in-tree by :mod:`pnraytracing_amd.build` (``__graft_entry__.build()``).
There is no fallback: if a library is missing or fails to load, the error is
raised to the caller (the product path never substitutes a CPU implementation).
"""
from __future__ import annotations

import ctypes
import os

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
DEVICE_LIB = os.environ.get("PNRT_DEVICE_LIB") or os.path.join(PKG_DIR, "libpnrt.so")
HOST_LIB = os.path.join(PKG_DIR, "libpnrt_host.so")

_cache: dict[str, ctypes.CDLL] = {}


class NativeLibraryError(RuntimeError):
    pass


def _load(path: str) -> ctypes.CDLL:
    lib = _cache.get(path)
    if lib is not None:
        return lib
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"{os.path.basename(path)} is not built ({path}); run "
            "`python -c 'import __graft_entry__ as g; g.build()'` first")
    try:
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - surfaced verbatim
        raise NativeLibraryError(f"failed to load {path}: {e}") from e
    _cache[path] = lib
    return lib


def host_lib() -> ctypes.CDLL:
    lib = _load(HOST_LIB)
    if not getattr(lib, "_pnrt_typed", False):
        _type_host(lib)
        lib._pnrt_typed = True
    return lib


def device_lib() -> ctypes.CDLL:
    lib = _load(DEVICE_LIB)
    if not getattr(lib, "_pnrt_typed", False):
        _type_device(lib)
        lib._pnrt_typed = True
    return lib


P = ctypes.c_void_p
F = ctypes.POINTER(ctypes.c_float)
I32 = ctypes.POINTER(ctypes.c_int32)
U8 = ctypes.POINTER(ctypes.c_uint8)
INT = ctypes.c_int
PINT = ctypes.POINTER(ctypes.c_int)


class Xform(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("angle_deg", ctypes.c_float), ("v", ctypes.c_float * 3)]


class SceneInfo(ctypes.Structure):
    _fields_ = [("n_vertices", ctypes.c_int), ("n_materials", ctypes.c_int),
                ("n_triangles", ctypes.c_int), ("n_nodes", ctypes.c_int),
                ("n_lights", ctypes.c_int), ("lights_sum_area", ctypes.c_float),
                ("max_depth", ctypes.c_int)]


class Camera(ctypes.Structure):
    """``pnrt_camera`` (camera.hpp:28-30 uniforms)."""
    _fields_ = [("eye", ctypes.c_float * 3), ("lower_left", ctypes.c_float * 3),
                ("horizontal", ctypes.c_float * 3), ("vertical", ctypes.c_float * 3)]


class DeviceInfo(ctypes.Structure):
    _fields_ = [("n_interior", ctypes.c_int), ("n_triangles", ctypes.c_int),
                ("max_depth", ctypes.c_int), ("device_bytes", ctypes.c_int64),
                ("root_is_leaf", ctypes.c_int), ("stack_limit", ctypes.c_int),
                ("has_leaf_table", ctypes.c_int)]


K_CLASSES = ("primary", "gen", "setup", "trace", "shade", "blend", "v1")   # PNRT_K_* order


class Profile(ctypes.Structure):
    _fields_ = [("ms", ctypes.c_double * len(K_CLASSES)), ("launches", ctypes.c_int64 * len(K_CLASSES))]


AOV_NAMES = ("position", "normal", "albedo")   # PNRT_AOV_* order
AOV_POSITION, AOV_NORMAL, AOV_ALBEDO = range(3)
AOV_COUNT = len(AOV_NAMES)


class DenoiseParams(ctypes.Structure):
    """``pnrt_denoise_params``."""
    _fields_ = [("levels", ctypes.c_int), ("sigma_color", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_position", ctypes.c_float)]


class DenoiseVarianceParams(ctypes.Structure):
    """``pnrt_denoise_variance_params``."""
    _fields_ = [("levels", ctypes.c_int), ("sigma_variance", ctypes.c_float), ("sigma_normal", ctypes.c_float),
                ("sigma_position", ctypes.c_float)]


class ConvergenceStats(ctypes.Structure):
    """``pnrt_convergence_stats`` (48 bytes)."""
    _fields_ = [("n_pixels", ctypes.c_int64), ("n_measured", ctypes.c_int64), ("n_above", ctypes.c_int64),
                ("sum_q16", ctypes.c_int64), ("max_error", ctypes.c_float), ("min_frames", ctypes.c_uint32),
                ("max_frames", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class AdaptiveStats(ctypes.Structure):
    """``pnrt_adaptive_stats`` (40 bytes)."""
    _fields_ = [("n_pixels", ctypes.c_int64), ("n_active_pixels", ctypes.c_int64), ("n_tiles", ctypes.c_int64),
                ("n_active_tiles", ctypes.c_int64), ("frames_per_batch", ctypes.c_uint32), ("n_batches", ctypes.c_uint32)]


class ReprojectParams(ctypes.Structure):
    """``pnrt_reproject_params`` (16 bytes)."""
    _fields_ = [("normal_min", ctypes.c_float), ("position_tolerance", ctypes.c_float), ("max_history", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class ReprojectStats(ctypes.Structure):
    """``pnrt_reproject_stats`` (48 bytes)."""
    _fields_ = [("n_pixels", ctypes.c_int64), ("n_reprojected", ctypes.c_int64), ("n_disoccluded", ctypes.c_int64),
                ("n_missed", ctypes.c_int64), ("sum_frames", ctypes.c_int64), ("max_frames", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


DISPLAY_SOURCES = ("accum", "denoised", "external")   # PNRT_DISPLAY_* order
DISPLAY_TONES = ("clamp", "reinhard", "aces")         # PNRT_TONE_* order
DISPLAY_TRANSFERS = ("linear", "srgb")                # PNRT_TRANSFER_* order
LUMA_BINS = 512                                       # PNRT_LUMA_BINS


class DisplayParams(ctypes.Structure):
    """``pnrt_display_params`` (32 bytes)."""
    _fields_ = [("source", ctypes.c_int), ("tone", ctypes.c_int), ("transfer", ctypes.c_int), ("bottom_first", ctypes.c_int),
                ("exposure", ctypes.c_float), ("white", ctypes.c_float), ("src_device", ctypes.c_void_p)]


class LumaHistogram(ctypes.Structure):
    """``pnrt_luma_histogram`` (4112 bytes)."""
    _fields_ = [("n_pixels", ctypes.c_int64), ("n_counted", ctypes.c_int64), ("bins", ctypes.c_int64 * LUMA_BINS)]


class LensParams(ctypes.Structure):
    """``pnrt_lens_params`` (16 bytes; include/pnrt_host.h)."""
    _fields_ = [("aa_width", ctypes.c_float), ("lens_radius", ctypes.c_float), ("focus_distance", ctypes.c_float),
                ("reserved", ctypes.c_uint32)]


CAM_MODELS = ("pinhole", "ortho", "equirect", "fisheye")   # PNRT_CAM_* order


class Ray(ctypes.Structure):
    """``pnrt_ray`` (32 bytes)."""
    _fields_ = [("origin", ctypes.c_float * 3), ("reserved0", ctypes.c_float), ("direction", ctypes.c_float * 3),
                ("reserved1", ctypes.c_float)]


class RayCamera(ctypes.Structure):
    """``pnrt_ray_camera`` (76 bytes)."""
    _fields_ = [("model", ctypes.c_int), ("camera", Camera), ("fov_deg", ctypes.c_float), ("aa_width", ctypes.c_float),
                ("lens_radius", ctypes.c_float), ("focus_distance", ctypes.c_float), ("per_pixel", ctypes.c_int),
                ("reserved", ctypes.c_int)]


class Placement(ctypes.Structure):
    """``pnrt_placement`` (72 bytes)."""
    _fields_ = [("model", ctypes.c_int), ("matrix", ctypes.c_float * 16), ("reserved", ctypes.c_int)]


QUERY_CLOSEST, QUERY_ANY = 0, 1                # PNRT_QUERY_*


class Hit(ctypes.Structure):
    """``pnrt_hit`` (64 bytes; the word layout is in include/pnrt.h)."""
    _fields_ = [("w", ctypes.c_uint32 * 16)]


def _sig(lib, name, res, *args):
    fn = getattr(lib, name)
    fn.restype = res
    fn.argtypes = list(args)


def _type_host(lib):
    _sig(lib, "pnrt_host_last_error", ctypes.c_char_p)
    _sig(lib, "pnrt_model_matrix", INT, ctypes.POINTER(Xform), INT, F)
    _sig(lib, "pnrt_normal_matrix", INT, F, F)
    _sig(lib, "pnrt_scene_create", P)
    _sig(lib, "pnrt_scene_destroy", None, P)
    _sig(lib, "pnrt_scene_add_material", INT, P, F)
    _sig(lib, "pnrt_scene_add_mesh", INT, P, INT, INT, F, F, F, F, F, F, INT, I32, INT)
    _sig(lib, "pnrt_scene_build", INT, P)
    _sig(lib, "pnrt_scene_get_info", INT, P, ctypes.POINTER(SceneInfo))
    _sig(lib, "pnrt_scene_pack", INT, P, F, F, F, F, F)
    _sig(lib, "pnrt_scene_tri_bounds", INT, P, F)
    _sig(lib, "pnrt_scene_set_bvh", INT, P, I32, F, INT, INT)
    _sig(lib, "pnrt_bvh_build_cpu", INT, F, INT, F, INT, PINT, I32, PINT)
    _sig(lib, "pnrt_bvh_refit_cpu", INT, F, INT, F, INT, F, INT)
    _sig(lib, "pnrt_scene_relight", INT, F, INT, F, INT, F, INT, F, INT, PINT, ctypes.POINTER(ctypes.c_float))
    _sig(lib, "pnrt_camera_update", INT, F, F, F, ctypes.c_float, ctypes.c_float, F)
    _sig(lib, "pnrt_camera_pixel_ray", INT, F, INT, INT, INT, INT, F)
    _sig(lib, "pnrt_hdr_decode_rgbe", INT, U8, ctypes.c_int64, PINT, PINT, F)
    _sig(lib, "pnrt_hdr_build_table", INT, F, INT, INT, F)
    _sig(lib, "pnrt_mesh_quad", INT, ctypes.c_float, F, F, F, I32, PINT, PINT)
    _sig(lib, "pnrt_mesh_displaced_sphere", INT, INT, INT, ctypes.c_float, F, ctypes.c_float,
         ctypes.c_uint32, F, F, F, I32, PINT, PINT)
    _sig(lib, "pnrt_mesh_teapot", INT, F, F, F, I32, PINT, PINT)
    _sig(lib, "pnrt_hdr_synthetic", INT, INT, INT, ctypes.c_uint32, F)
    _sig(lib, "pnrt_camera_sequence", INT, F, INT, INT, ctypes.POINTER(LensParams), ctypes.c_uint32, ctypes.c_uint32, F)


def _type_device(lib):
    _sig(lib, "pnrt_version", ctypes.c_char_p)
    _sig(lib, "pnrt_create", INT, INT, ctypes.POINTER(P))
    _sig(lib, "pnrt_destroy", None, P)
    _sig(lib, "pnrt_last_error", ctypes.c_char_p, P)
    _sig(lib, "pnrt_set_stream", INT, P, P)
    _sig(lib, "pnrt_upload_scene", INT, P, F, INT, F, INT, F, INT, F, INT, F, INT, ctypes.c_float)
    _sig(lib, "pnrt_upload_texture", INT, P, INT, U8, INT, INT, INT)
    _sig(lib, "pnrt_update_materials", INT, P, INT, INT, F)
    _sig(lib, "pnrt_update_vertices", INT, P, INT, INT, F, F, ctypes.c_float)
    _sig(lib, "pnrt_update_vertices_device", INT, P, INT, INT, P, F, ctypes.c_float)
    _sig(lib, "pnrt_read_bvh_boxes", INT, P, F, INT)
    _sig(lib, "pnrt_define_model", INT, P, INT, INT, F, PINT)
    _sig(lib, "pnrt_define_model_device", INT, P, INT, INT, P, PINT)
    _sig(lib, "pnrt_place_models", INT, P, ctypes.POINTER(Placement), INT, INT)
    _sig(lib, "pnrt_read_vertices", INT, P, INT, INT, F)
    _sig(lib, "pnrt_upload_env", INT, P, F, F, INT, INT)
    _sig(lib, "pnrt_set_frame", INT, P, INT, INT, ctypes.POINTER(Camera), INT)
    _sig(lib, "pnrt_set_options", INT, P, INT)
    _sig(lib, "pnrt_render", INT, P, ctypes.c_uint32, ctypes.c_uint32, INT, INT, INT)
    _sig(lib, "pnrt_batch_plan", INT, P, ctypes.c_uint32, INT, INT, INT, ctypes.POINTER(ctypes.c_uint32),
         ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64))
    _sig(lib, "pnrt_reset_accum", INT, P)
    _sig(lib, "pnrt_read_accum", INT, P, F)
    _sig(lib, "pnrt_accum_device_ptr", P, P)
    _sig(lib, "pnrt_pack_rows", INT, P, P, INT, INT, INT)
    _sig(lib, "pnrt_unpack_rows", INT, P, P, P, INT, INT, INT)
    _sig(lib, "pnrt_synchronize", INT, P)
    _sig(lib, "pnrt_get_device_info", INT, P, ctypes.POINTER(DeviceInfo))
    _sig(lib, "pnrt_debug_math", INT, P, INT, F, F, F, INT)
    _sig(lib, "pnrt_profile_enable", INT, P, INT)
    _sig(lib, "pnrt_profile_select", INT, P, INT)
    _sig(lib, "pnrt_get_stream", P, P)
    _sig(lib, "pnrt_upload_env_build", INT, P, F, INT, INT)
    _sig(lib, "pnrt_read_env_table", INT, P, F)
    _sig(lib, "pnrt_profile_read", INT, P, ctypes.POINTER(Profile))
    _sig(lib, "pnrt_bvh_build", INT, P, F, INT, F, INT, PINT, I32, PINT)
    _sig(lib, "pnrt_render_guides", INT, P)
    _sig(lib, "pnrt_read_aov", INT, P, INT, F)
    _sig(lib, "pnrt_aov_device_ptr", P, P, INT)
    _sig(lib, "pnrt_denoise", INT, P, ctypes.POINTER(DenoiseParams))
    _sig(lib, "pnrt_denoise_variance", INT, P, ctypes.POINTER(DenoiseVarianceParams))
    _sig(lib, "pnrt_read_denoised", INT, P, F)
    _sig(lib, "pnrt_denoised_device_ptr", P, P)
    _sig(lib, "pnrt_enable_moments", INT, P, INT)
    _sig(lib, "pnrt_moments_device_ptr", P, P)
    _sig(lib, "pnrt_read_moments", INT, P, F)
    _sig(lib, "pnrt_read_error", INT, P, F)
    _sig(lib, "pnrt_convergence", INT, P, ctypes.c_float, INT, INT, INT, ctypes.POINTER(ConvergenceStats))
    _sig(lib, "pnrt_render_adaptive", INT, P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.c_uint32, INT, INT, INT,
         ctypes.POINTER(AdaptiveStats))
    _sig(lib, "pnrt_reproject", INT, P, ctypes.POINTER(Camera), ctypes.POINTER(ReprojectParams), ctypes.POINTER(ReprojectStats))
    _sig(lib, "pnrt_reproject_view", INT, P, ctypes.POINTER(RayCamera), ctypes.POINTER(RayCamera), ctypes.POINTER(ReprojectParams),
         ctypes.POINTER(ReprojectStats))
    _sig(lib, "pnrt_display", INT, P, ctypes.POINTER(DisplayParams))
    _sig(lib, "pnrt_read_display", INT, P, U8)
    _sig(lib, "pnrt_display_device_ptr", P, P)
    _sig(lib, "pnrt_luma_histogram_read", INT, P, INT, P, INT, INT, INT, ctypes.POINTER(LumaHistogram))
    _sig(lib, "pnrt_exposure_from_histogram", INT, ctypes.POINTER(LumaHistogram), INT, INT, ctypes.c_float,
         ctypes.POINTER(ctypes.c_float))
    _sig(lib, "pnrt_query_rays", INT, P, F, ctypes.c_int64, INT, ctypes.POINTER(Hit))
    _sig(lib, "pnrt_query_rays_device", INT, P, P, ctypes.c_int64, INT, P)
    _sig(lib, "pnrt_render_cameras", INT, P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Camera), INT, INT, INT)
    _sig(lib, "pnrt_cameras_batch_plan", INT, P, ctypes.c_uint32, INT, INT, INT, ctypes.POINTER(ctypes.c_uint32),
         ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64))
    _sig(lib, "pnrt_render_rays", INT, P, ctypes.c_uint32, ctypes.c_uint32, P, ctypes.c_int64, INT, INT, INT)
    _sig(lib, "pnrt_render_rays_adaptive", INT, P, ctypes.c_uint32, ctypes.c_uint32, P, ctypes.c_int64, ctypes.c_float,
         ctypes.c_uint32, INT, INT, INT, ctypes.POINTER(AdaptiveStats))
    _sig(lib, "pnrt_render_guides_rays", INT, P, P)
    _sig(lib, "pnrt_make_rays", INT, P, ctypes.POINTER(RayCamera), ctypes.c_uint32, ctypes.c_uint32, P, ctypes.c_int64)


def fptr(a) -> ctypes.POINTER(ctypes.c_float):
    """float32 numpy array -> float* (None -> NULL)."""
    if a is None:
        return None
    assert a.dtype.name == "float32" and a.flags["C_CONTIGUOUS"], "need contiguous float32"
    return a.ctypes.data_as(F)


def iptr(a):
    if a is None:
        return None
    assert a.dtype.name == "int32" and a.flags["C_CONTIGUOUS"], "need contiguous int32"
    return a.ctypes.data_as(I32)


def u8ptr(a):
    if a is None:
        return None
    assert a.dtype.name == "uint8" and a.flags["C_CONTIGUOUS"], "need contiguous uint8"
    return a.ctypes.data_as(U8)
