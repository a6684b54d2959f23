"""``PathTracer``: the host-side operator over ``libpnrt.so`` (include/pnrt.h).

It is the headless replacement of the GL part of main.cpp: upload the packed
arrays (main.cpp:409-524), set the per-frame uniforms (main.cpp:606-611),
dispatch frames (main.cpp:613) and read the progressive accumulation image.
All compute runs in the HIP library; if it is missing this module raises.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _native as N
from .host import PackedScene

TRAVERSE_EXACT = 0
TRAVERSE_ZCULL = 1
KERNEL_V1 = 0x100      # | with a traverse mode: one-lane-per-pixel A/B baseline kernel
SERIAL = 0x200         # | measurement: one call in flight, full trace grid (exclusive kernel times)
# pnrt_denoise(ctx, NULL)'s parameters (include/pnrt.h)
DENOISE_DEFAULTS = {"levels": 5, "sigma_color": 2.0, "sigma_normal": 0.25, "sigma_position": 0.5}

# pnrt_denoise_variance(ctx, NULL)'s parameters (include/pnrt.h)
DENOISE_VARIANCE_DEFAULTS = {"levels": 5, "sigma_variance": 4.0, "sigma_normal": 0.25, "sigma_position": 0.5}

# pnrt_reproject(ctx, from, NULL, ...)'s parameters (include/pnrt.h)
REPROJECT_DEFAULTS = {"normal_min": 0.9, "position_tolerance": 0.02, "max_history": 32}


class PnrtError(RuntimeError):
    pass


# ---- marshalling: each rule of the C ABI's Python side once -------------------------------------------------
def _u32(who, **values):
    """(ctypes would truncate 2**32 + 5 to 5 without a word)"""
    for name, v in values.items():
        if not 0 <= v <= 0xFFFFFFFF:
            raise ValueError(f"{who}: {name} = {v} is outside 0 .. 2**32 - 1")


def _i64(who, **values):
    for name, v in values.items():
        if not -2 ** 63 <= v < 2 ** 63:
            raise ValueError(f"{who}: {name} = {v} does not fit 64 bits")


def _camera(uniforms) -> "N.Camera":
    """The (4, 3) uniforms eye, lower_left, horizontal, vertical as a ``pnrt_camera``."""
    return N.Camera(*(tuple(map(float, r)) for r in np.asarray(uniforms, np.float32).reshape(4, 3)))


def _params(struct, defaults: dict, *given):
    """A parameter struct by reference, arguments left out at the header's defaults -- or None (NULL: the library's
    own defaults) when nothing was given."""
    if all(v is None for v in given):
        return None
    return ctypes.byref(struct(*(d if v is None else v for d, v in zip(defaults.values(), given))))


def _as_dict(st) -> dict:
    """A statistics struct's fields (but ``reserved``)."""
    return {f: getattr(st, f) for f, *_ in st._fields_ if f != "reserved"}


class PathTracer:
    def __init__(self, device: int = 0):
        self._lib = N.device_lib()
        ctx = ctypes.c_void_p()
        rc = self._lib.pnrt_create(device, ctypes.byref(ctx))
        if rc == -1:     # PNRT_E_ARG: the only argument besides the device is the environment's cap
            raise PnrtError(f"pnrt_create(device={device}) failed ({rc}): PNRT_BATCH_BYTES="
                            f"{os.environ.get('PNRT_BATCH_BYTES')!r} is not a decimal byte count")
        if rc != 0:
            raise PnrtError(f"pnrt_create(device={device}) failed ({rc}): no usable HIP device")
        self._ctx = ctx
        self._device = device
        self._stream = 0                 # set_stream's handle (0: the context's own stream)
        self.width = self.height = 0

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.pnrt_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc, what):
        if rc != 0:
            e = PnrtError(f"{what} failed ({rc}): {self._lib.pnrt_last_error(self._ctx).decode()}")
            e.code = rc                  # the PNRT_E_* code
            raise e

    # ---- uploads ---------------------------------------------------------------------
    def upload_scene(self, p: PackedScene):
        V, M, T, Nd, L = (np.ascontiguousarray(a, np.float32) for a in p.arrays())
        self._ck(self._lib.pnrt_upload_scene(self._ctx, N.fptr(V), len(V), N.fptr(M), len(M), N.fptr(T), len(T),
                                             N.fptr(Nd), len(Nd), N.fptr(L) if len(L) else None, len(L),
                                             ctypes.c_float(p.lights_sum_area)), "pnrt_upload_scene")

    def update_materials(self, first: int, records: np.ndarray):
        """Overwrite materials first.. with (n, 18) records in place (pnrt_update_materials:
        the material panel's glTexSubImage1D edit, ImGuiLayer.hpp:73-83)."""
        rec = np.ascontiguousarray(records, np.float32).reshape(-1, 18)
        self._ck(self._lib.pnrt_update_materials(self._ctx, first, len(rec), N.fptr(rec)), "pnrt_update_materials")

    @staticmethod
    def _lights_args(lights, lights_sum_area):
        if lights is None:
            return None, None, ctypes.c_float(0.0)
        L = np.ascontiguousarray(lights, np.float32).reshape(-1, 3)
        if lights_sum_area is None:          # main.cpp:392: the last prefix area
            lights_sum_area = float(L[-1, 1]) if len(L) else 0.0
        # (an empty list still has to say "recompute": a non-NULL pointer nobody reads)
        keep = L if len(L) else np.zeros((1, 3), np.float32)
        return keep, N.fptr(keep), ctypes.c_float(lights_sum_area)

    def update_vertices(self, first: int, vertices: np.ndarray, lights: np.ndarray | None = None,
                        lights_sum_area: float | None = None):
        """Overwrite vertex records first.. with (n, 15) world-space records in place and
        refit the BVH boxes on the device (pnrt_update_vertices; synchronous): the tree's
        topology stays, every box follows the new positions.  ``lights`` None keeps the
        light list's prefix areas (no emissive triangle changed area); otherwise the
        uploaded list with new areas ((n_lights, 3), the same triangle indices; see
        ``host.refit_packed``), ``lights_sum_area`` defaulting to its last prefix.  Reset
        the accumulation afterwards, as a redraw does."""
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 15)
        keep, lp, ls = self._lights_args(lights, lights_sum_area)
        self._ck(self._lib.pnrt_update_vertices(self._ctx, first, len(v), N.fptr(v) if len(v) else None, lp, ls),
                 "pnrt_update_vertices")

    def update_vertices_device(self, first: int, count: int, ptr: int, lights: np.ndarray | None = None,
                               lights_sum_area: float | None = None):
        """The same from device memory (pnrt_update_vertices_device): ``ptr`` holds ``count``
        records of 15 floats, 4-byte aligned, on the context's device."""
        keep, lp, ls = self._lights_args(lights, lights_sum_area)
        self._ck(self._lib.pnrt_update_vertices_device(self._ctx, first, count, ctypes.c_void_p(ptr or 0), lp, ls),
                 "pnrt_update_vertices_device")

    def define_model(self, first: int, model8) -> int:
        """Keep a device copy of the (n, 8) MODEL-space records -- position 3, normal 3,
        texcoord 2 (``host.model_records``) -- of vertices first .. first + n - 1, for
        ``place_models`` (pnrt_define_model).  ``model8`` is a numpy array, or a torch
        tensor on the context's device (pnrt_define_model_device).  Returns the model's id:
        0, 1, 2, ... in definition order, until the next ``upload_scene``."""
        mid = ctypes.c_int(-1)
        if hasattr(model8, "data_ptr"):
            if model8.dtype.itemsize != 4 or not model8.is_contiguous() or model8.numel() % 8:
                raise ValueError("define_model: a contiguous float32 tensor of (n, 8) records")
            self._ck(self._lib.pnrt_define_model_device(self._ctx, first, model8.numel() // 8, ctypes.c_void_p(model8.data_ptr()),
                                                        ctypes.byref(mid)), "pnrt_define_model_device")
        else:
            rec = np.ascontiguousarray(model8, np.float32).reshape(-1, 8)
            self._ck(self._lib.pnrt_define_model(self._ctx, first, len(rec), N.fptr(rec) if len(rec) else None, ctypes.byref(mid)),
                     "pnrt_define_model")
        return mid.value

    def place_models(self, placements, relight: bool = False):
        """Move models on the device: ``placements`` is a sequence of (id, matrix) with the
        16 column-major floats ``host.model_matrix`` returns; every model's world-space
        records are rewritten from its model-space copy and the BVH refit once
        (pnrt_place_models; synchronous, as ``update_vertices``).  ``relight`` recomputes
        the light list's prefix areas from the new positions -- every entry's; False keeps
        them (no emissive triangle changed area).  Reset the accumulation afterwards."""
        placements = list(placements)
        arr = (N.Placement * max(len(placements), 1))()
        for k, (mid, matrix) in enumerate(placements):
            arr[k].model = int(mid)
            arr[k].matrix[:] = np.asarray(matrix, np.float32).reshape(16).tolist()
        self._ck(self._lib.pnrt_place_models(self._ctx, arr, len(placements), int(relight)), "pnrt_place_models")

    def read_vertices(self, first: int, count: int) -> np.ndarray:
        """The (count, 8) vertex records the device holds from ``first`` on: position 3,
        normal 3, texcoord 2 -- floats 0-5 and 12-13 of a packed record (pnrt_read_vertices)."""
        out = np.zeros((max(int(count), 0), 8), np.float32)
        self._ck(self._lib.pnrt_read_vertices(self._ctx, first, count, N.fptr(out) if len(out) else None), "pnrt_read_vertices")
        return out

    def read_bvh_boxes(self, nodes: np.ndarray) -> np.ndarray:
        """A copy of ``nodes`` -- the (nn, 12) pre-order node array that was uploaded -- with
        floats 0-5 of every node replaced by the box the device holds (pnrt_read_bvh_boxes)."""
        out = np.array(nodes, np.float32, order="C").reshape(-1, 12)
        self._ck(self._lib.pnrt_read_bvh_boxes(self._ctx, N.fptr(out), len(out)), "pnrt_read_bvh_boxes")
        return out

    def upload_texture(self, slot: int, pixels: np.ndarray, width: int, height: int, channels: int):
        px = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        self._ck(self._lib.pnrt_upload_texture(self._ctx, slot, N.u8ptr(px), width, height, channels),
                 "pnrt_upload_texture")

    def upload_env(self, rgb: np.ndarray | None, table: np.ndarray | None):
        if rgb is None:
            self._ck(self._lib.pnrt_upload_env(self._ctx, None, None, 0, 0), "pnrt_upload_env")
            return
        rgb = np.ascontiguousarray(rgb, np.float32)
        table = np.ascontiguousarray(table, np.float32)
        h, w = rgb.shape[:2]
        self._ck(self._lib.pnrt_upload_env(self._ctx, N.fptr(rgb), N.fptr(table), w, h), "pnrt_upload_env")

    def upload_env_build(self, rgb: np.ndarray):
        """Environment with its RandomHDR table built on the GPU (pt_env.h)."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        h, w = rgb.shape[:2]
        self._ck(self._lib.pnrt_upload_env_build(self._ctx, N.fptr(rgb), w, h), "pnrt_upload_env_build")
        self._env_shape = (h, w)

    def read_env_table(self) -> np.ndarray:
        return self._read_image(self._lib.pnrt_read_env_table, channels=(3,), size=self._env_shape)

    def build_bvh(self, tri_bounds: np.ndarray):
        """GPU BuildBVH (pnrt_bvh_build): (nodes (nn, 12) float32, order (n,) int32, max_depth)
        from per-triangle Bound + boundCenter (n, 9) -- the host build's result, bit for bit."""
        tb = np.ascontiguousarray(tri_bounds, np.float32).reshape(-1, 9)
        n = len(tb)
        cap = max(2 * n - 1, 1)
        nodes = np.empty((cap, 12), np.float32)
        order = np.empty(n, np.int32)
        nn, md = ctypes.c_int(), ctypes.c_int()
        self._ck(self._lib.pnrt_bvh_build(self._ctx, N.fptr(tb), n, N.fptr(nodes), cap, ctypes.byref(nn), N.iptr(order),
                                          ctypes.byref(md)), "pnrt_bvh_build")
        return nodes[:nn.value].copy(), order, md.value

    def set_frame(self, width: int, height: int, camera: np.ndarray, max_depth: int = 4):
        cam = _camera(camera)
        self._ck(self._lib.pnrt_set_frame(self._ctx, width, height, ctypes.byref(cam), max_depth), "pnrt_set_frame")
        self.width, self.height = width, height

    def set_options(self, traverse_mode: int):
        self._ck(self._lib.pnrt_set_options(self._ctx, traverse_mode), "pnrt_set_options")

    def stream_handle(self) -> int:
        """The context's own hipStream_t (for torch.cuda.ExternalStream)."""
        return int(self._lib.pnrt_get_stream(self._ctx) or 0)

    def set_stream(self, stream_handle: int | None):
        self._ck(self._lib.pnrt_set_stream(self._ctx, ctypes.c_void_p(stream_handle or 0)), "pnrt_set_stream")
        self._stream = stream_handle or 0

    def current_stream_handle(self) -> int:
        """The hipStream_t the context queues on now: ``set_stream``'s, or its own."""
        return self._stream or self.stream_handle()

    def load(self, cfg, traverse_mode: int = TRAVERSE_ZCULL):
        """Upload a :class:`pnraytracing_amd.scenes.SceneConfig`."""
        self.upload_scene(cfg.packed)
        for slot, (px, w, h, ch) in enumerate(cfg.textures):
            self.upload_texture(slot, px, w, h, ch)
        self.upload_env(cfg.env_rgb, cfg.env_table)
        self.set_frame(cfg.width, cfg.height, cfg.camera, cfg.max_depth)
        self.set_options(traverse_mode)

    # ---- frames ----------------------------------------------------------------------
    def render(self, first_frame: int, n_frames: int, band: int = 1, n_shards: int = 1, shard: int = 0):
        _u32("render", first_frame=first_frame, n_frames=n_frames)
        self._ck(self._lib.pnrt_render(self._ctx, first_frame, n_frames, band, n_shards, shard), "pnrt_render")

    def batch_plan(self, n_frames: int, band: int = 1, n_shards: int = 1, shard: int = 0) -> dict:
        """The batches ``render`` would run for such a call at the current frame size
        (pnrt_batch_plan): frames per full batch, number of batches, and the bytes of one
        full batch as PNRT_BATCH_BYTES measures them."""
        return self._plan("batch_plan", n_frames, band, n_shards, shard)

    def _plan(self, which, n_frames, band, n_shards, shard) -> dict:
        _u32(which, n_frames=n_frames)
        fpb, nb, by = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_int64()
        self._ck(getattr(self._lib, "pnrt_" + which)(self._ctx, n_frames, band, n_shards, shard, ctypes.byref(fpb),
                                                     ctypes.byref(nb), ctypes.byref(by)), "pnrt_" + which)
        return {"frames_per_batch": fpb.value, "n_batches": nb.value, "batch_bytes": by.value}

    def render_cameras(self, first_frame: int, cameras, band: int = 1, n_shards: int = 1, shard: int = 0):
        """``render`` with a camera per frame (pnrt_render_cameras): frame ``first_frame + k``
        is rendered with ``cameras[k]`` -- an (n, 12) or (n, 4, 3) float32 array of eye,
        lower_left, horizontal, vertical (``host.camera_sequence`` makes one for a pixel
        filter and a lens) -- in place of ``set_frame``'s camera, which stays current for
        every other call.  Asynchronous; the array is copied during the call."""
        cams = np.asarray(cameras)
        if cams.dtype != np.float32 or cams.ndim not in (2, 3) or cams.shape[1:] not in ((12,), (4, 3)):
            raise ValueError("render_cameras: cameras must be an (n, 12) or (n, 4, 3) float32 array")
        cams = np.ascontiguousarray(cams).reshape(-1, 12)
        _u32("render_cameras", first_frame=first_frame)
        self._ck(self._lib.pnrt_render_cameras(self._ctx, first_frame, len(cams),
                                               ctypes.cast(cams.ctypes.data, ctypes.POINTER(N.Camera)) if len(cams) else None,
                                               band, n_shards, shard), "pnrt_render_cameras")

    def cameras_batch_plan(self, n_frames: int, band: int = 1, n_shards: int = 1, shard: int = 0) -> dict:
        """``batch_plan`` for a ``render_cameras`` call (pnrt_cameras_batch_plan): the same
        rules with the 48-byte camera-ray record per path counted in ``batch_bytes``."""
        return self._plan("cameras_batch_plan", n_frames, band, n_shards, shard)

    # ---- caller ray buffers ---------------------------------------------------------------
    @staticmethod
    def _rays_ptr(rays) -> int:
        """A device ray buffer as an address: a torch tensor on the device (its data pointer), an integer, or None (0)."""
        if rays is None:
            return 0
        if isinstance(rays, int):
            return rays
        if hasattr(rays, "data_ptr") and hasattr(rays, "is_cuda"):
            if not rays.is_cuda:
                raise ValueError("rays must be a tensor on the device (or an integer device pointer)")
            if not rays.is_contiguous():
                raise ValueError("rays must be contiguous")
            return int(rays.data_ptr())
        raise ValueError("rays must be a torch tensor on the device or an integer device pointer")

    def render_rays(self, first_frame: int, n_frames: int, rays, frame_stride: int = 0, band: int = 1, n_shards: int = 1,
                    shard: int = 0):
        """``render`` from caller rays (pnrt_render_rays): pixel (x, y) of frame ``first_frame + k``
        starts from record ``k * frame_stride + y * width + x`` of ``rays`` -- a torch tensor on
        the device or an integer device pointer, 16-byte aligned, 8 floats per record (origin,
        -, direction, -), one record per pixel of the whole image.  ``frame_stride`` 0: one set
        serves every frame.  A record with a non-finite float or a zero direction is no ray:
        frame colour 0.  Asynchronous; the buffer is not copied -- keep it unchanged (and
        alive) until the work has completed."""
        _u32("render_rays", first_frame=first_frame, n_frames=n_frames)
        _i64("render_rays", frame_stride=frame_stride)
        ptr = self._rays_ptr(rays)
        self._ck(self._lib.pnrt_render_rays(self._ctx, first_frame, n_frames, ctypes.c_void_p(ptr), frame_stride, band, n_shards,
                                            shard), "pnrt_render_rays")

    def render_guides_rays(self, rays):
        """``render_guides`` with the camera rays of one set of ``width * height`` records
        (pnrt_render_guides_rays); asynchronous.  The guides carry no camera: ``denoise``,
        ``denoise_variance`` and ``read_aov`` accept them until the frame size, the scene or
        the traversal mode changes or ``render_guides`` / ``reproject`` replaces them."""
        ptr = self._rays_ptr(rays)
        self._ck(self._lib.pnrt_render_guides_rays(self._ctx, ctypes.c_void_p(ptr)), "pnrt_render_guides_rays")

    @staticmethod
    def ray_camera(model, camera, fov_deg: float = 180.0, aa_width: float = 0.0, lens_radius: float = 0.0,
                   focus_distance: float = 0.0, per_pixel: int = 0, reserved: int = 0) -> "N.RayCamera":
        """A ``pnrt_ray_camera``: ``model`` a name of ``CAM_MODELS`` or its number, ``camera`` the (4, 3) uniforms."""
        return N.RayCamera(PathTracer._enum("camera model", N.CAM_MODELS, model), _camera(camera), fov_deg, aa_width, lens_radius,
                           focus_distance, int(per_pixel), int(reserved))

    def make_rays(self, model, camera, first_frame: int = 0, n_sets: int = 1, frame_stride: int | None = None, out=None,
                  **params):
        """Ray sets of a camera model made on the device (pnrt_make_rays; asynchronous on the
        context's stream): ``n_sets`` sets for frames ``first_frame ..`` at the current frame
        size, ``frame_stride`` records apart (None: ``width * height``, or 0 for one set).
        ``params`` are ``ray_camera``'s (fov_deg, aa_width, lens_radius, focus_distance,
        per_pixel).  Returns the buffer: ``out`` when given (a float32 tensor on the device,
        or an integer pointer), else a new float32 tensor of shape (records, 8) -- allocated
        and filled on the wrapped context stream."""
        _u32("make_rays", first_frame=first_frame, n_sets=n_sets)
        pix = self.width * self.height
        if frame_stride is None:
            frame_stride = pix if n_sets > 1 else 0
        rc = self.ray_camera(model, camera, **params)
        if out is None:
            import torch
            records = pix if (frame_stride == 0 or n_sets == 0) else (n_sets - 1) * frame_stride + pix
            dev = torch.device("cuda", self._device)
            with torch.cuda.stream(torch.cuda.ExternalStream(self.current_stream_handle(), device=dev)):
                out = torch.empty((max(records, 1), 8), dtype=torch.float32, device=dev)
        ptr = self._rays_ptr(out)
        self._ck(self._lib.pnrt_make_rays(self._ctx, ctypes.byref(rc), first_frame, n_sets, ctypes.c_void_p(ptr), frame_stride),
                 "pnrt_make_rays")
        return out

    def reset_accum(self):
        self._ck(self._lib.pnrt_reset_accum(self._ctx), "pnrt_reset_accum")

    def synchronize(self):
        self._ck(self._lib.pnrt_synchronize(self._ctx), "pnrt_synchronize")

    def read_accum(self) -> np.ndarray:
        return self._read_image(self._lib.pnrt_read_accum)

    def _read_image(self, fn, *args, channels=(4,), dtype=np.float32, size=None) -> np.ndarray:
        """A (H, W[, C]) image of the frame's size (or ``size``) read through the library's ``fn(ctx, *args, out)``."""
        out = np.empty((*(size or (self.height, self.width)), *channels), dtype)
        self._ck(fn(self._ctx, *args, N.u8ptr(out) if dtype is np.uint8 else N.fptr(out)), fn.__name__)
        return out

    def accum_ptr(self) -> int:
        return int(self._lib.pnrt_accum_device_ptr(self._ctx) or 0)

    # ---- guide images and the denoised preview -------------------------------------------
    def render_guides(self):
        """First-hit position / normal / albedo images of the whole frame for the current
        camera, scene and traversal mode (pnrt_render_guides); asynchronous."""
        self._ck(self._lib.pnrt_render_guides(self._ctx), "pnrt_render_guides")

    def read_aov(self, name) -> np.ndarray:
        """One guide image, (H, W, 4) float32, row 0 = bottom: ``"position"`` (w = hit flag),
        ``"normal"`` (w = material id, -1 on a miss) or ``"albedo"`` (w = texture id or -1)."""
        return self._read_image(self._lib.pnrt_read_aov, self._enum("guide image", N.AOV_NAMES, name))

    def aov_ptr(self, name) -> int:
        return int(self._lib.pnrt_aov_device_ptr(self._ctx, self._enum("guide image", N.AOV_NAMES, name)) or 0)

    def denoise(self, levels: int | None = None, sigma_color: float | None = None, sigma_normal: float | None = None,
                sigma_position: float | None = None):
        """The a-trous preview of the accumulation image into the denoised image
        (pnrt_denoise); asynchronous.  Arguments left out take the library's defaults."""
        params = _params(N.DenoiseParams, DENOISE_DEFAULTS, levels, sigma_color, sigma_normal, sigma_position)
        self._ck(self._lib.pnrt_denoise(self._ctx, params), "pnrt_denoise")

    def denoise_variance(self, levels: int | None = None, sigma_variance: float | None = None,
                         sigma_normal: float | None = None, sigma_position: float | None = None):
        """The variance-guided a-trous preview into the same denoised image
        (pnrt_denoise_variance); asynchronous.  ``sigma_variance`` counts standard errors of
        the centre pixel, taken from the sample moments, which must cover the accumulation
        (``enable_moments`` before the frames).  Arguments left out take the library's defaults."""
        params = _params(N.DenoiseVarianceParams, DENOISE_VARIANCE_DEFAULTS, levels, sigma_variance, sigma_normal, sigma_position)
        self._ck(self._lib.pnrt_denoise_variance(self._ctx, params), "pnrt_denoise_variance")

    def read_denoised(self) -> np.ndarray:
        return self._read_image(self._lib.pnrt_read_denoised)

    def denoised_ptr(self) -> int:
        return int(self._lib.pnrt_denoised_device_ptr(self._ctx) or 0)

    # ---- the display transform and auto exposure ------------------------------------------
    @staticmethod
    def _enum(what, names, v) -> int:
        if isinstance(v, str):
            if v not in names:
                raise ValueError(f"unknown {what} {v!r}: one of {names}")
            return names.index(v)
        return int(v)

    def display(self, source="accum", tone="clamp", transfer="linear", exposure: float = 1.0, white: float = 4.0,
                bottom_first: bool = False, src_ptr: int | None = None):
        """One of the float images to the 8-bit RGBA display image on the device
        (pnrt_display; asynchronous): ``source`` ``"accum"``, ``"denoised"`` or ``"external"``
        (then ``src_ptr``: a device image of width*height float4, row 0 = bottom), times
        ``exposure``, through the ``tone`` curve ``"clamp"``, ``"reinhard"`` (white point
        ``white``) or ``"aces"`` and the ``transfer`` ``"linear"`` or ``"srgb"``.  The
        defaults are the reference's display, ``image.to_display`` plus alpha."""
        p = N.DisplayParams(self._enum("display source", N.DISPLAY_SOURCES, source),
                            self._enum("tone curve", N.DISPLAY_TONES, tone),
                            self._enum("transfer", N.DISPLAY_TRANSFERS, transfer),
                            int(bottom_first), exposure, white, ctypes.c_void_p(src_ptr or 0))
        self._ck(self._lib.pnrt_display(self._ctx, ctypes.byref(p)), "pnrt_display")

    def read_display(self) -> np.ndarray:
        """The display image, (H, W, 4) uint8, alpha 255; top row first unless the last
        ``display`` asked for ``bottom_first`` (pnrt_read_display; synchronises)."""
        return self._read_image(self._lib.pnrt_read_display, dtype=np.uint8)

    def display_ptr(self) -> int:
        return int(self._lib.pnrt_display_device_ptr(self._ctx) or 0)

    def luma_histogram(self, source="accum", band: int = 1, n_shards: int = 1, shard: int = 0,
                       src_ptr: int | None = None) -> dict:
        """The luminance histogram of a display source over the rows of a shard selector
        (pnrt_luma_histogram_read; synchronous): ``n_pixels``, ``n_counted`` and ``bins``,
        a (512,) int64 array, 16 bins per octave, luminance 1.0 in bin 256.  Histograms of
        disjoint selectors add up (``merge_histograms``)."""
        h = N.LumaHistogram()
        self._ck(self._lib.pnrt_luma_histogram_read(self._ctx, self._enum("display source", N.DISPLAY_SOURCES, source),
                                                    ctypes.c_void_p(src_ptr or 0), band, n_shards, shard, ctypes.byref(h)),
                 "pnrt_luma_histogram_read")
        return {"n_pixels": h.n_pixels, "n_counted": h.n_counted, "bins": np.array(h.bins, np.int64)}

    # ---- ray queries ---------------------------------------------------------------------
    def query_rays(self,rays: np.ndarray, any_hit: bool = False) -> np.ndarray:
        """The closest hit (or, with ``any_hit``, whether anything is hit) of caller rays
        against the uploaded scene (pnrt_query_rays; synchronous): rays (n, 7) float32 =
        origin, direction, tMax -> (n, 16) uint32 records, see ``decode_hits``.  The
        renderer's own traversal; needs no ``set_frame`` and changes no image."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
        out = np.empty((len(r), 16), np.uint32)
        self._ck(self._lib.pnrt_query_rays(self._ctx, N.fptr(r) if len(r) else None, len(r),
                                           N.QUERY_ANY if any_hit else N.QUERY_CLOSEST,
                                           out.ctypes.data_as(ctypes.POINTER(N.Hit)) if len(r) else None), "pnrt_query_rays")
        return out

    def query_rays_device(self, rays_ptr: int, n: int, out_ptr: int, any_hit: bool = False):
        """The same from device memory into device memory (pnrt_query_rays_device):
        ``rays_ptr`` n x 7 floats, ``out_ptr`` n x 64 bytes, 16-byte aligned.  Asynchronous
        on the context's stream, after everything already queued there."""
        self._ck(self._lib.pnrt_query_rays_device(self._ctx, ctypes.c_void_p(rays_ptr or 0), n,
                                                  N.QUERY_ANY if any_hit else N.QUERY_CLOSEST, ctypes.c_void_p(out_ptr or 0)),
                 "pnrt_query_rays_device")

    # ---- sample moments and the convergence measure --------------------------------------
    def enable_moments(self, on: bool = True):
        """Keep per-pixel moments of the frames' luminance from now on (pnrt_enable_moments):
        the blend of every ``render`` batch folds its frames in.  Waits for the calls in
        flight; disabling keeps the image, enabling again keeps its data."""
        self._ck(self._lib.pnrt_enable_moments(self._ctx, int(bool(on))), "pnrt_enable_moments")

    def read_moments(self) -> np.ndarray:
        """The moments image, (H, W, 4) float32, row 0 = bottom: mean luminance, M2, 0, and
        the frame count n as uint32 bits (``m[..., 3].view(np.uint32)``)."""
        return self._read_image(self._lib.pnrt_read_moments)

    def read_error(self) -> np.ndarray:
        """The clamped relative standard error of every pixel, (H, W) float32, +inf where
        fewer than two frames were folded in (pnrt_read_error)."""
        return self._read_image(self._lib.pnrt_read_error, channels=())

    def moments_ptr(self) -> int:
        return int(self._lib.pnrt_moments_device_ptr(self._ctx) or 0)

    def convergence(self, threshold: float, band: int = 1, n_shards: int = 1, shard: int = 0) -> dict:
        """Statistics of the error over the rows of a shard selector (pnrt_convergence,
        synchronous): the fields of ``pnrt_convergence_stats`` and ``mean_error``."""
        st = N.ConvergenceStats()
        self._ck(self._lib.pnrt_convergence(self._ctx, ctypes.c_float(threshold), band, n_shards, shard, ctypes.byref(st)),
                 "pnrt_convergence")
        return _with_mean_error(_as_dict(st))

    def render_adaptive(self, first: int, n: int, threshold: float, min_frames: int = 8, band: int = 1, n_shards: int = 1,
                        shard: int = 0) -> dict:
        """Frames ``first .. first + n - 1`` for the pixels of the selector's rows that have
        not converged (pnrt_render_adaptive): fewer than ``max(min_frames, 2)`` frames, or a
        relative standard error above ``threshold``.  Needs the sample moments enabled since
        the accumulation was last reset.  Waits for the calls in flight, evaluates the mask
        once, then queues the frames like ``render``.  Returns the fields of
        ``pnrt_adaptive_stats``; ``n = 0`` only asks how much is left."""
        _u32("render_adaptive", first=first, n=n, min_frames=min_frames)
        st = N.AdaptiveStats()
        self._ck(self._lib.pnrt_render_adaptive(self._ctx, first, n, ctypes.c_float(threshold), min_frames, band, n_shards,
                                                shard, ctypes.byref(st)), "pnrt_render_adaptive")
        return _as_dict(st)

    def render_rays_adaptive(self, first: int, n: int, rays, frame_stride: int, threshold: float, min_frames: int = 8,
                             band: int = 1, n_shards: int = 1, shard: int = 0) -> dict:
        """``render_adaptive`` over caller rays (pnrt_render_rays_adaptive): the active pixels
        receive the frames ``render_rays`` would render from ``rays`` / ``frame_stride`` (its
        buffer rules; the records of inactive pixels do not matter), folded at the weight of
        the pixel's own count.  ``threshold 0, min_frames 0xFFFFFFFF`` makes every pixel
        active.  Returns the fields of ``pnrt_adaptive_stats``."""
        _u32("render_rays_adaptive", first=first, n=n, min_frames=min_frames)
        _i64("render_rays_adaptive", frame_stride=frame_stride)
        ptr = self._rays_ptr(rays)
        st = N.AdaptiveStats()
        self._ck(self._lib.pnrt_render_rays_adaptive(self._ctx, first, n, ctypes.c_void_p(ptr), frame_stride,
                                                     ctypes.c_float(threshold), min_frames, band, n_shards, shard, ctypes.byref(st)),
                 "pnrt_render_rays_adaptive")
        return _as_dict(st)

    def reproject(self, from_camera: np.ndarray, normal_min: float | None = None, position_tolerance: float | None = None,
                  max_history: int | None = None) -> dict:
        """After a camera move: resample the accumulation and the moments from the view
        ``from_camera`` ((4, 3) uniforms, as ``set_frame`` takes them) they were rendered
        with into the current camera (pnrt_reproject; synchronous, whole image).  History
        of another surface is rejected through the guide images of both views; a
        reprojected pixel keeps ``min(its taps' frame counts, max_history)`` frames, a
        disoccluded or missed one starts at zero.  Continue with
        ``render_adaptive(first >= 1, ...)``, which weighs every pixel by its own count.
        Leaves the guide images valid for the current camera.  Arguments left out take
        the library's defaults.  Returns the fields of ``pnrt_reproject_stats``."""
        cam = _camera(from_camera)
        params = self._reproject_params("reproject", normal_min, position_tolerance, max_history)
        st = N.ReprojectStats()
        self._ck(self._lib.pnrt_reproject(self._ctx, ctypes.byref(cam), params, ctypes.byref(st)), "pnrt_reproject")
        return _as_dict(st)

    @staticmethod
    def _reproject_params(who, normal_min, position_tolerance, max_history):
        """``pnrt_reproject_params`` by reference, or None (the library's defaults) when nothing was given."""
        if max_history is not None:
            _u32(who, max_history=max_history)
        return _params(N.ReprojectParams, REPROJECT_DEFAULTS, normal_min, position_tolerance, max_history)

    def reproject_view(self, from_view, to_view, normal_min: float | None = None, position_tolerance: float | None = None,
                       max_history: int | None = None) -> dict:
        """``reproject`` with both views given as camera models (pnrt_reproject_view;
        synchronous, whole image): from the view ``from_view`` the accumulation was rendered
        with into ``to_view``, each a ``RayCamera`` (``ray_camera``) or a ``(model, camera,
        fov_deg)`` tuple -- the model's centre rays; jitter and lens fields are checked and
        ignored.  The ``set_frame`` camera is not read.  An equirectangular ``from_view``
        wraps in x; a pixel of ``to_view`` without a ray counts as missed.  Continue with
        ``render_rays_adaptive(first, n, rays, stride, 0.0, 0xFFFFFFFF)``.  Leaves the guide
        images of ``to_view``'s centre rays (``make_rays`` + ``render_guides_rays``).
        Arguments left out take the library's defaults.  Returns the fields of
        ``pnrt_reproject_stats``."""
        views = [v if isinstance(v, N.RayCamera) else self.ray_camera(*v) for v in (from_view, to_view)]
        params = self._reproject_params("reproject_view", normal_min, position_tolerance, max_history)
        st = N.ReprojectStats()
        self._ck(self._lib.pnrt_reproject_view(self._ctx, ctypes.byref(views[0]), ctypes.byref(views[1]), params, ctypes.byref(st)),
                 "pnrt_reproject_view")
        return _as_dict(st)

    def pack_rows(self, dst_ptr: int, band: int, n_shards: int, shard: int):
        self._ck(self._lib.pnrt_pack_rows(self._ctx, ctypes.c_void_p(dst_ptr), band, n_shards, shard), "pnrt_pack_rows")

    def unpack_rows(self, src_ptr: int, dst_ptr: int, band: int, n_shards: int, shard: int):
        """Shard `shard`'s packed rows (device buffer) into their rows of a device image
        (height x width x 4 floats), on the context stream (pnrt_unpack_rows)."""
        self._ck(self._lib.pnrt_unpack_rows(self._ctx, ctypes.c_void_p(src_ptr), ctypes.c_void_p(dst_ptr), band,
                                            n_shards, shard), "pnrt_unpack_rows")

    def device_info(self) -> dict:
        info = N.DeviceInfo()
        self._ck(self._lib.pnrt_get_device_info(self._ctx, ctypes.byref(info)), "pnrt_get_device_info")
        return _as_dict(info)

    def profile_enable(self, on: bool = True):
        """Bracket every kernel launch with HIP events on the launch stream (resets totals)."""
        self._ck(self._lib.pnrt_profile_enable(self._ctx, int(bool(on))), "pnrt_profile_enable")

    def profile_select(self, classes=None):
        """Kernel classes to time (names of K_CLASSES; None = all)."""
        mask = -1 if classes is None else sum(1 << N.K_CLASSES.index(k) for k in classes)
        self._ck(self._lib.pnrt_profile_select(self._ctx, mask), "pnrt_profile_select")

    def profile_read(self) -> dict:
        """{kernel class: (total ms, launches)} since profile_enable (synchronises)."""
        p = N.Profile()
        self._ck(self._lib.pnrt_profile_read(self._ctx, ctypes.byref(p)), "pnrt_profile_read")
        return {k: (p.ms[i], int(p.launches[i])) for i, k in enumerate(N.K_CLASSES)}

    def version(self) -> str:
        """pnrt_version(): library version + sha256 of the device sources it was built from."""
        return self._lib.pnrt_version().decode()

    def debug_math(self, fn: int, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
        a = np.ascontiguousarray(a, np.float32)
        b = None if b is None else np.ascontiguousarray(b, np.float32)
        out = np.empty_like(a)
        self._ck(self._lib.pnrt_debug_math(self._ctx, fn, N.fptr(a), N.fptr(b), N.fptr(out), len(a)), "pnrt_debug_math")
        return out


def decode_hits(records: np.ndarray) -> dict:
    """The named fields of ``query_rays`` records ((n, 16) uint32, or one record): hit
    (bool), position (n, 3), normal (n, 3), uv (n, 2), texture_id, material_id (int32), t
    (the hit's time), t_max (the ray's tMax afterwards), triangle (int32 index into the
    uploaded triangles, -1 without a hit), invalid (bool: a non-finite or zero-direction
    ray, not traced).  Without a hit, and for an any-hit query, position .. t are zero."""
    w = np.ascontiguousarray(records, np.uint32).reshape(-1, 16)
    f, i = w.view(np.float32), w.view(np.int32)
    return {"hit": w[:, 0] != 0, "position": f[:, 1:4], "normal": f[:, 4:7], "uv": f[:, 7:9],
            "texture_id": i[:, 9], "material_id": i[:, 10], "t": f[:, 11], "t_max": f[:, 12],
            "triangle": i[:, 13], "invalid": (w[:, 14] & 1) != 0}


CONVERGENCE_FIELDS = ("n_pixels", "n_measured", "n_above", "sum_q16", "max_error", "min_frames", "max_frames")


def _with_mean_error(d: dict) -> dict:
    d["mean_error"] = d["sum_q16"] / 65536 / d["n_measured"] if d["n_measured"] else 0.0
    return d


def merge_convergence(stats: list) -> dict:
    """The statistics of the union of disjoint row sets from each set's own
    (``PathTracer.convergence`` dicts): counts and ``sum_q16`` add, ``max_error`` and
    ``max_frames`` take the max, ``min_frames`` the min -- over the sets that have
    pixels (a set without rows reports zeros, which say nothing about the minimum)."""
    some = [s for s in stats if s["n_pixels"]]
    out = {k: sum(s[k] for s in some) for k in ("n_pixels", "n_measured", "n_above", "sum_q16")}
    out["max_error"] = max((s["max_error"] for s in some), default=0.0)
    out["min_frames"] = min((s["min_frames"] for s in some), default=0)
    out["max_frames"] = max((s["max_frames"] for s in some), default=0)
    return _with_mean_error(out)


def merge_histograms(hists: list) -> dict:
    """The histogram of the union of disjoint row sets (``PathTracer.luma_histogram``
    dicts): every field adds."""
    return {"n_pixels": sum(h["n_pixels"] for h in hists), "n_counted": sum(h["n_counted"] for h in hists),
            "bins": sum((np.asarray(h["bins"], np.int64) for h in hists), np.zeros(N.LUMA_BINS, np.int64))}


def exposure_from_histogram(hist: dict, low: int = 50, high: int = 950, key: float = 0.18) -> float:
    """The exposure that brings the histogram's trimmed mean bin -- the pixels between
    the ``low`` and ``high`` permille of the counted ones -- to the luminance ``key``
    (pnrt_exposure_from_histogram: host code, integer arithmetic, a 1/16-stop grid)."""
    bins = np.asarray(hist["bins"], np.int64)
    if bins.shape != (N.LUMA_BINS,):
        raise ValueError(f"exposure_from_histogram: need {N.LUMA_BINS} bins, got {bins.shape}")
    h = N.LumaHistogram(int(hist["n_pixels"]), int(hist["n_counted"]), (ctypes.c_int64 * N.LUMA_BINS)(*map(int, bins)))
    out = ctypes.c_float()
    rc = N.device_lib().pnrt_exposure_from_histogram(ctypes.byref(h), low, high, ctypes.c_float(key), ctypes.byref(out))
    if rc != 0:
        e = PnrtError(f"pnrt_exposure_from_histogram failed ({rc}): need 0 <= low < high <= 1000 and a finite key > 0")
        e.code = rc
        raise e
    return out.value


def shard_rows(height: int, band: int, n_shards: int, shard: int) -> np.ndarray:
    """Rows y with (y // band) % n_shards == shard, increasing (pnrt_pack_rows order)."""
    y = np.arange(height)
    return y[(y // band) % n_shards == shard]
