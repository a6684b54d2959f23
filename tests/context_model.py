"""TEST INFRASTRUCTURE: a CPU model of one pnrt context -- ``ModelTracer`` answers the calls
of ``PathTracer`` (the same method names and argument forms) from plain numpy state and the
pinned restatements of this directory: pyoracle.Oracle (render_colors, intersect),
moments_ref, adaptive_ref, reproject_ref, refit_ref, place_ref, atrous_ref, atrous_var_ref,
display_ref and guides_common.

The model knows no pipes, streams, epochs or caches: every call recomputes what it needs
from the scene arrays as they stand, so after any sequence of calls its images are what a
context that kept nothing between calls would hold.  Its rules are the contract's
(include/pnrt.h), not the library's code: which calls zero the accumulation,
which leave the guide images stale, when the moments cover the accumulation, which calls
are refused (``PnrtError`` with the same ``code``).  What a guide, denoised or display image
"was rendered for" is kept beside the image as plain values -- camera, size, traversal
mode and the number of scene-changing calls so far -- and compared when the contract says
the image must still fit.

Out of scope: ``render_cameras`` (the oracle has no jittered camera); ray sets other than
the pinhole set of a camera (``render_rays`` / ``render_rays_adaptive`` take the rays of
``make_rays("pinhole", camera)`` with aa_width 0 and no lens, which tests/test_gpu_rays.py
pins to ``render``: the model renders that camera; ``reproject_view`` and
``render_guides_rays`` are not modelled); ``dist``, several contexts and ``set_stream``;
``PNRT_BATCH_BYTES`` and ``PNRT_SERIAL``, which are per process and change no image.
Argument errors (PNRT_E_ARG) are not modelled: the sequences make none."""
from __future__ import annotations

import types

import numpy as np

import adaptive_ref as A
import atrous_ref as AT
import atrous_var_ref as AV
import display_ref as D
import moments_ref as R
import place_ref as P
import pyoracle
import refit_ref as RF
import reproject_ref as RP
from guides_common import camera_rays, sample_albedo
from pnraytracing_amd import host as H
from pnraytracing_amd.tracer import (DENOISE_DEFAULTS, DENOISE_VARIANCE_DEFAULTS, KERNEL_V1, REPROJECT_DEFAULTS, TRAVERSE_ZCULL,
                                     PnrtError, _with_mean_error, shard_rows)

F = np.float32
U = np.uint32
E_STATE = -3


def refuse(what: str):
    e = PnrtError(f"model: {what}")
    e.code = E_STATE
    raise e


def _given(defaults: dict, values) -> dict:
    return {k: (d if v is None else v) for (k, d), v in zip(defaults.items(), values)}


class ModelTracer:
    def __init__(self, device: int = 0):
        self.has_scene = False
        self.width = self.height = 0
        self.camera = None
        self.depth = 4
        self.mode, self.v1 = TRAVERSE_ZCULL, False
        self.textures = {}
        self.env_rgb = self.env_table = None
        self.models = []
        self.accum = self.moments = None
        self.moments_on = self.moments_ever = self.cover = False
        self.scene_calls = 0                 # scene-changing calls so far (what guide images remember)
        self.guides = None                   # {"position", "normal", "albedo", "for": _fits()}
        self.denoised = self.disp = None

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        pass

    # ---- the scene ---------------------------------------------------------------------------
    def upload_scene(self, p):
        self.V, self.M, self.T, self.Nd, self.L = (np.array(a, F, order="C") for a in p.arrays())
        self.L = self.L.reshape(-1, 3)
        self.sum_area = float(p.lights_sum_area)
        self.tree_depth = p.max_depth
        self.M_uploaded = self.M.copy()
        self.models = []
        self.has_scene = True
        self.scene_calls += 1

    def load(self, cfg, traverse_mode: int = TRAVERSE_ZCULL):
        self.upload_scene(cfg.packed)
        for slot, (px, w, h, ch) in enumerate(cfg.textures):
            self.upload_texture(slot, px, w, h, ch)
        self.upload_env(cfg.env_rgb, cfg.env_table)
        self.set_frame(cfg.width, cfg.height, cfg.camera, cfg.max_depth)
        self.set_options(traverse_mode)

    def update_materials(self, first: int, records):
        rec = np.asarray(records, F).reshape(-1, 18)
        self.M[first:first + len(rec)] = rec
        self.scene_calls += 1

    def _refit(self):
        self.Nd = RF.refit_ref(self.V, self.T, self.Nd)

    def update_vertices(self, first: int, vertices, lights=None, lights_sum_area=None):
        rec = np.asarray(vertices, F).reshape(-1, 15)
        self.V[first:first + len(rec)] = rec
        if lights is not None:
            self.L = np.array(lights, F).reshape(-1, 3)
            self.sum_area = float(self.L[-1, 1]) if lights_sum_area is None else float(lights_sum_area)
        self._refit()
        self.scene_calls += 1

    def define_model(self, first: int, model8) -> int:
        self.models.append((int(first), np.array(model8, F).reshape(-1, 8)))
        return len(self.models) - 1

    def place_models(self, placements, relight: bool = False):
        for mid, matrix in placements:
            first, rec = self.models[mid]
            self.V[first:first + len(rec), [0, 1, 2, 3, 4, 5, 12, 13]] = P.place_ref(rec, np.asarray(matrix, F).reshape(16))
        self._refit()
        if relight:                          # every entry's area from the new positions; the list is the uploaded one
            _, L, s = H.scene_relight(self.V, self.T, self.M_uploaded)
            assert np.array_equal(L[:, 0], self.L[:, 0])
            self.L, self.sum_area = L, s
        self.scene_calls += 1

    def read_vertices(self, first: int, count: int):
        return P.words8(self.V[first:first + count])

    def read_bvh_boxes(self, nodes):
        out = np.array(nodes, F, order="C").reshape(-1, 12)
        out[:, 0:6] = self.Nd[:, 0:6]
        return out

    def upload_texture(self, slot: int, pixels, width: int, height: int, channels: int):
        self.textures[slot] = (np.array(pixels, np.uint8).reshape(-1), width, height, channels)
        self.scene_calls += 1

    def upload_env(self, rgb, table):
        self.env_rgb = None if rgb is None else np.array(rgb, F)
        self.env_table = None if rgb is None else np.array(table, F)
        self.scene_calls += 1

    def upload_env_build(self, rgb):
        self.upload_env(rgb, H.hdr_table(np.asarray(rgb, F)))

    # ---- the frame ---------------------------------------------------------------------------
    def set_frame(self, width: int, height: int, camera, max_depth: int = 4):
        if (width, height) != (self.width, self.height) or self.accum is None:
            self.accum = np.zeros((height, width, 4), F)
            self.width, self.height = width, height
            if self.moments_ever:            # zeroed together with the accumulation
                self.moments = R.zeros(height, width)
                self.cover = True
        self.camera = np.array(camera, F).reshape(4, 3)
        self.depth = max_depth

    def set_options(self, traverse_mode: int):
        self.mode, self.v1 = traverse_mode & 0xFF, bool(traverse_mode & KERNEL_V1)

    def _cfg(self, camera=None):
        packed = H.PackedScene(self.V, self.M, self.T, self.Nd, self.L, self.sum_area, self.tree_depth)
        tex = [self.textures[k] for k in range(len(self.textures))]
        return types.SimpleNamespace(packed=packed, textures=tex, env_rgb=self.env_rgb, env_table=self.env_table,
                                     camera=self.camera if camera is None else np.asarray(camera, F).reshape(4, 3),
                                     width=self.width, height=self.height, max_depth=self.depth)

    def _need_scene_frame(self, who):
        if not self.has_scene or self.camera is None:
            refuse(f"{who}: upload_scene and set_frame first")

    def _need_moments(self, who):
        if not self.moments_on or self.moments is None:
            refuse(f"{who}: the sample moments are not enabled")
        if not self.cover:
            refuse(f"{who}: the moments do not cover the accumulation")

    def colors(self, first: int, n: int):
        """The clamped colours of frames first .. first + n - 1 of the scene as it stands: (n, H, W, 3)."""
        c, st = pyoracle.Oracle(self._cfg()).render_colors(first, n)
        assert st["stack_overflow"] == 0
        return c

    # ---- rendering ---------------------------------------------------------------------------
    def _render(self, who, first, n, band, n_shards, shard, uncover_before_rows):
        rows = shard_rows(self.height, band, n_shards, shard)
        if n == 0:
            return
        if uncover_before_rows or len(rows):
            if not self.moments_on:
                self.cover = False
        if len(rows) == 0:
            return
        c = self.colors(first, n)[:, rows]
        frames = range(first, first + n)
        self.accum[rows] = R.blend(self.accum[rows], c, frames)
        if self.moments_on:
            self.moments[rows] = R.update(self.moments[rows], c, frames)

    def render(self, first_frame: int, n_frames: int, band: int = 1, n_shards: int = 1, shard: int = 0):
        self._need_scene_frame("render")
        if self.v1 and self.moments_on:
            refuse("render: PNRT_KERNEL_V1 cannot update the sample moments")
        self._render("render", first_frame, n_frames, band, n_shards, shard, True)

    def make_rays(self, model, camera, **params):
        """The pinhole set of `camera`: the model renders the camera itself (see the module's scope)."""
        assert model == "pinhole" and not params
        return np.array(camera, F).reshape(4, 3)

    def _rays_camera(self, rays):
        assert np.array_equal(rays, self.camera), "the model takes the pinhole set of the current camera only"

    def render_rays(self, first_frame: int, n_frames: int, rays, frame_stride: int = 0, band: int = 1, n_shards: int = 1,
                    shard: int = 0):
        self._need_scene_frame("render_rays")
        if self.v1:
            refuse("render_rays: PNRT_KERNEL_V1 renders the pnrt_set_frame camera only")
        self._rays_camera(rays)
        self._render("render_rays", first_frame, n_frames, band, n_shards, shard, False)

    def render_adaptive(self, first: int, n: int, threshold: float, min_frames: int = 8, band: int = 1, n_shards: int = 1,
                        shard: int = 0) -> dict:
        self._need_scene_frame("render_adaptive")
        self._need_moments("render_adaptive")
        if self.v1:
            refuse("render_adaptive: PNRT_KERNEL_V1 has no per-frame colours")
        c = self.colors(first, n) if n else []
        self.accum, self.moments, stats = A.render(self.accum, self.moments, c, range(first, first + n), threshold, min_frames,
                                                   band, n_shards, shard)
        return stats

    def render_rays_adaptive(self, first: int, n: int, rays, frame_stride: int, threshold: float, min_frames: int = 8,
                             band: int = 1, n_shards: int = 1, shard: int = 0) -> dict:
        self._need_scene_frame("render_rays_adaptive")
        self._need_moments("render_rays_adaptive")
        if self.v1:
            refuse("render_rays_adaptive: PNRT_KERNEL_V1 has no per-frame colours")
        self._rays_camera(rays)
        return self.render_adaptive(first, n, threshold, min_frames, band, n_shards, shard)

    # ---- accumulation state ------------------------------------------------------------------
    def reset_accum(self):
        if self.accum is None:
            return
        self.accum[...] = 0
        if self.moments is not None:
            self.moments[...] = 0
            self.cover = True

    def synchronize(self):
        pass

    def enable_moments(self, on: bool = True):
        if on and self.moments is None and self.accum is not None:
            self.moments = R.zeros(self.height, self.width)
            self.cover = True
        if on:
            self.moments_ever = True
        self.moments_on = bool(on)

    def read_accum(self):
        if self.accum is None:
            refuse("read_accum: no frame")
        return self.accum.copy()

    def _need_moments_image(self, who):
        if not self.moments_ever or self.moments is None:
            refuse(f"{who}: enable_moments first")

    def read_moments(self):
        self._need_moments_image("read_moments")
        return self.moments.copy()

    def read_error(self):
        self._need_moments_image("read_error")
        return R.error(self.moments)

    def convergence(self, threshold: float, band: int = 1, n_shards: int = 1, shard: int = 0) -> dict:
        self._need_moments_image("convergence")
        st = R.stats(self.moments, threshold, shard_rows(self.height, band, n_shards, shard))
        st["max_error"] = float(F(st["max_error"]))
        return _with_mean_error(st)

    # ---- first hits, guide images, queries -----------------------------------------------------
    def _fits(self, camera=None):
        """What images made now for `camera` are made for."""
        cam = self.camera if camera is None else np.asarray(camera, F).reshape(4, 3)
        return (cam.tobytes(), self.width, self.height, self.mode, self.scene_calls)

    def first_hits(self, camera=None):
        """The three guide images of a camera, (H, W, 4) each, from the oracle's closest hits."""
        cfg = self._cfg(camera)
        orc = pyoracle.Oracle(cfg)
        rays = camera_rays(cfg)
        o = orc.intersect(rays, 0, 0)
        n = len(o)
        hit = o[:, 0] != 0
        tex, mat = o[:, 9].view(np.int32), o[:, 10].view(np.int32)
        pos, nrm, alb = (np.zeros((n, 4), F) for _ in range(3))
        pos[:, :3] = o[:, 1:4].view(F)
        pos[:, 3] = hit
        nrm[:, :3] = o[:, 4:7].view(F)
        nrm[:, 3] = np.where(hit, mat, -1)
        pos[~hit, :3] = 0
        nrm[~hit, :3] = 0
        em = self.M[np.clip(mat, 0, None), 0:3]
        emissive = hit & np.any(em != 0, axis=1)
        want = self.M[np.clip(mat, 0, None), 3:6].copy()
        want[emissive] = em[emissive]
        for t in np.unique(tex[hit & ~emissive & (tex >= 0)]):
            k = hit & ~emissive & (tex == t)
            want[k] = sample_albedo(self.textures[int(t)], o[k, 7].view(F), o[k, 8].view(F)) if int(t) in self.textures else 0
        alb[hit, :3] = want[hit]
        if self.env_rgb is not None and (~hit).any():
            d = np.ascontiguousarray(rays[~hit, 3:6]).view(U)
            alb[~hit, :3] = orc.shade_eval(12, d).view(F)
        alb[:, 3] = np.where(hit, tex, -1)
        shape = (self.height, self.width, 4)
        return {"position": pos.reshape(shape), "normal": nrm.reshape(shape), "albedo": alb.reshape(shape)}

    def first_hit_image(self):
        """What a kept primary record carries, per pixel: the hit's position, normal and material with that
        material's emission, or the miss colour -- (H * W, 14) uint32 words."""
        g = self.first_hits()
        mat = g["normal"][..., 3].astype(np.int64)
        em = np.where((mat >= 0)[..., None], self.M[np.clip(mat, 0, None), 0:3], g["albedo"][..., :3])
        return np.concatenate([g["position"], g["normal"], g["albedo"][..., 3:4], em, mat[..., None].astype(F)],
                              axis=-1).astype(F).reshape(self.width * self.height, -1).view(U)

    def render_guides(self):
        self._need_scene_frame("render_guides")
        self.guides = dict(self.first_hits(), **{"for": self._fits()})

    def read_aov(self, name):
        if self.guides is None:
            refuse("read_aov: render_guides first")
        if self.guides["position"].shape[:2] != (self.height, self.width):
            refuse("read_aov: the guide images have another size than the frame")
        return self.guides[name].copy()

    def _need_guides(self, who):
        if self.guides is None:
            refuse(f"{who}: render_guides first")
        if self.guides["for"] != self._fits():
            refuse(f"{who}: the guide images are stale")

    def query_rays(self, rays, any_hit: bool = False):
        if not self.has_scene:
            refuse("query_rays: upload_scene first")
        cfg = self._cfg(self.camera if self.camera is not None else np.zeros((4, 3), F))
        return pyoracle.Oracle(cfg).intersect(np.asarray(rays, F).reshape(-1, 7), 1 if any_hit else 0, 0)

    # ---- the previews --------------------------------------------------------------------------
    def denoise(self, levels=None, sigma_color=None, sigma_normal=None, sigma_position=None):
        self._need_scene_frame("denoise")
        self._need_guides("denoise")
        g = self.guides
        self.denoised = AT.atrous_ref(self.accum, g["position"], g["normal"], g["albedo"], self.M,
                                      **_given(DENOISE_DEFAULTS, (levels, sigma_color, sigma_normal, sigma_position)))

    def denoise_variance(self, levels=None, sigma_variance=None, sigma_normal=None, sigma_position=None):
        self._need_scene_frame("denoise_variance")
        if not self.moments_ever or self.moments is None:
            refuse("denoise_variance: the sample moments were never enabled")
        if not self.cover:
            refuse("denoise_variance: the moments do not cover the accumulation")
        self._need_guides("denoise_variance")
        g = self.guides
        self.denoised = AV.atrous_var_ref(self.accum, g["position"], g["normal"], g["albedo"], self.M, self.moments,
                                          **_given(DENOISE_VARIANCE_DEFAULTS, (levels, sigma_variance, sigma_normal, sigma_position)))

    def _sized(self, img, who, what):
        if img is None:
            refuse(f"{who}: {what} first")
        if img.shape[:2] != (self.height, self.width):
            refuse(f"{who}: the image has another size than the frame")
        return img

    def read_denoised(self):
        return self._sized(self.denoised, "read_denoised", "denoise").copy()

    def _source(self, who, source):
        if self.accum is None:
            refuse(f"{who}: set_frame first")
        if source == "accum":
            return self.accum
        assert source == "denoised"
        return self._sized(self.denoised, who, "denoise")

    def display(self, source="accum", tone="clamp", transfer="linear", exposure: float = 1.0, white: float = 4.0,
                bottom_first: bool = False, src_ptr=None):
        self.disp = D.display_ref(self._source("display", source), tone, transfer, exposure, white, bottom_first)

    def read_display(self):
        return self._sized(self.disp, "read_display", "display").copy()

    def luma_histogram(self, source="accum", band: int = 1, n_shards: int = 1, shard: int = 0, src_ptr=None) -> dict:
        return D.histogram_ref(self._source("luma_histogram", source), shard_rows(self.height, band, n_shards, shard))

    # ---- reprojection --------------------------------------------------------------------------
    def reproject(self, from_camera, normal_min=None, position_tolerance=None, max_history=None) -> dict:
        self._need_scene_frame("reproject")
        self._need_moments("reproject")
        if self.v1:
            refuse("reproject: PNRT_KERNEL_V1 keeps no sample moments")
        cam_a = np.asarray(from_camera, F).reshape(4, 3)
        a, b = self.first_hits(cam_a), self.first_hits()
        self.accum, self.moments, stats = RP.reproject(self.accum, self.moments, a["position"], a["normal"], b["position"],
                                                       b["normal"], cam_a, self.width, self.height,
                                                       _given(REPROJECT_DEFAULTS, (normal_min, position_tolerance, max_history)))
        self.guides = dict(b, **{"for": self._fits()})       # valid for the current camera on return
        return stats
