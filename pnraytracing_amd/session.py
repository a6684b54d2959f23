"""Headless replacement of main.cpp's interactive render loop (main.cpp:573-630).

``CameraController`` is ``Camera`` (camera.hpp:4-77) with the controls the
mouse callbacks call (main.cpp:96-142), glm-exact in libpnrt_host.so.
``InteractiveSession.frame(redraw)`` is one loop iteration: when the scene or
camera is being changed (the GUI combo, a pressed mouse button or a scroll
event, main.cpp:592) the frame is rendered with MAX_BOUNCE_DEPTH 1 and
frameCount 0 -- the progressive mean then overwrites the image (a = 1/(0+1)) --
and the counter is not advanced (main.cpp:628); otherwise MAX_BOUNCE_DEPTH 4
and frameCount, then ++frameCount.  All rendering goes through libpnrt.so.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .host import camera_pixel_ray, camera_sequence, model_matrix, model_records
from .tracer import PathTracer, PnrtError, decode_hits, exposure_from_histogram

PINHOLE = ("pinhole", 180.0, 0)                      # set_camera_model never called: (model, fov_deg, per_pixel)
EVERY_PIXEL = (0.0, 0xFFFFFFFF)                      # the (threshold, min_frames) that make every pixel active
E_STATE = -3                                         # PNRT_E_STATE


class CameraState(ctypes.Structure):
    _fields_ = [("eye", ctypes.c_float * 3), ("center", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
                ("fov_deg", ctypes.c_float), ("aspect", ctypes.c_float),
                ("u", ctypes.c_float * 3), ("v", ctypes.c_float * 3), ("w", ctypes.c_float * 3),
                ("distance", ctypes.c_float),
                ("lower_left", ctypes.c_float * 3), ("horizontal", ctypes.c_float * 3),
                ("vertical", ctypes.c_float * 3)]


def _lib():
    lib = N.host_lib()
    if not getattr(lib, "_pnrt_cam_typed", False):
        P = ctypes.POINTER(CameraState)
        for name, args in (("pnrt_camera_state_init", [P, N.F, N.F, N.F, ctypes.c_float, ctypes.c_float]),
                           ("pnrt_camera_rotate", [P, ctypes.c_float, ctypes.c_float]),
                           ("pnrt_camera_translate", [P, ctypes.c_float, ctypes.c_float]),
                           ("pnrt_camera_zoom", [P, ctypes.c_float])):
            fn = getattr(lib, name)
            fn.restype = ctypes.c_int
            fn.argtypes = args
        lib._pnrt_cam_typed = True
    return lib


class CameraController:
    """``Camera`` + its interactive controls (camera.hpp:33-65)."""

    def __init__(self, eye, center, up, fov_deg: float, aspect: float):
        self.state = CameraState()
        a = [np.ascontiguousarray(v, np.float32) for v in (eye, center, up)]
        rc = _lib().pnrt_camera_state_init(ctypes.byref(self.state), *(N.fptr(x) for x in a),
                                           ctypes.c_float(fov_deg), ctypes.c_float(aspect))
        if rc < 0:
            raise ValueError("camera_state_init failed")

    def rotate(self, dx: float, dy: float) -> bool:        # left-button drag (main.cpp:127-129)
        return _lib().pnrt_camera_rotate(ctypes.byref(self.state), dx, dy) == 1

    def translate(self, dx: float, dy: float) -> bool:     # right-button drag: UpdateTranslateUV(-dx, dy)
        return _lib().pnrt_camera_translate(ctypes.byref(self.state), -dx, dy) == 1

    def zoom(self, yoffset: float) -> bool:                # scroll (main.cpp:139-142)
        return _lib().pnrt_camera_zoom(ctypes.byref(self.state), yoffset) == 1

    def uniforms(self) -> np.ndarray:
        """(4, 3): camera.eye, lowerLeftCorner, horizontal, vertical (main.cpp:606-610)."""
        s = self.state
        return np.array([list(s.eye), list(s.lower_left), list(s.horizontal), list(s.vertical)], np.float32)

    def record(self) -> np.ndarray:
        """All 31 floats of the state (eye center up fov aspect u v w distance llc hor ver)."""
        s = self.state
        return np.array([*s.eye, *s.center, *s.up, s.fov_deg, s.aspect, *s.u, *s.v, *s.w, s.distance,
                         *s.lower_left, *s.horizontal, *s.vertical], np.float32)


class InteractiveSession:
    """main.cpp:573-630 without the window: one ``frame()`` per loop iteration."""

    # A session's private state as it starts (here, not in __init__: a session made with __new__ has it too)
    _rendered_view = None                            # the view of the last call that rendered: (uniforms, model, fov_deg)
    _counts_differ = False                           # reproject_view left pixels with different frame counts
    _lens = None                                     # set_lens: (aa_width, lens_radius, focus_distance)
    _model = None                                    # set_camera_model: (model, fov_deg, per_pixel)
    _rays = None                                     # the ray buffer of the last frame (alive while its call runs)
    _guide_rays = None                               # the ray buffer of the guide images, and what it was made for:
    _guide_view = None                               # (camera uniforms, model, fov_deg, size); None: camera-keyed guides

    def __init__(self, tracer, width: int, height: int, camera: CameraController, max_bounce_depth: int = 4):
        self.pt = tracer
        self.width, self.height = width, height
        self.camera = camera
        self.max_bounce_depth = max_bounce_depth
        self.frame_count = 0

    def set_lens(self, aa_width: float = 1.0, lens_radius: float = 0.0, focus_distance: float | None = None):
        """Anti-aliasing and depth of field for the still frames: from now on ``frame()``
        and ``frame_counted()`` render frame ``frame_count`` with that frame's camera of
        ``host.camera_sequence`` (a box pixel filter ``aa_width`` pixels wide, a thin lens of
        ``lens_radius`` world units focused ``focus_distance`` from the eye -- ``focus_on``
        sets it from a pixel) through ``PathTracer.render_cameras``.  A redraw stays the
        reference's un-jittered depth-1 frame 0.  Never called, nothing changes."""
        if lens_radius > 0 and focus_distance is None:
            focus_distance = self._lens[2] if self._lens else None
            if focus_distance is None:
                raise ValueError("set_lens: a lens needs a focus_distance (or focus_on(px, py) first)")
        if lens_radius > 0 and self._model is not None and self._model[0] != "pinhole":
            raise ValueError(f"set_lens: a lens needs the pinhole model (set_camera_model: {self._model[0]!r})")
        self._lens = (float(aa_width), float(lens_radius), None if focus_distance is None else float(focus_distance))

    def set_camera_model(self, model, fov_deg: float = 180.0, per_pixel: bool = False):
        """Another camera model for the still frames: from now on ``frame()`` and
        ``frame_counted()`` make the rays of frame ``frame_count`` on the device
        (``PathTracer.make_rays``: ``"pinhole"``, ``"ortho"``, ``"equirect"`` or ``"fisheye"``
        over the controller's uniforms, with ``set_lens``'s pixel filter and -- pinhole only --
        lens, sampled per frame or, with ``per_pixel``, per pixel) and render them with
        ``PathTracer.render_rays``; ``preview()`` takes its guide images from the model's
        un-jittered rays (the pinhole model keeps ``render_guides``), made again whenever the
        camera, the model or ``fov_deg`` has changed since; ``reproject()`` is refused under
        another model than pinhole (``reproject_view()`` works under every model and across a
        change of model).  A redraw stays the reference's depth-1 frame 0 of the pinhole camera when the
        model is pinhole, and is the same frame through the ray path otherwise.  Never
        called, nothing changes."""
        name = N.CAM_MODELS[PathTracer._enum("camera model", N.CAM_MODELS, model)]
        if name != "pinhole" and self._lens is not None and self._lens[1] > 0:
            raise ValueError("set_camera_model: a lens (set_lens) needs the pinhole model")
        self._model = (name, float(fov_deg), int(bool(per_pixel)))

    def _view(self, cam):
        """(uniforms, model, fov_deg): the view the still frames render with camera uniforms ``cam``."""
        name, fov, _ = self._model or PINHOLE
        return (cam, name, fov)

    def _set_frame(self, depth: int):
        """The controller's uniforms, set as the tracer's camera at that bounce depth."""
        cam = self.camera.uniforms()
        self.pt.set_frame(self.width, self.height, cam, depth)
        return cam

    def _remember(self, cam):
        """A call rendered (or reprojected into) the view of ``cam``: what the next reprojection starts from."""
        self._rendered_view = self._view(cam)

    def _model_rays(self, cam, n: int, jitter: bool = True):
        """(rays, frame_stride) of frames frame_count .. + n - 1 for the camera model (none set: the pinhole model's)."""
        name, fov, per_pixel = self._model or PINHOLE
        aa, radius, focus = self._lens if (self._lens is not None and jitter) else (0.0, 0.0, None)
        lens = radius > 0 and focus is not None
        still = not (aa > 0 or lens)                 # no sample: one set serves every frame
        self._rays = self.pt.make_rays(name, cam, self.frame_count, 1 if still else n, fov_deg=fov, aa_width=aa,
                                       lens_radius=radius if lens else 0.0, focus_distance=focus if lens else 0.0,
                                       per_pixel=per_pixel)
        return self._rays, 0 if (still or n == 1) else self.width * self.height

    def focus_on(self, px: int, py: int) -> bool:
        """Focus on what is under pixel (px, py): ``focus_distance`` becomes the distance of
        ``pick(px, py)``'s hit along the view axis (the plane in focus is parallel to the
        image plane).  Nothing changes on a miss.  Returns whether the pixel hit."""
        rec = self.pick(px, py)
        if not rec["hit"]:
            return False
        s = self.camera.state
        eye = np.array(list(s.eye), np.float64)
        axis = -np.array(list(s.w), np.float64)      # the view direction (camera.hpp: w = normalize(eye - center))
        d = float(np.dot(np.asarray(rec["position"], np.float64) - eye, axis))
        if not d > 0:
            return False
        aa, radius = (self._lens[0], self._lens[1]) if self._lens else (1.0, 0.0)
        self._lens = (aa, radius, d)
        return True

    def _lens_cameras(self, cam, n: int) -> np.ndarray:
        aa, radius, focus = self._lens
        return camera_sequence(cam, self.width, self.height, self.frame_count, n, aa, radius,
                               focus if (radius > 0 and focus is not None) else 0.0)

    def _source(self, cam, n: int, redraw: bool = False, by_count: bool = False) -> tuple:
        """Where the primary rays of frames frame_count .. + n - 1 come from: ("plain",) -- the tracer's own pinhole
        rays of ``cam`` --, ("cameras", sequence) or ("rays", buffer, frame_stride), the buffer kept alive in ``_rays``.

        * A redraw is un-jittered: plain under no model or the pinhole model, the model's centre rays otherwise.
        * A camera model means ray sets.
        * A lens alone means a camera sequence for frames blended by frame number, and the pinhole model's ray sets
          for frames blended by each pixel's own count (``by_count``): there is no adaptive call over cameras.
        * Neither: plain."""
        if redraw:
            return ("plain",) if (self._model or PINHOLE)[0] == "pinhole" else ("rays", *self._model_rays(cam, n, jitter=False))
        if self._model is not None or (by_count and self._lens is not None):
            return ("rays", *self._model_rays(cam, n))
        return ("cameras", self._lens_cameras(cam, n)) if self._lens is not None else ("plain",)

    def _issue(self, source: tuple, n: int, by_count: tuple | None = None, *selector):
        """Frames frame_count .. + n - 1 from ``source`` over the rows of a shard ``selector`` (band, n_shards, shard;
        left out: the whole image), blended by frame number -- or, with ``by_count`` = (threshold, min_frames), by each
        pixel's own count, for the pixels still active: the adaptive call's statistics."""
        kind, *what = source
        if by_count is None:
            if kind == "rays":
                return self.pt.render_rays(self.frame_count, n, *what, *selector)
            if kind == "cameras":
                return self.pt.render_cameras(self.frame_count, *what, *selector)
            return self.pt.render(self.frame_count, n, *selector)   # main.cpp:612-613
        if kind == "rays":
            return self.pt.render_rays_adaptive(self.frame_count, n, *what, *by_count, *selector)
        assert kind == "plain", "no adaptive call over cameras"
        return self.pt.render_adaptive(self.frame_count, n, *by_count, *selector)

    def frame(self, redraw: bool = False, band: int = 1, n_shards: int = 1, shard: int = 0):
        if redraw:                                   # main.cpp:592-596
            depth = 1
            self.frame_count = 0
            self._counts_differ = False              # the image starts again: every pixel at one count
        else:                                        # main.cpp:597-601
            depth = self.max_bounce_depth
        cam = self._set_frame(depth)
        self._issue(self._source(cam, 1, redraw), 1, None, band, n_shards, shard)
        self._remember(cam)
        if not redraw:                               # main.cpp:628
            self.frame_count += 1
        return depth, self.frame_count

    def render_until(self, threshold: float, fraction: float = 0.95, max_frames: int = 1024, check_every: int = 8):
        """``frame()`` after ``frame()`` until the image has converged: every pixel measured
        (two frames or more) and at most ``1 - fraction`` of them with a relative standard
        error above ``threshold`` -- asked of the library every ``check_every`` frames
        (``PathTracer.convergence`` waits for the frames in flight) -- or until this call
        has rendered ``max_frames`` frames.  Enables the sample moments itself.  Returns
        (the last statistics -- None when ``max_frames`` left no check --, frames rendered)."""
        if check_every < 1:
            raise ValueError("render_until: check_every must be >= 1")
        self.pt.enable_moments(True)
        stats, done = None, 0
        while done < max_frames:
            self.frame()
            done += 1
            if done % check_every == 0 or done == max_frames:
                stats = self.pt.convergence(threshold)
                if stats["n_measured"] == stats["n_pixels"] and stats["n_above"] <= (1.0 - fraction) * stats["n_measured"]:
                    break
        return stats, done

    def render_adaptive_until(self, threshold: float, max_frames: int = 1024, frames_per_call: int = 8, min_frames: int = 8):
        """Adaptive calls of ``frames_per_call`` frames (the last one shorter), continuing
        ``frame_count``, until a call finds no pixel active -- every pixel of the image has
        ``max(min_frames, 2)`` frames and a relative standard error of at most ``threshold``
        (``PathTracer.render_adaptive``) -- or until this call has issued ``max_frames``
        frames.  Converged pixels receive no more frames.  With ``set_camera_model`` or
        ``set_lens`` in force every call makes its frames' rays (the lens alone: the
        ``"pinhole"`` model's, the frames ``set_camera_model("pinhole")`` renders) and goes
        through ``PathTracer.render_rays_adaptive``.  Enables the sample moments itself.
        Returns (the last call's statistics -- None when ``max_frames`` left no call --,
        frames issued)."""
        if frames_per_call < 1:
            raise ValueError("render_adaptive_until: frames_per_call must be >= 1")
        self.pt.enable_moments(True)
        stats, done = None, 0
        while done < max_frames:
            n = min(frames_per_call, max_frames - done)
            cam = self._set_frame(self.max_bounce_depth)
            stats = self._issue(self._source(cam, n, by_count=True), n, (threshold, min_frames))
            if stats["n_active_pixels"] == 0:        # nothing was rendered: the frames were not issued
                break
            self._remember(cam)
            self.frame_count += n
            done += n
        return stats, done

    def reproject(self, **params) -> dict:
        """After ``self.camera`` changed, in place of ``frame(redraw=True)``: carry the
        accumulation and the sample moments over into the new view
        (``PathTracer.reproject``, whose ``params`` these are) from the camera of the last
        call that rendered.  Sets the frame to the new camera at the full bounce depth,
        keeps ``frame_count`` and remembers the new camera, so moves chain.  Continue
        with ``frame_counted()``.  Needs the sample moments enabled since the
        accumulation was last reset (``frame_counted``, ``render_until`` and
        ``render_adaptive_until`` enable them).  Returns the call's statistics."""
        if self._model is not None and self._model[0] != "pinhole":
            raise ValueError(f"reproject: the {self._model[0]!r} camera model has no reprojection (pinhole views only): "
                             "reproject_view() takes every model")
        if self.frame_count == 0 or self._rendered_view is None:
            raise ValueError("reproject: nothing was rendered yet (frame_count == 0)")
        cam = self._set_frame(self.max_bounce_depth)
        stats = self.pt.reproject(self._rendered_view[0], **params)
        self._guide_view = None                      # it left camera-keyed guides of the new view
        self._remember(cam)
        return stats

    def reproject_view(self, **params) -> dict:
        """``reproject()`` under any camera model (``set_camera_model``) and across a change
        of model or ``fov_deg`` -- a switch from pinhole to fisheye keeps the image: carry
        the accumulation and the sample moments over from the view of the last call that
        rendered (its uniforms, model and ``fov_deg``) into the view the still frames render
        now (``PathTracer.reproject_view``, whose ``params`` these are).  Sets the frame at
        the full bounce depth, keeps ``frame_count`` and remembers the new view, so moves
        chain.  Two pinhole views are ``reproject()``.  The call leaves the guide images of
        the new view: ``preview()`` does not render them again.  Continue with
        ``frame_counted()``.  Returns the call's statistics."""
        if self.frame_count == 0 or self._rendered_view is None:
            raise ValueError("reproject_view: nothing was rendered yet (frame_count == 0)")
        (cam_a, model_a, fov_a), (model_b, fov_b, _) = self._rendered_view, self._model or PINHOLE
        if model_a == "pinhole" and model_b == "pinhole":
            return self.reproject(**params)
        cam = self._set_frame(self.max_bounce_depth)
        stats = self.pt.reproject_view((model_a, cam_a, fov_a), (model_b, cam, fov_b), **params)
        self._counts_differ = True                   # frame_counted() continues at every pixel's own count
        self._guide_rays = None                      # (the library made the new view's guides from rays of its own)
        if model_b != "pinhole":
            self._guide_view = self._guide_want()
        else:
            # Ray-made guides are accepted for any camera, and under the pinhole model the session relies on the
            # library's own staleness check, which they would defeat: camera-keyed ones instead
            self.pt.render_guides()
            self._guide_view = None
        self._remember(cam)
        return stats

    def frame_counted(self, n: int = 1) -> dict:
        """``n`` frames for every pixel, each blended at the weight of the pixel's own frame
        count (one ``PathTracer.render_adaptive`` call with every pixel active): what
        continues a reprojected image, whose pixels hold different counts.  Enables the
        sample moments itself and advances ``frame_count`` by ``n``.  With ``set_lens`` the
        frames are ``render_cameras``'s instead: frame ``frame_count + k`` with its camera of
        the sequence, blended at the weight of that frame number (the statistics then
        report every pixel active and the call's batch plan).  The per-pixel-count form
        of those frames is ``PathTracer.render_rays_adaptive`` with ``threshold 0,
        min_frames 0xFFFFFFFF``: after ``reproject_view()`` -- until the next redraw -- the
        frames of a camera model or a lens go through it, so that a disoccluded pixel
        takes the next frame whole."""
        self.pt.enable_moments(True)
        cam = self._set_frame(self.max_bounce_depth)
        # after reproject_view the pixels hold different counts: the frames' rays at every pixel's own weight
        source = self._source(cam, n, by_count=self._counts_differ)
        if self._counts_differ or source == ("plain",):
            stats = self._issue(source, n, EVERY_PIXEL)
        else:                                        # by frame number: the statistics of a call with every pixel active
            self._issue(source, n)
            plan = self.pt.cameras_batch_plan(n)
            npix, ntiles = self.width * self.height, ((self.width + 7) // 8) * ((self.height + 7) // 8)
            stats = {"n_pixels": npix, "n_active_pixels": npix, "n_tiles": ntiles, "n_active_tiles": ntiles,
                     "frames_per_batch": plan["frames_per_batch"], "n_batches": plan["n_batches"]}
        self._remember(cam)
        self.frame_count += n
        return stats

    def edit_vertices(self, first: int, vertices, lights=None, lights_sum_area=None):
        """A model was moved, scaled or deformed: overwrite its vertex records and refit the
        BVH in place (``PathTracer.update_vertices``, whose arguments these are), then the
        depth-1 redraw frame of main.cpp:592-596, as any other edit of the scene is shown.
        Returns ``frame(True)``'s result."""
        self.pt.update_vertices(first, vertices, lights=lights, lights_sum_area=lights_sum_area)
        return self.frame(True)

    def define_model(self, first: int, mesh) -> int:
        """Tell the device which model vertices ``first`` .. hold: ``mesh``'s model-space records
        (``host.model_records``) are kept there for ``move_model``.  Returns the model's id
        (``PathTracer.define_model``)."""
        return self.pt.define_model(first, model_records(mesh))

    def move_model(self, model_id: int, ops, relight: bool = False):
        """The gizmo drag: place the model under ``host.model_matrix(ops)`` on the device
        (``PathTracer.place_models`` -- the matrix goes up, not the vertices), then the depth-1
        redraw frame, as ``edit_vertices``.  ``relight`` when the model is a light whose area
        changes.  Returns ``frame(True)``'s result."""
        self.pt.place_models([(model_id, model_matrix(ops))], relight=relight)
        return self.frame(True)

    def pick(self, px: int, py: int) -> dict:
        """What is under pixel (px, py) -- row 0 = bottom, as ``PathTracer.read_aov`` --: the
        decoded record (``tracer.decode_hits``, one ray: scalars and vectors) of the closest
        hit of that pixel's camera ray, the ray ``frame()`` traces for it.  The selection
        the reference's material panel makes from a combo box of names
        (ImGuiLayer.hpp:37-49): ``pick(x, y)["material_id"]`` names the record
        ``PathTracer.update_materials`` edits.  Changes no image."""
        if not (0 <= px < self.width and 0 <= py < self.height):
            raise ValueError(f"pick: pixel ({px}, {py}) is outside the {self.width}x{self.height} frame")
        ray = camera_pixel_ray(self.camera.uniforms(), px, py, self.width, self.height)
        return {k: v[0] for k, v in decode_hits(self.pt.query_rays(ray)).items()}

    def _guide_want(self):
        """What ray-made guide images must have been made for to show the view the still frames render; None
        when that view is the camera's own (no model, or pinhole): camera-keyed guides, whose staleness the
        library judges itself."""
        if self._model is None or self._model[0] == "pinhole":
            return None
        name, fov, _ = self._model
        return (self.camera.uniforms().tobytes(), name, fov, self.width, self.height)

    def _render_guides(self):
        """The guide images of the view the still frames render: the camera's, or the camera model's centre rays."""
        want = self._guide_want()
        if want is None:
            self._guide_rays = None
            self.pt.render_guides()
        else:
            _, name, fov, _, _ = want
            self._guide_rays = self.pt.make_rays(name, self.camera.uniforms(), 0, 1, fov_deg=fov)
            self.pt.render_guides_rays(self._guide_rays)
        self._guide_view = want

    def _filtered(self, run, curable):
        """The guide images of this view, then the filter ``run``; on the library's stale-guides refusal -- a
        PNRT_E_STATE whose text ``curable`` accepts -- the guides are rendered and the filter runs once more.
        Guide images made from rays carry no camera, so the library cannot tell that they belong to another view:
        the session remembers what it made them for and renders them again when that has changed."""
        if self._guide_want() != self._guide_view:
            self._render_guides()
        try:
            run()
        except PnrtError as e:
            if getattr(e, "code", 0) != E_STATE or not curable(str(e)):
                raise
            self._render_guides()
            run()

    def preview(self, **params):
        """The denoised preview of the accumulation image as it stands (after ``frame()``,
        before the display: main.cpp:613 / :618-628).  The guide images are rendered only
        when the camera or the scene changed since the last call -- the library says so
        (PNRT_E_STATE from pnrt_denoise); under another camera model than pinhole the guides
        are made from rays and carry no camera, so there the session itself compares the
        view they were made for -- then the image is filtered.  ``params`` are
        ``PathTracer.denoise``'s; read the result with ``PathTracer.read_denoised()``."""
        self._filtered(lambda: self.pt.denoise(**params), lambda text: True)     # its PNRT_E_STATE: no guides yet, or stale ones

    def show(self, denoised: bool = False, auto_exposure: bool = False, **display_params) -> np.ndarray:
        """The frame as a screen takes it (main.cpp:618-628's display, converted on the
        device): the accumulation image -- or, with ``denoised``, the preview that
        ``preview()`` / ``preview_variance()`` wrote -- through ``PathTracer.display``, whose
        ``display_params`` these are (tone, transfer, exposure, white, bottom_first), read
        back as (H, W, 4) uint8.  With ``auto_exposure`` the luminance histogram of the
        shown image is taken first and the exposure derived from it
        (``tracer.exposure_from_histogram`` at its defaults), in place of any ``exposure``
        given."""
        source = "denoised" if denoised else "accum"
        if auto_exposure:
            display_params["exposure"] = exposure_from_histogram(self.pt.luma_histogram(source))
        self.pt.display(source=source, **display_params)
        return self.pt.read_display()

    def preview_variance(self, **params):
        """``preview()`` with the variance-guided filter (``PathTracer.denoise_variance``,
        whose ``params`` these are).  The library checks the sample moments before the
        guide images, so a PNRT_E_STATE that names ``render_guides`` is about the guides
        alone: only then are they rendered and the filter tried again.  A PNRT_E_STATE
        about the moments (never enabled, or not covering the accumulation) is raised
        with its message."""
        self._filtered(lambda: self.pt.denoise_variance(**params), lambda text: "render_guides" in text)
