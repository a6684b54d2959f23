"""pnrt_reproject_view exists in include/pnrt.h, in the ctypes layer, in the built library and in
the Python classes; InteractiveSession.reproject_view against a fake tracer; the committed
resource-usage listings (no GPU needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from pnraytracing_amd import _native as N
from pnraytracing_amd import session, tracer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "pnrt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_header_declares_the_entry_point():
    assert re.search(r"int\s+pnrt_reproject_view\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*const\s+pnrt_ray_camera\s*\*\s*from\s*,"
                     r"\s*const\s+pnrt_ray_camera\s*\*\s*to\s*,\s*const\s+pnrt_reproject_params\s*\*\s*\w*\s*,"
                     r"\s*pnrt_reproject_stats\s*\*\s*\w*\s*\)", CODE)
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)      # no new profile class
    assert CODE.index("pnrt_ray_camera;") < CODE.index("pnrt_reproject_view")
    doc = HEADER[HEADER.index("pnrt_reproject with both views given as camera models"):HEADER.index("int pnrt_reproject_view")]
    for words in ("centre rays", "always rendered", "wraps in x", "primary miss", "ray buffers", "sample-aware", "multi-GPU",
                  "lending", "which of the two"):
        assert words in doc, words
    # the ray call's comment: reprojection of the four models' views is no longer out of scope, arbitrary ray sets are
    out = HEADER[HEADER.index("Out of scope: reprojection across"):HEADER.index("} pnrt_ray;")]
    assert "arbitrary" in out and "pnrt_reproject_view" in out and "adaptive" not in out


def test_library_exports_the_symbol_typed():
    fn = N.device_lib().pnrt_reproject_view          # AttributeError: the built library lacks the symbol
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.POINTER(N.RayCamera), ctypes.POINTER(N.RayCamera),
                                 ctypes.POINTER(N.ReprojectParams), ctypes.POINTER(N.ReprojectStats)]
    cam = N.RayCamera()
    assert fn(None, ctypes.byref(cam), ctypes.byref(cam), None, None) == -1      # PNRT_E_ARG: a NULL context


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_reproject_view.h" in build.DEVICE_DEPS and "pt_reproject.h" in build.DEVICE_DEPS
    assert len(set(build.DEVICE_DEPS)) == len(build.DEVICE_DEPS)
    assert all(os.path.exists(os.path.join(build.CSRC, d)) for d in build.DEVICE_DEPS)
    src = open(os.path.join(build.CSRC, "pnrt_device.hip")).read()
    assert '#include "pt_reproject_view.h"' in src


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.reproject_view)
    assert list(sig.parameters)[1:] == ["from_view", "to_view", "normal_min", "position_tolerance", "max_history"]
    assert all(sig.parameters[k].default is inspect.Parameter.empty for k in ("from_view", "to_view"))
    assert [sig.parameters[k].default for k in ("normal_min", "position_tolerance", "max_history")] == [None, None, None]
    sig = inspect.signature(session.InteractiveSession.reproject_view)
    assert [p.kind for p in list(sig.parameters.values())[1:]] == [inspect.Parameter.VAR_KEYWORD]
    # the existing calls keep their signatures
    sig = inspect.signature(tracer.PathTracer.reproject)
    assert list(sig.parameters)[1:] == ["from_camera", "normal_min", "position_tolerance", "max_history"]
    sig = inspect.signature(session.InteractiveSession.reproject)
    assert [p.kind for p in list(sig.parameters.values())[1:]] == [inspect.Parameter.VAR_KEYWORD]
    assert "reproject_view" in session.InteractiveSession.set_camera_model.__doc__


def test_tracer_passes_views_and_parameters():
    """PathTracer.reproject_view over a fake library: tuples become pnrt_ray_camera records, RayCamera objects pass
    as they are, parameters left out are the library's defaults (a NULL params when none is given)."""
    calls = []

    class Lib:
        @staticmethod
        def pnrt_reproject_view(ctx, a, b, params, st):
            calls.append((a._obj, b._obj, None if params is None else params._obj))
            st._obj.n_pixels, st._obj.n_reprojected = 64, 9
            return 0

    pt = tracer.PathTracer.__new__(tracer.PathTracer)
    pt._lib, pt._ctx = Lib, None
    pt._ck = lambda rc, what: None
    cam = np.arange(12, dtype=np.float32).reshape(4, 3)
    st = pt.reproject_view(("fisheye", cam, 200.0), tracer.PathTracer.ray_camera("equirect", cam + 1))
    assert st == {"n_pixels": 64, "n_reprojected": 9, "n_disoccluded": 0, "n_missed": 0, "sum_frames": 0, "max_frames": 0}
    a, b, params = calls[-1]
    assert (a.model, a.fov_deg, list(a.camera.eye), list(a.camera.vertical)) == (3, 200.0, [0, 1, 2], [9, 10, 11])
    assert (b.model, list(b.camera.eye)) == (2, [1, 2, 3]) and params is None
    pt.reproject_view(("ortho", cam, 180.0), ("pinhole", cam, 180.0), max_history=8)
    a, b, params = calls[-1]
    assert (a.model, b.model) == (1, 0)
    assert (round(params.normal_min, 6), round(params.position_tolerance, 6), params.max_history, params.reserved) == (0.9, 0.02, 8, 0)
    with pytest.raises(ValueError):
        pt.reproject_view(("ortho", cam, 180.0), ("pinhole", cam, 180.0), max_history=-1)


# ---- InteractiveSession.reproject_view against a fake tracer ---------------------------------------------------
class _FakeTracer:
    def __init__(self):
        self.log = []
        self.guides = False

    def enable_moments(self, on=True):
        self.log.append(("enable_moments", bool(on)))

    def set_frame(self, w, h, cam, depth=4):
        self.log.append(("set_frame", w, h, depth))

    def render(self, first, n, band=1, n_shards=1, shard=0):
        self.log.append(("render", first, n))

    def render_adaptive(self, first, n, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        self.log.append(("render_adaptive", first, n))
        return {"n_pixels": 64, "n_active_pixels": 64, "n_tiles": 1, "n_active_tiles": 1, "frames_per_batch": n, "n_batches": 1}

    def cameras_batch_plan(self, n, band=1, n_shards=1, shard=0):
        return {"frames_per_batch": n, "n_batches": 1, "batch_bytes": 1}

    def make_rays(self, model, camera, first_frame=0, n_sets=1, frame_stride=None, out=None, **params):
        self.log.append(("make_rays", model, first_frame, n_sets, dict(params)))
        return ("rays", len(self.log))

    def render_rays(self, first, n, rays, frame_stride=0, band=1, n_shards=1, shard=0):
        self.log.append(("render_rays", first, n))

    def render_rays_adaptive(self, first, n, rays, frame_stride, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        self.log.append(("render_rays_adaptive", first, n, threshold, min_frames))
        return {"n_pixels": 64, "n_active_pixels": 64, "n_tiles": 1, "n_active_tiles": 1, "frames_per_batch": n, "n_batches": 1}

    def render_guides(self):
        self.log.append(("render_guides",))
        self.guides = True

    def render_guides_rays(self, rays):
        self.log.append(("render_guides_rays", rays))
        self.guides = True

    def denoise(self, **params):
        assert self.guides
        self.log.append(("denoise",))

    def reproject(self, from_camera, normal_min=None, position_tolerance=None, max_history=None):
        self.log.append(("reproject", np.asarray(from_camera, np.float32).copy(), max_history))
        self.guides = True
        return {"n_pixels": 64, "n_reprojected": 9}

    def reproject_view(self, from_view, to_view, normal_min=None, position_tolerance=None, max_history=None):
        (ma, ca, fa), (mb, cb, fb) = from_view, to_view
        self.log.append(("reproject_view", (ma, np.asarray(ca, np.float32).copy(), fa), (mb, np.asarray(cb, np.float32).copy(), fb),
                         max_history))
        self.guides = True
        return {"n_pixels": 64, "n_reprojected": 7}


def _session(pt):
    cam = session.CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, 1.0)
    return session.InteractiveSession(pt, 8, 8, cam, max_bounce_depth=3), cam


def test_session_reproject_view_needs_rendered_frames():
    pt = _FakeTracer()
    s, _ = _session(pt)
    s.set_camera_model("fisheye")
    with pytest.raises(ValueError):
        s.reproject_view()
    s.frame(redraw=True)                             # a redraw leaves frame_count at 0
    with pytest.raises(ValueError):
        s.reproject_view()
    assert not any(c[0].startswith("reproject") for c in pt.log)


def test_session_reproject_view_under_fisheye_chains():
    pt = _FakeTracer()
    s, cam = _session(pt)
    s.set_camera_model("fisheye", fov_deg=200.0)
    s.frame_counted(2)
    u0 = cam.uniforms()
    cam.rotate(5.0, 2.0)
    u1 = cam.uniforms()
    st = s.reproject_view(max_history=8)
    assert st["n_reprojected"] == 7 and s.frame_count == 2
    assert pt.log[-2] == ("set_frame", 8, 8, 3)      # the full depth
    name, a, b, cap = pt.log[-1]
    assert name == "reproject_view" and cap == 8
    assert (a[0], a[2], b[0], b[2]) == ("fisheye", 200.0, "fisheye", 200.0)
    assert np.array_equal(a[1], u0) and np.array_equal(b[1], u1) and not np.array_equal(u0, u1)
    # the call left the new view's guides: the preview makes none
    n = len(pt.log)
    s.preview()
    assert [c[0] for c in pt.log[n:]] == ["denoise"]
    cam.rotate(3.0, 0.0)                             # a second move, no frame in between: from the first move's view
    s.reproject_view()
    assert np.array_equal(pt.log[-1][1][1], u1) and np.array_equal(pt.log[-1][2][1], cam.uniforms())
    # the pixels hold different counts now: the frames that follow are blended at every pixel's own
    assert s.frame_counted()["n_active_pixels"] == 64
    assert [c[0] for c in pt.log[-4:]] == ["enable_moments", "set_frame", "make_rays", "render_rays_adaptive"]
    assert pt.log[-1] == ("render_rays_adaptive", 2, 1, 0.0, 0xFFFFFFFF) and s.frame_count == 3
    cam.rotate(1.0, 0.0)                             # the camera moved since: the preview's guides are stale again
    s.preview()
    assert [c[0] for c in pt.log[-3:]] == ["make_rays", "render_guides_rays", "denoise"]
    with pytest.raises(ValueError):
        s.reproject()                                # unchanged: pinhole views only
    assert "reproject_view" in str(pytest.raises(ValueError, s.reproject).value)
    s.frame(redraw=True)                             # the image starts again: frame-number weights as before
    s.frame_counted(2)
    assert pt.log[-1] == ("render_rays", 0, 2)


def test_session_model_switch_keeps_the_image():
    pt = _FakeTracer()
    s, cam = _session(pt)
    s.frame_counted(2)                               # no model: the pinhole camera's frames
    u = cam.uniforms()
    s.set_camera_model("fisheye", fov_deg=220.0)
    s.reproject_view()
    name, a, b, _ = pt.log[-1]
    assert name == "reproject_view" and (a[0], b[0], b[2]) == ("pinhole", "fisheye", 220.0)
    assert np.array_equal(a[1], u) and np.array_equal(b[1], u)
    assert "render_guides" not in [c[0] for c in pt.log]
    s.set_camera_model("fisheye", fov_deg=120.0)     # another fov_deg is another view
    s.reproject_view()
    assert (pt.log[-1][1][0], pt.log[-1][1][2], pt.log[-1][2][2]) == ("fisheye", 220.0, 120.0)
    s.set_camera_model("pinhole")                    # back to the pinhole: camera-keyed guides behind the call
    s.reproject_view()
    assert [c[0] for c in pt.log[-3:]] == ["set_frame", "reproject_view", "render_guides"]
    assert (pt.log[-2][1][0], pt.log[-2][2][0]) == ("fisheye", "pinhole")
    n = len(pt.log)
    s.preview()
    assert [c[0] for c in pt.log[n:]] == ["denoise"]
    assert s.frame_count == 2


def test_session_two_pinhole_views_are_reproject():
    for model in (None, "pinhole"):
        pt = _FakeTracer()
        s, cam = _session(pt)
        if model:
            s.set_camera_model(model)
        s.frame_counted(2)
        u0 = cam.uniforms()
        cam.rotate(5.0, 2.0)
        st = s.reproject_view(max_history=4)
        assert st["n_reprojected"] == 9
        assert [c[0] for c in pt.log[-2:]] == ["set_frame", "reproject"] and pt.log[-1][2] == 4
        assert np.array_equal(pt.log[-1][1], u0)
        assert not any(c[0] == "reproject_view" for c in pt.log)
        u1 = cam.uniforms()
        cam.rotate(1.0, 0.0)
        s.reproject()                                # and reproject() chains with it
        assert np.array_equal(pt.log[-1][1], u1)


# ---- the pre-existing kernels compile to what they compiled to -------------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(REPO, "profiles", "reproject_view", name)):
        if line.startswith("#") or not line.strip():
            continue
        kernel, numbers = line.rsplit("|", 1)
        rows[kernel.strip()] = numbers.split()
    return rows


def test_existing_kernels_keep_their_resources():
    """profiles/reproject_view/resource_usage_{parent,this}.txt (tools/resource_usage.py): every kernel of
    the parent commit is in this tree with the same numbers -- but pt_reproject_kernel, whose taps became
    a function it shares (DESIGN.md 31.3 gives both lines): it keeps its waves per SIMD --; the three new
    instantiations use no scratch, spill nothing and hold no AGPRs."""
    parent, this = _listing("resource_usage_parent.txt"), _listing("resource_usage_this.txt")
    assert len(parent) >= 60
    for kernel, numbers in parent.items():
        if kernel != "pt_reproject_kernel":
            assert this.get(kernel) == numbers, kernel
    new = sorted(set(this) - set(parent))
    assert new == ["pt_reproject_view_kernel<1>", "pt_reproject_view_kernel<2>", "pt_reproject_view_kernel<3>"]
    for k in new + ["pt_reproject_kernel"]:
        sgpr, vgpr, agpr, scratch, occ, sspill, vspill, lds = (int(v) for v in this[k])
        assert (agpr, scratch, sspill, vspill, lds) == (0, 0, 0, 0, 0), k
    assert int(this["pt_reproject_kernel"][4]) >= int(parent["pt_reproject_kernel"][4])      # waves per SIMD
