"""pnrt_render_rays / pnrt_render_guides_rays / pnrt_make_rays exist in the header, in the
ctypes layer, in the built library and in the Python classes, with one layout;
InteractiveSession.set_camera_model and the multi-GPU pass-through against fake tracers; the
committed resource-usage listings (no GPU needed)."""
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
W = r"\s*\w*\s*"


def test_header_declares_the_entry_points():
    assert re.search(r"int\s+pnrt_render_rays\s*\(\s*pnrt_ctx\s*\*" + W + r",\s*uint32_t" + W + r",\s*uint32_t" + W +
                     r",\s*const\s+void\s*\*" + W + r",\s*int64_t" + W + r",\s*int" + W + r",\s*int" + W + r",\s*int" + W + r"\)", CODE)
    assert re.search(r"int\s+pnrt_render_guides_rays\s*\(\s*pnrt_ctx\s*\*" + W + r",\s*const\s+void\s*\*" + W + r"\)", CODE)
    assert re.search(r"int\s+pnrt_make_rays\s*\(\s*pnrt_ctx\s*\*" + W + r",\s*const\s+pnrt_ray_camera\s*\*" + W + r",\s*uint32_t" + W +
                     r",\s*uint32_t" + W + r",\s*void\s*\*" + W + r",\s*int64_t" + W + r"\)", CODE)
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)      # no new profile class
    assert len(N.K_CLASSES) == 7 and ctypes.sizeof(N.Profile) == 7 * 16
    for k, name in enumerate(("PINHOLE", "ORTHO", "EQUIRECT", "FISHEYE")):
        assert re.search(rf"#define\s+PNRT_CAM_{name}\s+{k}\b", CODE), name
    assert N.CAM_MODELS == ("pinhole", "ortho", "equirect", "fisheye")
    doc = HEADER[HEADER.index("Caller ray buffers"):HEADER.index("int pnrt_render_rays")]
    for words in ("Out of scope", "adaptive variant", "host-array form", "tMax", "never normalised", "no ray"):
        assert words in doc, words
    # the earlier entry points keep their declarations
    assert re.search(r"int\s+pnrt_render_cameras\s*\(\s*pnrt_ctx\s*\*\s*ctx,\s*uint32_t\s+first_frame,\s*uint32_t\s+n_frames,"
                     r"\s*const\s+pnrt_camera\s*\*\s*cameras,\s*int\s+band_rows,\s*int\s+n_shards,\s*int\s+shard\)", CODE)
    assert re.search(r"int\s+pnrt_render_guides\s*\(\s*pnrt_ctx\s*\*\s*ctx\s*\)", CODE)


def _struct_fields(name):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + name + r"\s*;", CODE)
    assert m, f"{name} not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    return fields


def test_struct_layouts_are_the_headers():
    assert _struct_fields("pnrt_ray") == [("origin[3]", "float"), ("reserved0", "float"), ("direction[3]", "float"),
                                          ("reserved1", "float")]
    assert ctypes.sizeof(N.Ray) == 32
    assert [getattr(N.Ray, n).offset for n, _ in N.Ray._fields_] == [0, 12, 16, 28]
    assert re.search(r"pnrt_ray;\s*/\* 32 bytes \*/", HEADER)
    fields = _struct_fields("pnrt_ray_camera")
    assert fields == [("model", "int"), ("camera", "pnrt_camera"), ("fov_deg", "float"), ("aa_width", "float"),
                      ("lens_radius", "float"), ("focus_distance", "float"), ("per_pixel", "int"), ("reserved", "int")]
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "pnrt_camera": N.Camera}
    assert list(N.RayCamera._fields_) == [(n, ctype[t]) for n, t in fields]
    assert ctypes.sizeof(N.RayCamera) == 76              # the documented size
    assert re.search(r"pnrt_ray_camera;\s*/\* 76 bytes \*/", HEADER)
    assert [getattr(N.RayCamera, n).offset for n, _ in fields] == [0, 4, 52, 56, 60, 64, 68, 72]


def test_library_exports_the_symbols_typed():
    lib = N.device_lib()                                 # AttributeError: the built library lacks a symbol
    fn = lib.pnrt_render_rays
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int]
    fn = lib.pnrt_render_guides_rays
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p]
    fn = lib.pnrt_make_rays
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.POINTER(N.RayCamera), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                 ctypes.c_int64]
    # a NULL context is refused before anything is touched
    assert lib.pnrt_render_rays(None, 0, 1, None, 0, 1, 1, 0) == -1
    assert lib.pnrt_render_guides_rays(None, None) == -1
    assert lib.pnrt_make_rays(None, None, 0, 1, None, 0) == -1


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_rays.h" in build.DEVICE_DEPS
    assert len(set(build.DEVICE_DEPS)) == len(build.DEVICE_DEPS)
    assert os.path.exists(os.path.join(build.CSRC, "pt_rays.h"))
    assert "c_abi_rays.c" in build.ABI_CALLERS and callable(build.build_rays_abi_caller)
    src = open(os.path.join(build.CSRC, "pt_rays.h")).read()
    for name in ("pt_rays_wf", "pt_make_rays_kernel"):
        assert name in src, name
    wf = open(os.path.join(build.CSRC, "pt_wf.h")).read()
    assert re.search(r"struct\s+WfRays\s*\{\s*const\s+float4\s*\*\s*rays;[^}]*int64_t\s+frame_stride;", wf)


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.render_rays)
    assert list(sig.parameters)[1:] == ["first_frame", "n_frames", "rays", "frame_stride", "band", "n_shards", "shard"]
    assert [sig.parameters[k].default for k in ("frame_stride", "band", "n_shards", "shard")] == [0, 1, 1, 0]
    assert list(inspect.signature(tracer.PathTracer.render_guides_rays).parameters)[1:] == ["rays"]
    sig = inspect.signature(tracer.PathTracer.make_rays)
    assert list(sig.parameters)[1:5] == ["model", "camera", "first_frame", "n_sets"]
    sig = inspect.signature(session.InteractiveSession.set_camera_model)
    assert list(sig.parameters)[1:] == ["model", "fov_deg", "per_pixel"]
    # the existing loop keeps its signatures
    assert list(inspect.signature(session.InteractiveSession.frame).parameters)[1:] == ["redraw", "band", "n_shards", "shard"]
    assert list(inspect.signature(tracer.PathTracer.render_cameras).parameters)[1:] == ["first_frame", "cameras", "band", "n_shards",
                                                                                        "shard"]


# ---- InteractiveSession.set_camera_model against a fake tracer ----------------------------------------
class _FakeTracer:
    def __init__(self):
        self.log = []
        self.guides = False

    def enable_moments(self, on=True):
        self.log.append(("enable_moments", bool(on)))

    def set_frame(self, w, h, cam, depth=4):
        self.log.append(("set_frame", w, h, depth))

    def render(self, first, n, band=1, n_shards=1, shard=0):
        self.log.append(("render", first, n, band, n_shards, shard))

    def render_cameras(self, first, cameras, band=1, n_shards=1, shard=0):
        self.log.append(("render_cameras", first, len(cameras)))

    def render_adaptive(self, first, n, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        self.log.append(("render_adaptive", first, n))
        return {"n_pixels": 64, "n_active_pixels": 64, "n_tiles": 1, "n_active_tiles": 1, "frames_per_batch": n, "n_batches": 1}

    def cameras_batch_plan(self, n, band=1, n_shards=1, shard=0):
        return {"frames_per_batch": n, "n_batches": 1, "batch_bytes": 1}

    def make_rays(self, model, camera, first_frame=0, n_sets=1, frame_stride=None, out=None, **params):
        self.log.append(("make_rays", model, first_frame, n_sets, dict(params)))
        return ("rays", len(self.log))

    def render_rays(self, first, n, rays, frame_stride=0, band=1, n_shards=1, shard=0):
        self.log.append(("render_rays", first, n, rays, frame_stride, band, n_shards, shard))

    def render_guides(self):
        self.log.append(("render_guides",))
        self.guides = True

    def render_guides_rays(self, rays):
        self.log.append(("render_guides_rays", rays))
        self.guides = True

    def denoise(self, **params):
        if not self.guides:
            e = tracer.PnrtError("denoise: render_guides first")
            e.code = -3
            raise e
        self.log.append(("denoise",))

    def denoise_variance(self, **params):
        if not self.guides:
            e = tracer.PnrtError("denoise_variance: render_guides first")
            e.code = -3
            raise e
        self.log.append(("denoise_variance",))


def _session(pt):
    cam = session.CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, 1.0)
    return session.InteractiveSession(pt, 8, 8, cam), cam


def test_session_without_set_camera_model_is_todays():
    pt = _FakeTracer()
    s, _ = _session(pt)
    s.frame()
    s.frame(True)
    s.set_lens()
    s.frame(band=2, n_shards=3, shard=1)
    s.frame_counted(2)
    s.preview()
    assert [c[0] for c in pt.log] == ["set_frame", "render", "set_frame", "render", "set_frame", "render_cameras", "enable_moments",
                                      "set_frame", "render_cameras", "render_guides", "denoise"]


def test_session_fisheye_routes_every_frame_through_the_rays():
    pt = _FakeTracer()
    s, _ = _session(pt)
    s.set_camera_model("fisheye", fov_deg=200.0)
    s.frame()
    assert pt.log[-2] == ("make_rays", "fisheye", 0, 1, {"fov_deg": 200.0, "aa_width": 0.0, "lens_radius": 0.0,
                                                         "focus_distance": 0.0, "per_pixel": 0})
    assert pt.log[-1] == ("render_rays", 0, 1, ("rays", 2), 0, 1, 1, 0) and s.frame_count == 1
    s.frame(band=2, n_shards=3, shard=1)
    assert pt.log[-1][:3] == ("render_rays", 1, 1) and pt.log[-1][4:] == (0, 2, 3, 1)
    s.frame(True)                                        # a redraw: depth-1 frame 0, the same model, no samples
    assert pt.log[-3] == ("set_frame", 8, 8, 1) and pt.log[-2][:4] == ("make_rays", "fisheye", 0, 1)
    assert pt.log[-1][:3] == ("render_rays", 0, 1) and s.frame_count == 0
    st = s.frame_counted(3)                              # no samples: one set serves the three frames
    assert pt.log[-2][:4] == ("make_rays", "fisheye", 0, 1) and pt.log[-1][:3] == ("render_rays", 0, 3) and pt.log[-1][4] == 0
    assert st["n_active_pixels"] == st["n_pixels"] == 64 and s.frame_count == 3
    s.preview()
    assert [c[0] for c in pt.log[-3:]] == ["make_rays", "render_guides_rays", "denoise"]
    assert pt.log[-3][1:4] == ("fisheye", 0, 1) and pt.log[-3][4]["fov_deg"] == 200.0
    assert not any(c[0] in ("render", "render_cameras", "render_adaptive", "render_guides") for c in pt.log)
    pt.guides = False
    s.preview_variance()
    assert [c[0] for c in pt.log[-3:]] == ["make_rays", "render_guides_rays", "denoise_variance"]


def test_session_renders_ray_guides_again_when_the_view_changes():
    """The library accepts ray-made guides for any camera (the fake says yes to every denoise once it has guides):
    the session must notice a camera move, another fov_deg and another model itself."""
    pt = _FakeTracer()
    s, cam = _session(pt)
    s.set_camera_model("fisheye", fov_deg=200.0)
    s.frame()
    s.preview()
    s.preview()                                          # nothing changed: only the filter
    assert [c[0] for c in pt.log[-4:]] == ["make_rays", "render_guides_rays", "denoise", "denoise"]
    cam.rotate(5.0, 2.0)
    s.preview()
    assert [c[0] for c in pt.log[-3:]] == ["make_rays", "render_guides_rays", "denoise"]
    s.set_camera_model("fisheye", fov_deg=120.0)
    s.preview_variance()
    assert [c[0] for c in pt.log[-3:]] == ["make_rays", "render_guides_rays", "denoise_variance"] and pt.log[-3][4]["fov_deg"] == 120.0
    s.set_camera_model("equirect")
    s.preview()
    assert [c[0] for c in pt.log[-3:]] == ["make_rays", "render_guides_rays", "denoise"] and pt.log[-3][1] == "equirect"
    s.preview()
    assert [c[0] for c in pt.log[-2:]] == ["denoise", "denoise"]
    s.set_camera_model("pinhole")                        # camera-keyed guides again, though the library would take the old ones
    s.preview()
    assert [c[0] for c in pt.log[-2:]] == ["render_guides", "denoise"]
    s.preview()
    assert [c[0] for c in pt.log[-2:]] == ["denoise", "denoise"]


def test_session_refusals_do_not_depend_on_call_order():
    pt = _FakeTracer()
    s, _ = _session(pt)
    s.set_camera_model("fisheye")
    with pytest.raises(ValueError):
        s.set_lens(1.0, 0.1, 3.0)                        # a lens after the model, as before it
    s.set_lens(1.0)                                      # the pixel filter alone is any model's
    s.frame()
    with pytest.raises(ValueError):
        s.reproject()                                    # pinhole views only
    s2, _ = _session(_FakeTracer())
    s2.set_lens(1.0, 0.1, 3.0)
    with pytest.raises(ValueError):
        s2.set_camera_model("ortho")


def test_session_pinhole_model_samples_per_pixel_and_redraws_as_the_reference():
    pt = _FakeTracer()
    s, _ = _session(pt)
    s.set_lens(1.0, 0.1, focus_distance=3.0)
    s.set_camera_model("pinhole", per_pixel=True)
    s.frame()
    assert pt.log[-2] == ("make_rays", "pinhole", 0, 1, {"fov_deg": 180.0, "aa_width": 1.0, "lens_radius": 0.1,
                                                         "focus_distance": 3.0, "per_pixel": 1})
    assert pt.log[-1][:3] == ("render_rays", 0, 1)
    st = s.frame_counted(4)                              # a set per frame
    assert pt.log[-2][:4] == ("make_rays", "pinhole", 1, 4) and pt.log[-1][:3] == ("render_rays", 1, 4) and pt.log[-1][4] == 64
    assert st["n_batches"] == 1 and s.frame_count == 5
    s.frame(True)                                        # the reference's depth-1 frame 0 of the pinhole camera
    assert pt.log[-2:] == [("set_frame", 8, 8, 1), ("render", 0, 1, 1, 1, 0)] and s.frame_count == 0


def test_dist_passes_the_call_through_with_its_selector():
    torch = pytest.importorskip("torch")
    del torch
    from pnraytracing_amd import dist
    src = inspect.getsource(dist)
    m = re.search(r"def render_rays\(self, first_frame: int, n_frames: int, rays, frame_stride: int = 0\):.*?\n(?=    def )", src,
                  flags=re.S)
    assert m and "self.tracer.render_rays(first_frame, n_frames, rays, frame_stride, self.band, self.world, self.rank)" in m.group(0)

    class T:
        width, height = 16, 16

        def render_rays(self, *a):
            self.got = a

    t = T()
    sf = dist.ShardedFrame(t, band=4, device="cpu", shard=(3, 1))
    sf.render_rays(5, 2, 4096, 256)
    assert t.got == (5, 2, 4096, 256, 4, 3, 1)


# ---- the pre-existing kernels compile to what they compiled to -------------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(REPO, "profiles", "rays", name)):
        if line.startswith("#") or not line.strip():
            continue
        kernel, numbers = line.rsplit("|", 1)
        rows[kernel.strip()] = numbers.split()
    return rows


def test_existing_kernels_keep_their_resources():
    """profiles/rays/resource_usage_{parent,this}.txt (tools/resource_usage.py): every kernel
    of the parent commit is in this tree with the same numbers; the new instantiations use no
    scratch and spill no vector register -- no more than their WfCams twins."""
    parent, this = _listing("resource_usage_parent.txt"), _listing("resource_usage_this.txt")
    assert len(parent) >= 55
    for kernel, numbers in parent.items():
        assert this.get(kernel) == numbers, kernel
    new = sorted(set(this) - set(parent))
    assert new == ["pt_make_rays_kernel", "pt_rays_wf<8, false, false>", "pt_rays_wf<8, false, true>", "pt_rays_wf<8, true, false>",
                   "pt_rays_wf<8, true, true>", "pt_wf_gen_setup<WfRays>", "pt_wf_shade_setup<false, WfRays>",
                   "pt_wf_shade_setup<true, WfRays>"]
    twin = {"pt_rays_wf<8, false, false>": "pt_camera_rays_wf<8, false>", "pt_rays_wf<8, false, true>": "pt_camera_rays_wf<8, false>",
            "pt_rays_wf<8, true, false>": "pt_camera_rays_wf<8, true>", "pt_rays_wf<8, true, true>": "pt_camera_rays_wf<8, true>",
            "pt_wf_gen_setup<WfRays>": "pt_wf_gen_setup<WfCams>", "pt_wf_shade_setup<false, WfRays>": "pt_wf_shade_setup<false, WfCams>",
            "pt_wf_shade_setup<true, WfRays>": "pt_wf_shade_setup<true, WfCams>"}
    for k in new:
        sgpr, vgpr, agpr, scratch, occ, sspill, vspill, lds = (int(v) for v in this[k])
        assert (scratch, vspill, agpr) == (0, 0, 0), k
        if k in twin:
            t = [int(v) for v in this[twin[k]]]
            assert scratch <= t[3] and vspill <= t[6] and lds == t[7], (k, twin[k])
    # the new gen / shade instantiations sit where their twins do
    for a in ("pt_wf_gen_setup<WfRays>", "pt_wf_shade_setup<false, WfRays>", "pt_wf_shade_setup<true, WfRays>"):
        assert this[a][4] == this[twin[a]][4] and this[a][1] == this[twin[a]][1], a       # occupancy, VGPRs
