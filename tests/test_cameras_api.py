"""pnrt_render_cameras / pnrt_camera_sequence exist in the two headers, in the ctypes
layer, in the built libraries and in the Python classes, with one layout;
InteractiveSession.set_lens / focus_on and the multi-GPU pass-through against fake
tracers; the committed resource-usage listings (no GPU needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from pnraytracing_amd import _native as N
from pnraytracing_amd import host, session, tracer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "pnrt.h")).read()
HOST_HEADER = open(os.path.join(REPO, "include", "pnrt_host.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
HOST_CODE = re.sub(r"/\*.*?\*/", "", HOST_HEADER, flags=re.S)
W = r"\s*\w*\s*"


def test_headers_declare_the_entry_points():
    assert re.search(r"int\s+pnrt_render_cameras\s*\(\s*pnrt_ctx\s*\*" + W + r",\s*uint32_t" + W + r",\s*uint32_t" + W +
                     r",\s*const\s+pnrt_camera\s*\*" + W + r",\s*int" + W + r",\s*int" + W + r",\s*int" + W + r"\)", CODE)
    assert re.search(r"int\s+pnrt_cameras_batch_plan\s*\(\s*pnrt_ctx\s*\*" + W + r",\s*uint32_t" + W + r",\s*int" + W + r",\s*int" +
                     W + r",\s*int" + W + r",\s*uint32_t\s*\*" + W + r",\s*uint32_t\s*\*" + W + r",\s*int64_t\s*\*" + W + r"\)", CODE)
    assert re.search(r"int\s+pnrt_camera_sequence\s*\(\s*const\s+float\s+\w+\[12\]\s*,\s*int" + W + r",\s*int" + W +
                     r",\s*const\s+pnrt_lens_params\s*\*" + W + r",\s*uint32_t" + W + r",\s*uint32_t" + W + r",\s*float\s*\*" + W +
                     r"\)", HOST_CODE)
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)      # no new profile class
    assert len(N.K_CLASSES) == 7 and ctypes.sizeof(N.Profile) == 7 * 16
    # pnrt_batch_plan keeps its declaration
    assert re.search(r"int\s+pnrt_batch_plan\s*\(\s*pnrt_ctx\s*\*\s*ctx,\s*uint32_t\s+n_frames,\s*int\s+band_rows,\s*int\s+n_shards,"
                     r"\s*int\s+shard,\s*uint32_t\s*\*\s*frames_per_batch,\s*uint32_t\s*\*\s*n_batches,\s*int64_t\s*\*\s*batch_bytes\)", CODE)
    doc = HEADER[HEADER.index("Per-frame cameras"):HEADER.index("int pnrt_render_cameras")]
    for words in ("Out of scope", "adaptive variant", "device-array form", "per-pixel"):      # the header says what is out of scope
        assert words in doc, words


def test_lens_params_layout_is_the_headers():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pnrt_lens_params\s*;", HOST_CODE)
    assert m, "pnrt_lens_params not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    assert fields == [("aa_width", "float"), ("lens_radius", "float"), ("focus_distance", "float"), ("reserved", "uint32_t")]
    ctype = {"float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    assert list(N.LensParams._fields_) == [(n, ctype[t]) for n, t in fields]
    assert ctypes.sizeof(N.LensParams) == 16
    assert [getattr(N.LensParams, n).offset for n, _ in fields] == [0, 4, 8, 12]
    assert ctypes.sizeof(N.Camera) == 48             # pnrt_camera_sequence's records are pnrt_render_cameras'


def test_libraries_export_the_symbols_typed():
    fn = N.device_lib().pnrt_render_cameras          # AttributeError: the built library lacks the symbol
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(N.Camera), ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int]
    fn = N.device_lib().pnrt_cameras_batch_plan
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == list(N.device_lib().pnrt_batch_plan.argtypes)
    fn = N.host_lib().pnrt_camera_sequence
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [N.F, ctypes.c_int, ctypes.c_int, ctypes.POINTER(N.LensParams), ctypes.c_uint32, ctypes.c_uint32,
                                 N.F]


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_cameras.h" in build.DEVICE_DEPS
    assert os.path.exists(os.path.join(build.CSRC, "pt_cameras.h"))
    assert callable(build.build_cameras_abi_caller)


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.render_cameras)
    assert list(sig.parameters)[1:] == ["first_frame", "cameras", "band", "n_shards", "shard"]
    assert [sig.parameters[k].default for k in ("band", "n_shards", "shard")] == [1, 1, 0]
    sig = inspect.signature(host.camera_sequence)
    assert list(sig.parameters) == ["camera", "width", "height", "first_frame", "n_frames", "aa_width", "lens_radius",
                                    "focus_distance"]
    sig = inspect.signature(session.InteractiveSession.set_lens)
    assert list(sig.parameters)[1:] == ["aa_width", "lens_radius", "focus_distance"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [1.0, 0.0, None]
    assert list(inspect.signature(session.InteractiveSession.focus_on).parameters)[1:] == ["px", "py"]
    # the existing loop keeps its signatures
    assert list(inspect.signature(session.InteractiveSession.frame).parameters)[1:] == ["redraw", "band", "n_shards", "shard"]
    assert list(inspect.signature(tracer.PathTracer.render).parameters)[1:] == ["first_frame", "n_frames", "band", "n_shards", "shard"]


# ---- InteractiveSession.set_lens / focus_on against a fake tracer ---------------------------------------
class _FakeTracer:
    def __init__(self, hit=True):
        self.log = []
        self.hit = hit

    def enable_moments(self, on=True):
        self.log.append(("enable_moments", bool(on)))

    def set_frame(self, w, h, cam, depth=4):
        self.log.append(("set_frame", w, h, depth))

    def render(self, first, n, band=1, n_shards=1, shard=0):
        self.log.append(("render", first, n, band, n_shards, shard))

    def render_cameras(self, first, cameras, band=1, n_shards=1, shard=0):
        self.log.append(("render_cameras", first, np.array(cameras), band, n_shards, shard))

    def render_adaptive(self, first, n, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        self.log.append(("render_adaptive", first, n))
        return {"n_pixels": 64, "n_active_pixels": 64, "n_tiles": 1, "n_active_tiles": 1, "frames_per_batch": n, "n_batches": 1}

    def cameras_batch_plan(self, n, band=1, n_shards=1, shard=0):
        return {"frames_per_batch": n, "n_batches": 1, "batch_bytes": 1}

    def query_rays(self, rays, any_hit=False):
        rec = np.zeros((1, 16), np.uint32)
        if self.hit:                                 # a hit at (0, 2.8, 1): 6 along the Cornell camera's axis
            rec[0, 0] = 1
            rec[0, 1:4] = np.array([0.0, 2.8, 1.0], np.float32).view(np.uint32)
        return rec


def _session(pt):
    cam = session.CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, 1.0)
    return session.InteractiveSession(pt, 8, 8, cam), cam


def test_session_without_set_lens_is_todays():
    pt = _FakeTracer()
    s, _ = _session(pt)
    s.frame()
    s.frame(True)
    s.frame(band=2, n_shards=3, shard=1)
    s.frame_counted(2)
    assert [c[0] for c in pt.log] == ["set_frame", "render", "set_frame", "render", "set_frame", "render", "enable_moments",
                                      "set_frame", "render_adaptive"]
    assert pt.log[1] == ("render", 0, 1, 1, 1, 0) and pt.log[5] == ("render", 0, 1, 2, 3, 1)


def test_session_set_lens_routes_still_frames():
    pt = _FakeTracer()
    s, cam = _session(pt)
    s.set_lens()                                     # aa_width 1, no lens
    s.frame()
    s.frame(band=2, n_shards=3, shard=1)
    kind, first, cams, band, nsh, shard = pt.log[-1]
    assert (kind, first, band, nsh, shard) == ("render_cameras", 1, 2, 3, 1) and s.frame_count == 2
    want = host.camera_sequence(cam.uniforms(), 8, 8, 1, 1, 1.0, 0.0, 0.0)
    assert np.array_equal(cams.view(np.uint32), want.view(np.uint32))
    s.frame(True)                                    # a redraw stays the reference's un-jittered depth-1 frame 0
    assert pt.log[-2:] == [("set_frame", 8, 8, 1), ("render", 0, 1, 1, 1, 0)] and s.frame_count == 0
    st = s.frame_counted(3)                          # frames 0..2 with their cameras, moments enabled
    kind, first, cams, *_ = pt.log[-1]
    assert (kind, first, len(cams)) == ("render_cameras", 0, 3) and pt.log[-3] == ("enable_moments", True)
    assert np.array_equal(cams.view(np.uint32), host.camera_sequence(cam.uniforms(), 8, 8, 0, 3, 1.0).view(np.uint32))
    assert st["n_active_pixels"] == st["n_pixels"] == 64 and s.frame_count == 3
    assert not any(c[0] == "render_adaptive" for c in pt.log)


def test_session_focus_on():
    pt = _FakeTracer(hit=True)
    s, cam = _session(pt)
    with pytest.raises(ValueError):
        s.set_lens(1.0, 0.1)                         # a lens needs a focus distance
    assert s.focus_on(4, 4) is True
    assert s._lens[2] == pytest.approx(6.0, abs=1e-6)
    s.set_lens(0.5, 0.1)                             # keeps it
    assert s._lens == (0.5, 0.1, s._lens[2]) and s._lens[2] == pytest.approx(6.0, abs=1e-6)
    s.frame()
    want = host.camera_sequence(cam.uniforms(), 8, 8, 0, 1, 0.5, 0.1, s._lens[2])
    assert np.array_equal(pt.log[-1][2].view(np.uint32), want.view(np.uint32))
    s.set_lens(1.0, 0.1, focus_distance=3.0)
    assert s._lens == (1.0, 0.1, 3.0)
    miss = _FakeTracer(hit=False)
    s2, _ = _session(miss)
    assert s2.focus_on(4, 4) is False and s2._lens is None


def test_dist_passes_the_call_through_with_its_selector():
    torch = pytest.importorskip("torch")
    del torch
    from pnraytracing_amd import dist
    src = inspect.getsource(dist)
    m = re.search(r"def render_cameras\(self, first_frame: int, cameras\):.*?\n(?=    def )", src, flags=re.S)
    assert m and "self.tracer.render_cameras(first_frame, cameras, self.band, self.world, self.rank)" in m.group(0)


# ---- the pre-existing kernels compile to what they compiled to -------------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(REPO, "profiles", "cameras", name)):
        if line.startswith("#") or not line.strip():
            continue
        kernel, numbers = line.rsplit("|", 1)
        rows[kernel.strip()] = numbers.split()
    return rows


def test_existing_kernels_keep_their_resources():
    """profiles/cameras/resource_usage_{parent,this}.txt (tools/resource_usage.py): every
    kernel of the parent commit is in this tree with the same numbers; the five new
    instantiations use no scratch and spill no vector register."""
    parent, this = _listing("resource_usage_parent.txt"), _listing("resource_usage_this.txt")
    assert len(parent) >= 50
    for kernel, numbers in parent.items():
        assert this.get(kernel) == numbers, kernel
    new = sorted(set(this) - set(parent))
    assert new == ["pt_camera_rays_wf<8, false>", "pt_camera_rays_wf<8, true>", "pt_wf_gen_setup<WfCams>",
                   "pt_wf_shade_setup<false, WfCams>", "pt_wf_shade_setup<true, WfCams>"]
    for k in new:
        sgpr, vgpr, agpr, scratch, occ, sspill, vspill, lds = (int(v) for v in this[k])
        assert (scratch, vspill, agpr) == (0, 0, 0), k
    # the new gen / shade instantiations sit where the default ones do
    for a, b in (("pt_wf_gen_setup<WfCams>", "pt_wf_gen_setup"), ("pt_wf_shade_setup<false, WfCams>", "pt_wf_shade_setup<false>"),
                 ("pt_wf_shade_setup<true, WfCams>", "pt_wf_shade_setup<true>")):
        assert this[a][4] == this[b][4] and this[a][7] == this[b][7], (a, b)        # occupancy, LDS
