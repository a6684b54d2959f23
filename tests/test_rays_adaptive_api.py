"""pnrt_render_rays_adaptive exists in the header, in the ctypes layer, in the built library and
in the Python classes; InteractiveSession.render_adaptive_until under a camera model or a lens
and the multi-GPU pass-through against fake tracers; the committed resource-usage listings
(no GPU needed)."""
import ctypes
import inspect
import os
import re

import pytest

from pnraytracing_amd import _native as N
from pnraytracing_amd import session, tracer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "pnrt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
W = r"\s*\w*\s*"


def test_header_declares_the_entry_point():
    assert re.search(r"int\s+pnrt_render_rays_adaptive\s*\(\s*pnrt_ctx\s*\*" + W + r",\s*uint32_t" + W + r",\s*uint32_t" + W +
                     r",\s*const\s+void\s*\*" + W + r",\s*int64_t" + W + r",\s*float" + W + r",\s*uint32_t" + W + r",\s*int" + W +
                     r",\s*int" + W + r",\s*int" + W + r",\s*pnrt_adaptive_stats\s*\*" + W + r"\)", CODE)
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)      # no new profile class
    assert len(N.K_CLASSES) == 7 and ctypes.sizeof(N.Profile) == 7 * 16
    assert ctypes.sizeof(N.AdaptiveStats) == 40 and re.search(r"pnrt_adaptive_stats;\s*/\* 40 bytes \*/", HEADER)
    # the semantics are stated by reference to the two calls it joins
    doc = HEADER[HEADER.index("pnrt_render_adaptive over caller ray buffers"):HEADER.index("int pnrt_render_rays_adaptive")]
    for words in ("pnrt_render_adaptive's", "pnrt_render_rays'", "bit for bit", "no ray", "PNRT_K_PRIMARY", "PNRT_BATCH_BYTES"):
        assert words in doc, words
    # the ray call no longer lists the adaptive variant as out of scope; the camera call points at the rays
    rays_doc = HEADER[HEADER.index("Caller ray buffers"):HEADER.index("int pnrt_render_rays")]
    assert "pnrt_render_rays_adaptive" in rays_doc
    assert "adaptive" not in rays_doc[rays_doc.index("Out of scope"):]
    cams_doc = HEADER[HEADER.index("Per-frame cameras"):HEADER.index("int pnrt_render_cameras")]
    assert "pnrt_render_rays_adaptive" in cams_doc[cams_doc.index("Out of scope"):]


def test_library_exports_the_symbol_typed():
    fn = N.device_lib().pnrt_render_rays_adaptive        # AttributeError: the built library lacks the symbol
    P, INT, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    assert fn.restype is INT
    assert list(fn.argtypes) == [P, U32, U32, P, ctypes.c_int64, ctypes.c_float, U32, INT, INT, INT, ctypes.POINTER(N.AdaptiveStats)]
    assert fn(None, 0, 1, None, 0, 0.5, 2, 1, 1, 0, None) == -1          # a NULL context is refused before anything is touched


def test_device_deps_and_the_abi_caller():
    from pnraytracing_amd import build
    for h in ("pt_wf.h", "pt_rays.h", "pt_adaptive.h"):
        assert h in build.DEVICE_DEPS
    assert len(set(build.DEVICE_DEPS)) == len(build.DEVICE_DEPS)
    assert "c_abi_rays_adaptive.c" in build.ABI_CALLERS and callable(build.build_rays_adaptive_abi_caller)
    wf = open(os.path.join(build.CSRC, "pt_wf.h")).read()
    assert "wf_coords_adaptive_wave" in wf and "wf_pack_get" in wf
    # the built library holds the call's instantiations (the host code names them through one dispatch, so its text does
    # not spell them): pt_wf_gen_setup<WfAdapt, WfRays>, pt_wf_shade_setup<true / false, WfAdapt, WfRays>,
    # pt_rays_wf<WF_STACK, true / false, false, WfAdapt>, by their mangled names
    N.device_lib()
    lib = open(N.DEVICE_LIB, "rb").read()
    for inst in (rb"pt_wf_gen_setupIJ7WfAdapt6WfRaysEE", rb"pt_wf_shade_setupILb1EJ7WfAdapt6WfRaysEE", rb"pt_wf_shade_setupILb0EJ7WfAdapt6WfRaysEE",
                 rb"pt_rays_wfILi\d+ELb1ELb0EJ7WfAdaptEE", rb"pt_rays_wfILi\d+ELb0ELb0EJ7WfAdaptEE"):
        assert re.search(inst, lib), inst


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.render_rays_adaptive)
    assert list(sig.parameters)[1:] == ["first", "n", "rays", "frame_stride", "threshold", "min_frames", "band", "n_shards", "shard"]
    assert [sig.parameters[k].default for k in ("min_frames", "band", "n_shards", "shard")] == [8, 1, 1, 0]
    # the existing calls keep their signatures
    assert list(inspect.signature(tracer.PathTracer.render_adaptive).parameters)[1:] == ["first", "n", "threshold", "min_frames", "band",
                                                                                         "n_shards", "shard"]
    sig = inspect.signature(session.InteractiveSession.render_adaptive_until)
    assert list(sig.parameters)[1:] == ["threshold", "max_frames", "frames_per_call", "min_frames"]
    assert "render_rays_adaptive" in session.InteractiveSession.frame_counted.__doc__
    assert "0xFFFFFFFF" in session.InteractiveSession.frame_counted.__doc__


# ---- render_adaptive_until against a fake tracer ---------------------------------------------------
class _FakeTracer:
    """`left` pixels stay active until `converge_at` frames were issued."""

    def __init__(self, converge_at, n_pixels=64):
        self.converge_at, self.n_pixels = converge_at, n_pixels
        self.log, self.enabled, self.frames = [], 0, 0

    def enable_moments(self, on=True):
        self.enabled += 1 if on else 0

    def set_frame(self, w, h, cam, depth=4):
        self.log.append(("set_frame", w, h, depth))

    def _stats(self, n):
        left = 0 if self.frames >= self.converge_at else self.n_pixels - self.frames
        if left:
            self.frames += n
        return {"n_pixels": self.n_pixels, "n_active_pixels": left, "n_tiles": 1, "n_active_tiles": 1 if left else 0,
                "frames_per_batch": n if left else 0, "n_batches": 1 if left else 0}

    def render(self, *a):
        raise AssertionError("render_adaptive_until issues adaptive calls only")

    render_rays = render_cameras = render

    def render_adaptive(self, first, n, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        assert self.enabled
        self.log.append(("render_adaptive", first, n, threshold, min_frames))
        return self._stats(n)

    def make_rays(self, model, camera, first_frame=0, n_sets=1, frame_stride=None, out=None, **params):
        self.log.append(("make_rays", model, first_frame, n_sets, dict(params)))
        return ("rays", len(self.log))

    def render_rays_adaptive(self, first, n, rays, frame_stride, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        assert self.enabled, "render_adaptive_until must enable the moments before the first call"
        self.log.append(("render_rays_adaptive", first, n, rays, frame_stride, threshold, min_frames))
        return self._stats(n)


def _session(pt):
    cam = session.CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, 1.0)
    return session.InteractiveSession(pt, 8, 8, cam)


def _calls(pt):
    return [c for c in pt.log if c[0] != "set_frame"]


def test_fisheye_makes_rays_then_renders_them_adaptively():
    pt = _FakeTracer(converge_at=10**9)
    s = _session(pt)
    s.set_camera_model("fisheye", fov_deg=200.0)
    stats, frames = s.render_adaptive_until(0.25, max_frames=8, frames_per_call=4, min_frames=3)
    calls = _calls(pt)
    assert [c[0] for c in calls] == ["make_rays", "render_rays_adaptive"] * 2
    still = {"fov_deg": 200.0, "aa_width": 0.0, "lens_radius": 0.0, "focus_distance": 0.0, "per_pixel": 0}
    assert calls[0] == ("make_rays", "fisheye", 0, 1, still) and calls[2] == ("make_rays", "fisheye", 4, 1, still)
    # no samples: one set serves the call's frames, stride 0; the rays are the ones just made
    assert calls[1] == ("render_rays_adaptive", 0, 4, ("rays", 2), 0, 0.25, 3)
    assert calls[3] == ("render_rays_adaptive", 4, 4, ("rays", 5), 0, 0.25, 3)
    assert frames == 8 and s.frame_count == 8 and stats["n_active_pixels"] > 0 and pt.enabled == 1
    # with samples: a set per frame, width * height records apart
    s.set_lens(1.0)
    s.render_adaptive_until(0.25, max_frames=3, frames_per_call=3)
    calls = _calls(pt)[-2:]
    assert calls[0] == ("make_rays", "fisheye", 8, 3, dict(still, aa_width=1.0))
    assert calls[1][:3] == ("render_rays_adaptive", 8, 3) and calls[1][4] == 64 and s.frame_count == 11


def test_a_lens_alone_goes_through_the_pinhole_model():
    pt = _FakeTracer(converge_at=10**9)
    s = _session(pt)
    s.set_lens(1.0, 0.1, focus_distance=3.0)
    s.render_adaptive_until(0.5, max_frames=5, frames_per_call=5)
    a, b = _calls(pt)
    assert a == ("make_rays", "pinhole", 0, 5, {"fov_deg": 180.0, "aa_width": 1.0, "lens_radius": 0.1, "focus_distance": 3.0,
                                                "per_pixel": 0})
    assert b == ("render_rays_adaptive", 0, 5, ("rays", 2), 64, 0.5, 8)
    # ... the frames set_camera_model("pinhole") renders
    pt2 = _FakeTracer(converge_at=10**9)
    s2 = _session(pt2)
    s2.set_lens(1.0, 0.1, focus_distance=3.0)
    s2.set_camera_model("pinhole")
    s2.render_adaptive_until(0.5, max_frames=5, frames_per_call=5)
    assert _calls(pt2) == [a, b]


def test_it_stops_when_nothing_is_active_and_continues_the_frame_count():
    pt = _FakeTracer(converge_at=20)
    s = _session(pt)
    s.set_camera_model("equirect")
    s.frame_count = 5
    stats, frames = s.render_adaptive_until(0.125, max_frames=1000)
    calls = [c for c in _calls(pt) if c[0] == "render_rays_adaptive"]
    # calls of 8 frames at 5, 13, 21; the call at 29 finds nothing active and renders nothing
    assert [c[1:3] for c in calls] == [(5, 8), (13, 8), (21, 8), (29, 8)]
    assert stats["n_active_pixels"] == 0 and frames == 24 and s.frame_count == 29
    pt = _FakeTracer(converge_at=10**9)
    s = _session(pt)
    s.set_camera_model("ortho")
    assert s.render_adaptive_until(0.01, max_frames=0) == (None, 0) and _calls(pt) == []


def test_without_lens_or_model_it_is_todays():
    """(passes before the feature too: the plain session issues pnrt_render_adaptive calls only)"""
    pt = _FakeTracer(converge_at=10**9)
    s = _session(pt)
    stats, frames = s.render_adaptive_until(0.01, max_frames=20, frames_per_call=6, min_frames=3)
    assert _calls(pt) == [("render_adaptive", f, n, 0.01, 3) for f, n in ((0, 6), (6, 6), (12, 6), (18, 2))]
    assert frames == 20 and s.frame_count == 20


def test_dist_passes_the_call_through_with_its_selector():
    pytest.importorskip("torch")
    from pnraytracing_amd import dist

    class T:
        width, height = 16, 16

        def render_rays_adaptive(self, *a):
            self.got = a
            return {"n_active_pixels": 7}

    t = T()
    sf = dist.ShardedFrame(t, band=4, device="cpu", shard=(3, 1))
    assert sf.render_rays_adaptive(5, 2, 4096, 256, 0.25, 6) == {"n_active_pixels": 7}
    assert t.got == (5, 2, 4096, 256, 0.25, 6, 4, 3, 1)


# ---- the pre-existing kernels compile to what they compiled to -------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(REPO, "profiles", "rays_adaptive", name)):
        if line.startswith("#") or not line.strip():
            continue
        kernel, numbers = line.rsplit("|", 1)
        rows[kernel.strip()] = numbers.split()
    return rows


def test_existing_kernels_keep_their_resources():
    """profiles/rays_adaptive/resource_usage_{parent,this}.txt (tools/resource_usage.py): every kernel
    of the parent commit is in this tree with the same numbers; the new instantiations use no
    scratch and spill no vector register, and sit at their twins' occupancy."""
    parent, this = _listing("resource_usage_parent.txt"), _listing("resource_usage_this.txt")
    assert len(parent) >= 63
    for kernel, numbers in parent.items():
        assert this.get(kernel) == numbers, kernel
    twin = {"pt_rays_wf<8, false, false, WfAdapt>": "pt_rays_wf<8, false, false>",
            "pt_rays_wf<8, true, false, WfAdapt>": "pt_rays_wf<8, true, false>",
            "pt_wf_gen_setup<WfAdapt, WfRays>": "pt_wf_gen_setup<WfRays>",
            "pt_wf_shade_setup<false, WfAdapt, WfRays>": "pt_wf_shade_setup<false, WfRays>",
            "pt_wf_shade_setup<true, WfAdapt, WfRays>": "pt_wf_shade_setup<true, WfRays>"}
    assert sorted(set(this) - set(parent)) == sorted(twin)
    for k, t in twin.items():
        sgpr, vgpr, agpr, scratch, occ, sspill, vspill, lds = (int(v) for v in this[k])
        assert (scratch, vspill, agpr) == (0, 0, 0), k
        assert occ == int(this[t][4]) and lds == int(this[t][7]), (k, t)
