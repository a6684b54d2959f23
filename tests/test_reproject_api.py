"""pnrt_reproject exists in include/pnrt.h, in the ctypes layer, in the built library and
in the Python classes, with one layout; InteractiveSession.reproject / frame_counted
against a fake tracer; the committed resource-usage listings (no GPU needed)."""
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
CTYPE = {"int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}


def test_header_declares_the_entry_point():
    assert re.search(r"int\s+pnrt_reproject\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*const\s+pnrt_camera\s*\*\s*\w*\s*,"
                     r"\s*const\s+pnrt_reproject_params\s*\*\s*\w*\s*,\s*pnrt_reproject_stats\s*\*\s*\w*\s*\)", CODE)
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)      # no new profile class
    doc = HEADER[HEADER.index("Temporal reprojection"):HEADER.index("pnrt_reproject_params;")]
    assert "multi-GPU" in doc and "shard" in doc                 # the header says what is out of scope


def _header_fields(struct):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", CODE)
    assert m, f"{struct} not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(n.strip(), typ) for n in names.split(",")]
    return fields


def test_struct_layouts_are_the_headers():
    fields = _header_fields("pnrt_reproject_params")
    assert fields == [("normal_min", "float"), ("position_tolerance", "float"), ("max_history", "uint32_t"),
                      ("reserved", "uint32_t")]
    assert list(N.ReprojectParams._fields_) == [(n, CTYPE[t]) for n, t in fields]
    assert ctypes.sizeof(N.ReprojectParams) == 16
    assert [getattr(N.ReprojectParams, n).offset for n, _ in fields] == [0, 4, 8, 12]
    fields = _header_fields("pnrt_reproject_stats")
    assert fields == [("n_pixels", "int64_t"), ("n_reprojected", "int64_t"), ("n_disoccluded", "int64_t"),
                      ("n_missed", "int64_t"), ("sum_frames", "int64_t"), ("max_frames", "uint32_t"), ("reserved", "uint32_t")]
    assert list(N.ReprojectStats._fields_) == [(n, CTYPE[t]) for n, t in fields]
    assert ctypes.sizeof(N.ReprojectStats) == 48
    assert [getattr(N.ReprojectStats, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 40, 44]


def test_library_exports_the_symbol_typed():
    fn = N.device_lib().pnrt_reproject               # AttributeError: the built library lacks the symbol
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.POINTER(N.Camera), ctypes.POINTER(N.ReprojectParams),
                                 ctypes.POINTER(N.ReprojectStats)]


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_reproject.h" in build.DEVICE_DEPS
    assert os.path.exists(os.path.join(build.CSRC, "pt_reproject.h"))


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.reproject)
    assert list(sig.parameters)[1:] == ["from_camera", "normal_min", "position_tolerance", "max_history"]
    assert sig.parameters["from_camera"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in ("normal_min", "position_tolerance", "max_history")] == [None, None, None]
    assert tracer.REPROJECT_DEFAULTS == {"normal_min": 0.9, "position_tolerance": 0.02, "max_history": 32}
    sig = inspect.signature(session.InteractiveSession.reproject)
    assert [p.kind for p in list(sig.parameters.values())[1:]] == [inspect.Parameter.VAR_KEYWORD]
    sig = inspect.signature(session.InteractiveSession.frame_counted)
    assert list(sig.parameters)[1:] == ["n"] and sig.parameters["n"].default == 1
    # the existing loop keeps its signatures
    sig = inspect.signature(session.InteractiveSession.frame)
    assert list(sig.parameters)[1:] == ["redraw", "band", "n_shards", "shard"]
    sig = inspect.signature(session.InteractiveSession.render_adaptive_until)
    assert list(sig.parameters)[1:] == ["threshold", "max_frames", "frames_per_call", "min_frames"]


# ---- InteractiveSession.reproject / frame_counted against a fake tracer ---------------------------------
class _FakeTracer:
    def __init__(self):
        self.log = []

    def enable_moments(self, on=True):
        self.log.append(("enable_moments", bool(on)))

    def set_frame(self, w, h, cam, depth=4):
        self.log.append(("set_frame", w, h, float(np.asarray(cam)[0, 0]), depth))

    def render(self, first, n, band=1, n_shards=1, shard=0):
        self.log.append(("render", first, n))

    def render_adaptive(self, first, n, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        self.log.append(("render_adaptive", first, n, threshold, min_frames))
        return {"n_pixels": 16, "n_active_pixels": 16, "n_tiles": 1, "n_active_tiles": 1, "frames_per_batch": n, "n_batches": 1}

    def reproject(self, from_camera, normal_min=None, position_tolerance=None, max_history=None):
        self.log.append(("reproject", float(np.asarray(from_camera)[0, 0]), normal_min, position_tolerance, max_history))
        return {"n_pixels": 16, "n_reprojected": 9, "n_disoccluded": 4, "n_missed": 3, "sum_frames": 27, "max_frames": 3}


class _Cam:
    """A camera whose uniforms carry a tag in eye.x."""

    def __init__(self):
        self.tag = 1.0

    def uniforms(self):
        u = np.zeros((4, 3), np.float32)
        u[0, 0] = self.tag
        return u


def test_session_reproject_needs_rendered_frames():
    pt = _FakeTracer()
    s = session.InteractiveSession(pt, 4, 4, _Cam())
    with pytest.raises(ValueError):
        s.reproject()
    s.frame(redraw=True)                             # a redraw leaves frame_count at 0
    assert s.frame_count == 0
    with pytest.raises(ValueError):
        s.reproject()
    assert not any(c[0] == "reproject" for c in pt.log)


def test_session_reproject_order_and_chained_moves():
    pt = _FakeTracer()
    cam = _Cam()
    s = session.InteractiveSession(pt, 4, 4, cam, max_bounce_depth=3)
    assert s.frame_counted(2)["n_active_pixels"] == 16
    assert pt.log == [("enable_moments", True), ("set_frame", 4, 4, 1.0, 3), ("render_adaptive", 0, 2, 0.0, 0xFFFFFFFF)]
    assert s.frame_count == 2
    s.frame()                                        # the plain loop is remembered too
    assert pt.log[-2:] == [("set_frame", 4, 4, 1.0, 3), ("render", 2, 1)] and s.frame_count == 3
    del pt.log[:]
    cam.tag = 2.0                                    # the first move
    st = s.reproject(max_history=8)
    assert st["n_reprojected"] == 9
    assert pt.log == [("set_frame", 4, 4, 2.0, 3), ("reproject", 1.0, None, None, 8)]       # new camera set, `from` the old one
    assert s.frame_count == 3                        # kept
    cam.tag = 3.0                                    # a second move without a frame in between: from the first move's camera
    s.reproject()
    assert pt.log[-2:] == [("set_frame", 4, 4, 3.0, 3), ("reproject", 2.0, None, None, None)] and s.frame_count == 3
    s.frame_counted()
    assert pt.log[-3:] == [("enable_moments", True), ("set_frame", 4, 4, 3.0, 3), ("render_adaptive", 3, 1, 0.0, 0xFFFFFFFF)]
    assert s.frame_count == 4
    cam.tag = 4.0
    s.reproject(normal_min=0.5, position_tolerance=0.1)
    assert pt.log[-1] == ("reproject", 3.0, 0.5, 0.1, None)


def test_session_reproject_after_render_adaptive_until():
    pt = _FakeTracer()
    cam = _Cam()
    s = session.InteractiveSession(pt, 4, 4, cam)
    s.render_adaptive_until(0.1, max_frames=8)
    assert s.frame_count == 8
    cam.tag = 5.0
    s.reproject()
    assert pt.log[-1] == ("reproject", 1.0, None, None, None) and s.frame_count == 8


# ---- the pre-existing kernels compile to what they compiled to -------------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(REPO, "profiles", "reproject", name)):
        if line.startswith("#") or not line.strip():
            continue
        kernel, numbers = line.rsplit("|", 1)
        rows[kernel.strip()] = numbers.split()
    return rows


def test_existing_kernels_keep_their_resources():
    """profiles/reproject/resource_usage_{parent,this}.txt (tools/resource_usage.py): every
    kernel of the parent commit is in this tree with the same numbers; the one new kernel
    uses no scratch, no spills and no LDS."""
    parent, this = _listing("resource_usage_parent.txt"), _listing("resource_usage_this.txt")
    assert len(parent) >= 50
    for kernel, numbers in parent.items():
        assert this.get(kernel) == numbers, kernel
    new = sorted(set(this) - set(parent))
    assert len(new) == 1 and "pt_reproject_kernel" in new[0]
    sgpr, vgpr, agpr, scratch, occ, sspill, vspill, lds = (int(v) for v in this[new[0]])
    assert (scratch, sspill, vspill, lds) == (0, 0, 0, 0)
