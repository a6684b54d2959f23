"""The in-place geometry edit exists in include/pnrt.h and include/pnrt_host.h, in the
ctypes layer, in both built libraries and in the Python classes (no GPU needed)."""
import ctypes
import inspect
import os
import re

import numpy as np

from pnraytracing_amd import _native as N
from pnraytracing_amd import host, session, tracer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _code(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


CODE, HOST_CODE = _code("pnrt.h"), _code("pnrt_host.h")


def test_header_declares_the_entry_points():
    ctx = r"pnrt_ctx\s*\*\s*\w*"
    tail = r"\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*float\s+\w+\s*\)"
    assert re.search(r"int\s+pnrt_update_vertices\s*\(\s*" + ctx + r"\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+"
                     + tail, CODE)
    assert re.search(r"int\s+pnrt_update_vertices_device\s*\(\s*" + ctx + r"\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*const\s+void\s*\*\s*\w+" + tail, CODE)
    assert re.search(r"int\s+pnrt_read_bvh_boxes\s*\(\s*" + ctx + r"\s*,\s*float\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", CODE)
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)      # no new profile class
    assert len(N.K_CLASSES) == 7 and ctypes.sizeof(N.Profile) == 7 * 16
    assert re.search(r"int\s+pnrt_bvh_refit_cpu\s*\(\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", HOST_CODE)
    assert re.search(r"int\s+pnrt_scene_relight\s*\(\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,"
                     r"\s*int\s+\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*int\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", HOST_CODE)


def test_header_states_the_rule():
    """The first-of-equals rule is what makes -0 / +0 come out as the builder has them."""
    for name in ("pnrt.h", "pnrt_host.h"):
        text = " ".join(open(os.path.join(REPO, "include", name)).read().replace("*", " ").split())
        assert "(y < x) ? y : x" in text and "(x < y) ? y : x" in text, name
        assert "earlier operand stays" in text.lower(), name


def test_libraries_export_the_symbols_typed():
    P, I, F, f = ctypes.c_void_p, ctypes.c_int, N.F, ctypes.c_float
    lib = N.device_lib()                             # AttributeError: the built library lacks a symbol
    for name, args in {"pnrt_update_vertices": [P, I, I, F, F, f], "pnrt_update_vertices_device": [P, I, I, P, F, f],
                       "pnrt_read_bvh_boxes": [P, F, I]}.items():
        fn = getattr(lib, name)
        assert fn.restype is I and list(fn.argtypes) == args, name
    hl = N.host_lib()
    for name, args in {"pnrt_bvh_refit_cpu": [F, I, F, I, F, I],
                       "pnrt_scene_relight": [F, I, F, I, F, I, F, I, N.PINT, ctypes.POINTER(f)]}.items():
        fn = getattr(hl, name)
        assert fn.restype is I and list(fn.argtypes) == args, name


def test_null_context_is_an_argument_error():
    lib = N.device_lib()
    v = np.zeros(15, np.float32)
    assert lib.pnrt_update_vertices(None, 0, 1, N.fptr(v), None, 0.0) == -1
    assert lib.pnrt_update_vertices_device(None, 0, 1, None, None, 0.0) == -1
    assert lib.pnrt_read_bvh_boxes(None, N.fptr(v), 1) == -1


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_refit.h" in build.DEVICE_DEPS
    assert os.path.exists(os.path.join(build.CSRC, "pt_refit.h"))
    assert callable(build.build_refit_abi_caller)


def test_python_layer_has_the_methods():
    def params(fn):
        return [(k, p.default) for k, p in list(inspect.signature(fn).parameters.items())[1:]]

    E = inspect.Parameter.empty
    assert params(tracer.PathTracer.update_vertices) == [("first", E), ("vertices", E), ("lights", None),
                                                          ("lights_sum_area", None)]
    assert params(tracer.PathTracer.update_vertices_device) == [("first", E), ("count", E), ("ptr", E), ("lights", None),
                                                                 ("lights_sum_area", None)]
    assert params(tracer.PathTracer.read_bvh_boxes) == [("nodes", E)]
    assert params(session.InteractiveSession.edit_vertices) == [("first", E), ("vertices", E), ("lights", None),
                                                                 ("lights_sum_area", None)]
    assert list(inspect.signature(host.refit_packed).parameters) == ["packed", "first", "vertices"]
    assert callable(host.model_vertices) and callable(host.bvh_refit_cpu) and callable(host.scene_relight)


class _FakeTracer:
    def __init__(self):
        self.log = []

    def update_vertices(self, first, vertices, lights=None, lights_sum_area=None):
        self.log.append(("update_vertices", first, len(vertices), lights, lights_sum_area))

    def set_frame(self, w, h, cam, depth):
        self.log.append(("set_frame", depth))

    def render(self, first, n, *shard):
        self.log.append(("render", first, n))


class _Cam:
    def uniforms(self):
        return np.zeros((4, 3), np.float32)


def test_session_edit_is_the_update_then_the_depth_one_redraw():
    pt = _FakeTracer()
    s = session.InteractiveSession(pt, 4, 4, _Cam())
    s.frame_count = 5
    assert s.edit_vertices(3, np.zeros((2, 15), np.float32), lights="L", lights_sum_area=2.5) == (1, 0)
    assert pt.log == [("update_vertices", 3, 2, "L", 2.5), ("set_frame", 1), ("render", 0, 1)]   # main.cpp:592-596
    assert s.frame_count == 0
