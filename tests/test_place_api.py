"""Placing models by a matrix exists in include/pnrt.h and include/pnrt_host.h, in the
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
    head = r"\s*\(\s*" + ctx + r"\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,"
    assert re.search(r"int\s+pnrt_define_model" + head + r"\s*const\s+float\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)", CODE)
    assert re.search(r"int\s+pnrt_define_model_device" + head + r"\s*const\s+void\s*\*\s*\w+\s*,\s*int\s*\*\s*\w+\s*\)", CODE)
    assert re.search(r"int\s+pnrt_place_models\s*\(\s*" + ctx + r"\s*,\s*const\s+pnrt_placement\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*int\s+\w+\s*\)", CODE)
    assert re.search(r"int\s+pnrt_read_vertices" + head + r"\s*float\s*\*\s*\w+\s*\)", CODE)
    assert re.search(r"typedef\s+struct\s*\{\s*int\s+model\s*;\s*float\s+matrix\s*\[\s*16\s*\]\s*;\s*int\s+reserved\s*;\s*\}\s*"
                     r"pnrt_placement\s*;", CODE)
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)      # no new profile class
    assert len(N.K_CLASSES) == 7 and ctypes.sizeof(N.Profile) == 7 * 16
    assert re.search(r"int\s+pnrt_normal_matrix\s*\(\s*const\s+float\s+\w+\s*\[\s*16\s*\]\s*,\s*float\s+\w+\s*\[\s*16\s*\]\s*\)",
                     HOST_CODE)


def test_header_states_the_arithmetic_and_the_relight_rule():
    text = " ".join(open(os.path.join(REPO, "include", "pnrt.h")).read().replace("*", " ").split())
    flat = text.replace(" ", "")
    assert "pos[r]=(M[0][r]p.x+M[1][r]p.y)+(M[2][r]p.z+M[3][r]1.0f)" in flat
    assert "normal[r]=(N[0][r]n.x+N[1][r]n.y)+(N[2][r]n.z+N[3][r]1.0f)" in flat
    assert "replaces every entry's area" in text.lower() and "untouched lights" in text


def test_placement_is_72_bytes():
    assert ctypes.sizeof(N.Placement) == 72
    assert [(n, ctypes.sizeof(t)) for n, t in N.Placement._fields_] == [("model", 4), ("matrix", 64), ("reserved", 4)]


def test_libraries_export_the_symbols_typed():
    P, I, F = ctypes.c_void_p, ctypes.c_int, N.F
    lib = N.device_lib()                             # AttributeError: the built library lacks a symbol
    for name, args in {"pnrt_define_model": [P, I, I, F, N.PINT], "pnrt_define_model_device": [P, I, I, P, N.PINT],
                       "pnrt_place_models": [P, ctypes.POINTER(N.Placement), I, I], "pnrt_read_vertices": [P, I, I, F]}.items():
        fn = getattr(lib, name)
        assert fn.restype is I and list(fn.argtypes) == args, name
    fn = N.host_lib().pnrt_normal_matrix
    assert fn.restype is I and list(fn.argtypes) == [F, F]


def test_null_context_is_an_argument_error():
    lib = N.device_lib()
    v = np.zeros(8, np.float32)
    mid = ctypes.c_int(7)
    assert lib.pnrt_define_model(None, 0, 1, N.fptr(v), ctypes.byref(mid)) == -1
    assert lib.pnrt_define_model_device(None, 0, 1, None, ctypes.byref(mid)) == -1
    assert lib.pnrt_place_models(None, (N.Placement * 1)(), 1, 0) == -1
    assert lib.pnrt_read_vertices(None, 0, 1, N.fptr(v)) == -1
    assert mid.value == 7


def test_normal_matrix_refuses_null():
    out = np.zeros(16, np.float32)
    assert N.host_lib().pnrt_normal_matrix(None, N.fptr(out)) < 0
    assert N.host_lib().pnrt_normal_matrix(N.fptr(out), None) < 0


def test_build_knows_the_new_sources():
    from pnraytracing_amd import build
    assert "pt_place.h" in build.DEVICE_DEPS and "pn_glm.h" in build.DEVICE_DEPS
    for name in ("pt_place.h", "pn_glm.h"):
        assert os.path.exists(os.path.join(build.CSRC, name))
    assert "c_abi_place.c" in build.ABI_CALLERS and callable(build.build_place_abi_caller)


def test_glm_helpers_have_one_copy():
    """inverse and transpose live in the shared header; the host library includes it."""
    from pnraytracing_amd import build
    src = open(os.path.join(build.CSRC, "host", "pnrt_host.cpp")).read()
    hdr = open(os.path.join(build.CSRC, "pn_glm.h")).read()
    dev = open(os.path.join(build.CSRC, "pnrt_device.hip")).read()
    assert '#include "../pn_glm.h"' in src and '#include "pn_glm.h"' in dev
    assert "Coef00" in hdr and "Coef00" not in src and "Coef00" not in dev
    assert len(re.findall(r"\bmat4\s+transpose\s*\(", hdr)) == 1 and not re.search(r"\bmat4\s+transpose\s*\(", src)


def test_python_layer_has_the_methods():
    def params(fn):
        return [(k, p.default) for k, p in list(inspect.signature(fn).parameters.items())[1:]]

    E = inspect.Parameter.empty
    assert params(tracer.PathTracer.define_model) == [("first", E), ("model8", E)]
    assert params(tracer.PathTracer.place_models) == [("placements", E), ("relight", False)]
    assert params(tracer.PathTracer.read_vertices) == [("first", E), ("count", E)]
    assert params(session.InteractiveSession.define_model) == [("first", E), ("mesh", E)]
    assert params(session.InteractiveSession.move_model) == [("model_id", E), ("ops", E), ("relight", False)]
    assert list(inspect.signature(host.normal_matrix).parameters) == ["m"]
    assert list(inspect.signature(host.model_records).parameters) == ["mesh"]


def test_model_records_zero_what_a_mesh_lacks():
    P = np.arange(6, dtype=np.float32).reshape(2, 3)
    rec = host.model_records(host.Mesh(P, None, None, np.arange(3, dtype=np.int32)))
    assert rec.dtype == np.float32 and rec.shape == (2, 8)
    assert np.array_equal(rec[:, 0:3], P) and not rec[:, 3:].any()
    q = host.mesh_quad(1.0)
    rec = host.model_records(q)
    assert np.array_equal(rec[:, 0:3], q.positions) and np.array_equal(rec[:, 3:6], q.normals) and np.array_equal(rec[:, 6:8], q.texcoords)


class _FakeTracer:
    def __init__(self):
        self.log = []

    def define_model(self, first, model8):
        self.log.append(("define_model", first, np.asarray(model8).shape))
        return 4

    def place_models(self, placements, relight=False):
        self.log.append(("place_models", [(i, np.asarray(m).tobytes()) for i, m in placements], relight))

    def set_frame(self, w, h, cam, depth):
        self.log.append(("set_frame", depth))

    def render(self, first, n, *shard):
        self.log.append(("render", first, n))


class _Cam:
    def uniforms(self):
        return np.zeros((4, 3), np.float32)


def test_session_move_is_the_placement_then_the_depth_one_redraw():
    pt = _FakeTracer()
    s = session.InteractiveSession(pt, 4, 4, _Cam())
    assert s.define_model(6, host.mesh_quad(1.0)) == 4           # (a quad is two unshared triangles: 6 vertices)
    s.frame_count = 5
    ops = [host.translate(1, 2, 3), host.scale(2)]
    assert s.move_model(4, ops, relight=True) == (1, 0)
    assert pt.log == [("define_model", 6, (6, 8)), ("place_models", [(4, host.model_matrix(ops).tobytes())], True),
                      ("set_frame", 1), ("render", 0, 1)]            # main.cpp:592-596
    assert s.frame_count == 0
