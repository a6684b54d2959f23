"""pnrt_denoise_variance exists in include/pnrt.h, in the library, in the ctypes layer
and in the Python classes, with one layout and one set of defaults (no GPU needed)."""
import ctypes
import inspect
import os
import re

import pytest

from pnraytracing_amd import _native as N
from pnraytracing_amd import build, session, tracer

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pnrt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
FIELDS = [("levels", "int"), ("sigma_variance", "float"), ("sigma_normal", "float"), ("sigma_position", "float")]
E_STATE = -3


def test_header_declares_the_struct_and_the_function():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pnrt_denoise_variance_params\s*;", CODE)
    assert m, "pnrt_denoise_variance_params not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert fields == FIELDS
    assert re.search(r"int\s+pnrt_denoise_variance\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*const\s+pnrt_denoise_variance_params\s*\*", CODE)


def test_ctypes_struct_is_the_headers():
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert [(n, t) for n, t in N.DenoiseVarianceParams._fields_] == [(n, ctype[t]) for n, t in FIELDS]
    assert ctypes.sizeof(N.DenoiseVarianceParams) == 16
    assert [getattr(N.DenoiseVarianceParams, n).offset for n, _ in FIELDS] == [0, 4, 8, 12]
    # the fixed-sigma filter's struct is another type, untouched
    assert N.DenoiseVarianceParams is not N.DenoiseParams
    assert [n for n, _ in N.DenoiseParams._fields_] == ["levels", "sigma_color", "sigma_normal", "sigma_position"]


def test_library_exports_the_symbol_with_a_typed_signature():
    lib = N.device_lib()
    fn = lib.pnrt_denoise_variance                   # AttributeError: the library does not export it
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.POINTER(N.DenoiseVarianceParams)]
    assert fn(None, None) == -1                      # PNRT_E_ARG for a NULL context, before anything is touched


def test_defaults_are_the_headers_and_the_restatements():
    m = re.search(r"params == NULL: levels (\S+), sigma_variance (\S+), sigma_normal (\S+), sigma_position ([0-9.]+?)\.?\s", HEADER)
    assert m, "defaults not stated in pnrt.h"
    assert list(tracer.DENOISE_VARIANCE_DEFAULTS) == [n for n, _ in FIELDS]
    assert [float(v) for v in m.groups()] == [float(v) for v in tracer.DENOISE_VARIANCE_DEFAULTS.values()] == [5, 4, 0.25, 0.5]
    import atrous_var_ref
    assert atrous_var_ref.DEFAULTS == tracer.DENOISE_VARIANCE_DEFAULTS
    # pnrt_denoise keeps its own
    assert tracer.DENOISE_DEFAULTS == {"levels": 5, "sigma_color": 2.0, "sigma_normal": 0.25, "sigma_position": 0.5}


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.denoise_variance)
    assert list(sig.parameters)[1:] == [n for n, _ in FIELDS]
    assert all(p.default is None for p in list(sig.parameters.values())[1:])
    sig = inspect.signature(session.InteractiveSession.preview_variance)
    assert [p.kind for p in sig.parameters.values()][1:] == [inspect.Parameter.VAR_KEYWORD]
    assert inspect.signature(session.InteractiveSession.preview) == sig


def test_new_header_is_a_device_dependency():
    assert "pt_denoise_var.h" in build.DEVICE_DEPS
    assert os.path.exists(os.path.join(build.CSRC, "pt_denoise_var.h"))
    assert len(set(build.DEVICE_DEPS)) == len(build.DEVICE_DEPS)


def _state_error(msg):
    e = tracer.PnrtError(f"pnrt_denoise_variance failed ({E_STATE}): {msg}")
    e.code = E_STATE
    return e


class _FakeTracer:
    """The library's order of checks: the moments first, then the guides."""
    def __init__(self, moments="ok"):
        self.calls, self.valid, self.moments = [], False, moments

    def render_guides(self):
        self.calls.append("guides")
        self.valid = True

    def denoise(self, **kw):
        raise AssertionError("preview_variance must not call the fixed-sigma filter")

    def denoise_variance(self, **kw):
        if self.moments == "never":
            raise _state_error("denoise_variance: the sample moments were never enabled (pnrt_enable_moments(ctx, 1) before "
                               "the frames are rendered)")
        if self.moments == "uncovered":
            raise _state_error("denoise_variance: frames were rendered while the moments were disabled, so they do not cover "
                               "the accumulation (pnrt_reset_accum first)")
        if not self.valid:
            raise _state_error("denoise_variance: render_guides first" if "guides" not in self.calls else
                               "denoise_variance: the guide images are stale (camera, size, scene, materials, textures, "
                               "environment or traversal mode changed): render_guides again")
        self.calls.append(("denoise_variance", kw))


def _session(pt):
    s = session.InteractiveSession.__new__(session.InteractiveSession)
    s.pt = pt
    return s


def test_preview_variance_renders_guides_only_when_the_library_asks():
    pt = _FakeTracer()
    s = _session(pt)
    s.preview_variance(levels=3)
    s.preview_variance(levels=3)
    assert pt.calls == ["guides", ("denoise_variance", {"levels": 3}), ("denoise_variance", {"levels": 3})]
    pt.valid = False                      # a camera move / scene edit made the guides stale
    s.preview_variance()
    assert pt.calls[3:] == ["guides", ("denoise_variance", {})]


@pytest.mark.parametrize("moments,word", [("never", "never enabled"), ("uncovered", "do not cover")])
def test_preview_variance_lets_the_moments_errors_through(moments, word):
    pt = _FakeTracer(moments)
    with pytest.raises(tracer.PnrtError) as e:
        _session(pt).preview_variance(levels=2)
    assert e.value.code == E_STATE and word in str(e.value)
    assert pt.calls == []                 # no guide images rendered for an error they cannot cure


def test_preview_variance_raises_other_codes():
    class Bad(_FakeTracer):
        def denoise_variance(self, **kw):
            e = tracer.PnrtError("pnrt_denoise_variance failed (-1): denoise_variance: levels must be 1..5")
            e.code = -1
            raise e
    pt = Bad()
    with pytest.raises(tracer.PnrtError):
        _session(pt).preview_variance(levels=9)
    assert pt.calls == []


def test_library_messages_are_the_ones_the_session_tells_apart():
    """The session tells the guide errors from the moments errors by the words
    'render_guides' in pnrt_last_error(): pin them in the device source."""
    src = open(os.path.join(build.CSRC, "pnrt_device.hip")).read()
    body = src[src.index("int pnrt_denoise_variance("):]
    body = body[:body.index("\n}\n")]
    msgs = re.findall(r'set_err\(c, PNRT_E_STATE,\s*((?:"[^"]*"\s*)+)\)', body)
    msgs = ["".join(re.findall(r'"([^"]*)"', m)) for m in msgs]
    guides = [m for m in msgs if "render_guides" in m]
    assert len(msgs) == 5 and len(guides) == 2
    assert any("never enabled" in m for m in msgs) and any("do not cover" in m for m in msgs)
    # the moments are checked before the guides
    assert body.index("mom_cover") < body.index("guide_key")
