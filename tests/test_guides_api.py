"""The guide-image / denoise entry points exist in include/pnrt.h, in the ctypes
layer and in the Python classes, with one layout (no GPU needed)."""
import ctypes
import inspect
import os
import re

from pnraytracing_amd import _native as N
from pnraytracing_amd import session, tracer

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pnrt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

ENTRY_POINTS = ["pnrt_render_guides", "pnrt_read_aov", "pnrt_aov_device_ptr", "pnrt_denoise", "pnrt_read_denoised",
                "pnrt_denoised_device_ptr"]


def _define(name):
    m = re.search(rf"#define\s+{name}\s+(-?\d+)", CODE)
    assert m, f"{name} not defined in pnrt.h"
    return int(m.group(1))


def test_constants_agree():
    assert _define("PNRT_AOV_POSITION") == N.AOV_POSITION == N.AOV_NAMES.index("position") == 0
    assert _define("PNRT_AOV_NORMAL") == N.AOV_NORMAL == N.AOV_NAMES.index("normal") == 1
    assert _define("PNRT_AOV_ALBEDO") == N.AOV_ALBEDO == N.AOV_NAMES.index("albedo") == 2
    assert _define("PNRT_AOV_COUNT") == N.AOV_COUNT == len(N.AOV_NAMES) == 3


def test_header_declares_the_entry_points():
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(\s*pnrt_ctx\s*\*", CODE), name
    assert re.search(r"int\s+pnrt_denoise\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*const\s+pnrt_denoise_params\s*\*", CODE)
    assert re.search(r"int\s+pnrt_read_aov\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*,\s*float\s*\*", CODE)
    assert re.search(r"void\s*\*\s*pnrt_aov_device_ptr\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)", CODE)
    assert re.search(r"void\s*\*\s*pnrt_denoised_device_ptr\s*\(", CODE)


def test_denoise_params_layout_is_the_headers():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pnrt_denoise_params\s*;", CODE)
    assert m, "pnrt_denoise_params not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert fields == [("levels", "int"), ("sigma_color", "float"), ("sigma_normal", "float"), ("sigma_position", "float")]
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float}
    assert [(n, t) for n, t in N.DenoiseParams._fields_] == [(n, ctype[t]) for n, t in fields]
    assert ctypes.sizeof(N.DenoiseParams) == 16
    assert [getattr(N.DenoiseParams, n).offset for n, _ in fields] == [0, 4, 8, 12]


def test_signatures_are_typed():
    lib = N.device_lib()
    P, F, INT = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int
    want = {"pnrt_render_guides": (INT, [P]), "pnrt_read_aov": (INT, [P, INT, F]),
            "pnrt_aov_device_ptr": (P, [P, INT]), "pnrt_denoise": (INT, [P, ctypes.POINTER(N.DenoiseParams)]),
            "pnrt_read_denoised": (INT, [P, F]), "pnrt_denoised_device_ptr": (P, [P])}
    for name, (res, args) in want.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_python_layer_has_the_methods():
    for name in ("render_guides", "read_aov", "aov_ptr", "denoise", "read_denoised", "denoised_ptr"):
        assert callable(getattr(tracer.PathTracer, name)), name
    sig = inspect.signature(tracer.PathTracer.denoise)
    assert list(sig.parameters)[1:] == ["levels", "sigma_color", "sigma_normal", "sigma_position"]
    assert list(tracer.DENOISE_DEFAULTS) == ["levels", "sigma_color", "sigma_normal", "sigma_position"]
    assert callable(session.InteractiveSession.preview)


def test_python_defaults_are_the_headers():
    """pnrt.h states pnrt_denoise(ctx, NULL)'s parameters; tracer.DENOISE_DEFAULTS fills
    the arguments a caller leaves out with the same ones."""
    m = re.search(r"params == NULL: levels (\S+), sigma_color (\S+), sigma_normal (\S+), sigma_position ([0-9.]+?)\.?\s", HEADER)
    assert m, "defaults not stated in pnrt.h"
    assert [float(v) for v in m.groups()] == [float(v) for v in tracer.DENOISE_DEFAULTS.values()]
    import atrous_ref
    assert atrous_ref.DEFAULTS == tracer.DENOISE_DEFAULTS


class _FakeTracer:
    def __init__(self):
        self.calls, self.valid = [], False

    def render_guides(self):
        self.calls.append("guides")
        self.valid = True

    def denoise(self, **kw):
        if not self.valid:
            e = tracer.PnrtError("pnrt_denoise failed (-3)")
            e.code = -3
            raise e
        self.calls.append(("denoise", kw))


def test_preview_renders_guides_only_when_the_library_asks():
    pt = _FakeTracer()
    s = session.InteractiveSession.__new__(session.InteractiveSession)
    s.pt = pt
    s.preview(levels=3)
    s.preview(levels=3)
    assert pt.calls == ["guides", ("denoise", {"levels": 3}), ("denoise", {"levels": 3})]
    pt.valid = False                      # a camera move / scene edit made the guides stale
    s.preview()
    assert pt.calls[3:] == ["guides", ("denoise", {})]
