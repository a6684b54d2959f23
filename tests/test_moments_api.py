"""The sample-moments / convergence entry points exist in include/pnrt.h, in the
ctypes layer, in the built library and in the Python classes, with one layout;
InteractiveSession.render_until against a fake tracer (no GPU needed)."""
import ctypes
import inspect
import os
import re

from pnraytracing_amd import _native as N
from pnraytracing_amd import session, tracer

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pnrt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)

ENTRY_POINTS = ["pnrt_enable_moments", "pnrt_moments_device_ptr", "pnrt_read_moments", "pnrt_read_error",
                "pnrt_convergence"]


def test_header_declares_the_entry_points():
    for name in ENTRY_POINTS:
        assert re.search(rf"\b{name}\s*\(\s*pnrt_ctx\s*\*", CODE), name
    assert re.search(r"int\s+pnrt_enable_moments\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)", CODE)
    assert re.search(r"void\s*\*\s*pnrt_moments_device_ptr\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*\)", CODE)
    assert re.search(r"int\s+pnrt_read_moments\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*float\s*\*", CODE)
    assert re.search(r"int\s+pnrt_read_error\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*float\s*\*", CODE)
    assert re.search(r"int\s+pnrt_convergence\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*float\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*int\s+\w+\s*,\s*pnrt_convergence_stats\s*\*", CODE)


def test_convergence_stats_layout_is_the_headers():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pnrt_convergence_stats\s*;", CODE)
    assert m, "pnrt_convergence_stats not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert fields == [("n_pixels", "int64_t"), ("n_measured", "int64_t"), ("n_above", "int64_t"), ("sum_q16", "int64_t"),
                      ("max_error", "float"), ("min_frames", "uint32_t"), ("max_frames", "uint32_t"),
                      ("reserved", "uint32_t")]
    ctype = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32}
    assert [(n, t) for n, t in N.ConvergenceStats._fields_] == [(n, ctype[t]) for n, t in fields]
    assert ctypes.sizeof(N.ConvergenceStats) == 48
    assert [getattr(N.ConvergenceStats, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 36, 40, 44]


def test_library_exports_the_symbols_typed():
    lib = N.device_lib()
    P, F, INT = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int
    want = {"pnrt_enable_moments": (INT, [P, INT]), "pnrt_moments_device_ptr": (P, [P]),
            "pnrt_read_moments": (INT, [P, F]), "pnrt_read_error": (INT, [P, F]),
            "pnrt_convergence": (INT, [P, ctypes.c_float, INT, INT, INT, ctypes.POINTER(N.ConvergenceStats)])}
    assert sorted(want) == sorted(ENTRY_POINTS)
    for name, (res, args) in want.items():
        fn = getattr(lib, name)                      # AttributeError: the built library lacks the symbol
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_moments.h" in build.DEVICE_DEPS
    assert os.path.exists(os.path.join(build.CSRC, "pt_moments.h"))


def test_python_layer_has_the_methods():
    for name in ("enable_moments", "read_moments", "read_error", "moments_ptr", "convergence"):
        assert callable(getattr(tracer.PathTracer, name)), name
    sig = inspect.signature(tracer.PathTracer.convergence)
    assert list(sig.parameters)[1:] == ["threshold", "band", "n_shards", "shard"]
    assert [sig.parameters[k].default for k in ("band", "n_shards", "shard")] == [1, 1, 0]
    assert callable(tracer.merge_convergence)
    sig = inspect.signature(session.InteractiveSession.render_until)
    assert list(sig.parameters)[1:] == ["threshold", "fraction", "max_frames", "check_every"]
    assert sig.parameters["fraction"].default == 0.95 and sig.parameters["check_every"].default == 8


def test_merge_convergence_rule():
    a = {"n_pixels": 10, "n_measured": 8, "n_above": 3, "sum_q16": 5 * 65536, "max_error": 0.5, "min_frames": 1,
         "max_frames": 9}
    b = {"n_pixels": 6, "n_measured": 6, "n_above": 0, "sum_q16": 65536, "max_error": 0.75, "min_frames": 4,
         "max_frames": 5}
    empty = {"n_pixels": 0, "n_measured": 0, "n_above": 0, "sum_q16": 0, "max_error": 0.0, "min_frames": 0,
             "max_frames": 0}
    m = tracer.merge_convergence([a, empty, b])
    assert m == {"n_pixels": 16, "n_measured": 14, "n_above": 3, "sum_q16": 6 * 65536, "max_error": 0.75,
                 "min_frames": 1, "max_frames": 9, "mean_error": 6 / 14}
    assert tracer.merge_convergence([empty, empty]) == dict(empty, mean_error=0.0)
    assert tracer.merge_convergence([]) == dict(empty, mean_error=0.0)


class _FakeTracer:
    """Converges once `converge_at` frames are rendered: n_above drops to `left_above`."""

    def __init__(self, converge_at, n_pixels=100, left_above=5):
        self.converge_at, self.n_pixels, self.left_above = converge_at, n_pixels, left_above
        self.frames, self.asked_at, self.enabled, self.thresholds = [], [], 0, []

    def enable_moments(self, on=True):
        self.enabled += 1 if on else 0

    def set_frame(self, *a):
        pass

    def render(self, first, n, *a):
        assert self.enabled, "render_until must enable the moments before the first frame"
        self.frames.append(first)

    def convergence(self, threshold):
        self.asked_at.append(len(self.frames))
        self.thresholds.append(threshold)
        done = len(self.frames) >= self.converge_at
        measured = self.n_pixels if len(self.frames) >= 2 else 0
        return {"n_pixels": self.n_pixels, "n_measured": measured, "n_above": self.left_above if done else measured,
                "sum_q16": 0, "max_error": 0.0, "min_frames": len(self.frames), "max_frames": len(self.frames),
                "mean_error": 0.0}


class _Cam:
    def uniforms(self):
        return None


def _session(pt):
    return session.InteractiveSession(pt, 4, 4, _Cam())


def test_render_until_stops_on_the_criterion():
    pt = _FakeTracer(converge_at=20)
    s = _session(pt)
    stats, frames = s.render_until(0.125, max_frames=1000)
    assert frames == 24 and pt.frames == list(range(24)) and s.frame_count == 24
    assert pt.asked_at == [8, 16, 24] and pt.thresholds == [0.125] * 3       # only every check_every frames
    assert stats["n_above"] == 5 and pt.enabled == 1
    # 5 of 100 above is within 1 - 0.95; 6 of 100 is not: the run goes on to max_frames
    pt = _FakeTracer(converge_at=0, left_above=6)
    stats, frames = _session(pt).render_until(0.125, max_frames=16)
    assert frames == 16 and pt.asked_at == [8, 16] and stats["n_above"] == 6
    # a looser fraction accepts it at the first check
    pt = _FakeTracer(converge_at=0, left_above=6)
    assert _session(pt).render_until(0.125, fraction=0.9)[1] == 8


def test_render_until_needs_every_pixel_measured():
    """At check_every = 1 the first check sees one frame: n_measured = 0 is no convergence,
    although n_above = 0 <= 0."""
    pt = _FakeTracer(converge_at=0, left_above=0)
    stats, frames = _session(pt).render_until(0.5, check_every=1)
    assert frames == 2 and pt.asked_at == [1, 2] and stats["n_measured"] == 100


def test_render_until_honours_max_frames_and_check_every():
    pt = _FakeTracer(converge_at=10**9)
    stats, frames = _session(pt).render_until(0.01, max_frames=20, check_every=6)
    assert frames == 20 and len(pt.frames) == 20
    assert pt.asked_at == [6, 12, 18, 20]            # every 6th frame, and once at the end for the result
    assert stats["n_above"] == stats["n_measured"] == 100
    pt = _FakeTracer(converge_at=10**9)
    assert _session(pt).render_until(0.01, max_frames=0) == (None, 0)
    assert pt.frames == [] and pt.asked_at == []
    # it continues the session's frame numbering
    pt = _FakeTracer(converge_at=0)
    s = _session(pt)
    s.frame_count = 5
    assert s.render_until(0.1, max_frames=3, check_every=3)[1] == 3 and pt.frames == [5, 6, 7]
