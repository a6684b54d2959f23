"""The Python layer pinned call for call: what ``InteractiveSession`` asks of its tracer over the grid of camera
model x lens x pixel counts x entry point, what ``PathTracer`` passes to the C ABI for every public method and
every documented refusal, and every public signature and docstring of the layer (no GPU needed; the session
grid and the tracer log load no device library but for ``show(auto_exposure=True)``'s host-side exposure).

The golden files under tests/golden/ were recorded with the ``session.py`` and ``tracer.py`` of the commit before
DESIGN.md 35 (``python tests/test_python_layer_pins.py DIR`` writes what this tree records into DIR).  They say
what the layer did before it was folded and are not to be written again from the code under test.  To stay
small they hold every repeated item once, in a table (``_pack``), one item and one case (of the session: one
combination of the grid) to a line."""
import hashlib
import inspect
import itertools
import json
import os
import sys

import numpy as np

from recording_fakes import FakeCamera, FakeTensor, RecordingTracer, encode, outcome, recording_path_tracer

from pnraytracing_amd import dist, session, tracer

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the session grid -------------------------------------------------------------------------------------------
MODELS = {"none": None, "pinhole": ("pinhole",), "pinhole_per_pixel": ("pinhole", 180.0, True),
          "fisheye200": ("fisheye", 200.0), "equirect": ("equirect",), "ortho": ("ortho",)}
LENSES = {"none": None, "aa": ((1.0,), {}), "aa_lens": ((1.0, 0.1), {"focus_distance": 3.0})}
COUNTS = ("equal", "differ")
VERTS = np.arange(30, dtype=np.float32).reshape(2, 15)


class _Mesh:
    positions = np.arange(9, dtype=np.float32)
    normals = None
    texcoords = np.arange(6, dtype=np.float32)


def _rendered(s):
    """Two frames and a camera move: what a reprojection needs."""
    s.frame()
    s.frame()
    s.camera.rotate()


def _preview(s, fn):
    """Fresh guides, the same again, stale guides (the library's word), then a camera change."""
    out = [outcome(lambda: fn(levels=3)), outcome(fn)]
    s.pt.guides = "stale"
    out.append(outcome(fn))
    s.camera.rotate()
    out.append(outcome(fn))
    return out


ENTRIES = {
    "frame": lambda s: [outcome(s.frame), outcome(s.frame)],
    "frame_redraw": lambda s: [outcome(lambda: s.frame(True)), outcome(lambda: s.frame_counted(2))],
    "frame_shard": lambda s: [outcome(lambda: s.frame(band=4, n_shards=3, shard=1))],
    "frame_counted": lambda s: [outcome(lambda: s.frame_counted(3)), outcome(s.frame_counted)],
    "adaptive_until_converges": lambda s: [outcome(lambda: s.render_adaptive_until(0.25, max_frames=7, frames_per_call=3,
                                                                                    min_frames=3))],
    "adaptive_until_never": lambda s: [outcome(lambda: s.render_adaptive_until(0.25, max_frames=7, frames_per_call=3,
                                                                                min_frames=3))],
    "render_until": lambda s: [outcome(lambda: s.render_until(0.05, fraction=0.9, max_frames=6, check_every=3))],
    "render_until_capped": lambda s: [outcome(lambda: s.render_until(0.05, max_frames=3, check_every=4))],
    "reproject_nothing_rendered": lambda s: [outcome(s.reproject), outcome(s.reproject_view)],
    "reproject": lambda s: [_rendered(s), outcome(lambda: s.reproject(max_history=8)), outcome(s.frame_counted)],
    "reproject_view": lambda s: [_rendered(s), outcome(lambda: s.reproject_view(max_history=8)), outcome(s.preview),
                                 outcome(s.frame_counted), s.camera.rotate(), outcome(s.reproject_view)],
    "reproject_view_to_fisheye": lambda s: [_rendered(s), outcome(lambda: s.set_camera_model("fisheye", 150.0)),
                                            outcome(s.reproject_view), outcome(lambda: s.frame_counted(2)), outcome(s.preview)],
    "reproject_view_to_pinhole": lambda s: [_rendered(s), outcome(lambda: s.set_camera_model("pinhole")),
                                            outcome(s.reproject_view), outcome(lambda: s.frame_counted(2)), outcome(s.preview)],
    "preview": lambda s: _preview(s, s.preview),
    "preview_variance": lambda s: _preview(s, s.preview_variance),
    "preview_variance_moments_never": lambda s: [outcome(s.preview_variance)],
    "preview_variance_moments_uncovered": lambda s: [outcome(lambda: s.preview_variance(levels=2))],
    "edit_vertices": lambda s: [outcome(lambda: s.edit_vertices(5, VERTS, lights=np.ones((1, 3), np.float32)))],
    "move_model": lambda s: [outcome(lambda: s.define_model(4, _Mesh)),
                             outcome(lambda: s.move_model(0, [(0, 0.0, (1.0, 2.0, 3.0))], relight=True))],
    "pick": lambda s: [outcome(lambda: s.pick(3, 4)), outcome(lambda: s.pick(8, 0))],
    "focus_on": lambda s: [outcome(lambda: s.focus_on(3, 4)), outcome(s.frame), outcome(lambda: s.set_lens(1.0, 0.2)),
                           outcome(s.frame)],
    "show": lambda s: [outcome(lambda: s.show(auto_exposure=True)), outcome(lambda: s.show(denoised=True, tone="aces"))],
}
FAKES = {"adaptive_until_converges": {"converge_at": 5}, "render_until": {"convergence_script": (30, 5)},
         "preview_variance_moments_never": {"moments": "never"}, "preview_variance_moments_uncovered": {"moments": "uncovered"}}


def _setup(s, model, lens, counts):
    """The camera model, then the lens; ``differ``: two frames under another model first, then ``reproject_view()``
    into this one (without a model the session has two pinhole views and the counts stay equal).  The first
    refusal ends the set-up."""
    steps = []
    if counts == "differ":
        if MODELS[model] is not None:
            steps.append(lambda: s.set_camera_model("equirect" if model == "fisheye200" else "fisheye", 150.0))
        steps.append(lambda: s.frame_counted(2))
    if MODELS[model] is not None:
        steps.append(lambda: s.set_camera_model(*MODELS[model]))
    if LENSES[lens] is not None:
        steps.append(lambda: s.set_lens(*LENSES[lens][0], **LENSES[lens][1]))
    if counts == "differ":
        steps += [s.camera.rotate, s.reproject_view]
    out = []
    for step in steps:
        out.append(outcome(step))
        if "raises" in out[-1]:
            return out, False
    return out, True


def _state(s):
    return {"frame_count": s.frame_count, "lens": encode(s._lens)}


def record_session():
    """{"model/lens/counts": the set-up's outcomes, calls and state, and "entries": {entry: {"results", "calls",
    "state"} after it}}; a refused set-up has no entries."""
    rec = {}
    for model, lens, counts in itertools.product(MODELS, LENSES, COUNTS):
        for entry, run in ENTRIES.items():
            pt = RecordingTracer(**FAKES.get(entry, {}))
            s = session.InteractiveSession(pt, 8, 8, FakeCamera(), max_bounce_depth=3)
            setup, ok = _setup(s, model, lens, counts)
            before = {"setup": setup, "calls": list(pt.log), "state": _state(s)}
            combo = rec.setdefault(f"{model}/{lens}/{counts}", {**before, "entries": {}})
            assert {k: v for k, v in combo.items() if k != "entries"} == before      # the same set-up for every entry
            if not ok:
                break
            del pt.log[:]
            results = [r for r in run(s) if isinstance(r, dict)]
            combo["entries"][entry] = {"results": results, "calls": pt.log, "state": _state(s)}
    # the refusals of the setters in the other order, and the lens kept by focus_on
    s = session.InteractiveSession(RecordingTracer(), 8, 8, FakeCamera())
    rec["setters"] = [outcome(lambda: s.set_lens(1.0, 0.1)), outcome(lambda: s.set_lens(1.0, 0.1, 2.0)),
                      outcome(lambda: s.set_camera_model("fisheye")), outcome(lambda: s.set_camera_model(3)),
                      outcome(lambda: s.set_camera_model("wide")), outcome(lambda: s.set_camera_model(9)),
                      outcome(lambda: s.set_lens(2.0)),
                      outcome(lambda: s.set_camera_model(2, 90.0, per_pixel=1)), encode(s._model), encode(s._lens),
                      outcome(lambda: s.set_lens(1.0, 0.5)), outcome(lambda: s.render_until(0.1, check_every=0)),
                      outcome(lambda: s.render_adaptive_until(0.1, frames_per_call=0))]
    return _interned(rec)


def _interned(rec):
    """The same with every array description written once, in ``rec["arrays"]``, and "@k" where it stood."""
    table = []

    def walk(v):
        if isinstance(v, dict) and list(v) == ["array"]:
            if v["array"] not in table:
                table.append(v["array"])
            return f"@{table.index(v['array'])}"
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        return [walk(x) for x in v] if isinstance(v, list) else v
    rec = walk(rec)
    rec["arrays"] = table
    return rec


# ---- the tracer log ---------------------------------------------------------------------------------------------
CAM = np.arange(12, dtype=np.float32).reshape(4, 3)
RAYS = 0x4000
U32, I64 = (-1, 0, 2 ** 32 - 1, 2 ** 32), (-2 ** 63 - 1, -2 ** 63, 2 ** 63 - 1, 2 ** 63)


class _Packed:
    lights_sum_area = 2.5

    @staticmethod
    def arrays():
        return [np.arange(n, dtype=np.float64).reshape(-1, w) for n, w in ((30, 15), (18, 18), (6, 3), (24, 12), (3, 3))]


class _Cfg:
    packed, textures, env_rgb, env_table = _Packed, [(np.zeros(12, np.uint8), 2, 2, 3)], None, None
    width, height, camera, max_depth = 8, 8, CAM, 3


def _f32(*shape):
    return np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)


# one call of every public method with ordinary arguments: (method, args, kwargs)
ORDINARY = [
    ("upload_scene", (_Packed,), {}), ("update_materials", (2, _f32(2, 18)), {}),
    ("update_vertices", (1, _f32(2, 15)), {}), ("update_vertices", (1, _f32(2, 15)), {"lights": _f32(2, 3)}),
    ("update_vertices", (0, _f32(0, 15)), {"lights": _f32(0, 3), "lights_sum_area": 1.5}),
    ("update_vertices_device", (1, 2, 0x5000), {}), ("update_vertices_device", (1, 2, None), {"lights": _f32(1, 3)}),
    ("define_model", (3, _f32(2, 8)), {}), ("define_model", (3, _f32(0, 8)), {}), ("define_model", (3, FakeTensor()), {}),
    ("place_models", ([(0, _f32(16)), (2, _f32(4, 4))],), {"relight": True}), ("place_models", ([],), {}),
    ("read_vertices", (1, 2), {}), ("read_vertices", (1, 0), {}), ("read_bvh_boxes", (_f32(3, 12),), {}),
    ("upload_texture", (0, np.zeros((2, 2, 3), np.uint8), 2, 2, 3), {}), ("upload_env", (None, None), {}),
    ("upload_env", (_f32(2, 4, 3), _f32(2, 4, 3)), {}), ("upload_env_build", (_f32(2, 4, 3),), {}), ("read_env_table", (), {}),
    ("build_bvh", (_f32(2, 9),), {}), ("set_frame", (8, 8, CAM), {}), ("set_frame", (5, 3, CAM.reshape(12), 2), {}),
    ("set_options", (tracer.TRAVERSE_ZCULL | tracer.SERIAL,), {}), ("stream_handle", (), {}), ("set_stream", (0x9000,), {}),
    ("current_stream_handle", (), {}), ("set_stream", (None,), {}), ("current_stream_handle", (), {}), ("load", (_Cfg,), {}),
    ("render", (0, 4), {}), ("render", (5, 1, 8, 2, 1), {}), ("batch_plan", (4,), {}), ("batch_plan", (4, 8, 2, 1), {}),
    ("render_cameras", (2, _f32(3, 12)), {}), ("render_cameras", (2, _f32(2, 4, 3), 8, 2, 1), {}),
    ("render_cameras", (2, _f32(0, 12)), {}), ("cameras_batch_plan", (3,), {}), ("cameras_batch_plan", (3, 8, 2, 1), {}),
    ("render_rays", (0, 2, RAYS), {}), ("render_rays", (1, 2, FakeTensor(), 64, 8, 2, 1), {}), ("render_rays", (0, 1, None), {}),
    ("render_guides_rays", (RAYS,), {}), ("render_guides_rays", (None,), {}),
    ("ray_camera", ("fisheye", CAM), {"fov_deg": 200.0, "aa_width": 1.0, "per_pixel": True}), ("ray_camera", (1, CAM + 1), {}),
    ("make_rays", ("equirect", CAM), {"out": RAYS}),
    ("make_rays", ("pinhole", CAM, 3, 2), {"out": FakeTensor(), "aa_width": 1.0, "lens_radius": 0.1, "focus_distance": 3.0}),
    ("make_rays", (2, CAM, 0, 2, 100), {"out": RAYS, "fov_deg": 90.0}),
    ("reset_accum", (), {}), ("synchronize", (), {}), ("read_accum", (), {}), ("accum_ptr", (), {}),
    ("render_guides", (), {}), ("read_aov", ("normal",), {}), ("read_aov", (2,), {}), ("aov_ptr", ("albedo",), {}),
    ("denoise", (), {}), ("denoise", (3,), {}), ("denoise", (), {"sigma_normal": 0.5}),
    ("denoise", (2, 1.0, 0.125, 0.25), {}), ("denoise_variance", (), {}), ("denoise_variance", (), {"sigma_variance": 2.0}),
    ("denoise_variance", (4,), {"sigma_position": 1.0}), ("read_denoised", (), {}), ("denoised_ptr", (), {}),
    ("display", (), {}), ("display", ("denoised", "reinhard", "srgb", 2.0, 8.0, True), {}),
    ("display", ("external",), {"tone": 2, "src_ptr": 0x6000}), ("read_display", (), {}), ("display_ptr", (), {}),
    ("luma_histogram", (), {}), ("luma_histogram", ("external", 8, 2, 1), {"src_ptr": 0x6000}),
    ("query_rays", (_f32(2, 7),), {}), ("query_rays", (_f32(0, 7),), {"any_hit": True}),
    ("query_rays_device", (0x5000, 2, 0x6000), {}), ("query_rays_device", (0x5000, 2, 0x6000, True), {}),
    ("enable_moments", (), {}), ("enable_moments", (False,), {}), ("read_moments", (), {}), ("read_error", (), {}),
    ("moments_ptr", (), {}), ("convergence", (0.05,), {}), ("convergence", (0.05, 8, 2, 1), {}),
    ("render_adaptive", (2, 3, 0.05), {}), ("render_adaptive", (2, 3, 0.0, 0xFFFFFFFF, 8, 2, 1), {}),
    ("render_rays_adaptive", (2, 3, RAYS, 64, 0.05), {}), ("render_rays_adaptive", (2, 3, FakeTensor(), 0, 0.0, 0xFFFFFFFF, 8, 2, 1), {}),
    ("render_rays_adaptive", (2, 3, None, 0, 0.05), {}),
    ("reproject", (CAM,), {}), ("reproject", (CAM,), {"max_history": 8}), ("reproject", (CAM, 0.5), {}),
    ("reproject", (CAM, 0.5, 0.125, 0), {}), ("reproject_view", (("fisheye", CAM, 200.0), ("pinhole", CAM + 1, 180.0)), {}),
    ("reproject_view", (("ortho", CAM), tracer.PathTracer.ray_camera("equirect", CAM)), {"position_tolerance": 0.5}),
    ("reproject_view", ((0, CAM, 90.0), (3, CAM, 120.0), 0.5, 0.25, 2 ** 32 - 1), {}),
    ("pack_rows", (0x5000, 8, 2, 1), {}), ("unpack_rows", (0x5000, 0x6000, 8, 2, 1), {}), ("device_info", (), {}),
    ("profile_enable", (), {}), ("profile_select", (), {}), ("profile_select", (["trace", "shade"],), {}), ("profile_read", (), {}),
    ("version", (), {}), ("debug_math", (1, _f32(3)), {}), ("debug_math", (2, _f32(3), _f32(3)), {}),
    ("__enter__", (), {}), ("__exit__", (None, None, None), {}), ("close", (), {}),
]


def _bounds():
    """Every uint32 and int64 argument at both sides of both bounds."""
    ok = {"render": (0, 1), "batch_plan": (1,), "render_cameras": (0, _f32(1, 12)), "cameras_batch_plan": (1,),
          "render_rays": (0, 1, RAYS, 0), "make_rays": ("pinhole", CAM, 0, 1), "render_adaptive": (0, 1, 0.05, 8),
          "render_rays_adaptive": (0, 1, RAYS, 0, 0.05, 8)}
    u32 = {"render": (0, 1), "batch_plan": (0,), "render_cameras": (0,), "cameras_batch_plan": (0,), "render_rays": (0, 1),
           "make_rays": (2, 3), "render_adaptive": (0, 1, 3), "render_rays_adaptive": (0, 1, 5)}
    i64 = {"render_rays": (3,), "render_rays_adaptive": (3,)}
    for places, values in ((u32, U32), (i64, I64)):
        for name, where in places.items():
            for k, v in itertools.product(where, values):
                args = list(ok[name])
                args[k] = v
                yield name, tuple(args), ({"out": RAYS} if name == "make_rays" else {})
    for name, views in (("reproject", (CAM,)), ("reproject_view", (("ortho", CAM), ("pinhole", CAM)))):
        for v in U32:
            yield name, views, {"max_history": v}


REFUSALS = list(_bounds()) + [
    ("render_cameras", (0, _f32(2, 12).astype(np.float64)), {}), ("render_cameras", (0, _f32(2, 11)), {}),
    ("render_cameras", (0, _f32(24)), {}), ("render_cameras", (0, _f32(2, 3, 4)), {}),
    ("render_rays", (0, 1, FakeTensor(cuda=False)), {}), ("render_rays", (0, 1, FakeTensor(contiguous=False)), {}),
    ("render_rays", (0, 1, [1.0, 2.0]), {}), ("render_guides_rays", (FakeTensor(cuda=False),), {}),
    ("render_rays_adaptive", (0, 1, FakeTensor(contiguous=False), 0, 0.05), {}), ("render_rays_adaptive", (0, 1, 1.5, 0, 0.05), {}),
    ("make_rays", ("pinhole", CAM), {"out": FakeTensor(cuda=False)}), ("make_rays", ("wide", CAM), {"out": RAYS}),
    ("ray_camera", ("wide", CAM), {}), ("reproject_view", (("wide", CAM), ("pinhole", CAM)), {}),
    ("read_aov", ("depth",), {}), ("aov_ptr", ("depth",), {}), ("display", ("screen",), {}), ("display", (), {"tone": "filmic"}),
    ("display", (), {"transfer": "gamma"}), ("luma_histogram", ("screen",), {}),
    ("define_model", (0, FakeTensor(itemsize=2)), {}), ("define_model", (0, FakeTensor(contiguous=False)), {}),
    ("define_model", (0, FakeTensor(numel=12)), {}),
]


def record_tracer():
    """[{"call", "returns" | "raises", "c": the C calls it made}]: one recording ``PathTracer`` per group, the
    ordinary calls in one sequence (``read_env_table`` and the stream handle read what earlier calls left).  The
    refusals run a second time on a tracer without a library: what is refused is refused before the library is
    touched, and what is accepted fails there on the missing ``_lib``."""
    rec = []
    for group, bare in ((ORDINARY, False), (REFUSALS, False), (REFUSALS, True)):
        pt = recording_path_tracer()
        log = pt._lib.log
        if bare:
            del pt._lib
            pt._ctx = None
        for name, args, kwargs in group:
            n = len(log)
            r = outcome(lambda: getattr(pt, name)(*args, **kwargs), hash_arrays=False)
            if name == "__enter__":
                r = {"returns": "self" if r.get("returns") == "PathTracer" else r}
            rec.append({"call": [name, encode(args), encode(kwargs)], **r, "c": log[n:], "size": [pt.width, pt.height]})
    return rec


# ---- signatures and docstrings --------------------------------------------------------------------------------
def _described(obj):
    doc = inspect.getdoc(obj)
    return {"signature": str(inspect.signature(obj)), "doc": None if doc is None else hashlib.sha256(doc.encode()).hexdigest()[:16]}


def record_signatures():
    rec = {}
    for cls in (tracer.PathTracer, session.InteractiveSession, session.CameraController, dist.ShardedFrame):
        names = [n for n in vars(cls) if not n.startswith("_") or n in ("__init__", "__enter__", "__exit__", "__del__")]
        for n in sorted(names):
            attr = inspect.getattr_static(cls, n)
            kind = type(attr).__name__ if isinstance(attr, (staticmethod, classmethod, property)) else "method"
            fn = getattr(cls, n)
            rec[f"{cls.__module__.rsplit('.', 1)[-1]}.{cls.__name__}.{n}"] = {"kind": kind, **_described(fn)} if callable(fn) \
                else {"kind": "value", "value": encode(fn)}
        rec[f"{cls.__module__.rsplit('.', 1)[-1]}.{cls.__name__}"] = {"doc": cls.__doc__ and hashlib.sha256(
            inspect.getdoc(cls).encode()).hexdigest()[:16], "bases": [b.__name__ for b in cls.__bases__]}
    for n, fn in sorted(vars(tracer).items()):
        if inspect.isfunction(fn) and fn.__module__ == tracer.__name__ and not n.startswith("_"):
            rec[f"tracer.{n}"] = {"kind": "function", **_described(fn)}
    rec["tracer.constants"] = {n: encode(v) for n, v in sorted(vars(tracer).items())
                               if n.isupper() and isinstance(v, (int, dict, tuple))}
    rec["tracer.PnrtError"] = [b.__name__ for b in tracer.PnrtError.__mro__]
    return rec


RECORDERS = {"session_calls.json": record_session, "tracer_calls.json": record_tracer, "python_signatures.json": record_signatures}


def _json(rec):
    return json.loads(json.dumps(rec))           # tuples become lists, as in the file


# ---- the tests ------------------------------------------------------------------------------------------------------
PACKED = ("calls", "results", "setup", "c")      # lists whose items repeat from case to case: written once, in a table
ENTRY = ("results", "calls", "state")            # an entry of the session grid: written as a list of the three
PACKED_WHOLE = ("state", "size", "call", "returns", "raises")    # ... and values that do


def _pack(rec):
    """{"table": the distinct items of the ``PACKED`` lists, "cases": ``rec`` with their table numbers in their place}"""
    table, number = [], {}

    def walk(v, key=None):
        if key in PACKED_WHOLE:
            return number.setdefault(json.dumps(v), len(number))
        if isinstance(v, dict) and list(v) == list(ENTRY):
            return [walk(x, k) for k, x in v.items()]
        if isinstance(v, dict):
            return {k: walk(x, k) for k, x in v.items()}
        if isinstance(v, list) and key in PACKED:
            return [number.setdefault(json.dumps(x), len(number)) for x in v]
        return [walk(x) for x in v] if isinstance(v, list) else v
    cases = walk(rec)
    table = [json.loads(text) for text in number]
    return {"table": table, "cases": cases}


def _unpack(packed):
    def walk(v, key=None):
        if key in PACKED_WHOLE:
            return packed["table"][v]
        if isinstance(v, dict):
            return {k: dict(zip(ENTRY, (walk(y, e) for e, y in zip(ENTRY, x)))) if key == "entries" else walk(x, k) for k, x in v.items()}
        if isinstance(v, list):
            return [packed["table"][x] for x in v] if key in PACKED else [walk(x) for x in v]
        return v
    return walk(packed["cases"])


def _write(rec, path):
    """One table item and one case to a line, so that a change of a golden file reads as a diff of cases."""
    packed = _pack(_json(rec))
    line = lambda v: json.dumps(v, separators=(",", ":"))
    cases = packed["cases"]
    items = [f"{line(k)}:{line(v)}" for k, v in cases.items()] if isinstance(cases, dict) else [line(v) for v in cases]
    opening, closing = ("{", "}") if isinstance(cases, dict) else ("[", "]")
    with open(path, "w") as f:
        f.write('{"table":[\n' + ",\n".join(line(v) for v in packed["table"]) + '\n],\n"cases":' + opening + "\n"
                + ",\n".join(items) + "\n" + closing + "}\n")


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return _unpack(json.load(f))


def _compare(got, want, what):
    """Everything recorded, item by item, so that a failure names the case."""
    assert list(got) == list(want) if isinstance(want, dict) else len(got) == len(want), f"{what}: other cases than the golden's"
    for k in (want if isinstance(want, dict) else range(len(want))):
        assert got[k] == want[k], f"{what}[{k!r}]"


def test_session_calls_are_the_parents():
    got, want = _json(record_session()), _golden("session_calls.json")
    refused = 3 * len(COUNTS)                    # a lens radius with the fisheye, equirect and ortho models
    combos = len(MODELS) * len(LENSES) * len(COUNTS)
    assert len(want) == combos + 2               # and the setters, and the arrays
    grid = [v for k, v in want.items() if "/" in k]
    assert sorted(len(v["entries"]) for v in grid) == [0] * refused + [len(ENTRIES)] * (combos - refused)
    assert all(any("raises" in r for r in v["setup"]) != bool(v["entries"]) for v in grid)
    for k in want:                               # case by case, so that a failure names it
        if "/" in k:
            _compare(got[k].pop("entries"), want[k].pop("entries"), f"session[{k!r}]")
    _compare(got, want, "session")


def test_tracer_calls_are_the_parents():
    got, want = _json(record_tracer()), _golden("tracer_calls.json")
    assert len(want) == len(ORDINARY) + 2 * len(REFUSALS)
    _compare(got, want, "tracer")


def test_signatures_and_docstrings_are_the_parents():
    _compare(_json(record_signatures()), _golden("python_signatures.json"), "signature")


def test_every_public_tracer_method_is_called():
    called = {name for name, _, _ in ORDINARY}
    public = {n for n, v in vars(tracer.PathTracer).items() if callable(getattr(tracer.PathTracer, n)) and not n.startswith("_")}
    assert public <= called, sorted(public - called)
    golden = _golden("tracer_calls.json")
    assert not any("raises" in r for r in golden[:len(ORDINARY)])
    # a refusal comes before any C call; of the four values at a bound's two sides, two are accepted
    refused, bare = golden[len(ORDINARY):][:len(REFUSALS)], golden[len(ORDINARY) + len(REFUSALS):]
    assert all(("raises" in r) != bool(r["c"]) for r in refused)
    assert sum("raises" in r for r in refused) == len(REFUSALS) - len(list(_bounds())) // 2
    assert all("raises" in b and not b["c"] for b in bare)


def test_the_grid_reaches_every_arm():
    """The grid is only worth its size if every tracer call the session can make is in it."""
    made = {c[0] for combo in _golden("session_calls.json").values() if isinstance(combo, dict)
            for case in (combo, *combo["entries"].values()) for c in case["calls"]}
    assert len(_golden("session_calls.json")["arrays"]) > 20
    assert made >= {"render", "render_cameras", "render_rays", "render_adaptive", "render_rays_adaptive", "make_rays",
                    "cameras_batch_plan", "reproject", "reproject_view", "render_guides", "render_guides_rays", "denoise",
                    "denoise_variance", "convergence", "enable_moments", "set_frame", "update_vertices", "define_model",
                    "place_models", "query_rays", "luma_histogram", "display", "read_display"}


if __name__ == "__main__":
    os.makedirs(sys.argv[1], exist_ok=True)
    for fname, record in RECORDERS.items():
        _write(record(), os.path.join(sys.argv[1], fname))
