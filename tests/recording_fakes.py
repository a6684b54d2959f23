"""Two recording fakes for the Python layer (tests/test_python_layer_pins.py): a tracer that logs
what ``InteractiveSession`` asks of it, and a ``libpnrt.so`` stand-in that logs what ``PathTracer``
passes to the C ABI.  Arrays are logged as dtype, shape and the sha256 of their bytes."""
import ctypes
import hashlib
import inspect
import types

import numpy as np

from pnraytracing_amd import _native as N
from pnraytracing_amd import tracer

E_STATE = -3
_BYREF = type(ctypes.byref(ctypes.c_int()))
# the structs the library writes: logged as they come in, then filled
OUT_STRUCTS = (N.ConvergenceStats, N.AdaptiveStats, N.ReprojectStats, N.DeviceInfo, N.Profile, N.LumaHistogram)


def encode(v, hash_arrays=True):
    """A logged value as JSON takes it."""
    if v is None or isinstance(v, (str, bool, int, float)):
        return v
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return {"array": [str(a.dtype), list(a.shape)] + ([hashlib.sha256(a.tobytes()).hexdigest()] if hash_arrays else [])}
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, bytes):
        return v.decode()
    if isinstance(v, dict):
        return {str(k): encode(x, hash_arrays) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [encode(x, hash_arrays) for x in v]
    if isinstance(v, ctypes.Structure):
        return {type(v).__name__: {f: encode(getattr(v, f), hash_arrays) for f, *_ in v._fields_}}
    if isinstance(v, ctypes.Array):
        if len(v) <= 16 or isinstance(v[0], ctypes.Structure):
            return [encode(x, hash_arrays) for x in v]
        return encode(np.array(v), hash_arrays)
    if isinstance(v, _BYREF):
        return {"byref": encode(v._obj, hash_arrays)}
    if isinstance(v, ctypes.c_void_p):
        return {"void_p": v.value or 0}
    if isinstance(v, ctypes._SimpleCData):
        return {type(v).__name__: v.value}
    if isinstance(v, ctypes._Pointer):
        return "set" if v else "NULL"
    return getattr(v, "__name__", None) or type(v).__name__      # (a stand-in class or object of the tests)


def outcome(fn, hash_arrays=True):
    """What a call came to: its value, or the exception's type and text."""
    try:
        return {"returns": encode(fn(), hash_arrays)}
    except Exception as e:               # every refusal is part of the record
        return {"raises": [type(e).__name__, str(e)]}


def _state_error(fn, msg):
    e = tracer.PnrtError(f"pnrt_{fn} failed ({E_STATE}): {fn}: {msg}")
    e.code = E_STATE
    return e


STALE = ("the guide images are stale (camera, size, scene, materials, textures, environment or traversal mode changed): "
         "render_guides again")


class FakeCamera:
    """Uniforms that ``rotate`` changes, and the two fields of the controller's state ``focus_on`` reads."""

    def __init__(self):
        self.turn = 0

    def rotate(self, dx=1.0, dy=0.0):
        self.turn += 1
        return True

    def uniforms(self):
        return np.array([[0.25 * self.turn, 2.8, 7.0], [-1.0, 1.8, 5.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0]], np.float32)

    @property
    def state(self):
        return types.SimpleNamespace(eye=tuple(self.uniforms()[0]), w=(0.0, 0.0, 1.0))


class RecordingTracer:
    """A tracer that logs every call with its arguments as they were spelled -- [name, positional, keyword]: the
    suite has tracers and wrappers that take exactly the session's spelling -- after binding them to ``PathTracer``'s
    own signature, so that a call the real tracer would not take fails here too.

    ``converge_at``: the adaptive calls report no active pixel from that first frame on (None: never).
    ``convergence_script``: what successive ``convergence`` calls report as ``n_above``.
    ``guides``: "none", "valid" or "stale", as the library would judge the guide images; ``moments``: "ok",
    "never" or "uncovered" -- ``denoise`` and ``denoise_variance`` raise the library's PNRT_E_STATE texts."""

    def __init__(self, converge_at=None, convergence_script=(), guides="none", moments="ok"):
        self.log = []
        self.converge_at, self.convergence_script = converge_at, list(convergence_script)
        self.guides, self.moments = guides, moments
        self.n_ray_sets = 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        sig = inspect.signature(getattr(tracer.PathTracer, name))

        def call(*args, **kwargs):
            bound = sig.bind(None, *args, **kwargs)
            bound.apply_defaults()
            a = dict(list(bound.arguments.items())[1:])
            self.log.append([name, encode(args), encode(kwargs)])
            return getattr(self, "_" + name, lambda a: None)(a)
        return call

    def _adaptive(self, a):
        n_active = 0 if (self.converge_at is not None and a["first"] >= self.converge_at) else 64
        return {"n_pixels": 64, "n_active_pixels": n_active, "n_tiles": 1, "n_active_tiles": int(n_active > 0),
                "frames_per_batch": a["n"], "n_batches": 1}

    _render_adaptive = _render_rays_adaptive = _adaptive

    def _make_rays(self, a):
        self.n_ray_sets += 1
        return f"rays#{self.n_ray_sets}"

    def _cameras_batch_plan(self, a):
        return {"frames_per_batch": min(a["n_frames"], 2), "n_batches": (a["n_frames"] + 1) // 2, "batch_bytes": 4096}

    def _convergence(self, a):
        above = self.convergence_script.pop(0) if self.convergence_script else 0
        return {"n_pixels": 64, "n_measured": 64, "n_above": above, "sum_q16": 65536, "max_error": 0.5, "min_frames": 2,
                "max_frames": 9, "mean_error": 1 / 64}

    def _guides_made(self, a):
        self.guides = "valid"

    _render_guides = _render_guides_rays = _guides_made

    def _reproject(self, a):
        self.guides = "valid"
        return {"n_pixels": 64, "n_reprojected": 40, "n_disoccluded": 20, "n_missed": 4, "sum_frames": 80, "max_frames": 2}

    _reproject_view = _reproject

    def _filter(self, fn):
        if fn == "denoise_variance" and self.moments == "never":
            raise _state_error(fn, "the sample moments were never enabled (pnrt_enable_moments(ctx, 1) before the frames are "
                                   "rendered)")
        if fn == "denoise_variance" and self.moments == "uncovered":
            raise _state_error(fn, "frames were rendered while the moments were disabled, so they do not cover the accumulation "
                                   "(pnrt_reset_accum first)")
        if self.guides != "valid":
            raise _state_error(fn, "render_guides first" if self.guides == "none" else STALE)

    def _denoise(self, a):
        self._filter("denoise")

    def _denoise_variance(self, a):
        self._filter("denoise_variance")

    def _define_model(self, a):
        return 0

    def _query_rays(self, a):
        rec = np.zeros((1, 16), np.uint32)
        rec[0, 0] = 1
        rec.view(np.float32)[0, 1:4] = (0.5, 2.0, 1.0)
        rec.view(np.int32)[0, 10] = 3
        return rec

    def _luma_histogram(self, a):
        bins = np.zeros(N.LUMA_BINS, np.int64)
        bins[240:260] = 3
        return {"n_pixels": 64, "n_counted": 60, "bins": bins}

    def _read_display(self, a):
        return np.full((8, 8, 4), 7, np.uint8)


class FakeTensor:
    """What ``PathTracer`` asks of a torch tensor, without a device."""

    def __init__(self, ptr=0x7000, cuda=True, contiguous=True, itemsize=4, numel=16):
        self.is_cuda, self.dtype = cuda, types.SimpleNamespace(itemsize=itemsize)
        self._ptr, self._contiguous, self._numel = ptr, contiguous, numel
        self.__name__ = f"FakeTensor({ptr:#x}, cuda={cuda}, contiguous={contiguous}, itemsize={itemsize}, numel={numel})"

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return self._contiguous

    def numel(self):
        return self._numel


class RecordingLib:
    """``libpnrt.so`` as ``PathTracer`` sees it: every ``pnrt_*`` attribute logs (name, args) -- by-reference structs
    expanded to their fields, data pointers as "NULL" or "set" --, fills the out-parameters with fixed values and
    returns 0."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        if not name.startswith("pnrt_"):
            raise AttributeError(name)

        def call(*args):
            self.log.append([name, ["NULL" if a is None else encode(a) for a in args]])
            for a in args:
                if isinstance(a, _BYREF):
                    self._fill(a._obj)
            return b"pnrt-fake 0.0 (none) src 0" if name == "pnrt_version" else 0
        call.__name__ = name                     # (as a ctypes function has it)
        return call

    @staticmethod
    def _fill(obj):
        if isinstance(obj, ctypes._SimpleCData):
            obj.value = 3
        elif isinstance(obj, OUT_STRUCTS):
            for k, (f, t) in enumerate(obj._fields_):
                if issubclass(t, ctypes.Array):
                    getattr(obj, f)[:] = [k + 2 + i for i in range(t._length_)]
                else:
                    setattr(obj, f, k + 2)


def recording_path_tracer(width=8, height=8):
    """A ``PathTracer`` over a ``RecordingLib``; no library is loaded and no context made."""
    pt = tracer.PathTracer.__new__(tracer.PathTracer)
    pt._lib, pt._ctx, pt._device, pt._stream = RecordingLib(), ctypes.c_void_p(0x1234), 0, 0
    pt.width, pt.height = width, height
    return pt
