"""The ray-query entry points exist in include/pnrt.h, in the ctypes layer, in the
built libraries and in the Python classes, with one record layout; the host
library's pixel ray is the renderer's camera ray; decode_hits names the words of
a record.  No GPU needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from guides_common import bits, camera_rays, scene
from pnraytracing_amd import _native as N
from pnraytracing_amd import host as H
from pnraytracing_amd import session, tracer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "pnrt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)


def test_header_declares_the_entry_points():
    assert re.search(r"#define\s+PNRT_QUERY_CLOSEST\s+0\b", CODE) and re.search(r"#define\s+PNRT_QUERY_ANY\s+1\b", CODE)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+w\s*\[\s*16\s*\]\s*;\s*\}\s*pnrt_hit\s*;", CODE)
    assert re.search(r"int\s+pnrt_query_rays\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,"
                     r"\s*int\s+\w+\s*,\s*pnrt_hit\s*\*\s*\w+\s*\)", CODE)
    assert re.search(r"int\s+pnrt_query_rays_device\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*const\s+void\s*\*\s*\w+\s*,"
                     r"\s*int64_t\s+\w+\s*,\s*int\s+\w+\s*,\s*void\s*\*\s*\w+\s*\)", CODE)
    # the profile classes stay as they are: a query is timed as the primary class
    assert re.search(r"#define\s+PNRT_K_COUNT\s+7\b", CODE)
    assert (N.QUERY_CLOSEST, N.QUERY_ANY) == (0, 1)


def test_hit_record_is_64_bytes():
    assert ctypes.sizeof(N.Hit) == 64
    assert [(n, t) for n, t in N.Hit._fields_] == [("w", ctypes.c_uint32 * 16)]


def test_libraries_export_the_symbols_typed():
    lib = N.device_lib()
    P, F, INT, I64 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_int64
    want = {"pnrt_query_rays": (INT, [P, F, I64, INT, ctypes.POINTER(N.Hit)]),
            "pnrt_query_rays_device": (INT, [P, P, I64, INT, P])}
    for name, (res, args) in want.items():
        fn = getattr(lib, name)                      # AttributeError: the built library lacks the symbol
        assert fn.restype is res and list(fn.argtypes) == args, name
    fn = N.host_lib().pnrt_camera_pixel_ray
    assert fn.restype is INT and list(fn.argtypes) == [F, INT, INT, INT, INT, F]


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_query.h" in build.DEVICE_DEPS
    assert os.path.exists(os.path.join(build.CSRC, "pt_query.h"))


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.query_rays)
    assert list(sig.parameters)[1:] == ["rays", "any_hit"] and sig.parameters["any_hit"].default is False
    sig = inspect.signature(tracer.PathTracer.query_rays_device)
    assert list(sig.parameters)[1:] == ["rays_ptr", "n", "out_ptr", "any_hit"] and sig.parameters["any_hit"].default is False
    assert callable(tracer.decode_hits)
    assert list(inspect.signature(session.InteractiveSession.pick).parameters)[1:] == ["px", "py"]


@pytest.mark.parametrize("W,Hh", [(67, 45), (1, 1)])
def test_pixel_ray_is_the_renderers_camera_ray(W, Hh):
    """pnrt_camera_pixel_ray == CameraGetRay as the oracle's render loop calls it
    (guides_common.camera_rays restates it in float32 numpy), bit for bit, every pixel."""
    cfg = scene("c2", W, Hh)
    want = camera_rays(cfg)
    got = np.stack([H.camera_pixel_ray(cfg.camera, x, y, W, Hh) for y in range(Hh) for x in range(W)])
    assert got.shape == want.shape == (W * Hh, 7) and got.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(Exception):
        H.camera_pixel_ray(cfg.camera, 0, 0, 0, Hh)


def test_decode_hits_names_the_words():
    f = lambda x: int(np.float32(x).view(np.uint32))      # noqa: E731
    rec = np.zeros((3, 16), np.uint32)
    rec[0] = [1, f(1.5), f(-2.0), f(3.25), f(0.0), f(1.0), f(-0.0), f(0.25), f(0.75), 0xFFFFFFFF, 7, f(4.5), f(4.5), 42, 0, 0]
    rec[1, 12], rec[1, 13] = f(1e7), 0xFFFFFFFF           # a miss
    rec[2, 13], rec[2, 14] = 0xFFFFFFFF, 1                # an invalid ray
    d = tracer.decode_hits(rec)
    assert set(d) >= {"hit", "position", "normal", "uv", "texture_id", "material_id", "t", "triangle", "invalid"}
    assert d["hit"].tolist() == [True, False, False] and d["invalid"].tolist() == [False, False, True]
    assert d["position"][0].tolist() == [1.5, -2.0, 3.25] and d["normal"][0].tolist() == [0.0, 1.0, -0.0]
    assert np.signbit(d["normal"][0, 2]) and d["uv"][0].tolist() == [0.25, 0.75]
    assert d["texture_id"].tolist() == [-1, 0, 0] and d["material_id"].tolist() == [7, 0, 0]
    assert d["t"].tolist() == [4.5, 0.0, 0.0] and d["t_max"].tolist() == [4.5, 1e7, 0.0]
    assert d["triangle"].tolist() == [42, -1, -1]
    assert d["triangle"].dtype == np.int32 and d["material_id"].dtype == np.int32 and d["position"].dtype == np.float32
    one = tracer.decode_hits(rec[0])                       # one record: arrays of length 1
    assert one["triangle"].tolist() == [42] and one["position"].shape == (1, 3)


class _FakeTracer:
    def __init__(self):
        self.rays = None

    def query_rays(self, rays, any_hit=False):
        assert not any_hit
        self.rays = np.array(rays, np.float32)
        rec = np.zeros((1, 16), np.uint32)
        rec[0, 0], rec[0, 10], rec[0, 13] = 1, 3, 11
        return rec


class _Cam:
    def __init__(self, cam):
        self.cam = cam

    def uniforms(self):
        return self.cam


def test_pick_asks_for_the_pixels_camera_ray():
    cfg = scene("c2", 67, 45)
    pt = _FakeTracer()
    s = session.InteractiveSession(pt, 67, 45, _Cam(cfg.camera))
    rec = s.pick(13, 40)
    assert np.array_equal(bits(pt.rays.reshape(7)), bits(camera_rays(cfg)[40 * 67 + 13]))    # row 0 = bottom
    assert rec["hit"] and rec["material_id"] == 3 and rec["triangle"] == 11 and rec["position"].shape == (3,)
    for bad in ((67, 0), (0, 45), (-1, 0)):
        with pytest.raises(ValueError):
            s.pick(*bad)
