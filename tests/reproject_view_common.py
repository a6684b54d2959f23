"""Shared by tests/test_reproject_view_ref.py and tests/test_gpu_reproject_view.py -- TEST
INFRASTRUCTURE: the views of the pnrt_reproject_view tests (a camera model over the cameras
and moves of reproject_common), the guide images of a view's centre rays from the CPU
oracle, the replay of every case through tests/reproject_view_ref.py, and the statistics
recorded per case."""
from __future__ import annotations

import functools

import numpy as np

import pyoracle
import rays_ref as R
import reproject_common as C
import reproject_view_ref as VR
from guides_common import scene
from pnraytracing_amd import host as H
from pnraytracing_amd.session import CameraController

F = np.float32
W, Hh = C.W, C.H
FLOAT_MAX = F(10000000.0)
MODELS = R.MODELS
FISHEYE_FOVS = (60.0, 200.0, 360.0)                  # the round trip's


def oblique(w: int, h: int) -> np.ndarray:
    """A camera off every axis, with a tilted up vector."""
    return np.asarray(H.camera_update((1.5, 3.1, 6.0), (0.2, 2.5, -0.4), (0.1, 1.0, 0.05), 50.0, F(w) / F(h)), F).reshape(4, 3)


@functools.lru_cache(maxsize=None)
def _seam(which: str, w: int, h: int):
    """Inside the Cornell box, looking out of its open front: the seam of an equirectangular view
    (the direction -f) faces the back wall.  seam_b: the same after a small rotate."""
    c = CameraController((0.3, 2.5, 3.0), (0.3, 2.5, 10.0), (0, 1, 0), 45.0, F(w) / F(h))
    if which == "seam_b":
        assert c.rotate(4.0, 2.0)
    cam = c.uniforms()
    cam.setflags(write=False)
    return cam


def camera(name: str, which: str, w: int, h: int) -> np.ndarray:
    """(4, 3) uniforms: "identity" and reproject_common's moves from the scene's camera, or a seam camera."""
    return _seam(which, w, h) if which.startswith("seam") else C.camera_b(name, which, w, h)


# An equirectangular pixel of a 67x45 image is 5.4 x 4 degrees: neighbouring hits lie 9 % of their distance apart
# and more on a slanted surface, so the default position tolerance of 2 % -- chosen for pixels of a degree or
# less -- would leave no pixel with four valid taps.  The cases whose `from` view is that coarse (the
# equirectangular ones and the 180-degree fisheye) run at a tolerance of 13 %, at which the table still holds
# disocclusions; the same-model fisheye cases use a 40-degree fisheye (0.6 degrees per pixel) at the defaults.
COARSE = (("position_tolerance", 0.13),)
FISHEYE_FOV = 40.0

# case -> (scene, from, to, params), a view as (model, camera name, fov_deg): every model with both views its own,
# on two scenes and two moves; two changes of model at one camera; the equirectangular seam.
CASES = {f"{m}-{n}-{mv}": (n, (m, "identity", FISHEYE_FOV), (m, mv, FISHEYE_FOV), COARSE if m == "equirect" else ())
         for m in MODELS for n in ("c1", "c2wide") for mv in ("rotate", "translate")}
CASES["pinhole-to-fisheye"] = ("c1", ("pinhole", "identity", 180.0), ("fisheye", "identity", 180.0), ())
CASES["fisheye-to-equirect"] = ("c1", ("fisheye", "identity", 180.0), ("equirect", "identity", 180.0), COARSE)
CASES["seam"] = ("c1", ("equirect", "seam_a", 180.0), ("equirect", "seam_b", 180.0), COARSE)


def view_of(name: str, spec, w: int, h: int):
    """(model, camera (4, 3), fov_deg): what PathTracer.reproject_view and reproject_view_ref take."""
    model, which, fov = spec
    return (model, camera(name, which, w, h), fov)


def case_views(case: str, w: int = W, h: int = Hh):
    """(scene, from view, to view, params as a dict) of a case."""
    name, a, b, params = CASES[case]
    return name, view_of(name, a, w, h), view_of(name, b, w, h), dict(params)


@functools.lru_cache(maxsize=None)
def _oracle(name: str, w: int, h: int):
    return pyoracle.Oracle(scene(name, w, h))


@functools.lru_cache(maxsize=None)
def oracle_guides(name: str, spec, w: int, h: int):
    """(position, normal) guide images, (h, w, 4) each, of the centre rays of a view: the oracle's
    closest hits of rays_ref's set (tests/test_gpu_rays.py pins pnrt_render_guides_rays to the same
    records).  A pixel without a ray is a miss."""
    model, cam, fov = view_of(name, spec, w, h)
    r = R.make_set(model, cam, w, h, 0, fov_deg=fov)
    is_ray = np.isfinite(r).all(axis=1) & r[:, 4:7].any(axis=1)
    r7 = np.concatenate([r[is_ray, 0:3], r[is_ray, 4:7], np.full((int(is_ray.sum()), 1), FLOAT_MAX, F)], axis=1)
    o = np.zeros((w * h, 13), np.uint32)
    if is_ray.any():
        o[is_ray] = _oracle(name, w, h).intersect(r7, kind=0, sem=0)
    hit = o[:, 0] != 0
    pos, nrm = np.zeros((h * w, 4), F), np.zeros((h * w, 4), F)
    pos[:, :3] = o[:, 1:4].view(F)
    pos[:, 3] = hit
    nrm[:, :3] = o[:, 4:7].view(F)
    nrm[:, 3] = np.where(hit, o[:, 10].view(np.int32), -1)
    pos[~hit, :3] = 0
    nrm[~hit, :3] = 0
    pos, nrm = pos.reshape(h, w, 4), nrm.reshape(h, w, 4)
    pos.setflags(write=False)
    nrm.setflags(write=False)
    return pos, nrm


@functools.lru_cache(maxsize=None)
def replay_views(name: str, a, b, w: int = W, h: int = Hh, params: tuple = ()):
    """reproject_view_ref over reproject_common.state() and the oracle's guide images of both views
    -> (accum, moments, stats, valid taps per pixel (h, w), -1 on a miss)."""
    acc, mom = C.state(name, w, h)
    pa, na = oracle_guides(name, a, w, h)
    pb, nb = oracle_guides(name, b, w, h)
    return VR.reproject(acc, mom, pa, na, pb, nb, view_of(name, a, w, h), w, h, dict(params))


def replay(case: str):
    name, a, b, params = CASES[case]
    return replay_views(name, a, b, W, Hh, params)


# (n_reprojected, n_disoccluded, n_missed, sum_frames, max_frames) of replay(case) at 67x45 with the case's
# parameters, as recorded when the feature was specified.
TABLE = {"pinhole-c1-rotate": (2650, 343, 22, 5458, 5),
         "pinhole-c1-translate": (2424, 361, 230, 4990, 5),
         "pinhole-c2wide-rotate": (422, 166, 2427, 1469, 5),
         "pinhole-c2wide-translate": (143, 456, 2416, 488, 5),
         "ortho-c1-rotate": (2562, 453, 0, 5144, 5),
         "ortho-c1-translate": (1376, 1639, 0, 2788, 5),
         "ortho-c2wide-rotate": (2860, 155, 0, 5798, 5),
         "ortho-c2wide-translate": (2419, 596, 0, 4916, 5),
         "equirect-c1-rotate": (185, 2, 2828, 370, 2),
         "equirect-c1-translate": (171, 16, 2828, 342, 2),
         "equirect-c2wide-rotate": (184, 3, 2828, 497, 5),
         "equirect-c2wide-translate": (169, 18, 2828, 434, 5),
         "fisheye-c1-rotate": (2213, 145, 657, 4505, 5),
         "fisheye-c1-translate": (2047, 313, 655, 4177, 5),
         "fisheye-c2wide-rotate": (2207, 151, 657, 4502, 5),
         "fisheye-c2wide-translate": (2040, 320, 655, 4163, 5),
         "pinhole-to-fisheye": (224, 152, 2639, 454, 5),
         "fisheye-to-equirect": (183, 1, 2831, 367, 3),
         "seam": (1254, 2, 1759, 2511, 5)}
