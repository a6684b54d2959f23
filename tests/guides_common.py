"""Shared by tests/test_gpu_guides.py and tests/test_gpu_denoise*.py -- TEST
INFRASTRUCTURE: the small scenes and shapes of the guide-image / denoise tests,
the camera rays restated in float32 numpy, and the oracle's sample_albedo
restated the same way."""
from __future__ import annotations

import functools

import numpy as np

from pnraytracing_amd import scenes as S

F = np.float32

# 67x45: no multiple of 8, and lower than 2 * 2 * 16, so the level-4 taps (spacing 16)
# fall outside on both sides in y; 8x8: one tile; 1x1
SHAPES = [(67, 45), (8, 8), (1, 1)]
SCENES = ["c1", "c2", "c3", "c2wide"]


@functools.lru_cache(maxsize=None)
def scene(name: str, width: int, height: int):
    """c1: area light (emissive pass-through pixels, no misses); c2: the bunny stand-in
    and the environment; c3: two textures, one of odd width; c2wide: c2 through a wider
    lens -- the one with misses that show the environment."""
    if name == "c1":
        return S.cornell_c1(width, height, spp=1)
    if name == "c2":
        return S.bunny_c2(width, height, spp=1, nu=24, nv=12, env=True)
    if name == "c3":
        return S.marry_c3(width, height, spp=1, nu=16, nv=12)
    if name == "c2wide":
        # The Cornell camera's 45-degree frustum passes through the box's open front, so
        # every camera ray of c2 hits a wall.  At 100 degrees the rays around the box miss.
        import dataclasses
        from pnraytracing_amd import host as H
        cam = H.camera_update((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 100.0, F(width) / F(height))
        return dataclasses.replace(scene("c2", width, height), name="C2-bunny-wide", camera=cam)
    raise KeyError(name)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F).view(np.uint32)


def camera_rays(cfg) -> np.ndarray:
    """CameraGetRay (oracle/pn_oracle.c:272-283, called with s = (float)px / (float)width,
    t = (float)py / (float)height) for every pixel, row 0 = bottom: (H * W, 7) float32 =
    origin, dir, tMax."""
    eye, llc, hor, ver = np.asarray(cfg.camera, F).reshape(4, 3)
    W, H = cfg.width, cfg.height
    py, px = np.mgrid[0:H, 0:W]
    s = (px.astype(F) / F(W)).astype(F).reshape(-1, 1)
    t = (py.astype(F) / F(H)).astype(F).reshape(-1, 1)
    d = (((llc + (s * hor).astype(F)).astype(F) + (t * ver).astype(F)).astype(F) - eye).astype(F)
    sq = (d * d).astype(F)
    ln = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(F) + sq[:, 2]).astype(F)).astype(F)
    d = (d / ln[:, None]).astype(F)
    rays = np.empty((H * W, 7), F)
    rays[:, 0:3] = eye
    rays[:, 3:6] = d
    rays[:, 6] = F(10000000.0)
    return rays


def _wrap_repeat(fl: np.ndarray, n: int) -> np.ndarray:
    q = np.floor((fl / F(n)).astype(F)).astype(F)
    m = (fl - (F(n) * q).astype(F)).astype(F)
    m = np.minimum(np.maximum(m, F(0)), F(n))
    i = m.astype(np.int64)
    i = np.where(i >= n, i - n, i)
    i = np.where(i < 0, i + n, i)
    return np.where(fl != fl, 0, i)


def sample_albedo(texture, u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """sample_albedo (oracle/pn_oracle.c:232-247): REPEAT, LINEAR at level 0 of an 8-bit
    texture (pixels, w, h, ch) as glTexImage2D reads it (UNPACK_ALIGNMENT 4); (n, 3) float32."""
    import pyoracle
    px, w, h, ch = texture
    stride = (w * ch + 3) & ~3
    data = pyoracle.gl_unpacked(px, w, h, ch)
    u, v = np.asarray(u, F), np.asarray(v, F)
    fu = ((u * F(w)).astype(F) - F(0.5)).astype(F)
    fv = ((v * F(h)).astype(F) - F(0.5)).astype(F)
    flu, flv = np.floor(fu).astype(F), np.floor(fv).astype(F)
    a, b = (fu - flu).astype(F), (fv - flv).astype(F)
    i0, i1 = _wrap_repeat(flu, w), _wrap_repeat((flu + F(1)).astype(F), w)
    j0, j1 = _wrap_repeat(flv, h), _wrap_repeat((flv + F(1)).astype(F), h)

    def fetch(i, j):
        out = np.zeros((len(i), 3), F)
        for k in range(min(ch, 3)):
            out[:, k] = (data[j * stride + i * ch + k].astype(F) / F(255.0)).astype(F)
        return out

    t00, t10, t01, t11 = fetch(i0, j0), fetch(i1, j0), fetch(i0, j1), fetch(i1, j1)
    one = F(1)
    w00 = ((one - a) * (one - b)).astype(F)[:, None]
    w10 = (a * (one - b)).astype(F)[:, None]
    w01 = ((one - a) * b).astype(F)[:, None]
    w11 = (a * b).astype(F)[:, None]
    r = ((w00 * t00).astype(F) + (w10 * t10).astype(F)).astype(F)
    r = (r + (w01 * t01).astype(F)).astype(F)
    return (r + (w11 * t11).astype(F)).astype(F)
