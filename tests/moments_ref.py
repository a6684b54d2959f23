"""TEST INFRASTRUCTURE: DESIGN.md section 21 (the per-pixel sample moments, the
relative standard error and the convergence statistics of pnrt_enable_moments /
pnrt_read_error / pnrt_convergence) restated in float32 numpy, one rounded
operation per line -- what pt_moments.h must compute, bit for bit."""
from __future__ import annotations

import numpy as np

F = np.float32
U = np.uint32
N_MAX = 0xFFFFFFFF


def luminance(c: np.ndarray) -> np.ndarray:
    """Y = ((0.2126f * c.x) + (0.7152f * c.y)) + (0.0722f * c.z), every operation rounded."""
    c = np.asarray(c, F)
    r = (F(0.2126) * c[..., 0]).astype(F)
    g = (F(0.7152) * c[..., 1]).astype(F)
    b = (F(0.0722) * c[..., 2]).astype(F)
    return ((r + g).astype(F) + b).astype(F)


def zeros(height: int, width: int) -> np.ndarray:
    return np.zeros((height, width, 4), F)


def update(moments: np.ndarray, colors, frame_numbers) -> np.ndarray:
    """Fold the per-frame colour images `colors` (each (H, W, >= 3)), whose frame numbers
    are `frame_numbers`, into a copy of the (H, W, 4) moments image, in the order given."""
    m = np.array(moments, F)
    mean, m2 = m[..., 0].copy(), m[..., 1].copy()
    n = m[..., 3].copy().view(U)
    for c, f in zip(colors, frame_numbers):
        y = luminance(c)
        if f == 0:                                   # frame 0 overwrites the accumulation: restart with it
            n[...] = 0
            mean[...] = 0
            m2[...] = 0
        n = np.where(n == N_MAX, n, n + U(1)).astype(U)
        d = (y - mean).astype(F)
        # (float)n rounds a uint32 to the nearest float32: numpy converts uint32 -> float32 the same way
        r = (F(1) / n.astype(F)).astype(F)
        mean = (mean + (d * r).astype(F)).astype(F)
        m2 = (m2 + (d * (y - mean).astype(F)).astype(F)).astype(F)
    out = np.zeros_like(m)
    out[..., 0], out[..., 1] = mean, m2
    out[..., 3] = n.view(F)
    return out


def frames_of(moments: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(moments[..., 3]).view(U)


def error(moments: np.ndarray) -> np.ndarray:
    """e_c per pixel, (H, W) float32; +inf where n < 2."""
    mean, m2, n = moments[..., 0], moments[..., 1], frames_of(moments)
    measured = n >= 2
    nn = np.where(measured, n, U(2))                 # (any n >= 2: the unmeasured pixels are overwritten below)
    with np.errstate(all="ignore"):
        var = (m2 / (nn - U(1)).astype(F)).astype(F)
        sem = np.sqrt((var / nn.astype(F)).astype(F)).astype(F)
        e = (sem / np.fmax(mean, F(1.0 / 256.0)).astype(F)).astype(F)
        ec = np.where(e <= F(65535.0), e, F(65535.0)).astype(F)      # NaN compares false: 65535
    return np.where(measured, ec, F(np.inf)).astype(F)


def stats(moments: np.ndarray, threshold: float, rows=None) -> dict:
    """pnrt_convergence_stats of the rows `rows` (default all), with mean_error as
    PathTracer.convergence adds it."""
    m = moments if rows is None else moments[np.asarray(rows, dtype=np.int64)]
    n = frames_of(m)
    out = {"n_pixels": int(n.size), "n_measured": 0, "n_above": 0, "sum_q16": 0, "max_error": 0.0, "min_frames": 0,
           "max_frames": 0}
    if n.size:
        e = error(m)
        meas = n >= 2
        em = e[meas]
        out["n_measured"] = int(meas.sum())
        out["n_above"] = int((em > F(threshold)).sum())
        # (uint32)(e_c * 65536.0f): e_c <= 65535, so the product is below 2^32; truncation
        out["sum_q16"] = int((em * F(65536.0)).astype(F).astype(np.int64).sum())
        out["max_error"] = float(em.max()) if em.size else 0.0
        out["min_frames"], out["max_frames"] = int(n.min()), int(n.max())
    out["mean_error"] = out["sum_q16"] / 65536 / out["n_measured"] if out["n_measured"] else 0.0
    return out


def blend(accum: np.ndarray, colors, frame_numbers) -> np.ndarray:
    """The progressive mean (ray_tracing.comp:988-991) of the same frames, for the replay
    check of the oracle-derived colours: acc = acc * (1 - a) + c * a, a = 1 / (float)(f + 1)."""
    acc = np.array(accum, F)
    for c, f in zip(colors, frame_numbers):
        a = F(1) / F(f + 1)
        acc[..., :3] = ((acc[..., :3] * (F(1) - a)).astype(F) + (np.asarray(c, F)[..., :3] * a).astype(F)).astype(F)
        acc[..., 3] = 1
    return acc
