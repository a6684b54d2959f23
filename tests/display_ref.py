"""The numpy restatement of DESIGN.md section 26 -- TEST INFRASTRUCTURE: the display
transform (``display_ref``), the luminance histogram (``histogram_ref``) and the
exposure derived from it (``exposure_ref``).  Float32 at every step, every product
and sum rounded on its own; the sRGB branch's pow is the oracle's PN-libm
(``pyoracle.math_eval(5, ...)``), the CPU twin of the device's pnm_pow."""
from __future__ import annotations

import numpy as np

F = np.float32
TONES = ("clamp", "reinhard", "aces")
TRANSFERS = ("linear", "srgb")
LUMA_BINS = 512
SRGB_EXPONENT = np.array([0x3ED55555], np.uint32).view(F)[0]      # 1.0f / 2.4f
# the floats nearest 2^(j/16)
T16 = np.array([0x3F800000, 0x3F85AAC3, 0x3F8B95C2, 0x3F91C3D3, 0x3F9837F0, 0x3F9EF532, 0x3FA5FED7, 0x3FAD583F,
                0x3FB504F3, 0x3FBD08A4, 0x3FC5672A, 0x3FCE248C, 0x3FD744FD, 0x3FE0CCDF, 0x3FEAC0C7, 0x3FF5257D],
               np.uint32).view(F)


def _pow(t: np.ndarray, e) -> np.ndarray:
    import pyoracle
    flat = np.ascontiguousarray(t, F).reshape(-1)
    return pyoracle.math_eval(5, flat, np.full_like(flat, e)).reshape(t.shape)


def tone_curve(s: np.ndarray, tone: str, white=4.0) -> np.ndarray:
    s = np.asarray(s, F)
    one = F(1)
    with np.errstate(all="ignore"):
        if tone == "clamp":
            return s
        if tone == "reinhard":
            w2 = F(F(white) * F(white))
            return ((s * (one + (s / w2).astype(F)).astype(F)).astype(F) / (one + s).astype(F)).astype(F)
        if tone == "aces":
            num = (s * ((F(2.51) * s).astype(F) + F(0.03)).astype(F)).astype(F)
            den = ((s * ((F(2.43) * s).astype(F) + F(0.59)).astype(F)).astype(F) + F(0.14)).astype(F)
            return (num / den).astype(F)
    raise KeyError(tone)


def transfer_curve(t: np.ndarray, transfer: str) -> np.ndarray:
    t = np.asarray(t, F)
    if transfer == "linear":
        return t
    if transfer == "srgb":
        low = (F(12.92) * t).astype(F)
        high = ((F(1.055) * _pow(t, SRGB_EXPONENT)).astype(F) - F(0.055)).astype(F)
        return np.minimum(np.where(t <= F(0.0031308), low, high).astype(F), F(1))
    raise KeyError(transfer)


def display_ref(img: np.ndarray, tone="clamp", transfer="linear", exposure=1.0, white=4.0, bottom_first=False) -> np.ndarray:
    """(H, W, 4) float32 image, row 0 = bottom -> (H, W, 4) uint8, top row first unless
    ``bottom_first``; alpha 255."""
    c = np.asarray(img, F)[..., :3]
    with np.errstate(all="ignore"):
        v = (c * F(exposure)).astype(F)
        s = np.where(v > F(0), v, F(0)).astype(F)             # NaN, negatives and -0 become +0
        s = np.minimum(s, F(65536))
        t = np.minimum(tone_curve(s, tone, white), F(1))
        u = transfer_curve(t, transfer)
        q = np.floor(((u * F(255)).astype(F) + F(0.5)).astype(F)).astype(np.uint8)
    out = np.full(c.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = q
    return np.ascontiguousarray(out if bottom_first else out[::-1])


def luma(img: np.ndarray) -> np.ndarray:
    c = np.asarray(img, F)
    with np.errstate(all="ignore"):
        return (((F(0.2126) * c[..., 0]).astype(F) + (F(0.7152) * c[..., 1]).astype(F)).astype(F)
                + (F(0.0722) * c[..., 2]).astype(F)).astype(F)


def luma_bins(y: np.ndarray):
    """(counted mask, bin) of luminances."""
    y = np.ascontiguousarray(y, F)
    with np.errstate(all="ignore"):
        counted = (y > F(0)) & np.isfinite(y)
    b = np.clip((y.view(np.uint32) >> 19).astype(np.int64) - 1776, 0, LUMA_BINS - 1)
    return counted, b


def histogram_ref(img: np.ndarray, rows=None) -> dict:
    """The histogram of the image's rows ``rows`` (all when None)."""
    a = np.asarray(img, F)
    if rows is not None:
        a = a[np.asarray(rows, np.int64)]
    y = luma(a).reshape(-1)
    counted, b = luma_bins(y)
    return {"n_pixels": int(y.size), "n_counted": int(counted.sum()),
            "bins": np.bincount(b[counted], minlength=LUMA_BINS).astype(np.int64)}


def exposure_mean_bin(hist: dict, low=50, high=950):
    """m of the definition, or None when no pixel lies between the cuts."""
    n = int(hist["n_counted"])
    lo, hi = n * low // 1000, n * high // 1000
    cum = S = C = 0
    for b, cnt in enumerate(int(v) for v in hist["bins"]):
        prev, cum = cum, cum + cnt
        k = max(0, min(cum, hi) - max(prev, lo))
        S += k * b
        C += k
    return None if C == 0 else (2 * S + C) // (2 * C)


def exposure_ref(hist: dict, low=50, high=950, key=0.18) -> np.float32:
    m = exposure_mean_bin(hist, low, high)
    if m is None:
        return F(1)
    k = 256 - m
    e = k // 16                                               # floor
    j = k - 16 * e
    return F(F(key) * F(np.ldexp(T16[j], e)))
