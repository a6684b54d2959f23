"""The denoised preview restated in float32 numpy -- TEST INFRASTRUCTURE.

Written from DESIGN.md section 20.2 (the definition of pnrt_denoise's result),
step by step and in its operation order, not from the kernel; exp2 is the
oracle's PN-libm one (pyoracle.math_eval(6, .)).  Every array stays float32 and
every operation is one IEEE binary32 operation, so the device's image must
equal this one bit for bit.
"""
from __future__ import annotations

import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)       # exact in binary32
ALBEDO_MIN = F(1.0 / 256.0)
DEFAULTS = {"levels": 5, "sigma_color": 2.0, "sigma_normal": 0.25, "sigma_position": 0.5}


def oracle_exp2(x: np.ndarray) -> np.ndarray:
    import pyoracle
    return pyoracle.math_eval(6, np.ascontiguousarray(x, F).reshape(-1)).reshape(x.shape)


def pn_max(a, b):
    """The project's max: b when b > a or a is NaN, else a."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.where((b > a) | (a != a), b, a).astype(F)


def passthrough(position: np.ndarray, normal: np.ndarray, materials: np.ndarray) -> np.ndarray:
    """Step 1: misses (position.w == 0) and hits on a material with an emission component != 0."""
    mats = np.asarray(materials, F).reshape(-1, 18)
    miss = position[..., 3] == 0
    mat = normal[..., 3].astype(np.int64)
    ok = (mat >= 0) & (mat < len(mats))
    em = mats[np.clip(mat, 0, len(mats) - 1), 0:3]
    return miss | (ok & np.any(em != 0, axis=-1))


def _dist2(a_tap, a_centre):
    d = (a_tap - a_centre).astype(F)
    sq = (d * d).astype(F)
    return ((sq[..., 0] + sq[..., 1]).astype(F) + sq[..., 2]).astype(F)


def atrous_ref(accum, position, normal, albedo, materials, levels=DEFAULTS["levels"],
               sigma_color=DEFAULTS["sigma_color"], sigma_normal=DEFAULTS["sigma_normal"],
               sigma_position=DEFAULTS["sigma_position"], exp2=oracle_exp2) -> np.ndarray:
    """(H, W, 4) float32 images, row 0 = bottom (read_accum / read_aov) -> the denoised image."""
    A, P, N, AL = (np.ascontiguousarray(a, F) for a in (accum, position, normal, albedo))
    Hh, W = A.shape[:2]
    assert 1 <= levels <= 5
    pt = passthrough(P, N, materials)
    with np.errstate(all="ignore"):
        m = pn_max(AL[..., :3], ALBEDO_MIN)                                # step 2
        c = (A[..., :3] / m).astype(F)
        sn, sp = F(sigma_normal), F(sigma_position)                        # step 3
        inv_n = F(1) / F(sn * sn)
        inv_p = F(1) / F(sp * sp)
        yy, xx = np.mgrid[0:Hh, 0:W]
        for i in range(levels):                                            # step 4
            s = 1 << i
            sc = F(F(sigma_color) * F(2.0 ** -i))
            inv_c = F(1) / F(sc * sc)
            Wt = np.zeros((Hh, W), F)
            S = np.zeros((Hh, W, 3), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = xx + dx * s, yy + dy * s
                    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                    qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                    valid = inside & ~pt[qy, qx]
                    cq = c[qy, qx]
                    e = ((_dist2(cq, c) * inv_c).astype(F) + (_dist2(N[qy, qx, :3], N[..., :3]) * inv_n).astype(F)).astype(F)
                    e = (e + (_dist2(P[qy, qx, :3], P[..., :3]) * inv_p).astype(F)).astype(F)
                    w = (F(H5[dy + 2] * H5[dx + 2]) * exp2((-e).astype(F))).astype(F)
                    Wt = np.where(valid, (Wt + w).astype(F), Wt)
                    S = np.where(valid[..., None], (S + (w[..., None] * cq).astype(F)).astype(F), S)
            c = (S / Wt[..., None]).astype(F)
        out = np.empty((Hh, W, 4), F)                                      # step 5
        out[..., :3] = (c * m).astype(F)
        out[..., 3] = F(1)
    out[pt] = A[pt]
    return out
