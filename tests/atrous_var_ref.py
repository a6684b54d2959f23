"""The variance-guided denoised preview restated in float32 numpy -- TEST INFRASTRUCTURE.

Written from DESIGN.md section 24.2 (the definition of pnrt_denoise_variance's
result), step by step and in its operation order, not from the kernel; exp2 is the
oracle's PN-libm one (pyoracle.math_eval(6, .)).  Every array stays float32 and
every operation is one IEEE binary32 operation, so the device's image must equal
this one bit for bit.
"""
from __future__ import annotations

import numpy as np

from atrous_ref import ALBEDO_MIN, H5, _dist2, oracle_exp2, passthrough, pn_max
from moments_ref import frames_of, luminance

F = np.float32
U = np.uint32
K3 = np.array([1 / 4, 1 / 2, 1 / 4], F)                       # exact in binary32
EPS = F(2.0 ** -20)
DEFAULTS = {"levels": 5, "sigma_variance": 4.0, "sigma_normal": 0.25, "sigma_position": 0.5}


def initial_variance(c0: np.ndarray, m: np.ndarray, moments: np.ndarray) -> np.ndarray:
    """Step 3: the variance of the mean luminance in demodulated units where n >= 2,
    lum(c0)^2 where the pixel is unmeasured."""
    n = frames_of(moments)
    measured = n >= 2
    nn = np.where(measured, n, U(2))                 # (any n >= 2: the unmeasured pixels are overwritten below)
    lm = luminance(m)
    v = (moments[..., 1] / (nn - U(1)).astype(F)).astype(F)
    v = (v / nn.astype(F)).astype(F)
    v = (v / (lm * lm).astype(F)).astype(F)
    l = luminance(c0)
    return np.where(measured, v, (l * l).astype(F)).astype(F)


def filter_passes(c, v, pt, N, P, levels, sigma_variance, sigma_normal, sigma_position, exp2):
    """Steps 4 and 5 on a demodulated colour image c (H, W, 3), its variance v (H, W), the
    pass-through mask pt and the guide vectors N, P (H, W, 3): (c^L, v^L).  Nothing is read
    from c or v where pt is set."""
    Hh, W = v.shape
    sv, sn, sp = F(sigma_variance), F(sigma_normal), F(sigma_position)
    inv_n = F(1) / F(sn * sn)
    inv_p = F(1) / F(sp * sp)
    yy, xx = np.mgrid[0:Hh, 0:W]
    for i in range(levels):
        s = 1 << i
        # 5a: the variance prefilter, 3x3 at unit spacing
        G = np.zeros((Hh, W), F)
        K = np.zeros((Hh, W), F)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                qx, qy = xx + dx, yy + dy
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                valid = inside & ~pt[qy, qx]
                k = F(K3[dy + 1] * K3[dx + 1])
                G = np.where(valid, (G + (k * v[qy, qx]).astype(F)).astype(F), G)
                K = np.where(valid, (K + k).astype(F), K)
        g = (G / K).astype(F)
        r = (F(1) / ((sv * np.sqrt(g).astype(F)).astype(F) + EPS).astype(F)).astype(F)
        # 5b: the taps
        lc = luminance(c)
        Wt = np.zeros((Hh, W), F)
        S = np.zeros((Hh, W, 3), F)
        V = np.zeros((Hh, W), F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qx, qy = xx + dx * s, yy + dy * s
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < Hh)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, Hh - 1)
                valid = inside & ~pt[qy, qx]
                cq = c[qy, qx]
                e = (np.abs((luminance(cq) - lc).astype(F)) * r).astype(F)
                e = (e + (_dist2(N[qy, qx], N) * inv_n).astype(F)).astype(F)
                e = (e + (_dist2(P[qy, qx], P) * inv_p).astype(F)).astype(F)
                w = (F(H5[dy + 2] * H5[dx + 2]) * exp2((-e).astype(F))).astype(F)
                Wt = np.where(valid, (Wt + w).astype(F), Wt)
                S = np.where(valid[..., None], (S + (w[..., None] * cq).astype(F)).astype(F), S)
                V = np.where(valid, (V + ((w * w).astype(F) * v[qy, qx]).astype(F)).astype(F), V)
        # 5c
        c = (S / Wt[..., None]).astype(F)
        v = (V / (Wt * Wt).astype(F)).astype(F)
    return c, v


def atrous_var_ref(accum, position, normal, albedo, materials, moments, levels=DEFAULTS["levels"],
                   sigma_variance=DEFAULTS["sigma_variance"], sigma_normal=DEFAULTS["sigma_normal"],
                   sigma_position=DEFAULTS["sigma_position"], exp2=oracle_exp2) -> np.ndarray:
    """(H, W, 4) float32 images, row 0 = bottom (read_accum / read_aov / read_moments) -> the
    denoised image."""
    A, P, N, AL, M = (np.ascontiguousarray(a, F) for a in (accum, position, normal, albedo, moments))
    assert 1 <= levels <= 5
    pt = passthrough(P, N, materials)                                      # step 1
    with np.errstate(all="ignore"):
        m = pn_max(AL[..., :3], ALBEDO_MIN)                                # step 2
        c = (A[..., :3] / m).astype(F)
        v = initial_variance(c, m, M)                                      # step 3
        c, v = filter_passes(c, v, pt, N[..., :3], P[..., :3], levels, sigma_variance, sigma_normal, sigma_position, exp2)
        out = np.empty(A.shape, F)                                         # step 6
        out[..., :3] = (c * m).astype(F)
        out[..., 3] = F(1)
    out[pt] = A[pt]
    return out
