"""TEST INFRASTRUCTURE: DESIGN.md section 25 (temporal reprojection, pnrt_reproject)
restated in float32 numpy, operation by operation: the projection of view B's first hits
into view A's image plane, the four bilinear taps and their validity tests, the normalised
blend of colour, mean and sample variance, the capped frame count and the statistics --
what pt_reproject.h must compute, bit for bit."""
from __future__ import annotations

import numpy as np

F = np.float32
U = np.uint32
DEFAULTS = {"normal_min": 0.9, "position_tolerance": 0.02, "max_history": 32}


def _dot(a, b):
    """dot of pt_common.h: (a.x * b.x + a.y * b.y) + a.z * b.z, every operation rounded."""
    return (((a[..., 0] * b[..., 0]).astype(F) + (a[..., 1] * b[..., 1]).astype(F)).astype(F)
            + (a[..., 2] * b[..., 2]).astype(F)).astype(F)


def _cross(a, b):
    """cross of pt_common.h: (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)."""
    def c(i, j):
        return ((a[..., i] * b[..., j]).astype(F) - (b[..., i] * a[..., j]).astype(F)).astype(F)
    return np.stack([c(1, 2), c(2, 0), c(0, 1)], axis=-1)


def project(posB, camA, W, H):
    """Steps 2 and 3: (taps, x0, y0, a, b, dd) per pixel of B -- whether the pixel has taps
    at all, the lower-left tap, the bilinear fractions and |d|^2."""
    eye, llc, hor, ver = (np.asarray(v, F) for v in np.asarray(camA, F).reshape(4, 3))
    P = np.asarray(posB, F)[..., :3]
    d = (P - eye).astype(F)
    L = (llc - eye).astype(F)
    Nv = _cross(hor, ver)
    k = (_dot(L, Nv) / _dot(d, Nv)).astype(F)
    q = ((k[..., None] * d).astype(F) - L).astype(F)
    NN = _dot(Nv, Nv)
    s = (_dot(_cross(q, ver), Nv) / NN).astype(F)
    t = (_dot(_cross(hor, q), Nv) / NN).astype(F)
    fx, fy = (s * F(W)).astype(F), (t * F(H)).astype(F)
    taps = (k > 0) & np.isfinite(k) & (fx >= F(-1)) & (fx < F(W)) & (fy >= F(-1)) & (fy < F(H))
    flx, fly = np.where(taps, np.floor(fx), F(0)).astype(F), np.where(taps, np.floor(fy), F(0)).astype(F)
    a, b = (fx - flx).astype(F), (fy - fly).astype(F)
    return taps, flx.astype(np.int64), fly.astype(np.int64), a, b, _dot(d, d)


def tap_table(accum, moments, posA, nrmA, posB, nrmB, camA, W, H, params=None):
    """Steps 2-4 for every pixel: (hit, valid (H, W, 4) bool, weights (H, W, 4), the taps'
    flat pixel indices (H, W, 4), clamped into the image)."""
    with np.errstate(all="ignore"):
        p = dict(DEFAULTS, **(params or {}))
        posB, nrmB = np.asarray(posB, F), np.asarray(nrmB, F)
        posA, nrmA = np.asarray(posA, F).reshape(-1, 4), np.asarray(nrmA, F).reshape(-1, 4)
        mom = np.asarray(moments, F).reshape(-1, 4)
        hit = posB[..., 3] != 0
        taps, x0, y0, a, b, dd = project(posB, camA, W, H)
        one = F(1)
        wgt = np.stack([((one - a) * (one - b)).astype(F), (a * (one - b)).astype(F), ((one - a) * b).astype(F),
                        (a * b).astype(F)], axis=-1)
        tol = F(p["position_tolerance"])
        lim = ((tol * tol).astype(F) * dd).astype(F)
        valid = np.zeros((H, W, 4), bool)
        index = np.zeros((H, W, 4), np.int64)
        for i in range(4):
            xi, yi = x0 + (i & 1), y0 + (i >> 1)
            inside = taps & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            at = np.clip(yi, 0, H - 1) * W + np.clip(xi, 0, W - 1)
            pa, na = posA[at], nrmA[at]
            e = (pa[..., :3] - posB[..., :3]).astype(F)
            n = mom[at][..., 3].view(U)
            valid[..., i] = (hit & inside & (wgt[..., i] > 0) & (pa[..., 3] == one) & (na[..., 3] == nrmB[..., 3])
                             & (_dot(na[..., :3], nrmB[..., :3]) >= F(p["normal_min"])) & (_dot(e, e) <= lim) & (n >= 1))
            index[..., i] = at
    return hit, valid, wgt, index


def reproject(accum, moments, posA, nrmA, posB, nrmB, camA, W, H, params=None):
    """One pnrt_reproject call -> (accumulation, moments, stats).  A: the camera `camA` the
    images were rendered with and its position / normal guide images; B: the new view's."""
    p = dict(DEFAULTS, **(params or {}))
    with np.errstate(all="ignore"):
        hit, valid, wgt, index = tap_table(accum, moments, posA, nrmA, posB, nrmB, camA, W, H, p)
        acc_in, mom_in = np.asarray(accum, F).reshape(-1, 4), np.asarray(moments, F).reshape(-1, 4)
        wsum = np.zeros((H, W), F)
        nmin = np.full((H, W), 0xFFFFFFFF, U)
        for i in range(4):
            v = valid[..., i]
            wsum = np.where(v, (wsum + wgt[..., i]).astype(F), wsum)
            nmin = np.where(v, np.minimum(nmin, mom_in[index[..., i]][..., 3].view(U)), nmin)
        col = np.zeros((H, W, 3), F)
        mean, s2 = np.zeros((H, W), F), np.zeros((H, W), F)
        for i in range(4):
            v = valid[..., i]
            r = (wgt[..., i] / wsum).astype(F)
            ta, tm = acc_in[index[..., i]], mom_in[index[..., i]]
            n = tm[..., 3].view(U)
            col = np.where(v[..., None], (col + (r[..., None] * ta[..., :3]).astype(F)).astype(F), col)
            mean = np.where(v, (mean + (r * tm[..., 0]).astype(F)).astype(F), mean)
            var = (tm[..., 1] / np.maximum(n - U(1), U(1)).astype(F)).astype(F)      # (valid: n >= 1)
            s2 = np.where(v, (s2 + (r * var).astype(F)).astype(F), s2)
        got = valid.any(axis=-1)
        n1 = np.minimum(nmin, U(p["max_history"]))
        acc = np.zeros((H, W, 4), F)
        mom = np.zeros((H, W, 4), F)
        acc[got, :3] = col[got]
        acc[got, 3] = 1
        mom[got, 0] = mean[got]
        mom[got, 1] = (s2 * (n1 - U(1)).astype(F)).astype(F)[got]
        mom[..., 3].view(U)[got] = n1[got]
    stats = {"n_pixels": W * H, "n_reprojected": int(got.sum()), "n_disoccluded": int((hit & ~got).sum()),
             "n_missed": int((~hit).sum()), "sum_frames": int(n1[got].astype(np.int64).sum()),
             "max_frames": int(n1[got].max()) if got.any() else 0}
    return acc, mom, stats
