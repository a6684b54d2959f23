"""TEST INFRASTRUCTURE: DESIGN.md section 31.2 (pnrt_reproject_view) restated in float32
numpy, operation by operation: the inverse map of each camera model of pnrt_make_rays --
the hit of view B's pixel to the continuous pixel coordinates (fx, fy) of view A --, the
tap table with the equirectangular view's wrap in x, and the blend, the capped count and
the statistics of section 25 -- what pt_reproject_view.h must compute, bit for bit.
pnm_atan2 is PN-libm's through the oracle (pyoracle.math_eval(2, y, x)); division and sqrt
are IEEE (numpy's).  A view is (model, camera (4, 3), fov_deg)."""
from __future__ import annotations

import numpy as np

import pyoracle
from rays_ref import DEG, HALF, MODELS, ONE, PI, TWO_PI, basis, cross, dot
from reproject_ref import DEFAULTS

F = np.float32
U = np.uint32


def atan2(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, F), np.asarray(x, F))
    return pyoracle.math_eval(2, np.ascontiguousarray(y).ravel(), np.ascontiguousarray(x).ravel()).reshape(y.shape)


def model_of(view) -> int:
    m = view[0]
    return MODELS.index(m) if isinstance(m, str) else int(m)


def inverse(P, view, W, H):
    """(fx, fy, front, dd) of points P (..., 3) in the view's image: section 31.2's table."""
    model = model_of(view)
    cam = np.asarray(view[1], F).reshape(4, 3)
    E, L, Hh, Vv = cam
    P = np.asarray(P, F)[..., :3]
    with np.errstate(all="ignore"):
        if model == 0:
            d = P - E
            Lr = L - E
            Nv = cross(Hh, Vv)
            k = dot(Lr, Nv) / dot(d, Nv)
            q = k[..., None] * d - Lr
            NN = dot(Nv, Nv)
            s, t = dot(cross(q, Vv), Nv) / NN, dot(cross(Hh, q), Nv) / NN
            front, dd = (k > 0) & ((k - k) == 0), dot(d, d)
        elif model == 1:
            _, _, f = basis(cam)
            q = P - L
            Nv = cross(Hh, Vv)
            NN = dot(Nv, Nv)
            s, t = dot(cross(q, Vv), Nv) / NN, dot(cross(Hh, q), Nv) / NN
            z = dot(q, f)
            front, dd = z > 0, z * z
        else:
            r, u, f = basis(cam)
            d = P - E
            X, Y, Z = dot(d, r), dot(d, u), dot(d, f)
            front, dd = np.ones(X.shape, bool), dot(d, d)
            if model == 2:
                phi = atan2(X, Z)
                theta = atan2(Y, np.sqrt(X * X + Z * Z))
                s, t = phi / TWO_PI + HALF, theta / PI + HALF
            elif model == 3:
                hyp = np.sqrt(X * X + Y * Y)
                theta = atan2(hyp, Z)
                rho = theta / ((F(view[2]) * DEG) * HALF)
                zero = hyp == 0
                a = np.where(zero, F(0), rho * (X / hyp))
                b = np.where(zero, F(0), rho * (Y / hyp))
                s, t = (a + ONE) * HALF, (b + ONE) * HALF
            else:
                raise ValueError(f"unknown model {model}")
        fx, fy = s * F(W), t * F(H)
    assert fx.dtype == F and fy.dtype == F and dd.dtype == F
    return fx, fy, front, dd


def project(posB, view, W, H):
    """(taps, x0, y0, a, b, dd) per pixel of B, as reproject_ref.project; x0 reaches W under
    an equirectangular view (fx == W passes its range test)."""
    fx, fy, front, dd = inverse(posB, view, W, H)
    wrap = model_of(view) == 2
    with np.errstate(all="ignore"):
        right = (fx <= F(W)) if wrap else (fx < F(W))
        taps = front & (fx >= F(-1)) & right & (fy >= F(-1)) & (fy < F(H))
        flx, fly = np.where(taps, np.floor(fx), F(0)).astype(F), np.where(taps, np.floor(fy), F(0)).astype(F)
        a, b = fx - flx, fy - fly
    return taps, flx.astype(np.int64), fly.astype(np.int64), a, b, dd


def tap_table(accum, moments, posA, nrmA, posB, nrmB, viewA, W, H, params=None):
    """reproject_ref.tap_table under view A's model: (hit, valid (H, W, 4), weights (H, W, 4),
    the taps' flat pixel indices (H, W, 4)).  An equirectangular view A wraps the tap column
    (xi < 0: xi + W; xi >= W: xi - W) and drops the x part of the `inside` test; the clamp
    behind the wrap only places a tap of weight 0 (column W + 1 of a one-column image)."""
    wrap = model_of(viewA) == 2
    with np.errstate(all="ignore"):
        p = dict(DEFAULTS, **(params or {}))
        posB, nrmB = np.asarray(posB, F), np.asarray(nrmB, F)
        posA, nrmA = np.asarray(posA, F).reshape(-1, 4), np.asarray(nrmA, F).reshape(-1, 4)
        mom = np.asarray(moments, F).reshape(-1, 4)
        hit = posB[..., 3] != 0
        taps, x0, y0, a, b, dd = project(posB, viewA, W, H)
        wgt = np.stack([(ONE - a) * (ONE - b), a * (ONE - b), (ONE - a) * b, a * b], axis=-1)
        tol = F(p["position_tolerance"])
        lim = (tol * tol) * dd
        valid = np.zeros((H, W, 4), bool)
        index = np.zeros((H, W, 4), np.int64)
        for i in range(4):
            xi, yi = x0 + (i & 1), y0 + (i >> 1)
            if wrap:
                xi = np.where(xi < 0, xi + W, np.where(xi >= W, xi - W, xi))
            inside = taps & (yi >= 0) & (yi < H)
            if not wrap:
                inside &= (xi >= 0) & (xi < W)
            at = np.clip(yi, 0, H - 1) * W + np.clip(xi, 0, W - 1)
            pa, na = posA[at], nrmA[at]
            e = pa[..., :3] - posB[..., :3]
            n = mom[at][..., 3].view(U)
            valid[..., i] = (hit & inside & (wgt[..., i] > 0) & (pa[..., 3] == ONE) & (na[..., 3] == nrmB[..., 3])
                             & (dot(na[..., :3], nrmB[..., :3]) >= F(p["normal_min"])) & (dot(e, e) <= lim) & (n >= 1))
            index[..., i] = at
    assert wgt.dtype == F and lim.dtype == F
    return hit, valid, wgt, index


def reproject(accum, moments, posA, nrmA, posB, nrmB, viewA, W, H, params=None):
    """One pnrt_reproject_view call -> (accumulation, moments, stats, valid taps per pixel
    (H, W), -1 on a miss).  A: the view the images were rendered with and the position /
    normal guide images of its centre rays; B: the guide images of the new view's."""
    p = dict(DEFAULTS, **(params or {}))
    with np.errstate(all="ignore"):
        hit, valid, wgt, index = tap_table(accum, moments, posA, nrmA, posB, nrmB, viewA, W, H, p)
        acc_in, mom_in = np.asarray(accum, F).reshape(-1, 4), np.asarray(moments, F).reshape(-1, 4)
        wsum = np.zeros((H, W), F)
        nmin = np.full((H, W), 0xFFFFFFFF, U)
        for i in range(4):
            v = valid[..., i]
            wsum = np.where(v, wsum + wgt[..., i], wsum)
            nmin = np.where(v, np.minimum(nmin, mom_in[index[..., i]][..., 3].view(U)), nmin)
        col = np.zeros((H, W, 3), F)
        mean, s2 = np.zeros((H, W), F), np.zeros((H, W), F)
        for i in range(4):
            v = valid[..., i]
            r = wgt[..., i] / wsum
            ta, tm = acc_in[index[..., i]], mom_in[index[..., i]]
            n = tm[..., 3].view(U)
            col = np.where(v[..., None], col + r[..., None] * ta[..., :3], col)
            mean = np.where(v, mean + r * tm[..., 0], mean)
            var = tm[..., 1] / np.maximum(n - U(1), U(1)).astype(F)      # (valid: n >= 1)
            s2 = np.where(v, s2 + r * var, s2)
        assert col.dtype == F and mean.dtype == F and s2.dtype == F
        got = valid.any(axis=-1)
        n1 = np.minimum(nmin, U(p["max_history"]))
        acc = np.zeros((H, W, 4), F)
        mom = np.zeros((H, W, 4), F)
        acc[got, :3] = col[got]
        acc[got, 3] = 1
        mom[got, 0] = mean[got]
        mom[got, 1] = (s2 * (n1 - U(1)).astype(F))[got]
        mom[..., 3].view(U)[got] = n1[got]
    stats = {"n_pixels": W * H, "n_reprojected": int(got.sum()), "n_disoccluded": int((hit & ~got).sum()),
             "n_missed": int((~hit).sum()), "sum_frames": int(n1[got].astype(np.int64).sum()),
             "max_frames": int(n1[got].max()) if got.any() else 0}
    return acc, mom, stats, np.where(hit, valid.sum(axis=-1), -1)
