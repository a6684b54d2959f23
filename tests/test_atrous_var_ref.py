"""tests/atrous_var_ref.py (the numpy restatement of DESIGN.md section 24.2 that
pnrt_denoise_variance is compared with) on small synthetic inputs: what the
variance does to an edge and to noise, the unmeasured-pixel branch of step 3, the
prefilter of step 5a beside a pass-through pixel (one pixel recomputed with
scalars), finiteness, and that nothing is read from a pass-through pixel."""
import numpy as np
import pytest

from atrous_ref import ALBEDO_MIN, H5, pn_max, passthrough
from atrous_var_ref import DEFAULTS, EPS, K3, atrous_var_ref, initial_variance
from moments_ref import luminance

F = np.float32
U = np.uint32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _materials():
    m = np.zeros((3, 18), F)
    m[0, 3:6] = 0.65                      # diffuse
    m[1, 3:6] = (0.1, 0.5, 0.2)
    m[2, 0:3] = (0.0, 60.0, 0.0)          # emissive in one component only
    return m


def _moments(mean, m2, n):
    out = np.zeros(mean.shape + (4,), F)
    out[..., 0], out[..., 1] = mean, m2
    out[..., 3] = np.broadcast_to(np.asarray(n, U), mean.shape).copy().view(F)
    return out


# ---- a luminance step edge on flat geometry ------------------------------------------------
EW, EH, EDGE = 48, 16, 24
LO, HI = 0.1, 0.4                         # the accumulation's grey levels left and right of the edge
N_FRAMES = 16


def _edge(sigma, seed=3):
    """One normal, coplanar positions, albedo 1/2; grey noise of standard deviation sigma on
    the accumulation and the moments that go with it: M2 / (n - 1) / n = sigma^2."""
    yy, xx = np.mgrid[0:EH, 0:EW]
    clean = np.where(xx < EDGE, F(LO), F(HI)).astype(F)
    noise = np.random.default_rng(seed).normal(0, sigma, (EH, EW)).astype(F) if sigma else np.zeros((EH, EW), F)
    accum = np.ones((EH, EW, 4), F)
    accum[..., :3] = (clean + noise)[..., None]
    pos = np.stack([xx * 0.01, yy * 0.01, np.zeros((EH, EW)), np.ones((EH, EW))], -1).astype(F)
    nrm = np.zeros((EH, EW, 4), F); nrm[..., 2] = 1
    alb = np.full((EH, EW, 4), 0.5, F)
    var = max(sigma, 1e-7) ** 2            # "near 0": a standard error of 1e-7
    mom = _moments(luminance(accum), np.full((EH, EW), var * N_FRAMES * (N_FRAMES - 1), F), N_FRAMES)
    return accum, pos, nrm, alb, mom, clean


def test_edge_survives_where_the_variance_is_near_zero():
    accum, pos, nrm, alb, mom, clean = _edge(0.0)
    out = atrous_var_ref(accum, pos, nrm, alb, _materials(), mom)
    lum_in, lum_out = luminance(accum), luminance(out)
    contrast = HI - LO
    for side in (np.s_[:, :EDGE], np.s_[:, EDGE:]):
        assert abs(float(lum_out[side].mean()) - float(lum_in[side].mean())) < contrast / 100
    # ... and not as a matter of means alone: no pixel moved by that much
    assert np.abs(lum_out - lum_in).max() < contrast / 100


def test_noise_in_the_flat_regions_drops():
    sigma = 0.01
    accum, pos, nrm, alb, mom, clean = _edge(sigma)
    out = atrous_var_ref(accum, pos, nrm, alb, _materials(), mom, levels=3)
    # the flat regions: further from the edge than the 2 * (1 + 2 + 4) pixels three levels reach
    flat = np.ones((EH, EW), bool)
    flat[:, EDGE - 14:EDGE + 14] = False
    assert flat.sum() >= 2 * 10 * EH

    def rmse(img):
        return float(np.sqrt(np.mean((luminance(img)[flat].astype(np.float64) - clean[flat]) ** 2)))
    before, after = rmse(accum), rmse(out)
    assert 0.5 * sigma < before < 2 * sigma
    # the 5x5 B3 kernel alone leaves sqrt(sum h^2)^2 = 0.27 of white noise; half is a safe bound
    assert after < 0.5 * before, (before, after)
    # the edge is still there: both sides' means within a standard deviation of the clean levels
    lum = luminance(out)
    assert abs(float(lum[:, :EDGE].mean()) - LO) < sigma and abs(float(lum[:, EDGE:].mean()) - HI) < sigma


# ---- a small irregular scene ---------------------------------------------------------------
W, H = 13, 9
PT = [(2, 3), (2, 4), (3, 3), (3, 4), (8, 12), (0, 7)]


def _scene(seed=5):
    rng = np.random.default_rng(seed)
    accum = rng.random((H, W, 4)).astype(F)
    accum[..., 3] = 1
    yy, xx = np.mgrid[0:H, 0:W]
    pos = np.stack([xx * 0.05, yy * 0.05, 0.01 * np.sin(xx * 0.7) + rng.normal(0, 0.002, (H, W)), np.ones((H, W))], -1).astype(F)
    n = np.stack([0.05 * np.cos(xx * 0.7), rng.normal(0, 0.02, (H, W)), np.ones((H, W))], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    nrm = np.concatenate([n, rng.integers(0, 2, (H, W, 1))], -1).astype(F)
    alb = np.concatenate([rng.random((H, W, 3)) * 0.9, -np.ones((H, W, 1))], -1).astype(F)
    alb[0, 0, :3] = (0.0, 1e-4, 0.5)      # below and above the 1/256 floor
    for y, x in PT:                       # misses
        pos[y, x] = 0
        nrm[y, x] = (0, 0, 0, -1)
        alb[y, x] = (0.3, 0.2, 0.9, -1)
    nrm[6, 2:6, 3] = 2                    # emissive hits
    cnt = rng.integers(2, 40, (H, W)).astype(U)
    cnt[1, 1], cnt[4, 9], cnt[7, 0] = 0, 1, 1          # unmeasured pixels
    accum[1, 1, :3] = 0                                # ... one of them never rendered
    mom = _moments(luminance(accum), (rng.random((H, W)) * 0.5).astype(F), cnt)
    mom[5, 5, 1] = 0                                   # a measured pixel without variance
    return accum, pos, nrm, alb, mom


def test_unmeasured_pixels_take_the_square_of_their_luminance():
    accum, pos, nrm, alb, mom = _scene()
    m = pn_max(alb[..., :3], ALBEDO_MIN)
    c0 = (accum[..., :3] / m).astype(F)
    v0 = initial_variance(c0, m, mom)
    for y, x in [(1, 1), (4, 9), (7, 0)]:
        l = luminance(c0[y, x])
        assert _bits(v0[y, x]) == _bits(F(l * l))
    assert v0[1, 1] == 0                               # finite, whatever M2 holds
    # a measured one, with scalars
    y, x = 3, 7
    n = int(mom[y, x, 3].view(U))
    assert n >= 2
    lm = luminance(m[y, x])
    want = F(F(F(mom[y, x, 1] / F(n - 1)) / F(n)) / F(lm * lm))
    assert _bits(v0[y, x]) == _bits(want)
    assert np.all(np.isfinite(v0))


def _one_pixel_one_level(y, x, accum, pos, nrm, alb, mats, mom, sv, sn, sp, exp2):
    """Section 24.2 for one pixel and levels = 1, with scalars and explicit loops."""
    pt = passthrough(pos, nrm, mats)
    m = pn_max(alb[..., :3], ALBEDO_MIN)
    c = (accum[..., :3] / m).astype(F)
    v = initial_variance(c, m, mom)
    hh, ww = pt.shape
    inn, ipp = F(1) / F(F(sn) * F(sn)), F(1) / F(F(sp) * F(sp))
    G = K = F(0)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            qy, qx = y + dy, x + dx
            if not (0 <= qy < hh and 0 <= qx < ww) or pt[qy, qx]:
                continue
            k = F(K3[dy + 1] * K3[dx + 1])
            G = F(G + F(k * v[qy, qx]))
            K = F(K + k)
    r = F(F(1) / F(F(F(sv) * np.sqrt(F(G / K))) + EPS))

    def d2(a, b):
        d = (a - b).astype(F)
        return F(F(F(d[0] * d[0]) + F(d[1] * d[1])) + F(d[2] * d[2]))
    lc = luminance(c[y, x])
    Wt = X = Y = Z = F(0)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            qy, qx = y + dy, x + dx
            if not (0 <= qy < hh and 0 <= qx < ww) or pt[qy, qx]:
                continue
            e = F(np.abs(F(luminance(c[qy, qx]) - lc)) * r)
            e = F(e + F(d2(nrm[qy, qx, :3], nrm[y, x, :3]) * inn))
            e = F(e + F(d2(pos[qy, qx, :3], pos[y, x, :3]) * ipp))
            w = F(F(H5[dy + 2] * H5[dx + 2]) * exp2(np.array([-e], F))[0])
            Wt = F(Wt + w)
            X, Y, Z = F(X + F(w * c[qy, qx, 0])), F(Y + F(w * c[qy, qx, 1])), F(Z + F(w * c[qy, qx, 2]))
    out = np.array([F(F(X / Wt) * m[y, x, 0]), F(F(Y / Wt) * m[y, x, 1]), F(F(Z / Wt) * m[y, x, 2]), 1], F)
    return out, G, K


def test_prefilter_skips_a_passthrough_neighbour():
    """(2, 2) has the misses (2, 3) and (3, 3) among its nine neighbours; (0, 0) has five
    outside the image; (4, 8) has the unmeasured (4, 9)."""
    from atrous_ref import oracle_exp2
    accum, pos, nrm, alb, mom = _scene()
    mats = _materials()
    p = {"sigma_variance": 3.0, "sigma_normal": 0.5, "sigma_position": 1.5}
    got = atrous_var_ref(accum, pos, nrm, alb, mats, mom, levels=1, **p)
    sums = {}
    for y, x in [(2, 2), (0, 0), (4, 8), (5, 5)]:
        want, G, K = _one_pixel_one_level(y, x, accum, pos, nrm, alb, mats, mom, p["sigma_variance"], p["sigma_normal"],
                                          p["sigma_position"], oracle_exp2)
        assert np.array_equal(_bits(got[y, x]), _bits(want)), (y, x)
        sums[(y, x)] = float(K)
    assert sums[(2, 2)] == 1 - 1 / 8 - 1 / 16          # the weights of (0, +1) and (+1, +1) are missing
    assert sums[(0, 0)] == 1 / 4 + 1 / 8 + 1 / 8 + 1 / 16
    assert sums[(4, 8)] == 1
    assert sums[(5, 5)] == 1 - 1 / 8 - 1 / 16          # the emissive hits (6, 4) and (6, 5)
    # the skipped neighbours' variance is not in G either: another value there changes nothing
    mom2 = mom.copy()
    mom2[2, 3, 1] = mom2[3, 3, 1] = 1e9
    again = atrous_var_ref(accum, pos, nrm, alb, mats, mom2, levels=1, **p)
    assert np.array_equal(_bits(again[2, 2]), _bits(got[2, 2]))


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_finite_inputs_give_finite_outputs(levels):
    accum, pos, nrm, alb, mom = _scene()
    pt = passthrough(pos, nrm, _materials())
    out = atrous_var_ref(accum, pos, nrm, alb, _materials(), mom, levels=levels)
    assert np.all(np.isfinite(out))
    assert np.array_equal(_bits(out[pt]), _bits(accum[pt]))
    assert np.all(out[~pt][:, 3] == 1)
    assert not np.array_equal(_bits(out[~pt]), _bits(accum[~pt]))
    # a black image with nothing measured: variance 0 everywhere, r = 2^20, still finite
    out0 = atrous_var_ref(np.zeros_like(accum), pos, nrm, alb, _materials(), np.zeros_like(mom), levels=levels)
    assert np.all(np.isfinite(out0)) and np.all(out0[~pt][:, :3] == 0)


@pytest.mark.parametrize("levels", [1, 4])
def test_nothing_is_read_from_a_passthrough_pixel(levels):
    """Its colour, its albedo and its moments may hold anything, NaN included."""
    accum, pos, nrm, alb, mom = _scene()
    mats = _materials()
    pt = passthrough(pos, nrm, mats)
    base = atrous_var_ref(accum, pos, nrm, alb, mats, mom, levels=levels)
    a2, al2, m2 = accum.copy(), alb.copy(), mom.copy()
    a2[pt] = (1e6, 0.0, np.nan, 0.0)
    al2[pt, :3] = (5.0, 0.0, 5.0)
    m2[pt] = _moments(np.full(1, np.inf, F), np.full(1, np.nan, F), 7)[0]
    out = atrous_var_ref(a2, pos, nrm, al2, mats, m2, levels=levels)
    assert np.array_equal(_bits(out[~pt]), _bits(base[~pt]))
    assert np.array_equal(_bits(out[pt]), _bits(a2[pt]))
    # ... whereas an ordinary pixel's variance does reach its neighbours
    m3 = mom.copy()
    m3[5, 8, 1] *= F(64)
    assert not pt[5, 8]
    out3 = atrous_var_ref(accum, pos, nrm, alb, mats, m3, levels=levels)
    assert not np.array_equal(_bits(out3[5, 7]), _bits(base[5, 7]))


def test_defaults():
    assert DEFAULTS == {"levels": 5, "sigma_variance": 4.0, "sigma_normal": 0.25, "sigma_position": 0.5}
    assert EPS == F(2.0 ** -20) and np.array_equal(K3, np.array([0.25, 0.5, 0.25], F))
