"""tests/atrous_ref.py (the numpy restatement of DESIGN.md section 20.2 the GPU
denoiser is compared with) on synthetic guides: its pass-through rule, the
weight 0 of pass-through taps, and the 1x1 image computed by hand."""
import numpy as np
import pytest

from atrous_ref import ALBEDO_MIN, atrous_ref, passthrough, pn_max

F = np.float32
W, H = 13, 9


def _materials():
    m = np.zeros((3, 18), F)
    m[0, 3:6] = 0.65                      # diffuse
    m[1, 3:6] = (0.1, 0.5, 0.2)
    m[2, 0:3] = (0.0, 60.0, 0.0)          # emissive in one component only
    m[2, 3:6] = 0.73
    return m


def _scene(seed=5):
    rng = np.random.default_rng(seed)
    accum = rng.random((H, W, 4)).astype(F)
    accum[..., 3] = 1
    # a gently curved surface: neighbouring taps keep weights well above zero
    yy, xx = np.mgrid[0:H, 0:W]
    pos = np.stack([xx * 0.05, yy * 0.05, 0.01 * np.sin(xx * 0.7) + rng.normal(0, 0.002, (H, W)), np.ones((H, W))], -1).astype(F)
    n = np.stack([0.05 * np.cos(xx * 0.7), rng.normal(0, 0.02, (H, W)), np.ones((H, W))], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    mat = rng.integers(0, 2, (H, W, 1))
    nrm = np.concatenate([n, mat], -1).astype(F)
    alb = np.concatenate([rng.random((H, W, 3)) * 0.9, -np.ones((H, W, 1))], -1).astype(F)
    alb[0, 0, :3] = (0.0, 1e-4, 0.5)      # below and above the 1/256 floor
    # misses: a block and a scattered few; emissive hits: a row segment
    for y, x in [(2, 3), (2, 4), (3, 3), (3, 4), (8, 12), (0, 7)]:
        pos[y, x] = 0
        nrm[y, x] = (0, 0, 0, -1)
        alb[y, x] = (0.3, 0.2, 0.9, -1)
    nrm[6, 2:6, 3] = 2
    return accum, pos, nrm, alb


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_passthrough_rule():
    accum, pos, nrm, alb = _scene()
    pt = passthrough(pos, nrm, _materials())
    want = np.zeros((H, W), bool)
    for y, x in [(2, 3), (2, 4), (3, 3), (3, 4), (8, 12), (0, 7)]:
        want[y, x] = True
    want[6, 2:6] = True
    assert np.array_equal(pt, want)


@pytest.mark.parametrize("levels", [1, 3, 5])
def test_passthrough_pixels_come_back_bit_identical(levels):
    accum, pos, nrm, alb = _scene()
    accum[2, 3] = (0.25, 7.0, -0.0, 0.5)          # any four floats, alpha included
    pt = passthrough(pos, nrm, _materials())
    out = atrous_ref(accum, pos, nrm, alb, _materials(), levels=levels)
    assert np.array_equal(_bits(out[pt]), _bits(accum[pt]))
    assert np.all(out[~pt][:, 3] == 1)
    assert np.all(np.isfinite(out[~pt]))
    assert not np.array_equal(_bits(out[~pt]), _bits(accum[~pt]))     # the others are filtered


@pytest.mark.parametrize("levels", [1, 4])
def test_passthrough_pixel_contributes_nothing(levels):
    """Its colour (and its guides) may change: no other pixel's output does."""
    accum, pos, nrm, alb = _scene()
    mats = _materials()
    pt = passthrough(pos, nrm, mats)
    base = atrous_ref(accum, pos, nrm, alb, mats, levels=levels)
    a2, n2, al2 = accum.copy(), nrm.copy(), alb.copy()
    a2[pt] = (1e6, 0.0, 123.0, 0.0)
    al2[pt, :3] = (5.0, 5.0, 5.0)
    n2[6, 2:6, :3] = (0.0, 1.0, 0.0)               # the emissive hits' normals
    out = atrous_ref(a2, pos, n2, al2, mats, levels=levels)
    assert np.array_equal(_bits(out[~pt]), _bits(base[~pt]))
    assert np.array_equal(_bits(out[pt]), _bits(a2[pt]))
    # ... whereas an ordinary pixel's colour does reach its neighbours
    a3 = accum.copy()
    a3[5, 8, :3] += F(0.125)
    assert not pt[5, 8]
    out3 = atrous_ref(a3, pos, nrm, alb, mats, levels=levels)
    assert not np.array_equal(_bits(out3[5, 7]), _bits(base[5, 7]))


def test_one_pixel_image_by_hand():
    """1x1, one level: only the centre tap is inside, e = 0, exp2(0) = 1, w = 9/64:
    c1 = (w * c0) / w per channel, and the output is c1 * max(albedo, 1/256)."""
    accum = np.array([[[0.3, 0.7, 0.011, 1.0]]], F)
    pos = np.array([[[1.0, 2.0, 3.0, 1.0]]], F)
    nrm = np.array([[[0.0, 0.6, 0.8, 0.0]]], F)
    alb = np.array([[[0.65, 1e-3, 0.0, -1.0]]], F)
    out = atrous_ref(accum, pos, nrm, alb, _materials(), levels=1)
    m = pn_max(alb[0, 0, :3], ALBEDO_MIN)
    assert np.array_equal(m, np.array([0.65, 1 / 256, 1 / 256], F))
    w = F(F(0.375) * F(0.375)) * F(1.0)
    want = np.empty(4, F)
    for k in range(3):
        c0 = F(accum[0, 0, k] / m[k])
        c1 = F(F(F(0) + F(w * c0)) / F(F(0) + w))
        want[k] = F(c1 * m[k])
    want[3] = 1
    assert np.array_equal(_bits(out[0, 0]), _bits(want))
    # the round trip is not the identity in general, but it is within an ulp or two
    assert np.allclose(out[0, 0, :3], accum[0, 0, :3], rtol=4 * 2.0 ** -24, atol=0)


def test_one_pixel_passthrough():
    accum = np.array([[[0.3, 0.7, 0.011, 1.0]]], F)
    zero = np.zeros((1, 1, 4), F)
    nrm = np.array([[[0, 0, 0, -1]]], F)
    out = atrous_ref(accum, zero, nrm, zero, _materials(), levels=5)
    assert np.array_equal(_bits(out), _bits(accum))


def test_uniform_image_is_a_fixed_point_up_to_rounding():
    """Constant colour over constant albedo and flat guides: every weight is h, the
    mean of equal values is that value up to the sums' rounding."""
    accum = np.full((H, W, 4), 0.4, F)
    pos = np.zeros((H, W, 4), F); pos[..., 3] = 1
    nrm = np.zeros((H, W, 4), F); nrm[..., 2] = 1
    alb = np.full((H, W, 4), 0.5, F)
    out = atrous_ref(accum, pos, nrm, alb, _materials(), levels=5)
    assert np.allclose(out[..., :3], 0.4, rtol=1e-5, atol=0)
