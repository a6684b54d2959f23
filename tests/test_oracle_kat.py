"""Oracle known-answer tests and PN-libm accuracy."""
import ctypes

import numpy as np
import pytest

import pyoracle
from pnraytracing_amd import scenes as S


def stream(x, y, f, n=3):
    L = pyoracle.lib()
    s = ctypes.c_uint32(((x * 1973 + y * 9277 + f * 26699) | 1) & 0xFFFFFFFF)
    return [L.pno_wang_hash(ctypes.byref(s)) for _ in range(n)]


def test_wang_hash_streams():
    # ray_tracing.comp:499-506 seeded as :977-979
    assert stream(0, 0, 0) == [663891101, 1738326990, 801461103]
    assert stream(100, 37, 0) == [1655212983, 1951060585, 2443051288]
    assert stream(100, 37, 3) == [2397685232, 4113837163, 1495352338]


def test_sobol_first_point_is_half():
    L = pyoracle.lib()
    # gray(1) = 1 and V[32 d] = 2^31 for every dimension
    assert all(L.pno_sobol(d, 1) == 0.5 for d in range(8))


def _gray(i):
    return i ^ (i >> 1)


def _sobol_indices():
    idx = [1 << j for j in range(32)] + [0xFFFFFFFF]
    for k in (8, 16, 24, 31):                     # grayCode(frameCount + 1) around a new top bit
        idx += [_gray(2**k - 1), _gray(2**k), _gray(2**k + 1)]
    rng = np.random.default_rng(20)
    return idx + [int(v) for v in rng.integers(0, 2**32, 1000, dtype=np.uint64)]


def test_sobol_matches_integer_reference():
    """pno_sobol(d, i) for all 8 dimensions against an integer reference built from
    the committed direction table (tests/golden/sobol_v.json): the XOR of the
    table entries of i's set bits in Python ints, then the shader's one float
    multiply -- exactly, for every single bit (bits 8..31 are the ones frame
    numbers above 255 set), all bits, the gray codes around 2^8, 2^16, 2^24 and
    2^31, and 1000 random 32-bit indices."""
    import json
    import os
    V = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sobol_v.json")))["V"]
    assert len(V) == 256 and all(0 <= v < 2**32 for v in V)
    L = pyoracle.lib()
    scale = np.float32(1) / np.float32(0xFFFFFFFF)
    for d in range(8):
        for i in _sobol_indices():
            r = 0
            for j in range(32):
                if (i >> j) & 1:
                    r ^= V[32 * d + j]
            want = np.float32(r) * scale
            got = np.float32(L.pno_sobol(d, i))
            assert got.view(np.uint32) == want.view(np.uint32), (d, hex(i), got, want)
    # a sample of exactly 1.0, outside [0, 1): the shader's own arithmetic, kept as it is
    assert L.pno_sobol(1, 0x80000000) == 1.0


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7FFFFFFF), a)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b)
    return np.abs(a - b)


@pytest.mark.parametrize("fn,lo,hi,ref,tol", [
    (0, -7.0, 7.0, np.sin, 4), (1, -7.0, 7.0, np.cos, 4),
    (3, -1.0, 1.0, np.arcsin, 3), (4, 1e-6, 100.0, np.log, 3), (6, -20.0, 20.0, np.exp2, 3)])
def test_libm_accuracy(fn, lo, hi, ref, tol):
    """PN-libm vs correctly rounded double on the argument ranges the shader
    uses (absolute error near zeros of sin/cos measured against 1e-7)."""
    x = np.linspace(lo, hi, 200001, dtype=np.float32)
    got = pyoracle.math_eval(fn, x)
    exact = ref(x.astype(np.float64))
    err = np.abs(got.astype(np.float64) - exact)
    ok = (_ulps(got, exact.astype(np.float32)) <= tol) | (err <= 2e-7)
    assert ok.all(), (x[~ok][:5], got[~ok][:5], exact[~ok][:5])


def test_atan2_accuracy():
    rng = np.random.default_rng(1)
    y = rng.uniform(-3, 3, 100000).astype(np.float32)
    x = rng.uniform(-3, 3, 100000).astype(np.float32)
    got = pyoracle.math_eval(2, y, x).astype(np.float64)
    assert np.max(np.abs(got - np.arctan2(y.astype(np.float64), x.astype(np.float64)))) < 1e-6
    assert pyoracle.math_eval(2, np.zeros(1, np.float32), np.zeros(1, np.float32))[0] == 0.0


def test_pow_matches_glsl_definition():
    a = np.float32(np.linspace(1e-6, 0.01, 1000))
    y = np.float32(np.linspace(0.0, 1.0, 1000))
    got = pyoracle.math_eval(5, a, y).astype(np.float64)
    np.testing.assert_allclose(got, np.power(a.astype(np.float64), y.astype(np.float64)), rtol=2e-6)


def test_oracle_progressive_mean_is_order_exact():
    """4 frames in one call == 4 single-frame calls (the accumulate contract)."""
    o = pyoracle.Oracle(S.cornell_c1(64, 64))
    a, _ = o.render(0, 4)
    b = np.zeros_like(a)
    for f in range(4):
        o.render(f, 1, accum=b)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_oracle_rows_are_independent():
    """Any row partition renders the same pixels (the multi-GPU sharding premise)."""
    o = pyoracle.Oracle(S.cornell_c1(48, 48))
    full, _ = o.render(3, 2)
    part = np.zeros_like(full)
    o.render(3, 2, rows=(0, 48), y_step=2, accum=part)
    o.render(3, 2, rows=(1, 48), y_step=2, accum=part)
    np.testing.assert_array_equal(full.view(np.uint32), part.view(np.uint32))


def test_oracle_c1_stats_sane():
    o = pyoracle.Oracle(S.cornell_c1(32, 32))
    acc, st = o.render(0, 1)
    assert st["samples"] == 32 * 32 and st["stack_overflow"] == 0
    assert np.isfinite(acc).all() and (acc[..., :3] >= 0).all() and (acc[..., :3] <= 1).all()
    assert (acc[..., 3] == 1).all()


def test_c1_image_fixture_is_current_oracle():
    """tests/golden/c1_oracle_image.npz (the C-ABI caller's expected image) is the
    current oracle's render, bit for bit."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_c1_image
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "c1_oracle_image.npz"))
    np.testing.assert_array_equal(make_c1_image.render().view(np.uint32), gold["image"].view(np.uint32))


@pytest.mark.parametrize("name", ["c1", "c2wide", "c3"])
def test_render_colors_are_the_frames_the_render_blends(name):
    """Oracle.render_colors hands out the clamped colour of any frame: blended by moments_ref.blend, frames
    0..12 give Oracle.render's accumulation bit for bit, and at frames 0, 1, 3, 7 and 15 the colours are
    the ones moments_common.anchor derives from single-frame renders."""
    import moments_ref as R
    from guides_common import bits, scene
    from moments_common import ANCHOR_FRAMES, anchor
    w, h = 13, 9
    o = pyoracle.Oracle(scene(name, w, h))
    acc, st = o.render(0, 13)
    colors, cst = o.render_colors(0, 13)
    assert colors.shape == (13, h, w, 3) and colors.dtype == np.float32
    assert (colors >= 0).all() and (colors <= 1).all() and colors.any()
    assert cst["samples"] == st["samples"] == 13 * w * h and cst["accum_rmw"] == 0 and st["stack_overflow"] == 0
    replay = R.blend(np.zeros((h, w, 4), np.float32), colors, range(13))
    assert np.array_equal(bits(replay), bits(acc))
    # a call that starts later, and rows: the same colours
    later, _ = o.render_colors(5, 3, rows=(2, 7), y_step=2)
    assert np.array_equal(bits(later[:, 2:7:2]), bits(colors[5:8, 2:7:2]))
    assert not later[:, [0, 1, 3, 5, 7, 8]].any()
    derived, _, _ = anchor(name, w, h)
    for f, c in zip(ANCHOR_FRAMES, derived):
        got, _ = o.render_colors(f, 1)
        assert np.array_equal(bits(got[0]), bits(c)), f"frame {f}"
