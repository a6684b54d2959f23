"""tests/moments_ref.py -- the numpy restatement of DESIGN.md section 21 -- checked
for sanity on the CPU: against a float64 two-pass variance (a sanity check of the
restatement, not a parity claim), the frame-0 restart, the unmeasured pixels, and
the additivity of the statistics over disjoint row sets."""
import numpy as np

import moments_ref as R
from pnraytracing_amd.tracer import merge_convergence, shard_rows

F = np.float32


def _frames(seed, k, h=9, w=13):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0, 1, (h, w, 3)).astype(F) for _ in range(k)]


def test_moments_match_a_two_pass_variance():
    cols = _frames(1, 24)
    m = R.update(R.zeros(9, 13), cols, range(24))
    assert (R.frames_of(m) == 24).all() and (m[..., 2] == 0).all()
    y = np.stack([R.luminance(c) for c in cols]).astype(np.float64)
    mean, m2 = y.mean(axis=0), ((y - y.mean(axis=0)) ** 2).sum(axis=0)
    assert np.allclose(m[..., 0], mean, rtol=1e-5, atol=0)
    big = m2 > 1e-6
    assert big.all()                                 # uniform colours: every pixel has a variance to compare
    assert np.allclose(m[..., 1][big], m2[big], rtol=1e-4, atol=0)
    # the error image follows from them
    e = R.error(m)
    want = np.sqrt(m2 / 23 / 24) / np.maximum(mean, 1 / 256)
    assert np.allclose(e, want, rtol=2e-4, atol=0)


def test_frame_zero_restarts():
    cols = _frames(2, 6)
    m = R.update(R.zeros(9, 13), cols[:4], [5, 6, 7, 8])
    assert (R.frames_of(m) == 4).all()
    again = R.update(m, cols[4:], [0, 1])            # the session's redraw: frame 0 again
    fresh = R.update(R.zeros(9, 13), cols[4:], [0, 1])
    assert np.array_equal(again.view(np.uint32), fresh.view(np.uint32))
    one = R.update(m, cols[4:5], [0])
    assert (R.frames_of(one) == 1).all() and (one[..., 1] == 0).all()
    assert np.array_equal(one[..., 0].view(np.uint32), R.luminance(cols[4]).view(np.uint32))


def test_unmeasured_pixels_and_the_clamp():
    m = R.zeros(2, 3)
    m[..., 3] = np.array([[0, 1, 2], [2, 2, 2]], np.uint32).view(F)
    m[0, 2, :2] = (0.5, 0.125)                       # var 0.125, sem 0.25, e 0.5
    m[1, 0, :2] = (0.0, 2.0)                         # mean below 1/256: divided by 1/256 -> 256
    m[1, 1, :2] = (1e-30, 3e38)                      # clamped
    m[1, 2, :2] = (1.0, np.nan)                      # NaN compares false: 65535
    e = R.error(m)
    assert np.isposinf(e[0, 0]) and np.isposinf(e[0, 1])
    assert e[0, 2] == F(0.5) and e[1, 0] == F(256.0) and e[1, 1] == F(65535.0) and e[1, 2] == F(65535.0)
    s = R.stats(m, 0.5)
    assert s == {"n_pixels": 6, "n_measured": 4, "n_above": 3, "sum_q16": 32768 + 256 * 65536 + 2 * 65535 * 65536,
                 "max_error": 65535.0, "min_frames": 0, "max_frames": 2,
                 "mean_error": (32768 + 256 * 65536 + 2 * 65535 * 65536) / 65536 / 4}
    assert R.stats(m, 0.5, rows=[]) == {"n_pixels": 0, "n_measured": 0, "n_above": 0, "sum_q16": 0, "max_error": 0.0,
                                        "min_frames": 0, "max_frames": 0, "mean_error": 0.0}


def test_frame_count_saturates():
    m = R.zeros(1, 1)
    m[..., 3] = np.array([0xFFFFFFFE], np.uint32).view(F)
    c = np.full((1, 1, 3), 0.5, F)
    m = R.update(m, [c], [7])
    assert R.frames_of(m)[0, 0] == 0xFFFFFFFF
    m = R.update(m, [c], [8])
    assert R.frames_of(m)[0, 0] == 0xFFFFFFFF


def test_statistics_of_disjoint_rows_add_up():
    h, w = 45, 7
    cols = _frames(3, 5, h, w)
    m = R.update(R.zeros(h, w), cols, range(5))
    # rows of shard 1 saw two frames fewer, one row saw a single frame (unmeasured)
    r1 = shard_rows(h, 8, 2, 1)
    m[r1] = R.update(R.zeros(h, w), cols[:3], range(3))[r1]
    m[44] = R.update(R.zeros(h, w), cols[:1], [0])[44]
    full = R.stats(m, 0.125)
    assert 0 < full["n_above"] < full["n_measured"] == (h - 1) * w < full["n_pixels"] == h * w
    assert (full["min_frames"], full["max_frames"]) == (1, 5)
    parts = [R.stats(m, 0.125, rows=shard_rows(h, 8, 2, k)) for k in range(2)]
    assert merge_convergence(parts) == full
    thirds = [R.stats(m, 0.125, rows=shard_rows(h, 4, 3, k)) for k in range(3)]
    assert merge_convergence(thirds + [R.stats(m, 0.125, rows=[])]) == full
