"""Shared by tests/test_gpu_moments*.py -- TEST INFRASTRUCTURE: exact per-frame
colours from the CPU oracle, which only hands out accumulation images.

Where the blend weight a = 1 / (f + 1) is a power of two, one frame rendered into
a zeroed image is 0 * (1 - a) + c * a = c * a exactly (as long as no nonzero
component of it is subnormal), so c = image * (f + 1), exactly.  `anchor` takes
frames 0, 1, 3, 7 and 15 that way, and asserts the premise itself: the numpy
replay of the blend over those colours must equal the oracle's own accumulation of
the same calls, bit for bit -- a scene where the trick fails is a test error, not
a false pass."""
from __future__ import annotations

import functools

import numpy as np

import moments_ref as R
import pyoracle
from guides_common import bits, scene

F = np.float32
ANCHOR_FRAMES = (0, 1, 3, 7, 15)
# the calls that render exactly those frames
ANCHOR_CALLS = ((0, 2), (3, 1), (7, 1), (15, 1))


@functools.lru_cache(maxsize=None)
def anchor(name: str, width: int, height: int):
    """(colours of ANCHOR_FRAMES, the oracle's accumulation of ANCHOR_CALLS, the
    restatement's moments of those colours); read-only arrays, computed once."""
    cfg = scene(name, width, height)
    o = pyoracle.Oracle(cfg)
    colors = []
    for f in ANCHOR_FRAMES:
        img, st = o.render(f, 1)
        assert st["stack_overflow"] == 0
        rgb = img[..., :3]
        tiny = (rgb != 0) & (np.abs(rgb) < np.finfo(F).tiny)
        assert not tiny.any(), "a subnormal component: the frame's colour is not recoverable exactly"
        c = (rgb * F(f + 1)).astype(F)
        assert np.array_equal(bits((c * (F(1) / F(f + 1))).astype(F)), bits(rgb)), "round trip of the colour"
        c.setflags(write=False)
        colors.append(c)
    acc = np.zeros((height, width, 4), F)
    for first, n in ANCHOR_CALLS:
        o.render(first, n, accum=acc)
    replay = R.blend(np.zeros((height, width, 4), F), colors, ANCHOR_FRAMES)
    assert np.array_equal(bits(replay[..., :3]), bits(acc[..., :3])), \
        f"{name} {width}x{height}: the replay of the blend over the derived colours is not the oracle's accumulation"
    mom = R.update(R.zeros(height, width), colors, ANCHOR_FRAMES)
    assert (mom[..., 1] >= 0).all()
    acc.setflags(write=False)
    mom.setflags(write=False)
    return tuple(colors), acc, mom
