"""The per-pixel sample moments, the error image and the convergence statistics
(pnrt_enable_moments / pnrt_read_moments / pnrt_read_error / pnrt_convergence,
pt_moments.h) against tests/moments_ref.py, the numpy restatement of DESIGN.md
section 21, on per-frame colours taken exactly from the CPU oracle
(tests/moments_common.py); batching, call shape, shards, lifecycle, and that a
context which never enables them launches and renders what it always did.

Tolerance: 0 ulp everywhere (uint32 views and integers compared)."""
import contextlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import moments_ref as R
import pyoracle
from guides_common import SHAPES, bits, scene
from moments_common import ANCHOR_CALLS, anchor
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_ZCULL, PathTracer, PnrtError, merge_convergence, shard_rows

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = SHAPES[0]
E_ARG, E_STATE = -1, -3


@pytest.fixture()
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, what
    bad = np.argwhere(g != w)
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.size} words differ, first {bad[:4].tolist()}"


def code_of(call, *a):
    with pytest.raises(PnrtError) as e:
        call(*a)
    return e.value.code


# ---- 4. anchor ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["c1", "c2wide", "c3"])
def test_anchor(pt, name, shape):
    w, h = shape
    _, acc, mom = anchor(name, w, h)
    pt.load(scene(name, w, h))
    assert pt.moments_ptr() == 0
    pt.enable_moments()
    assert pt.moments_ptr() != 0
    for first, n in ANCHOR_CALLS:
        pt.render(first, n)
    got = pt.read_moments()
    assert (R.frames_of(got) == 5).all()
    same(got, mom, f"{name} {w}x{h}: moments")
    same(pt.read_accum(), acc, f"{name} {w}x{h}: accumulation")
    same(pt.read_error(), R.error(mom), f"{name} {w}x{h}: error image")
    want = R.stats(mom, 0.25)
    st = pt.convergence(0.25)
    print(name, shape, st)
    assert st == want
    if shape == SHAPES[0]:                           # the comparison is not vacuous
        assert 0 < st["n_above"] < st["n_measured"] == w * h
        if name == "c1":
            assert 0.15 < st["n_above"] / st["n_measured"] < 0.22


# ---- 5. batching and call shape change nothing -----------------------------------------------------
def test_batching_and_call_shape(pt, tmp_path):
    cfg = scene("c2", W, H)
    pt.load(cfg)
    pt.enable_moments()
    plan = pt.batch_plan(12)
    assert plan["n_batches"] == 1
    pt.render(0, 12)
    mom, acc = pt.read_moments(), pt.read_accum()
    assert (R.frames_of(mom) == 12).all() and (mom[..., 1] > 0).any()
    ref, _ = pyoracle.Oracle(cfg).render(0, 12)
    same(acc, ref, "one call: accumulation vs the oracle")

    pt.reset_accum()
    for k in range(12):
        pt.render(k, 1)
    same(pt.read_moments(), mom, "twelve 1-frame calls: moments")
    same(pt.read_accum(), acc, "twelve 1-frame calls: accumulation")

    pt.reset_accum()
    pt.render(0, 5)
    pt.render(5, 7)                                  # (no wait in between)
    same(pt.read_moments(), mom, "5 + 7 frames: moments")
    same(pt.read_accum(), acc, "5 + 7 frames: accumulation")

    # a context capped to 4 frames per batch, in a child (the cap is read at creation)
    by = [pt.batch_plan(k)["batch_bytes"] for k in (4, 5)]
    out = str(tmp_path / "capped.bin")
    env = dict(os.environ, PNRT_BATCH_BYTES=str(by[0] + (by[1] - by[0]) // 2))
    r = subprocess.run([sys.executable, os.path.join(HERE, "moments_worker.py"), "c2", str(W), str(H), "12", out], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fpb, nb = (int(v) for v in r.stdout.split("plan")[1].split()[:2])
    assert (fpb, nb) == (4, 3) and nb >= 3
    got = np.fromfile(out, np.float32).reshape(2, H, W, 4)
    same(got[0], mom, "capped batches: moments")
    same(got[1], acc, "capped batches: accumulation")


# ---- 6. shards -------------------------------------------------------------------------------------
def test_shards(pt):
    pt.load(scene("c2", W, H))
    pt.enable_moments()
    pt.render(0, 6)
    mom, acc = pt.read_moments(), pt.read_accum()
    full = pt.convergence(0.25)
    assert full == R.stats(mom, 0.25) and 0 < full["n_above"] < full["n_pixels"] == W * H
    pt.reset_accum()
    assert not pt.read_moments().any()
    pt.render(0, 6, 8, 2, 0)
    half = pt.read_moments()
    r0, r1 = shard_rows(H, 8, 2, 0), shard_rows(H, 8, 2, 1)
    same(half[r0], mom[r0], "shard 0's rows after shard 0's call")
    assert not half[r1].any()
    pt.render(0, 6, 8, 2, 1)
    same(pt.read_moments(), mom, "both shards: moments")
    same(pt.read_accum(), acc, "both shards: accumulation")
    parts = [pt.convergence(0.25, 8, 2, k) for k in range(2)]
    assert [p["n_pixels"] for p in parts] == [len(r0) * W, len(r1) * W]
    assert parts == [R.stats(mom, 0.25, rows=r) for r in (r0, r1)]
    assert merge_convergence(parts) == full
    thirds = [pt.convergence(0.25, 4, 3, k) for k in range(3)]
    assert merge_convergence(thirds) == full
    zero = {"n_pixels": 0, "n_measured": 0, "n_above": 0, "sum_q16": 0, "max_error": 0.0, "min_frames": 0,
            "max_frames": 0, "mean_error": 0.0}
    assert pt.convergence(0.25, 64, 2, 1) == zero    # one band of >= 45 rows: shard 1 has none
    assert pt.convergence(0.25, 8, 8, 6) == zero     # bands 0..5 only
    assert code_of(pt.convergence, 0.25, 8, 2, 2) == E_ARG


# ---- 7. lifecycle ----------------------------------------------------------------------------------
def test_lifecycle(pt):
    colors, _, _ = anchor("c1", W, H)                # frames 0, 1, 3, ...
    cfg = scene("c1", W, H)
    pt.load(cfg)
    for call in (pt.read_moments, pt.read_error, lambda: pt.convergence(0.1)):
        assert code_of(call) == E_STATE              # never enabled
    pt.enable_moments()
    for bad in (-0.5, math.nan, math.inf, -math.inf):
        assert code_of(pt.convergence, bad) == E_ARG
    assert pt.convergence(0.0)["n_measured"] == 0

    # one frame: unmeasured
    pt.render(0, 1)
    m = pt.read_moments()
    same(m, R.update(R.zeros(H, W), colors[:1], [0]), "one frame")
    assert (R.frames_of(m) == 1).all() and (m[..., 1] == 0).all()
    assert np.isposinf(pt.read_error()).all()
    st = pt.convergence(0.25)
    assert (st["n_pixels"], st["n_measured"], st["n_above"], st["sum_q16"], st["max_error"]) == (W * H, 0, 0, 0, 0.0)
    assert (st["min_frames"], st["max_frames"], st["mean_error"]) == (1, 1, 0.0)

    # disable / enable keeps the data and skips the frames in between
    pt.render(1, 1)
    pt.enable_moments(False)
    ptr = pt.moments_ptr()
    pt.render(2, 1)
    pt.enable_moments(True)
    pt.enable_moments(True)                          # twice: keeps the data
    assert pt.moments_ptr() == ptr
    pt.render(3, 1)
    m = pt.read_moments()
    same(m, R.update(R.zeros(H, W), [colors[0], colors[1], colors[2]], [0, 1, 3]), "frames 0, 1, (2 skipped), 3")
    ref, _ = pyoracle.Oracle(cfg).render(0, 4)
    same(pt.read_accum(), ref, "the accumulation holds all four frames")
    assert (R.frames_of(m) == 3).all()

    # a frame-0 call restarts them (the session's redraw)
    pt.render(0, 1)
    m = pt.read_moments()
    assert (R.frames_of(m) == 1).all() and (m[..., 1] == 0).all()
    same(m[..., 0], R.luminance(colors[0]), "restart: the mean is frame 0's luminance")

    # reset_accum and a size change zero them
    pt.reset_accum()
    assert not pt.read_moments().any()
    pt.render(0, 2)
    assert (R.frames_of(pt.read_moments()) == 2).all()
    small = scene("c1", 8, 8)
    pt.set_frame(8, 8, small.camera, small.max_depth)
    m = pt.read_moments()
    assert m.shape == (8, 8, 4) and not m.any()
    assert pt.convergence(0.25)["n_pixels"] == 64 and pt.read_error().shape == (8, 8)

    # the one-kernel path has no per-frame colours
    pt.render(0, 2)
    before, mbefore = pt.read_accum(), pt.read_moments()
    pt.set_options(TRAVERSE_ZCULL | KERNEL_V1)
    assert code_of(pt.render, 2, 1) == E_STATE
    same(pt.read_accum(), before, "V1 refused: accumulation untouched")
    same(pt.read_moments(), mbefore, "V1 refused: moments untouched")
    pt.enable_moments(False)
    pt.render(2, 1)                                  # allowed again, and the moments stay
    same(pt.read_moments(), mbefore, "V1 with moments disabled: moments untouched")
    assert bits(pt.read_accum()).tobytes() != bits(before).tobytes()


def test_enable_before_the_frame(pt):
    """Enabled before pnrt_set_frame: the image comes with the frame."""
    pt.enable_moments()
    assert pt.moments_ptr() == 0
    cfg = scene("c1", 8, 8)
    pt.load(cfg)
    assert pt.moments_ptr() != 0
    pt.render(0, 2)
    assert (R.frames_of(pt.read_moments()) == 2).all()


# ---- 8. off means off ------------------------------------------------------------------------------
@contextlib.contextmanager
def capped_tracer(cap):
    os.environ["PNRT_BATCH_BYTES"] = str(cap)
    t = None
    try:
        t = PathTracer(0)
        yield t
    finally:
        del os.environ["PNRT_BATCH_BYTES"]
        if t is not None:
            t.close()


def test_off_means_off(pt):
    cfg = scene("c2", W, H)
    pt.load(cfg)
    by = [pt.batch_plan(k)["batch_bytes"] for k in (4, 5)]
    images, counts = [], []
    with capped_tracer(by[0] + (by[1] - by[0]) // 2) as t:
        t.load(cfg)
        assert t.batch_plan(12)["n_batches"] == 3
        for on in (False, True):
            if on:
                t.enable_moments()
            t.reset_accum()
            t.profile_enable(True)
            t.render(0, 12)
            images.append(t.read_accum())
            counts.append({k: v[1] for k, v in t.profile_read().items()})
            t.profile_enable(False)
        assert (R.frames_of(t.read_moments()) == 12).all()
    # (the second render finds the first one's primary records still valid: that class differs by design)
    for c in counts:
        del c["primary"]
    assert counts[0] == counts[1], "the launch counts of every other class"
    assert counts[0]["gen"] == counts[0]["blend"] == 3           # one blend per batch, with and without
    same(images[1], images[0], "accumulation with moments vs without")
    ref, _ = pyoracle.Oracle(cfg).render(0, 12)
    same(images[0], ref, "accumulation vs the oracle")
