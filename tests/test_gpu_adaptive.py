"""Adaptive sampling (pnrt_render_adaptive, pt_adaptive.h) against tests/adaptive_ref.py,
the numpy restatement of DESIGN.md section 22, on per-frame colours taken exactly from
the CPU oracle (tests/moments_common.py), and against the oracle's own accumulation
where a pixel's frames are contiguous; call shape, shards, batching, lifecycle.

Tolerance: 0 ulp everywhere (uint32 views and integers compared)."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as A
import moments_ref as R
import pyoracle
from guides_common import SHAPES, bits, scene
from moments_common import anchor
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = SHAPES[0]
E_ARG, E_STATE = -1, -3
ALL = 0xFFFFFFFF                                     # min_frames: every pixel active
ADAPTIVE_FRAMES = (3, 7, 15)                         # after pnrt_render(0, 2): the anchor's other frames

# The CPU replay of the anchor sequence (pixels with n = 2 / 3 / 4 / 5 frames at the end,
# active tiles of 54 per adaptive call), as recorded when the feature was specified.
REPLAY = {("c1", 0.5): ((2739, 114, 54, 108), (50, 35, 26)),
          ("c1", 0.125): ((1395, 294, 153, 1173), (54, 54, 54)),
          ("c2wide", 0.5): ((2676, 63, 35, 241), (16, 16, 16)),
          ("c3", 0.5): ((1126, 437, 273, 1179), (54, 54, 54))}


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


@functools.lru_cache(maxsize=None)
def replay(name, thresholds):
    """adaptive_ref over the anchor's colours: pnrt_render(0, 2), then one adaptive call per
    ADAPTIVE_FRAMES with thresholds[k] and min_frames = 2 -> [(accum, moments, stats)] after
    every call (stats None for the first)."""
    colors, _, _ = anchor(name, W, H)
    acc = R.blend(np.zeros((H, W, 4), np.float32), colors[:2], [0, 1])
    mom = R.update(R.zeros(H, W), colors[:2], [0, 1])
    steps = [(acc, mom, None)]
    for c, f, thr in zip(colors[2:], ADAPTIVE_FRAMES, thresholds):
        acc, mom, st = A.render(acc, mom, [c], [f], thr, 2)
        steps.append((acc, mom, st))
    return steps


def run_anchor(pt, name, thresholds):
    steps = replay(name, thresholds)
    pt.load(scene(name, W, H))
    pt.enable_moments()
    pt.render(0, 2)
    same(pt.read_accum(), steps[0][0], f"{name}: accumulation after pnrt_render(0, 2)")
    same(pt.read_moments(), steps[0][1], f"{name}: moments after pnrt_render(0, 2)")
    for k, (f, thr) in enumerate(zip(ADAPTIVE_FRAMES, thresholds)):
        st = pt.render_adaptive(f, 1, thr, 2)
        acc, mom, want = steps[k + 1]
        print(name, thr, f, st)
        assert st == want, f"{name}: stats of the call of frame {f}"
        same(pt.read_accum(), acc, f"{name}: accumulation after frame {f}")
        same(pt.read_moments(), mom, f"{name}: moments after frame {f}")
    return steps


# ---- 1. anchor replay ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,thr", sorted(REPLAY))
def test_anchor_replay(pt, name, thr):
    steps = replay(name, (thr,) * 3)
    n = R.frames_of(steps[-1][1])
    counts = tuple(int((n == k).sum()) for k in (2, 3, 4, 5))
    tiles = tuple(s[2]["n_active_tiles"] for s in steps[1:])
    print(name, thr, counts, tiles)
    # from the replay, not from the GPU: an input for which this fails is a test error
    assert sum(counts) == W * H and min(counts) >= 30, counts
    assert (counts, tiles) == REPLAY[(name, thr)]
    assert all(s[2]["n_tiles"] == 54 and s[2]["frames_per_batch"] == s[2]["n_batches"] == 1 for s in steps[1:])
    run_anchor(pt, name, (thr,) * 3)


# ---- 2. all active = plain -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_frames(name, w, h, counts):
    """The oracle's accumulation after counts[0], counts[1], ... frames (increasing)."""
    o = pyoracle.Oracle(scene(name, w, h))
    acc = np.zeros((h, w, 4), np.float32)
    out, done = [], 0
    for c in counts:
        _, st = o.render(done, c - done, accum=acc)
        assert st["stack_overflow"] == 0
        done = c
        out.append(acc.copy())
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["c1", "c3", "c2wide"])
def test_all_active_is_plain(pt, name, shape):
    w, h = shape
    pt.load(scene(name, w, h))
    pt.enable_moments()
    pt.render(0, 12)
    acc, mom = pt.read_accum(), pt.read_moments()
    same(acc, oracle_frames(name, w, h, (12,))[0], f"{name} {w}x{h}: pnrt_render(0, 12) vs the oracle")
    pt.reset_accum()
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    for first, n in ((0, 1), (1, 2), (3, 4), (7, 5)):
        st = pt.render_adaptive(first, n, 0.0, ALL)
        assert st == {"n_pixels": w * h, "n_active_pixels": w * h, "n_tiles": tiles, "n_active_tiles": tiles,
                      "frames_per_batch": n, "n_batches": 1}
    same(pt.read_accum(), acc, f"{name} {w}x{h}: accumulation, adaptive with everything active vs pnrt_render")
    same(pt.read_moments(), mom, f"{name} {w}x{h}: moments")
    assert (R.frames_of(mom) == 12).all()


# ---- 3. contiguous freeze against the oracle ---------------------------------------------------------
def test_contiguous_freeze_vs_oracle(pt):
    pt.load(scene("c1", W, H))
    pt.enable_moments()
    pt.render(0, 2)
    for first in (2, 4, 6):
        st = pt.render_adaptive(first, 2, 0.5, 2)
        assert 0 < st["n_active_pixels"] < W * H
    acc, n = pt.read_accum(), R.frames_of(pt.read_moments())
    assert np.isin(n, (2, 4, 6, 8)).all()
    want = np.zeros_like(acc)
    for k, img in zip((2, 4, 6, 8), oracle_frames("c1", W, H, (2, 4, 6, 8))):
        want[n == k] = img[n == k]
    same(acc, want, "every pixel is the oracle's accumulation of its own n frames")
    frozen = ~A.active(replay("c1", (0.5,) * 3)[0][1], 0.5, 2)       # the anchor replay's first call: same two frames
    assert int(frozen.sum()) == REPLAY[("c1", 0.5)][0][0] == 2739
    assert ((n == 2) == frozen).all() and (n[~frozen] > 2).all()
    print("pixels by n:", {k: int((n == k).sum()) for k in (2, 4, 6, 8)})


# ---- 4. reactivation ---------------------------------------------------------------------------------
def test_reactivation(pt):
    thresholds = (0.5, 0.5, 0.125)
    steps = run_anchor(pt, "c1", thresholds)
    before, after = R.frames_of(steps[2][1]), R.frames_of(steps[3][1])
    resumed = (before == 2) & (after == 3)           # frozen through both 0.5 calls, active at 0.125
    assert resumed.sum() >= 30, "frozen pixels resume"
    assert steps[3][2]["n_active_tiles"] > steps[2][2]["n_active_tiles"]


# ---- 5. shards ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", [8, 3])
def test_shards(pt, band):
    colors, _, _ = anchor("c1", W, H)
    steps = replay("c1", (0.5,) * 3)
    pt.load(scene("c1", W, H))
    pt.enable_moments()
    pt.render(0, 2)
    full = pt.render_adaptive(3, 1, 0.5, 2)
    acc, mom = pt.read_accum(), pt.read_moments()
    same(acc, steps[1][0], "full adaptive call: accumulation")
    assert full == steps[1][2]
    pt.reset_accum()
    pt.render(0, 2)
    racc, rmom, parts = steps[0][0], steps[0][1], []
    for shard in range(2):
        st = pt.render_adaptive(3, 1, 0.5, 2, band, 2, shard)
        racc, rmom, want = A.render(racc, rmom, [colors[2]], [3], 0.5, 2, band, 2, shard)
        assert st == want, f"band {band}, shard {shard}"
        same(pt.read_moments(), rmom, f"band {band}: moments after shard {shard}")
        parts.append(st)
    same(pt.read_accum(), acc, f"band {band}: both shards vs the full call, accumulation")
    same(pt.read_moments(), mom, f"band {band}: both shards vs the full call, moments")
    for key in ("n_pixels", "n_active_pixels"):
        assert sum(p[key] for p in parts) == full[key]
    if band == 8:                                    # whole tile rows per band: the tiles are the image's
        for key in ("n_tiles", "n_active_tiles"):
            assert sum(p[key] for p in parts) == full[key]
    else:                                            # bands cut the tiles: local-row tiling
        assert [p["n_tiles"] for p in parts] == [9 * 3, 9 * 3]       # 24 and 21 local rows
    assert pt.render_adaptive(3, 0, 0.5, 2, 64, 2, 1) == dict.fromkeys(full, 0)      # a shard without rows
    assert code_of(pt.render_adaptive, 3, 1, 0.5, 2, 8, 2, 2) == E_ARG


# ---- 6. batching, and a call right behind an unwaited pnrt_render --------------------------------------
def test_batching_and_unwaited_predecessor(pt, tmp_path):
    cfg = scene("c1", W, H)
    pt.load(cfg)
    pt.enable_moments()
    pt.render(0, 2)
    pt.synchronize()
    st = pt.render_adaptive(2, 6, 0.5, 2)
    mom, acc = pt.read_moments(), pt.read_accum()
    tiles = st["n_active_tiles"]
    assert (st["frames_per_batch"], st["n_batches"]) == (6, 1) and tiles == REPLAY[("c1", 0.5)][1][0]
    assert set(np.unique(R.frames_of(mom))) == {2, 8}

    # no wait between the two calls: the adaptive call waits itself
    pt.reset_accum()
    pt.render(0, 2)
    assert pt.render_adaptive(2, 6, 0.5, 2) == st
    same(pt.read_moments(), mom, "behind an unwaited pnrt_render: moments")
    same(pt.read_accum(), acc, "behind an unwaited pnrt_render: accumulation")

    # a context capped to 2 frames per adaptive batch, in a child (the cap is read at creation).
    # A frame of 8 * tiles x 8 pixels has exactly the call's path slots and colour bytes per frame.
    pt.set_frame(8 * tiles, 8, cfg.camera, cfg.max_depth)
    by = [pt.batch_plan(k)["batch_bytes"] for k in (2, 3)]
    out = str(tmp_path / "capped.bin")
    env = dict(os.environ, PNRT_BATCH_BYTES=str(by[0] + (by[1] - by[0]) // 2))
    r = subprocess.run([sys.executable, os.path.join(HERE, "adaptive_worker.py"), "c1", str(W), str(H), "6", "0.5", out],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fpb, nb, nt = (int(v) for v in r.stdout.split("plan")[1].split()[:3])
    assert (fpb, nb, nt) == (2, 3, tiles) and nb >= 3
    got = np.fromfile(out, np.float32).reshape(2, H, W, 4)
    same(got[0], mom, "capped batches: moments")
    same(got[1], acc, "capped batches: accumulation")


# ---- 7. lifecycle --------------------------------------------------------------------------------------
def launches(pt):
    return {k: v[1] for k, v in pt.profile_read().items()}


def test_lifecycle(pt):
    assert code_of(pt.render_adaptive, 0, 1, 0.5) == E_STATE         # no scene, no frame
    pt.enable_moments()
    assert code_of(pt.render_adaptive, 0, 1, 0.5) == E_STATE
    pt.enable_moments(False)
    cfg = scene("c1", W, H)
    pt.load(cfg)
    pt.render(0, 2)

    def untouched(call, code, what, moments=True):
        acc = pt.read_accum()
        mom = pt.read_moments() if moments else None
        assert code_of(call) == code, what
        same(pt.read_accum(), acc, what + ": accumulation untouched")
        if moments:
            same(pt.read_moments(), mom, what + ": moments untouched")

    t2 = PathTracer(0)                               # never enabled
    try:
        t2.load(cfg)
        t2.render(0, 1)
        acc = t2.read_accum()
        assert code_of(t2.render_adaptive, 1, 1, 0.5) == E_STATE
        same(t2.read_accum(), acc, "never enabled: accumulation untouched")
    finally:
        t2.close()
    untouched(lambda: pt.render_adaptive(2, 1, 0.5), E_STATE, "moments disabled")
    pt.enable_moments()                              # frames 0, 1 were rendered while they were disabled
    untouched(lambda: pt.render_adaptive(2, 1, 0.5), E_STATE, "the moments do not cover the accumulation")
    pt.reset_accum()
    assert pt.render_adaptive(0, 0, 0.5)["n_active_pixels"] == W * H
    pt.render(0, 2)
    pt.enable_moments(False)
    pt.enable_moments()                              # off and on without a render in between: still covered
    assert pt.render_adaptive(2, 0, 0.5, 2)["n_active_pixels"] > 0
    for bad in (-0.5, math.nan, math.inf, -math.inf):
        untouched(lambda: pt.render_adaptive(2, 1, bad), E_ARG, f"threshold {bad}")
    for sel in ((0, 1, 0), (8, 0, 0), (8, 2, 2), (8, 2, -1)):
        untouched(lambda: pt.render_adaptive(2, 1, 0.5, 2, *sel), E_ARG, f"selector {sel}")
    untouched(lambda: pt.render_adaptive(0xFFFFFFFF, 1, 0.5), E_ARG, "first_frame + n_frames > 0xFFFFFFFF")
    untouched(lambda: pt.render_adaptive(0xFFFFFFF0, 0x10, 0.5), E_ARG, "first_frame + n_frames > 0xFFFFFFFF")
    pt.set_options(TRAVERSE_ZCULL | KERNEL_V1)
    untouched(lambda: pt.render_adaptive(2, 1, 0.5), E_STATE, "PNRT_KERNEL_V1")
    pt.set_options(TRAVERSE_ZCULL)

    # nothing to render: statistics, and no launch of any class
    steps = replay("c1", (0.5,) * 3)
    acc, mom = pt.read_accum(), pt.read_moments()
    same(mom, steps[0][1], "two frames")
    pt.profile_enable(True)
    st = pt.render_adaptive(2, 0, 0.5, 2)
    assert st == dict(steps[1][2], frames_per_batch=0, n_batches=0) and 0 < st["n_active_tiles"] < st["n_tiles"]
    st = pt.render_adaptive(2, 3, 65535.0, 2)        # fully converged: e_c <= 65535 everywhere
    assert st == {"n_pixels": W * H, "n_active_pixels": 0, "n_tiles": 54, "n_active_tiles": 0, "frames_per_batch": 0,
                  "n_batches": 0}
    assert not any(launches(pt).values()), "nothing to render launches nothing"
    same(pt.read_accum(), acc, "nothing rendered: accumulation")
    same(pt.read_moments(), mom, "nothing rendered: moments")
    # ... and a call that renders: one gen and one blend per batch, depth traces and shades
    st = pt.render_adaptive(3, 1, 0.5, 2)
    n = launches(pt)
    assert (n["gen"], n["blend"], n["trace"], n["shade"]) == (1, 1, cfg.max_depth, cfg.max_depth)
    pt.profile_enable(False)
    same(pt.read_accum(), steps[1][0], "frame 3: accumulation")

    # pnrt_reset_accum restores full activity; min_frames keeps everything active until reached
    pt.reset_accum()
    st = pt.render_adaptive(0, 2, 65535.0, 2)
    assert st["n_active_pixels"] == W * H and st["n_active_tiles"] == 54
    same(pt.read_accum(), steps[0][0], "adaptive frames 0, 1 after the reset: accumulation")
    same(pt.read_moments(), steps[0][1], "adaptive frames 0, 1 after the reset: moments")
    assert pt.render_adaptive(2, 0, 65535.0, 3)["n_active_pixels"] == W * H
    assert pt.render_adaptive(2, 0, 65535.0, 2)["n_active_pixels"] == 0

    # a plain pnrt_render after adaptive calls behaves as before
    pt.render_adaptive(3, 1, 0.5, 2)
    pt.render(0, 2)                                  # frame 0 restarts both images
    same(pt.read_accum(), steps[0][0], "pnrt_render(0, 2) after adaptive calls: accumulation")
    same(pt.read_moments(), steps[0][1], "pnrt_render(0, 2) after adaptive calls: moments")
    assert pt.render_adaptive(3, 1, 0.5, 2) == steps[1][2]
    same(pt.read_accum(), steps[1][0], "and the adaptive call after it")


def test_small_frames(pt):
    """8x8 (one tile) and 1x1 (one pixel of one tile) through the anchor sequence."""
    for w, h in SHAPES[1:]:
        colors, _, _ = anchor("c3", w, h)
        pt.load(scene("c3", w, h))
        pt.enable_moments()
        pt.reset_accum()
        pt.render(0, 2)
        acc = R.blend(np.zeros((h, w, 4), np.float32), colors[:2], [0, 1])
        mom = R.update(R.zeros(h, w), colors[:2], [0, 1])
        thr = float(np.median(R.error(mom))) / 2     # the one pixel of 1x1 is above it (unless its two frames agree)
        for c, f in zip(colors[2:], ADAPTIVE_FRAMES):
            acc, mom, want = A.render(acc, mom, [c], [f], thr, 2)
            assert pt.render_adaptive(f, 1, thr, 2) == want
            same(pt.read_accum(), acc, f"{w}x{h}: accumulation after frame {f}")
            same(pt.read_moments(), mom, f"{w}x{h}: moments after frame {f}")
