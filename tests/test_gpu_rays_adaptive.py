"""pnrt_render_rays_adaptive: pnrt_render_adaptive over caller ray buffers.

Against pnrt_render_rays where every pixel is active, against pnrt_render_adaptive on the
pnrt_set_frame camera's own rays, against tests/adaptive_ref.py fed the CPU oracle's per-frame
colours (three pinhole cameras interleaved per pixel), and against itself around inactive and
no-ray records; batches, selectors, trees, frame numbers, stream order, refusals, the session.

"Partly active": after pnrt_render_rays(0, 4) with the moments on, the threshold is the median of
pnrt_read_error.  `mixed` asserts on the state read back that it holds active and inactive pixels,
a tile without an active pixel, a tile with some but not all of its pixels active and -- where the
frame has one: a width or height that is no multiple of 8 -- an active ragged tile.  After four
frames of these scenes every tile still holds a pixel above the median, so the rays of those four
frames carry "no ray" records over one whole tile (BLANK): colour 0 in every frame, error 0,
inactive at any threshold.  A frame of 40x24 or 48x32 has no ragged tile to ask for.

Tolerance: 0 ulp (uint32 views and integers compared) everywhere."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adaptive_ref as A
import moments_ref as MR
import pyoracle
import test_gpu_cameras as T          # its scenes and helpers; nothing runs on import
import test_gpu_rays as TR            # (likewise)
from pnraytracing_amd.tracer import KERNEL_V1, SERIAL, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
MODES = T.MODES
bits, same, load, scene = T.bits, T.same, T.load, T.scene
dev, host_of, look, elsewhere, lens_sets = TR.dev, TR.host_of, TR.look, TR.elsewhere, TR.lens_sets
E_ARG, E_STATE = -1, -3
ALL = 0xFFFFFFFF                                         # min_frames: every pixel active


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def at(rays, k, stride):
    """The address of set k of a ray tensor whose sets are `stride` records apart."""
    return int(rays.data_ptr()) + 32 * k * stride


def tiles_of(mask):
    """(active pixels, pixels inside the frame) of every 8x8 tile of an (H, W) bool image."""
    Hh, W = mask.shape
    ty, tx = (Hh + 7) // 8, (W + 7) // 8
    count = []
    for img in (mask, np.ones_like(mask)):
        p = np.zeros((ty * 8, tx * 8), bool)
        p[:Hh, :W] = img
        count.append(p.reshape(ty, 8, tx, 8).transpose(0, 2, 1, 3).reshape(ty * tx, 64).sum(axis=1))
    return count


def mixed(mask, what):
    act, inside = tiles_of(mask)
    assert mask.any() and (~mask).any(), what
    assert (act == 0).any(), f"{what}: no tile without an active pixel"
    assert ((act > 0) & (act < inside)).any(), f"{what}: no tile with some but not all pixels active"
    if mask.shape[0] % 8 or mask.shape[1] % 8:
        assert ((act > 0) & (inside < 64)).any(), f"{what}: no active ragged tile"


BLANK = (slice(0, 8), slice(8, 16))                      # tile 1: rows 0..7, columns 8..15


def blanked(pt, rays, stride, W, Hh):
    """Sets 0..3 of `rays` (the one set when stride is 0) with no-ray records over the BLANK tile."""
    pix = W * Hh
    h = host_of(pt, rays)[:(0 if stride == 0 else 3 * stride) + pix].copy()
    for k in range(1 if stride == 0 else 4):
        h[k * stride:k * stride + pix].reshape(Hh, W, 8)[BLANK] = 0.0
    return dev(h)


def start(pt, cfg, rays, stride, mode=TRAVERSE_ZCULL, depth=None, check=True):
    """The state the adaptive calls start from: frames 0..3 of `rays` without the BLANK tile, the
    moments on -> (the median threshold, accumulation, moments, mask of the active pixels at
    min_frames 2)."""
    load(pt, cfg, mode, depth)
    pt.enable_moments(True)
    pt.render_rays(0, 4, blanked(pt, rays, stride, cfg.width, cfg.height), stride)
    thr = float(F(np.median(pt.read_error())))
    acc, mom = pt.read_accum(), pt.read_moments()
    mask = A.active(mom, thr, 2)
    assert not mask[BLANK].any() and not acc[BLANK][..., :3].any()
    if check:
        mixed(mask, f"{cfg.name} {cfg.width}x{cfg.height}")
    return thr, acc, mom, mask


def want_stats(mask, n, chunk=None):
    act, _ = tiles_of(mask)
    nt = int((act > 0).sum())
    fpb, nb = A.plan(nt, n, chunk)
    return {"n_pixels": mask.size, "n_active_pixels": int(mask.sum()), "n_tiles": len(act), "n_active_tiles": nt,
            "frames_per_batch": fpb, "n_batches": nb}


# ---- 1. all active = plain ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("per_frame", [False, True], ids=["one-set", "set-per-frame"])
def test_all_active_is_render_rays(pt, per_frame, mode):
    cfg = scene("c1", 37, 19)                            # partial tiles in both directions
    pix = 37 * 19
    load(pt, cfg, mode)
    pt.enable_moments(True)
    if per_frame:
        stride = pix + 7
        rays = lens_sets(pt, cfg, 0, 6, stride, per_pixel=1)
    else:
        stride = 0
        rays = pt.make_rays("fisheye", cfg.camera, fov_deg=150.0)        # (with no-ray records outside its circle)
    pt.render_rays(0, 6, rays, stride)
    acc, mom = pt.read_accum(), pt.read_moments()
    assert acc[..., :3].any() and (MR.frames_of(mom) == 6).all()
    pt.set_frame(37, 19, elsewhere(cfg), cfg.max_depth)  # the pnrt_set_frame camera is ignored
    pt.reset_accum()
    for first in (0, 2, 4):
        st = pt.render_rays_adaptive(first, 2, at(rays, first, stride), stride, 0.0, ALL)
        assert st == {"n_pixels": pix, "n_active_pixels": pix, "n_tiles": 15, "n_active_tiles": 15, "frames_per_batch": 2,
                      "n_batches": 1}
    same(pt.read_accum(), acc, f"accumulation, mode {mode}")
    same(pt.read_moments(), mom, f"moments, mode {mode}")


# ---- 2. the pnrt_set_frame camera's rays = pnrt_render_adaptive -------------------------------------
def against_render_adaptive(pt, cfg, first, n, mode=TRAVERSE_ZCULL, check=True, sel=(1, 1, 0)):
    load(pt, cfg, mode)                                  # (the frame size the rays are made for)
    rays = pt.make_rays("pinhole", cfg.camera)
    thr, acc0, mom0, mask = start(pt, cfg, rays, 0, mode, check=check)
    assert 0 < mask.sum() < mask.size
    st_r = pt.render_rays_adaptive(first, n, rays, 0, thr, 2, *sel)
    acc_r, mom_r = pt.read_accum(), pt.read_moments()
    thr2, acc1, mom1, _ = start(pt, cfg, rays, 0, mode, check=False)     # the same state again
    assert thr2 == thr
    same(acc1, acc0, "the state is reproducible: accumulation")
    same(mom1, mom0, "the state is reproducible: moments")
    st_a = pt.render_adaptive(first, n, thr, 2, *sel)
    assert st_r == st_a and st_a["n_active_pixels"] > 0
    if sel == (1, 1, 0):
        assert st_a == want_stats(mask, n)
    same(acc_r, pt.read_accum(), f"{cfg.name} mode {mode}: accumulation")
    same(mom_r, pt.read_moments(), f"{cfg.name} mode {mode}: moments")
    assert T.n_differ(acc_r, acc0) > 0
    return mask, acc0, mom0, acc_r, mom_r


@pytest.mark.parametrize("mode", MODES)
def test_pinhole_rays_are_render_adaptive(pt, mode):
    mask, acc0, mom0, acc, mom = against_render_adaptive(pt, scene("c1", 67, 45), 4, 6, mode)
    # an inactive pixel keeps both records, an active one got the six frames
    assert np.array_equal(bits(acc[~mask]), bits(acc0[~mask])) and np.array_equal(bits(mom[~mask]), bits(mom0[~mask]))
    assert (MR.frames_of(mom)[mask] == 10).all() and (MR.frames_of(mom)[~mask] == 4).all()


# ---- 3. three cameras interleaved per pixel against the oracle --------------------------------------
ORACLE_FRAMES = (7, 15, 31)                              # blend weights 1 / (f + 1) that are powers of two (moments_common)


@functools.lru_cache(maxsize=None)
def interleaved_colors(name, W, Hh, depth):
    """The colour images of ORACLE_FRAMES where pixel (x, y) of frame f takes camera (x + 2y + f) % 3:
    the pixels of class g = (x + 2y) % 3 are the oracle's for camera (g + f) % 3, and one frame
    rendered into a zeroed image at a power-of-two weight gives its colour back exactly."""
    cfg = scene(name, W, Hh)
    cams = TR.three_cameras(cfg, name)
    x, y = np.meshgrid(np.arange(W), np.arange(Hh))
    cls = (x + 2 * y) % 3
    orc = pyoracle.Oracle(cfg)
    out = []
    for f in ORACLE_FRAMES:
        c = np.zeros((Hh, W, 3), F)
        for g in range(3):
            rgb = T.oracle_cameras(cfg, f, cams[(g + f) % 3].reshape(1, 12), depth, orc=orc)[..., :3]
            assert not ((rgb != 0) & (np.abs(rgb) < np.finfo(F).tiny)).any()
            full = (rgb * F(f + 1)).astype(F)
            assert np.array_equal(bits((full * (F(1) / F(f + 1))).astype(F)), bits(rgb))
            c[cls == g] = full[cls == g]
        c.setflags(write=False)
        out.append(c)
    return cls, out


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("name,W,Hh", [("c1", 40, 24), ("c2", 48, 32)])
def test_interleaved_cameras_match_the_oracle(pt, name, W, Hh, depth):
    cfg = scene(name, W, Hh)
    cls, colors = interleaved_colors(name, W, Hh, depth)
    load(pt, cfg, TRAVERSE_ZCULL, depth)
    per_cam = [host_of(pt, pt.make_rays("pinhole", c)).reshape(Hh, W, 8) for c in TR.three_cameras(cfg, name)]
    frames = (0, 1, 2, 3) + ORACLE_FRAMES
    sets = np.zeros((len(frames), Hh, W, 8), F)
    for s, f in enumerate(frames):
        for k in range(3):
            pick = (cls + f) % 3 == k
            sets[s][pick] = per_cam[k][pick]
    rays = dev(sets.reshape(-1, 8))
    pix = W * Hh
    thr, acc, mom, _ = start(pt, cfg, rays, pix, depth=depth)
    for k, f in enumerate(ORACLE_FRAMES):                # three consecutive calls, each with its own mask
        acc, mom, want = A.render(acc, mom, [colors[k]], [f], thr, 2)
        st = pt.render_rays_adaptive(f, 1, at(rays, 4 + k, pix), 0, thr, 2)
        print(name, depth, f, st)
        assert st == want and st["n_active_pixels"] > 0, f"{name} depth {depth}: statistics of the call of frame {f}"
        same(pt.read_accum(), acc, f"{name} depth {depth}: accumulation after frame {f}")
        same(pt.read_moments(), mom, f"{name} depth {depth}: moments after frame {f}")


# ---- 4. / 5. the records of inactive pixels, and no-ray records in active ones -------------------------
def test_inactive_records_do_not_matter_and_no_ray_records_are_black(pt):
    W, Hh = 37, 19
    cfg = scene("c2", W, Hh)
    pix, stride = W * Hh, W * Hh + 5
    load(pt, cfg)
    rays = lens_sets(pt, cfg, 0, 10, stride, per_pixel=1)
    thr, acc0, mom0, mask = start(pt, cfg, rays, stride)
    frames = list(range(4, 10))

    def call(buf):
        start(pt, cfg, rays, stride, check=False)
        st = pt.render_rays_adaptive(4, 6, at(buf, 4, stride), stride, thr, 2)
        return st, pt.read_accum(), pt.read_moments()

    st, acc, mom = call(rays)
    assert st == want_stats(mask, 6)
    assert np.array_equal(bits(acc[~mask]), bits(acc0[~mask])) and np.array_equal(bits(mom[~mask]), bits(mom0[~mask]))
    assert (MR.frames_of(mom)[mask] == 10).all()
    h = host_of(pt, rays).copy()
    sets = [h[k * stride:k * stride + pix].reshape(Hh, W, 8) for k in range(10)]      # (views into h)
    other = host_of(pt, pt.make_rays("pinhole", elsewhere(cfg))).reshape(Hh, W, 8)
    for what, fill in (("other valid rays", other), ("NaN", np.full((Hh, W, 8), np.nan, F))):
        for k in frames:
            sets[k][~mask] = fill[~mask]
        st2, acc2, mom2 = call(dev(h))
        assert st2 == st, what
        same(acc2, acc, f"inactive records overwritten by {what}: accumulation")
        same(mom2, mom, f"inactive records overwritten by {what}: moments")
    # no-ray records in active pixels: colour 0 in every frame of the call, folded like any other
    h = host_of(pt, rays).copy()
    sets = [h[k * stride:k * stride + pix].reshape(Hh, W, 8) for k in range(10)]
    where = np.argwhere(mask)
    spots = [tuple(where[i]) for i in (0, len(where) // 3, len(where) // 2, len(where) - 1)]
    for k in frames:
        sets[k][spots[0]][1] = np.nan                    # origin
        sets[k][spots[1]][6] = np.inf                    # direction
        sets[k][spots[2]][4:7] = 0.0                     # a direction of three zeros
        sets[k][spots[3]][0] = -np.inf
        sets[k][spots[0]][3] = sets[k][spots[1]][7] = np.nan             # (the reserved floats are never read)
    st3, acc3, mom3 = call(dev(h))
    black = np.zeros((Hh, W), bool)
    for y, x in spots:
        black[y, x] = True
    assert st3 == st
    assert np.array_equal(bits(acc3[~black]), bits(acc[~black])) and np.array_equal(bits(mom3[~black]), bits(mom[~black]))
    zacc, zmom, _ = A.render(acc0, mom0, [np.zeros((Hh, W, 3), F)] * 6, frames, thr, 2)
    assert np.array_equal(bits(acc3[black]), bits(zacc[black])) and np.array_equal(bits(mom3[black]), bits(zmom[black]))
    assert T.n_differ(acc3[black][None], acc[black][None]) > 0


# ---- 6. batches -----------------------------------------------------------------------------------
def launches(pt):
    return {k: v[1] for k, v in pt.profile_read().items()}


def test_two_batches_with_one_set(pt):
    cfg = scene("c1", 16, 8)
    load(pt, cfg)
    pt.enable_moments(True)
    rays = pt.make_rays("pinhole", cfg.camera)
    pt.render_rays(0, 130, rays, 0)
    acc, mom = pt.read_accum(), pt.read_moments()
    pt.reset_accum()
    pt.synchronize()
    pt.profile_enable(True)
    st = pt.render_rays_adaptive(0, 130, rays, 0, 0.0, ALL)
    got = pt.read_accum()
    n = launches(pt)
    pt.profile_enable(False)
    assert (st["frames_per_batch"], st["n_batches"], st["n_active_tiles"]) == (128, 2, 2)
    # one ray launch, one gen and one blend per batch (the mask step's three kernels are not timed)
    assert (n["primary"], n["gen"], n["blend"]) == (2, 2, 2), n
    assert n["trace"] == n["shade"] == 2 * cfg.max_depth and n["setup"] == n["v1"] == 0
    same(got, acc, "130 frames in two batches: accumulation")
    same(pt.read_moments(), mom, "130 frames in two batches: moments")


def test_capped_context_reads_each_batchs_sets(pt):
    cfg = scene("c1", 24, 16)
    pix, stride = 24 * 16, 24 * 16 + 11
    load(pt, cfg)
    rays = lens_sets(pt, cfg, 0, 10, stride, per_pixel=1)
    thr, _, _, mask = start(pt, cfg, rays, stride)
    st = pt.render_rays_adaptive(4, 6, at(rays, 4, stride), stride, thr, 2)
    acc, mom = pt.read_accum(), pt.read_moments()
    assert st == want_stats(mask, 6) and st["n_batches"] == 1
    # a frame of 8 * tiles x 8 pixels has exactly the call's path slots, colour bytes and record bytes per frame
    pt.set_frame(8 * st["n_active_tiles"], 8, cfg.camera, cfg.max_depth)
    by2, by3 = (pt.cameras_batch_plan(k)["batch_bytes"] for k in (2, 3))
    with T.capped_tracer((by2 + by3) // 2) as t:
        load(t, cfg)
        own = lens_sets(t, cfg, 0, 10, stride, per_pixel=1)
        start(t, cfg, own, stride, check=False)
        t.profile_enable(True)
        st2 = t.render_rays_adaptive(4, 6, at(own, 4, stride), stride, thr, 2)
        got = t.read_accum()
        n = launches(t)
        assert st2 == want_stats(mask, 6, 2) and (st2["frames_per_batch"], st2["n_batches"]) == (2, 3)
        assert (n["primary"], n["gen"], n["blend"]) == (3, 3, 3), n
        same(got, acc, "6 frames under a cap, 3 batches: accumulation")
        same(t.read_moments(), mom, "6 frames under a cap, 3 batches: moments")


# ---- 7. selectors and trees -----------------------------------------------------------------------
def test_shards_with_local_row_tiles(pt):
    W, Hh = 37, 19
    cfg = scene("c1", W, Hh)
    pix = W * Hh
    load(pt, cfg)
    rays = lens_sets(pt, cfg, 0, 7, pix, per_pixel=1)
    thr, _, _, mask = start(pt, cfg, rays, pix)
    full = pt.render_rays_adaptive(4, 3, at(rays, 4, pix), pix, thr, 2)
    acc, mom = pt.read_accum(), pt.read_moments()
    start(pt, cfg, rays, pix, check=False)
    parts = []
    y = np.arange(Hh)
    for shard in range(2):
        before = pt.read_accum()
        rows = (y // 8) % 2 == shard
        st = pt.render_rays_adaptive(4, 3, at(rays, 4, pix), pix, thr, 2, 8, 2, shard)
        # rows 0-7 and 16-18 are shard 0's: 11 local rows, two tile rows; rows 8-15 shard 1's: one
        sel = np.zeros_like(mask)
        sel[rows] = mask[rows]
        assert st == want_stats(sel[rows], 3), f"shard {shard}"
        got = pt.read_accum()
        assert np.array_equal(bits(got[~rows]), bits(before[~rows])), f"shard {shard} touched another shard's rows"
        parts.append(st)
    same(pt.read_accum(), acc, "both shards vs the full call: accumulation")
    same(pt.read_moments(), mom, "both shards vs the full call: moments")
    for key in ("n_pixels", "n_active_pixels"):
        assert sum(p[key] for p in parts) == full[key]
    assert [p["n_tiles"] for p in parts] == [10, 5]
    assert pt.render_rays_adaptive(4, 3, at(rays, 4, pix), pix, thr, 2, 64, 2, 1) == dict.fromkeys(full, 0)   # a shard without rows


@pytest.mark.parametrize("kind", ["root-leaf", "leaf200", "chain"])
def test_scene_kinds(pt, kind):
    W, Hh = 16, 8
    if kind == "root-leaf":
        cfg, want = T.root_leaf_scene(W, Hh), {"root_is_leaf": 1, "n_interior": 0}
    elif kind == "leaf200":
        cfg, want = T.leaf200_scene(W, Hh), {"has_leaf_table": 1, "n_interior": 1}
    else:
        pt.upload_scene(scene("c1", W, Hh).packed)
        D = pt.device_info()["stack_limit"] - 2
        cfg, want = T.fan_chain_scene(W, Hh, D), {"max_depth": D, "n_interior": D}
    pix = W * Hh
    for mode in MODES:
        load(pt, cfg, mode)
        info = pt.device_info()
        assert {k: info[k] for k in want} == want
        # an active pixel that got every frame since frame 0 is pnrt_render_rays' pixel (its count is frame + 1)
        sets = lens_sets(pt, cfg, 0, 7, pix, per_pixel=1)
        thr, acc0, mom0, mask = start(pt, cfg, sets, pix, mode, check=False)      # (two tiles: BLANK is one of them)
        assert 0 < mask.sum() < pix
        st = pt.render_rays_adaptive(4, 3, at(sets, 4, pix), pix, thr, 2)
        acc, mom = pt.read_accum(), pt.read_moments()
        assert st == want_stats(mask, 3)
        pt.reset_accum()
        pt.render_rays(0, 4, blanked(pt, sets, pix, W, Hh), pix)
        pt.render_rays(4, 3, at(sets, 4, pix), pix)
        full_acc, full_mom = pt.read_accum(), pt.read_moments()
        same(acc, np.where(mask[..., None], full_acc, acc0), f"{cfg.name} mode {mode}: accumulation")
        same(mom, np.where(mask[..., None], full_mom, mom0), f"{cfg.name} mode {mode}: moments")


# ---- 8. frame numbers -----------------------------------------------------------------------------
def test_high_first_frame(pt):
    cfg = scene("c1", 40, 24)
    first = 0xFFFFFF - 2                                 # (float)(frame + 1) stops being exact inside the call
    load(pt, cfg)
    rays = pt.make_rays("pinhole", cfg.camera)
    thr, acc0, mom0, mask = start(pt, cfg, rays, 0)
    frames = [first + k for k in range(6)]
    st = pt.render_rays_adaptive(first, 6, rays, 0, thr, 2)
    acc, mom = pt.read_accum(), pt.read_moments()
    start(pt, cfg, rays, 0, check=False)
    assert pt.render_adaptive(first, 6, thr, 2) == st == want_stats(mask, 6)
    acc_a, mom_a = pt.read_accum(), pt.read_moments()
    # both are the replay over the frames' own colours: a frame blended alone at weight 1 is its colour
    colors = {"rays": [], "camera": []}
    for f in frames:
        pt.reset_accum()
        pt.render_rays_adaptive(f, 1, rays, 0, 0.0, ALL)
        colors["rays"].append(pt.read_accum()[..., :3])
        pt.reset_accum()
        pt.render_adaptive(f, 1, 0.0, ALL)
        colors["camera"].append(pt.read_accum()[..., :3])
    for k in range(6):
        same(colors["rays"][k][None], colors["camera"][k][None], f"the colour of frame {frames[k]}")
    want_acc, want_mom, _ = A.render(acc0, mom0, colors["rays"], frames, thr, 2)
    print("high frames, pixels that differ: rays vs replay", T.n_differ(acc, want_acc), "camera vs replay", T.n_differ(acc_a, want_acc),
          "rays vs camera", T.n_differ(acc, acc_a))
    same(acc, want_acc, "high frames: the replay's accumulation")
    same(mom, want_mom, "high frames: the replay's moments")
    same(acc_a, acc, "high frames: pnrt_render_adaptive's accumulation")
    same(mom_a, mom, "high frames: pnrt_render_adaptive's moments")
    # a set per frame: set k belongs to frame first + k whatever the frame number (every pixel active in both)
    pix = 40 * 24
    sets = lens_sets(pt, cfg, first, 6, pix, per_pixel=1)
    load(pt, cfg)
    pt.enable_moments(True)
    pt.render_rays(0, 2, sets, pix)
    for k in range(6):
        pt.render_rays_adaptive(first + k, 1, at(sets, k, pix), 0, 0.0, ALL)
    acc, mom = pt.read_accum(), pt.read_moments()
    pt.reset_accum()
    pt.render_rays(0, 2, sets, pix)
    st = pt.render_rays_adaptive(first, 6, sets, pix, 0.0, ALL)
    assert (st["frames_per_batch"], st["n_batches"], st["n_active_pixels"]) == (6, 1, pix)
    same(pt.read_accum(), acc, "a set per frame, high frames: accumulation")
    same(pt.read_moments(), mom, "a set per frame, high frames: moments")
    assert (MR.frames_of(mom) == 8).all()


# ---- 9. ordering ----------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [TRAVERSE_ZCULL, TRAVERSE_ZCULL | SERIAL], ids=["pipelined", "serial"])
def test_rays_written_on_the_context_stream_just_before(pt, options):
    """The call's rays are written by torch kernels on the wrapped context stream, behind enough
    other work that they are still pending when pnrt_render_rays_adaptive is entered."""
    cfg = scene("c1", 40, 24)
    pix = 40 * 24
    load(pt, cfg, options)
    a = lens_sets(pt, cfg, 0, 4, pix, per_pixel=1)
    b = lens_sets(pt, cfg, 4, 5, pix, per_pixel=1)
    thr, _, _, mask = start(pt, cfg, a, pix, options, check=False)
    st = pt.render_rays_adaptive(4, 5, b, pix, thr, 2)
    acc, mom = pt.read_accum(), pt.read_moments()
    start(pt, cfg, a, pix, options, check=False)
    ext = torch.cuda.ExternalStream(pt.stream_handle(), device=torch.device("cuda", 0))
    late = torch.full_like(b, float("nan"))
    torch.cuda.synchronize()
    with torch.cuda.stream(ext):
        m = torch.ones((2048, 2048), device="cuda")
        for _ in range(20):
            m = (m @ m) * (1.0 / 2048.0)
        late.copy_(b * m[0, 0])                          # (m stays all ones: exact)
    assert pt.render_rays_adaptive(4, 5, late, pix, thr, 2) == st
    got = pt.read_accum()
    assert np.isfinite(got).all() and 0 < mask.sum() < pix
    same(got, acc, "rays written just before the call: accumulation")
    same(pt.read_moments(), mom, "rays written just before the call: moments")
    pt.set_options(TRAVERSE_ZCULL)


# ---- 10. every refusal ----------------------------------------------------------------------------
def code_of(call, *a):
    with pytest.raises(PnrtError) as e:
        call(*a)
    return e.value.code


def test_refusals_leave_both_images(pt):
    cfg = scene("c1", 16, 8)
    pix = 16 * 8
    buf = dev(np.zeros((2 * pix, 8), F))
    with PathTracer(0) as fresh:
        for step in ("nothing", "scene only"):
            assert code_of(fresh.render_rays_adaptive, 0, 1, buf, 0, 0.5) == E_STATE, step
            fresh.upload_scene(cfg.packed)
        load(fresh, cfg)                                 # the moments were never enabled
        fresh.render_rays(0, 1, buf)
        acc = fresh.read_accum()
        assert code_of(fresh.render_rays_adaptive, 1, 1, buf, 0, 0.5) == E_STATE
        same(fresh.read_accum(), acc, "moments not enabled: accumulation untouched")
    load(pt, cfg)
    rays = pt.make_rays("pinhole", cfg.camera, 0, 4, pix)
    pt.render_rays(0, 2, rays, pix)

    def untouched(code, what, *args, moments=True):
        acc = pt.read_accum()
        mom = pt.read_moments() if moments else None
        assert code_of(pt.render_rays_adaptive, *args) == code, what
        same(pt.read_accum(), acc, f"{what}: accumulation untouched")
        if moments:
            same(pt.read_moments(), mom, f"{what}: moments untouched")

    ok = (2, 2, rays, pix, 0.5, 2)
    untouched(E_STATE, "moments disabled", *ok, moments=False)
    pt.enable_moments(True)                              # frames 0, 1 were rendered while they were disabled
    untouched(E_STATE, "the moments do not cover the accumulation", *ok)
    pt.reset_accum()
    pt.render_rays(0, 2, rays, pix)
    for bad in (-0.5, math.nan, math.inf, -math.inf):
        untouched(E_ARG, f"threshold {bad}", 2, 2, rays, pix, bad, 2)
    for sel in ((0, 1, 0), (8, 0, 0), (8, 2, 2), (8, 2, -1)):
        untouched(E_ARG, f"selector {sel}", *ok, *sel)
    untouched(E_ARG, "first_frame + n_frames > 0xFFFFFFFF", 0xFFFFFFFF - 1, 2, rays, pix, 0.5, 2)
    untouched(E_ARG, "rays_dev == NULL with n_frames > 0", 2, 2, None, pix, 0.5, 2)
    for off in (4, 8, 12):
        untouched(E_ARG, f"a pointer {off} bytes off", 2, 2, int(rays.data_ptr()) + off, pix, 0.5, 2)
    for stride in (-1, 1, pix - 1, -pix, 2 ** 62, (2 ** 63 - 1) // 32):      # ... or the last set's end past 2^63 bytes
        untouched(E_ARG, f"frame_stride {stride}", 2, 2, rays, stride, 0.5, 2)
    pt.set_options(TRAVERSE_ZCULL | KERNEL_V1)
    untouched(E_STATE, "PNRT_KERNEL_V1", *ok)
    pt.set_options(TRAVERSE_ZCULL)
    # n_frames == 0 evaluates the mask, fills the statistics and queues nothing, with or without a buffer
    acc, mom = pt.read_accum(), pt.read_moments()
    thr = float(F(np.median(MR.error(mom))))
    pt.profile_enable(True)
    want = want_stats(A.active(mom, thr, 2), 0)
    assert pt.render_rays_adaptive(2, 0, None, 0, thr, 2) == want and pt.render_rays_adaptive(2, 0, rays, pix, thr, 2) == want
    assert pt.render_rays_adaptive(2, 2, rays, pix, 65535.0, 2)["n_active_pixels"] == 0     # converged: nothing queued
    assert not any(launches(pt).values()), "nothing to render launches nothing"
    pt.profile_enable(False)
    same(pt.read_accum(), acc, "nothing rendered: accumulation")
    same(pt.read_moments(), mom, "nothing rendered: moments")
    # ... and the call still works
    assert pt.render_rays_adaptive(2, 2, at(rays, 2, pix), pix, 0.0, ALL)["n_active_pixels"] == pix
    assert (MR.frames_of(pt.read_moments()) == 4).all()


# ---- 11. the session ------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ["fisheye", "lens"])
def test_session_render_adaptive_until(pt, view):
    from pnraytracing_amd.session import CameraController, InteractiveSession
    W, Hh = 40, 24
    cfg = scene("c2", W, Hh)
    load(pt, cfg)
    cam = CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, F(W) / F(Hh))
    sess = InteractiveSession(pt, W, Hh, cam)
    if view == "fisheye":
        sess.set_camera_model("fisheye", fov_deg=150.0)
        model, params = "fisheye", {"fov_deg": 150.0}
    else:
        sess.set_lens(1.0, 0.15, focus_distance=7.0)
        model, params = "pinhole", {"fov_deg": 180.0, "aa_width": 1.0, "lens_radius": 0.15, "focus_distance": 7.0}
    calls = []
    inner = pt.render_rays_adaptive

    def recording(first, n, rays, stride, threshold, min_frames):
        st = inner(first, n, rays, stride, threshold, min_frames)
        calls.append((first, n, stride, st))
        return st

    pt.render_rays_adaptive = recording
    try:
        thr = 0.05
        stats, frames = sess.render_adaptive_until(thr, max_frames=12, frames_per_call=3, min_frames=4)
    finally:
        del pt.render_rays_adaptive
    acc, mom = pt.read_accum(), pt.read_moments()
    active = [c[3]["n_active_pixels"] for c in calls]
    print(view, active)
    assert [c[:2] for c in calls] == [(0, 3), (3, 3), (6, 3), (9, 3)][:len(calls)] and len(calls) >= 3
    assert active[0] == active[1] == W * Hh              # min_frames 4: everything is active until the second call is done
    assert all(a >= b for a, b in zip(active, active[1:]))
    assert frames == sess.frame_count == sum(c[1] for c in calls if c[3]["n_active_pixels"])
    # the replay by hand: the same rays through the same calls
    pt.reset_accum()
    for first, n, stride, st in calls:
        still = stride == 0
        rays = pt.make_rays(model, cam.uniforms(), first, 1 if still else n, **params)
        assert pt.render_rays_adaptive(first, n, rays, stride, thr, 4) == st
    same(pt.read_accum(), acc, f"{view}: the replay's accumulation")
    same(pt.read_moments(), mom, f"{view}: the replay's moments")
    if view == "fisheye":
        rho = TR.R.fisheye_rho(W, Hh).reshape(Hh, W)
        assert not acc[rho > 1][:, :3].any() and acc[rho <= 1][:, :3].any()
        # colour 0 in every frame: converged as soon as min_frames allows, after the second call
        assert (MR.frames_of(mom)[rho > 1] == 6).all() and active[2] <= int((rho <= 1).sum()) < W * Hh
    pt.enable_moments(False)


# ---- every index checked --------------------------------------------------------------------------
def test_on_bounds_checked_library():
    """The pnrt_set_frame camera's rays against pnrt_render_adaptive, no-ray records in active pixels,
    a capped context's three batches and a shard on the `bounds` diagnostic library: every fetch and
    store index of the list, ray, gen, trace, shade and blend steps is checked against its array,
    and a violation is an error."""
    from pnraytracing_amd import build
    lib = build.variant_path("bounds")
    assert os.path.exists(lib), "variants/libpnrt_bounds.so not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(HERE, "rays_adaptive_worker.py")], env=dict(os.environ, PNRT_DEVICE_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RAYS-ADAPTIVE-WORKER-DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIAGNOSTIC BUILD" in r.stdout and r.stdout.count(": ok") == 4
