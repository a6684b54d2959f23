"""pnrt_render_rays, pnrt_render_guides_rays and pnrt_make_rays.

pnrt_make_rays against the numpy restatement (rays_ref.py); pnrt_render_rays against
pnrt_render, against the CPU oracle (pinhole rays of three cameras interleaved per pixel:
every pixel is the oracle's pixel for its own camera sequence) and against itself around
no-ray records; pnrt_render_guides_rays against the oracle's closest hits of the same rays.

Tolerance: 0 ulp (uint32 views compared) everywhere."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import moments_ref as MR
import pyoracle
import rays_ref as R
import test_gpu_cameras as T          # its scenes and helpers; nothing runs on import
from pnraytracing_amd import host as H
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
MODES = T.MODES
bits, same, load, scene = T.bits, T.same, T.load, T.scene
FLOAT_MAX = F(10000000.0)


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def dev(a):
    """A host array as a device tensor, complete before anything else is queued."""
    t = torch.from_numpy(np.ascontiguousarray(a, F)).cuda()
    torch.cuda.synchronize()
    return t


def host_of(pt, t):
    """A device tensor the context wrote, on the host."""
    pt.synchronize()
    return t.cpu().numpy()


def look(cfg, dx, dy, fov=None):
    """cfg's Cornell camera turned towards (dx, 2.8 + dy, 0)."""
    fov = 45.0 if fov is None else fov
    return np.asarray(H.camera_update((0, 2.8, 7), (dx, 2.8 + dy, 0), (0, 1, 0), fov, F(cfg.width) / F(cfg.height)), F).reshape(4, 3)


def elsewhere(cfg):
    """A camera that looks at something else entirely (the pnrt_set_frame camera the ray calls ignore)."""
    return look(cfg, 2.5, -1.5, 60.0)


# ---- 1. pnrt_make_rays against the numpy restatement ---------------------------------------------
CAM = np.asarray(H.camera_update((1.5, 3.1, 6.0), (0.2, 2.5, -0.4), (0.1, 1.0, 0.05), 50.0, F(67) / F(45)), F).reshape(4, 3)
VARIANTS = {
    "pinhole": [{}, {"aa_width": 1.0}, {"aa_width": 1.5, "per_pixel": 1},
                {"lens_radius": 0.2, "focus_distance": 6.0}, {"aa_width": 1.0, "lens_radius": 0.2, "focus_distance": 6.0, "per_pixel": 1}],
    "ortho": [{}, {"aa_width": 1.0}, {"aa_width": 1.0, "per_pixel": 1}],
    "equirect": [{}, {"aa_width": 1.0}, {"aa_width": 2.0, "per_pixel": 1}],
    "fisheye": [{"fov_deg": 180.0}, {"fov_deg": 220.0, "aa_width": 1.0}, {"fov_deg": 360.0, "aa_width": 1.0, "per_pixel": 1},
                {"fov_deg": 90.0}],
}


@pytest.mark.parametrize("W,Hh", [(67, 45), (8, 8), (1, 1)])
@pytest.mark.parametrize("model", R.MODELS)
def test_make_rays_equals_the_restatement(pt, model, W, Hh):
    pt.set_frame(W, Hh, CAM, 4)
    pix = W * Hh
    for params in VARIANTS[model]:
        # one set (frame_stride 0), frame 5
        got = host_of(pt, pt.make_rays(model, CAM, 5, 1, **params))
        want = R.make_set(model, CAM, W, Hh, 5, **params)
        assert got.shape == (pix, 8)
        assert np.array_equal(bits(got), bits(want)), (model, params, "stride 0")
        # three sets with a gap, across the frame number where (float)(frame + 1) stops being exact
        first, stride = 0xFFFFFF - 1, pix + 5
        buf = dev(np.full((2 * stride + pix, 8), 7.0, F))
        out = pt.make_rays(model, CAM, first, 3, stride, out=buf, **params)
        assert out is buf
        got = host_of(pt, buf)
        want = R.make_rays(model, CAM, W, Hh, first, 3, stride, fill=7.0, **params)
        assert np.array_equal(bits(got), bits(want)), (model, params, "three sets")
        assert (got[pix:stride] == 7.0).all() and (got[stride + pix:2 * stride] == 7.0).all()      # gap records untouched
    # frame_stride 0 with several sets: the set of first_frame, once
    params = VARIANTS[model][1]
    got = host_of(pt, pt.make_rays(model, CAM, 9, 4, 0, **params))
    assert np.array_equal(bits(got), bits(R.make_set(model, CAM, W, Hh, 9, **params)))


def test_make_rays_refusals(pt):
    W, Hh = 8, 8
    with PathTracer(0) as fresh:
        with pytest.raises(PnrtError) as e:
            fresh.make_rays("pinhole", CAM, 0, 1, out=dev(np.zeros((64, 8), F)))
        assert e.value.code == -3                        # before pnrt_set_frame
    pt.set_frame(W, Hh, CAM, 4)
    buf = dev(np.full((3 * 64, 8), 3.0, F))

    def refused(model, cam=CAM, first=0, n=1, out=buf, stride=0, **params):
        with pytest.raises(PnrtError) as e:
            pt.make_rays(model, cam, first, n, stride, out=out, **params)
        assert e.value.code == -1, str(e.value)

    refused(4)
    refused(-1)
    for i in (0, 5, 11):
        for v in (np.nan, np.inf):
            bad = CAM.copy()
            bad.reshape(-1)[i] = v
            refused("ortho", bad)
    for fov in (0.0, -10.0, 360.5, np.nan):
        refused("fisheye", fov_deg=fov)
    for v in (-1.0, np.nan, np.inf):
        refused("pinhole", aa_width=v)
        refused("pinhole", lens_radius=v, focus_distance=5.0)
    for model in ("ortho", "equirect", "fisheye"):
        refused(model, lens_radius=0.1, focus_distance=5.0)
    for focus in (0.0, -1.0, np.nan):
        refused("pinhole", lens_radius=0.1, focus_distance=focus)
    refused("pinhole", per_pixel=2)
    refused("pinhole", per_pixel=-1)
    refused("pinhole", reserved=1)
    refused("pinhole", out=buf.data_ptr() + 8)           # not 16-byte aligned
    refused("pinhole", out=0)                            # NULL
    refused("pinhole", n=2, stride=63)
    refused("pinhole", n=2, stride=-1)
    refused("pinhole", first=0xFFFFFFFF, n=2, stride=64)
    assert (host_of(pt, buf) == 3.0).all()               # nothing was written
    pt.make_rays("pinhole", CAM, 0, 0, 64, out=buf)      # n_sets == 0: nothing queued
    assert (host_of(pt, buf) == 3.0).all()


# ---- 2. pinhole rays without samples: pnrt_render's image -----------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_pinhole_rays_give_render(pt, mode):
    cfg = scene("c1", 37, 19)                            # partial tiles in both directions
    load(pt, cfg, mode)
    pt.render(0, 5)
    ref = pt.read_accum()
    assert ref[..., :3].any()
    pt.set_frame(37, 19, elsewhere(cfg), cfg.max_depth)  # the pnrt_set_frame camera is ignored
    pt.reset_accum()
    one = pt.make_rays("pinhole", cfg.camera)
    pt.render_rays(0, 5, one)
    same(pt.read_accum(), ref, f"one set, mode {mode}")
    pt.reset_accum()
    pix = 37 * 19
    sets = pt.make_rays("pinhole", cfg.camera, 0, 5, pix + 7)
    assert sets.shape == (4 * (pix + 7) + pix, 8)
    pt.render_rays(0, 5, sets, pix + 7)
    same(pt.read_accum(), ref, f"a set per frame, mode {mode}")
    pt.reset_accum()
    pt.render_rays(0, 5, int(one.data_ptr()))            # an integer pointer
    same(pt.read_accum(), ref, "an integer pointer")
    # ... and the ignored camera is what pnrt_render renders afterwards
    pt.reset_accum()
    pt.render(0, 1)
    assert T.n_differ(pt.read_accum(), ref) > pix // 2


# ---- 3. three cameras interleaved per pixel against the oracle ------------------------------------
def three_cameras(cfg, name):
    fov = 100.0 if name == "c2wide" else None
    return [look(cfg, *d, fov) for d in ((-0.45, 0.3), (0.4, -0.25), (0.1, 0.55))]


@functools.lru_cache(maxsize=None)
def interleaved_reference(name, W, Hh, depth):
    """Pixel (x, y) of frame f takes camera (x + 2y + f) % 3: the pixels of class g = (x + 2y) % 3
    see the camera sequence (g + f) % 3, f = 0..5, and are the oracle's pixels for it."""
    cfg = scene(name, W, Hh)
    cams = three_cameras(cfg, name)
    x, y = np.meshgrid(np.arange(W), np.arange(Hh))
    cls = (x + 2 * y) % 3
    pin = T.oracle_cameras(cfg, 0, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (6, 1)), depth)
    ref = np.zeros((Hh, W, 4), F)
    for g in range(3):
        img = T.oracle_cameras(cfg, 0, np.stack([cams[(g + f) % 3] for f in range(6)]), depth)
        # the cameras matter: more than half of the class image's lit pixels differ from the pnrt_set_frame camera's
        lit = img[..., :3].any(axis=-1) | pin[..., :3].any(axis=-1)
        differ = np.any(bits(img)[..., :3] != bits(pin)[..., :3], axis=-1)
        assert lit.sum() > 0 and differ.sum() > lit.sum() // 2, (name, depth, g, int(differ.sum()), int(lit.sum()))
        ref[cls == g] = img[cls == g]
    assert np.isfinite(ref).all()
    ref.setflags(write=False)
    return cls, ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [0, 1, 4])
@pytest.mark.parametrize("name,W,Hh", [("c1", 40, 24), ("c2wide", 48, 32)])
def test_interleaved_cameras_match_the_oracle(pt, name, W, Hh, depth, mode):
    cfg = scene(name, W, Hh)
    cls, ref = interleaved_reference(name, W, Hh, depth)
    load(pt, cfg, mode, depth)
    per_cam = [host_of(pt, pt.make_rays("pinhole", c)).reshape(Hh, W, 8) for c in three_cameras(cfg, name)]
    sets = np.zeros((6, Hh, W, 8), F)
    for f in range(6):
        for k in range(3):
            pick = (cls + f) % 3 == k
            sets[f][pick] = per_cam[k][pick]
    rays = dev(sets.reshape(-1, 8))
    pt.render_rays(0, 6, rays, W * Hh)
    same(pt.read_accum(), ref, f"{name} depth {depth} mode {mode}")


# ---- 4. guide images of a ray set against the oracle's closest hits -------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", ["fisheye", "equirect"])
def test_guides_of_a_ray_set(pt, model, mode):
    W, Hh = 48, 32
    cfg = scene("c2", W, Hh)
    load(pt, cfg, mode)
    # an eye inside the box, off its axes: most rays hit, those through the open front see the environment
    inside = np.asarray(H.camera_update((0.3, 2.5, 3.0), (0, 2.8, 0), (0, 1, 0), 45.0, F(W) / F(Hh)), F).reshape(4, 3)
    rays = pt.make_rays(model, inside, fov_deg=200.0)
    r = host_of(pt, rays)
    is_ray = r[:, 4:7].any(axis=1)
    if model == "fisheye":
        assert np.array_equal(~is_ray, R.fisheye_rho(W, Hh) > 1) and (~is_ray).sum() > 100
    else:
        assert is_ray.all()
    r7 = np.concatenate([r[is_ray, 0:3], r[is_ray, 4:7], np.full((int(is_ray.sum()), 1), FLOAT_MAX, F)], axis=1)
    o = np.zeros((W * Hh, 13), np.uint32)
    o[is_ray] = pyoracle.Oracle(cfg).intersect(r7, kind=0, sem=0)
    hit = o[:, 0] != 0
    assert hit.sum() > W * Hh // 3 and (is_ray & ~hit).sum() > 100
    pt.profile_enable(True)
    pt.render_guides_rays(rays)
    pos, nrm, alb = (pt.read_aov(k).reshape(-1, 4) for k in ("position", "normal", "albedo"))
    launches = {k: v[1] for k, v in pt.profile_read().items()}
    pt.profile_enable(False)
    assert launches["primary"] == 1 and launches["trace"] == launches["gen"] == 0
    assert np.array_equal(bits(pos[:, :3]), o[:, 1:4]) and np.array_equal(pos[:, 3], hit.astype(F))
    assert np.array_equal(bits(nrm[:, :3]), o[:, 4:7])
    assert np.array_equal(nrm[:, 3], np.where(hit, o[:, 10].view(np.int32), -1).astype(F))
    assert np.array_equal(alb[:, 3], np.where(hit, o[:, 9].view(np.int32), -1).astype(F))
    # records outside the fisheye circle are misses whose albedo is 0; rays that miss show the environment
    assert not pos[~is_ray].any() and not alb[~is_ray, :3].any() and (nrm[~is_ray, 3] == -1).all()
    assert alb[is_ray & ~hit, :3].any()
    # the preview accepts them, whatever the pnrt_set_frame camera; a scene edit makes them stale again
    pt.render_rays(0, 2, rays)
    pt.set_frame(W, Hh, elsewhere(cfg), cfg.max_depth)
    pt.denoise()
    out = pt.read_denoised()
    assert np.isfinite(out).all() and out[..., :3].any()
    assert pt.aov_ptr("position") and np.array_equal(bits(pt.read_aov("normal").reshape(-1, 4)), bits(nrm))
    pt.update_materials(0, np.asarray(cfg.packed.materials, F)[0:1])
    with pytest.raises(PnrtError) as e:
        pt.denoise()
    assert e.value.code == -3
    pt.render_guides_rays(rays)
    pt.denoise()
    # camera-keyed guides replace them and keep their own staleness rule
    pt.render_guides()
    pt.denoise()
    pt.set_frame(W, Hh, cfg.camera, cfg.max_depth)
    with pytest.raises(PnrtError) as e:
        pt.denoise()
    assert e.value.code == -3
    # the traversal mode is part of the key
    pt.render_guides_rays(rays)
    pt.set_options(MODES[0] if mode == MODES[1] else MODES[1])
    with pytest.raises(PnrtError) as e:
        pt.denoise()
    assert e.value.code == -3


# ---- 5. no-ray records ----------------------------------------------------------------------------
def test_no_ray_records_are_black_and_touch_nothing_else(pt):
    W, Hh = 40, 24
    cfg = scene("c2", W, Hh)
    frames = (0, 1, 3, 7)                                # blend weights that are powers of two (test_gpu_cameras)
    orc = pyoracle.Oracle(cfg)
    pin = np.asarray(cfg.camera, F).reshape(1, 12)
    colors = []
    for f in frames:
        rgb = T.oracle_cameras(cfg, f, pin, orc=orc)[..., :3]
        assert not ((rgb != 0) & (np.abs(rgb) < np.finfo(F).tiny)).any()
        colors.append((rgb * F(f + 1)).astype(F))
    load(pt, cfg)
    good = host_of(pt, pt.make_rays("pinhole", cfg.camera)).reshape(Hh, W, 8)
    spots = {(3, 5): ("origin", 1, np.nan), (17, 20): ("direction", 2, np.inf), (23, 39): ("direction", None, 0.0),
             (0, 0): ("origin", 0, -np.inf), (8, 8): ("direction", 0, np.nan)}
    bad = good.copy()
    for (y, x), (what, comp, v) in spots.items():
        base = 0 if what == "origin" else 4
        if comp is None:
            bad[y, x, 4:7] = 0.0
        else:
            bad[y, x, base + comp] = v
    bad[5, 5, 3], bad[5, 5, 7] = np.nan, np.inf          # the reserved floats are never read
    black = np.zeros((Hh, W), bool)
    for y, x in spots:
        black[y, x] = True
    results = {}
    for key, arr in (("good", good), ("bad", bad)):
        rays = dev(arr.reshape(-1, 8))
        pt.enable_moments(True)
        pt.reset_accum()
        pt.render_rays(0, 2, rays)
        pt.render_rays(3, 1, rays)
        pt.render_rays(7, 1, rays)
        results[key] = (pt.read_accum(), pt.read_moments())
        pt.enable_moments(False)
    (acc_g, mom_g), (acc_b, mom_b) = results["good"], results["bad"]
    assert acc_g[black][:, :3].any(axis=1).all()         # those pixels show something
    assert not acc_b[black][:, :3].any()                 # frame colour 0 in every frame
    assert np.array_equal(bits(acc_b[~black]), bits(acc_g[~black]))      # every other pixel keeps its bits
    assert np.array_equal(bits(mom_b[~black]), bits(mom_g[~black]))
    # the oracle's accumulation and moments, with Y = 0 in the no-ray pixels
    zeroed = [np.where(black[..., None], F(0), c) for c in colors]
    assert np.array_equal(bits(acc_g[..., :3]), bits(MR.blend(np.zeros((Hh, W, 4), F), colors, frames)[..., :3]))
    assert np.array_equal(bits(mom_g), bits(MR.update(MR.zeros(Hh, W), colors, frames)))
    assert np.array_equal(bits(mom_b), bits(MR.update(MR.zeros(Hh, W), zeroed, frames)))
    assert np.array_equal(bits(acc_b[..., :3]), bits(MR.blend(np.zeros((Hh, W, 4), F), zeroed, frames)[..., :3]))
    # the moments cover the accumulation: an adaptive call is accepted after ray frames
    pt.enable_moments(True)
    pt.reset_accum()
    pt.render_rays(0, 2, dev(bad.reshape(-1, 8)))
    assert pt.render_adaptive(2, 0, 0.0, 2)["n_pixels"] == W * Hh
    pt.enable_moments(False)
    pt.render_rays(2, 1, dev(bad.reshape(-1, 8)))        # frames the moments do not count break the cover
    pt.enable_moments(True)
    with pytest.raises(PnrtError) as e:
        pt.render_adaptive(3, 1, 0.0, 2)
    assert e.value.code == -3
    pt.enable_moments(False)


# ---- 6. the rest of the contract ------------------------------------------------------------------
def lens_sets(pt, cfg, first, n, stride=None, per_pixel=0):
    """A set per frame around cfg's camera: a one-pixel filter and a lens, sampled per frame --
    the cameras of T.lens_cameras up to the arithmetic -- or per pixel."""
    return pt.make_rays("pinhole", cfg.camera, first, n, stride, aa_width=1.0, lens_radius=0.15, focus_distance=7.0,
                        per_pixel=per_pixel)


def single_frames(pt, cfg, first, rays, stride, n):
    """The accumulation of frames first .. first + n - 1, one synchronised one-frame call each
    (every call a lone call on the context's stream, one batch, set k passed as its own buffer)."""
    pt.reset_accum()
    pix = cfg.width * cfg.height
    for k in range(n):
        pt.render_rays(first + k, 1, int(rays.data_ptr()) + 32 * k * stride)
        pt.synchronize()
    assert stride == 0 or stride >= pix
    return pt.read_accum()


def test_high_first_frame(pt):
    cfg = scene("c1", 40, 24)
    first = 0xFFFFFF - 2
    load(pt, cfg)
    # against the oracle: pinhole rays, where it can follow
    rays = pt.make_rays("pinhole", cfg.camera)
    pt.render_rays(first, 6, rays)
    same(pt.read_accum(), T.oracle_cameras(cfg, first, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (6, 1))), "pinhole, high frames")
    # a set per frame: set k belongs to frame first + k, whatever the frame number
    sets = lens_sets(pt, cfg, first, 6, per_pixel=1)
    ref = single_frames(pt, cfg, first, sets, 40 * 24, 6)
    pt.reset_accum()
    pt.render_rays(first, 6, sets, 40 * 24)
    same(pt.read_accum(), ref, "a set per frame, high frames")
    assert not np.array_equal(bits(host_of(pt, sets)), bits(host_of(pt, lens_sets(pt, cfg, 0, 6, per_pixel=1))))


def test_two_batches_with_one_set(pt):
    cfg = scene("c1", 16, 8)
    load(pt, cfg)
    plan = pt.cameras_batch_plan(130)
    assert (plan["frames_per_batch"], plan["n_batches"]) == (128, 2)
    ref = T.oracle_cameras(cfg, 0, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (130, 1)))
    rays = pt.make_rays("pinhole", cfg.camera)
    pt.set_frame(16, 8, elsewhere(cfg), cfg.max_depth)
    pt.synchronize()
    pt.profile_enable(True)
    pt.render_rays(0, 130, rays, 0)
    got = pt.read_accum()
    launches = {k: v[1] for k, v in pt.profile_read().items()}
    pt.profile_enable(False)
    same(got, ref, "130 frames in two batches")
    # one ray launch, one gen and one blend per batch; no setup / v1 class
    assert (launches["primary"], launches["gen"], launches["blend"]) == (2, 2, 2), launches
    assert launches["trace"] == launches["shade"] == 2 * cfg.max_depth and launches["setup"] == launches["v1"] == 0


def test_capped_context_reads_each_batchs_sets(pt):
    cfg = scene("c1", 24, 16)
    load(pt, cfg)
    by = [0] + [pt.cameras_batch_plan(k)["batch_bytes"] for k in range(1, 7)]
    cap = by[4] + (by[5] - by[4]) // 2                   # 4 frames fit, 5 do not: 12 frames = 3 batches
    pix, stride = 24 * 16, 24 * 16 + 11
    with T.capped_tracer(cap) as t:
        load(t, cfg)
        plan = t.cameras_batch_plan(12)
        assert (plan["frames_per_batch"], plan["n_batches"], plan["batch_bytes"]) == (4, 3, by[4])
        sets = lens_sets(t, cfg, 0, 12, stride, per_pixel=1)
        ref = single_frames(t, cfg, 0, sets, stride, 12)
        t.reset_accum()
        t.profile_enable(True)
        t.render_rays(0, 12, sets, stride)
        got = t.read_accum()
        launches = {k: v[1] for k, v in t.profile_read().items()}
        same(got, ref, "12 frames under a cap, 3 batches")
        assert (launches["primary"], launches["gen"], launches["blend"]) == (3, 3, 3), launches
        assert T.n_differ(ref, single_frames(t, cfg, 0, sets, 0, 12)) > pix // 2      # the sets differ: set 0 alone is another image


def test_shards_render_their_rows_only(pt):
    cfg = scene("c1", 40, 24)
    load(pt, cfg)
    sets = lens_sets(pt, cfg, 0, 3, per_pixel=1)
    ref = single_frames(pt, cfg, 0, sets, 40 * 24, 3)
    pt.reset_accum()
    y = np.arange(24)
    done = np.zeros(24, bool)
    for shard in range(3):
        pt.render_rays(0, 3, sets, 40 * 24, 4, 3, shard)
        got = pt.read_accum()
        done |= (y // 4) % 3 == shard
        same(got[done], ref[done], f"rows of shards 0..{shard}")
        assert not got[~done].any(), f"shard {shard} touched another shard's rows"
    assert done.all()
    before = pt.read_accum()
    pt.render_rays(3, 3, sets, 40 * 24, 24, 3, 1)        # a shard without rows queues nothing
    same(pt.read_accum(), before, "a shard without rows")


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
    pin = np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (3, 1))
    ref = T.oracle_cameras(cfg, 0, pin)
    assert ref[..., :3].any()
    for mode in MODES:
        load(pt, cfg, mode)
        info = pt.device_info()
        assert {k: info[k] for k in want} == want
        rays = pt.make_rays("pinhole", cfg.camera)
        pt.set_frame(W, Hh, elsewhere(cfg), cfg.max_depth)
        pt.render_rays(0, 3, rays)
        same(pt.read_accum(), ref, f"{cfg.name} mode {mode}")
        # a fisheye view of the same scene: the guides of its rays against the oracle
        fish = pt.make_rays("fisheye", cfg.camera, fov_deg=170.0)
        r = host_of(pt, fish)
        ok = r[:, 4:7].any(axis=1)
        o = np.zeros((W * Hh, 13), np.uint32)
        o[ok] = pyoracle.Oracle(cfg).intersect(np.concatenate([r[ok, 0:3], r[ok, 4:7], np.full((int(ok.sum()), 1), FLOAT_MAX, F)], axis=1),
                                               kind=0, sem=0)
        pt.render_guides_rays(fish)
        assert np.array_equal(bits(pt.read_aov("position").reshape(-1, 4)[:, :3]), o[:, 1:4]), f"{cfg.name} mode {mode}"


def test_rays_written_on_the_context_stream_just_before(pt):
    """A 40-frame call first (only a call behind another one runs on a pipe's worker stream),
    then the second call's rays are written by torch kernels on the wrapped context stream --
    behind enough other work that they are still pending when pnrt_render_rays returns."""
    cfg = scene("c1", 40, 24)
    load(pt, cfg)
    pix = 40 * 24
    a = lens_sets(pt, cfg, 0, 40, per_pixel=1)
    b = lens_sets(pt, cfg, 40, 5, per_pixel=1)
    ref = single_frames(pt, cfg, 0, a, pix, 40)
    for k in range(5):
        pt.render_rays(40 + k, 1, int(b.data_ptr()) + 32 * k * pix)
        pt.synchronize()
    ref = pt.read_accum()
    pt.reset_accum()
    pt.synchronize()
    ext = torch.cuda.ExternalStream(pt.stream_handle(), device=torch.device("cuda", 0))
    late = torch.full_like(b, float("nan"))
    torch.cuda.synchronize()
    pt.render_rays(0, 40, a, pix)
    with torch.cuda.stream(ext):
        m = torch.ones((2048, 2048), device="cuda")
        for _ in range(20):
            m = (m @ m) * (1.0 / 2048.0)
        late.copy_(b * m[0, 0])                          # (m stays all ones: exact)
    pt.render_rays(40, 5, late, pix)
    got = pt.read_accum()
    assert np.isfinite(got).all()
    same(got, ref, "rays written just before the call")


def test_render_afterwards_keeps_its_records(pt):
    cfg = scene("c2", 40, 24)
    pin = np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (2, 1))
    other = elsewhere(cfg)
    orc = pyoracle.Oracle(cfg)
    ref = T.oracle_cameras(cfg, 0, pin, orc=orc)
    T.oracle_cameras(cfg, 2, np.tile(other.reshape(1, 12), (3, 1)), acc=ref, orc=orc)
    T.oracle_cameras(cfg, 5, pin, acc=ref, orc=orc)
    load(pt, cfg)
    rays = pt.make_rays("pinhole", other)
    pt.synchronize()
    pt.profile_enable(True)
    pt.render(0, 2)
    pt.synchronize()
    n0 = pt.profile_read()["primary"][1]
    pt.render_rays(2, 3, rays)
    pt.synchronize()
    n1 = pt.profile_read()["primary"][1]
    pt.render(5, 2)                                      # its kept per-pixel records: no camera-ray launch
    got = pt.read_accum()
    n2 = pt.profile_read()["primary"][1]
    pt.profile_enable(False)
    same(got, ref, "render, render_rays, render")
    assert (n1 - n0, n2 - n1) == (1, 0), (n0, n1, n2)


def test_refusals_leave_the_accumulation(pt):
    cfg = scene("c1", 16, 8)
    pix = 16 * 8
    with PathTracer(0) as fresh:
        buf = dev(np.zeros((pix, 8), F))
        for step in ("nothing", "scene only"):
            with pytest.raises(PnrtError) as e:
                fresh.render_rays(0, 1, buf)
            assert e.value.code == -3, step              # PNRT_E_STATE
            with pytest.raises(PnrtError) as e:
                fresh.render_guides_rays(buf)
            assert e.value.code == -3, step
            fresh.upload_scene(cfg.packed)
    load(pt, cfg)
    rays = pt.make_rays("pinhole", cfg.camera, 0, 4, pix)
    pt.render_rays(0, 4, rays, pix)
    before = pt.read_accum()
    assert before[..., :3].any()

    def refused(code, *args):
        with pytest.raises(PnrtError) as e:
            pt.render_rays(*args)
        assert e.value.code == code, str(e.value)
        same(pt.read_accum(), before, f"after the refusal of {args[2:]}")

    for sel in ((0, 1, 0), (1, 0, 0), (1, 2, 2), (1, 2, -1)):
        refused(-1, 4, 4, rays, pix, *sel)
    refused(-1, 0xFFFFFFFF - 3, 4, rays, pix)            # first + 4 = 2^32 > 0xFFFFFFFF
    refused(-1, 4, 4, None, pix)                         # rays_dev == NULL with n_frames > 0
    for off in (4, 8, 12):
        refused(-1, 4, 4, int(rays.data_ptr()) + off, pix)
    for stride in (-1, 1, pix - 1, -pix, 2 ** 62, (2 ** 63 - 1) // 32 // 3):     # ... or the last set's end past 2^63 bytes
        refused(-1, 4, 4, rays, stride)
    for off in (4, 8):
        with pytest.raises(PnrtError) as e:
            pt.render_guides_rays(int(rays.data_ptr()) + off)
        assert e.value.code == -1
    with pytest.raises(PnrtError) as e:
        pt.render_guides_rays(None)
    assert e.value.code == -1
    # n_frames == 0 queues nothing, with or without a buffer
    pt.render_rays(4, 0, None)
    pt.render_rays(4, 0, rays, pix)
    same(pt.read_accum(), before, "after n_frames == 0")
    # PNRT_KERNEL_V1 renders the pnrt_set_frame camera only
    pt.set_options(TRAVERSE_ZCULL | KERNEL_V1)
    refused(-3, 4, 4, rays, pix)
    pt.set_options(TRAVERSE_ZCULL)
    # ... and the call still works
    pt.render_rays(4, 4, rays, 0)
    assert T.n_differ(pt.read_accum(), before) > 0


# ---- the interactive session ----------------------------------------------------------------------
def test_session_with_a_camera_model(pt):
    from pnraytracing_amd.session import CameraController, InteractiveSession
    W, Hh = 40, 24
    cfg = scene("c2", W, Hh)
    load(pt, cfg)
    cam = CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, F(W) / F(Hh))
    sess = InteractiveSession(pt, W, Hh, cam)
    sess.set_camera_model("pinhole")                     # the pinhole model without samples is the plain session
    orc = pyoracle.Oracle(cfg)
    acc = np.zeros((Hh, W, 4), F)
    for step, redraw in enumerate([False, False, True, False, False]):
        if redraw:
            cam.rotate(3.0, -1.0)
        fc = 0 if redraw else sess.frame_count
        depth, _ = sess.frame(redraw)
        T.oracle_cameras(cfg, fc, cam.uniforms().reshape(1, 12), depth, acc=acc, orc=orc)
        same(pt.read_accum(), acc, f"frame {step} (redraw={redraw})")
    sess.set_camera_model("fisheye", fov_deg=150.0)
    sess.frame(True)                                     # the same depth-1 frame 0 through the ray path
    img = pt.read_accum()
    rho = R.fisheye_rho(W, Hh).reshape(Hh, W)
    assert not img[rho > 1][:, :3].any() and img[rho <= 1][:, :3].any()
    sess.frame()
    sess.frame()
    assert sess.frame_count == 2
    sess.preview()
    out = pt.read_denoised()
    assert np.isfinite(out).all() and out[..., :3].any()
    pos = pt.read_aov("position")
    r = R.make_set("fisheye", cam.uniforms(), W, Hh, 0, fov_deg=150.0)        # the guides are the centre rays'
    ok = rho.reshape(-1) <= 1
    o = np.zeros((W * Hh, 13), np.uint32)
    o[ok] = orc.intersect(np.concatenate([r[ok, 0:3], r[ok, 4:7], np.full((int(ok.sum()), 1), FLOAT_MAX, F)], axis=1), kind=0, sem=0)
    assert np.array_equal(bits(pos.reshape(-1, 4)[:, :3]), o[:, 1:4]) and pos[..., 3].sum() == (o[:, 0] != 0).sum() > 100


def test_session_preview_follows_the_view(pt):
    """Guides made from rays carry no camera, so the library accepts them for any view: the session itself renders
    them again after a camera move, a change of fov_deg and a change of model, and goes back to camera-keyed guides
    with the pinhole model.  The position guide is the oracle's closest hit of the new view's rays every time."""
    from pnraytracing_amd.session import CameraController, InteractiveSession
    W, Hh = 40, 24
    cfg = scene("c2", W, Hh)
    load(pt, cfg)
    cam = CameraController((0.3, 2.5, 3.0), (0, 2.8, 0), (0, 1, 0), 45.0, F(W) / F(Hh))      # inside the box: most rays hit
    sess = InteractiveSession(pt, W, Hh, cam)
    orc = pyoracle.Oracle(cfg)

    def expect(model, fov):
        r = R.make_set(model, cam.uniforms(), W, Hh, 0, fov_deg=fov)
        ok = r[:, 4:7].any(axis=1)
        o = np.zeros((W * Hh, 13), np.uint32)
        o[ok] = orc.intersect(np.concatenate([r[ok, 0:3], r[ok, 4:7], np.full((int(ok.sum()), 1), FLOAT_MAX, F)], axis=1), kind=0, sem=0)
        assert (o[:, 0] != 0).sum() > 100
        return o[:, 1:4]

    def position():
        return bits(pt.read_aov("position").reshape(-1, 4)[:, :3])

    sess.set_camera_model("fisheye", fov_deg=150.0)
    sess.frame()
    sess.preview()
    first = expect("fisheye", 150.0)
    assert np.array_equal(position(), first)
    pt.profile_enable(True)
    sess.frame()
    sess.preview()                                       # nothing changed: the guides stay
    assert pt.profile_read()["primary"][1] == 1          # (the frame's own ray launch)
    pt.profile_enable(False)
    cam.rotate(25.0, -8.0)                               # a camera move
    sess.frame(True)
    sess.preview()
    moved = expect("fisheye", 150.0)
    assert np.count_nonzero(np.any(moved != first, axis=1)) > W * Hh // 4
    assert np.array_equal(position(), moved)
    sess.set_camera_model("fisheye", fov_deg=100.0)      # another fov_deg
    sess.frame(True)
    sess.preview()
    narrow = expect("fisheye", 100.0)
    assert np.any(narrow != moved) and np.array_equal(position(), narrow)
    sess.set_camera_model("equirect")                    # another model
    sess.frame(True)
    sess.preview()
    assert np.array_equal(position(), expect("equirect", 180.0))
    with pytest.raises(ValueError):
        sess.reproject()                                 # no reprojection across ray sets
    sess.set_camera_model("pinhole")                     # back to the camera's own view: camera-keyed guides again
    sess.frame(True)
    sess.preview()
    pin = expect("pinhole", 180.0)
    assert np.array_equal(position(), pin)
    cam.rotate(-10.0, 3.0)
    sess.frame(True)
    sess.preview()                                       # ... whose staleness the library judges
    assert np.any(expect("pinhole", 180.0) != pin) and np.array_equal(position(), expect("pinhole", 180.0))


# ---- every index checked --------------------------------------------------------------------------
def test_rays_on_bounds_checked_library():
    """Partial tiles, no-ray records (a fisheye's zeros; hand-made NaN and infinite floats), misses, the three scene kinds, a set per frame and a
    three-batch call on the `bounds` diagnostic library: every fetch and store index of the ray,
    gen, trace and shade kernels is checked against its array, and a violation is an error."""
    from pnraytracing_amd import build
    lib = build.variant_path("bounds")
    assert os.path.exists(lib), "variants/libpnrt_bounds.so not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(HERE, "rays_worker.py")], env=dict(os.environ, PNRT_DEVICE_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RAYS-WORKER-DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIAGNOSTIC BUILD" in r.stdout and r.stdout.count(": ok") == 16
