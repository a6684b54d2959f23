"""pnrt_render_cameras against the CPU oracle.

Frame first + k of a call is the reference's shader with cameras[k] as its camera
uniforms, so the oracle side is the oracle as it is, driven frame by frame: Oracle.frame's
four vectors set to cameras[k], then render(first + k, 1, accum=acc).

Tolerance: 0 ulp (uint32 views compared) everywhere."""
import contextlib
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import moments_ref as MR
import pyoracle
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.session import CameraController, InteractiveSession
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_cameras")
MODES = (TRAVERSE_ZCULL, TRAVERSE_EXACT)
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(got, ref, what):
    bad = np.argwhere(np.any(bits(got) != bits(ref), axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.shape[0] * got.shape[1]} pixels differ, first {bad[:5].tolist()}"


def n_differ(a, b):
    return int(np.count_nonzero(np.any(bits(a)[..., :3] != bits(b)[..., :3], axis=-1)))


@functools.lru_cache(maxsize=None)
def scene(name, W, Hh):
    if name == "c1":
        return S.cornell_c1(W, Hh, spp=1)
    if name == "c2":
        return S.bunny_c2(W, Hh, spp=1, nu=24, nv=12, env=True)
    if name == "c2wide":           # the rays around the box miss: the environment shows, by each frame's direction
        cam = H.camera_update((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 100.0, F(W) / F(Hh))
        return dataclasses.replace(scene("c2", W, Hh), name="C2-bunny-wide", camera=cam)
    raise KeyError(name)


def lens_cameras(cfg, first, n, aa=1.0, radius=0.15, focus=7.0):
    """The camera sequence around cfg's camera: a one-pixel filter and a lens."""
    return H.camera_sequence(cfg.camera, cfg.width, cfg.height, first, n, aa_width=aa, lens_radius=radius, focus_distance=focus)


def oracle_cameras(cfg, first, cams, depth=None, acc=None, orc=None):
    """The oracle's accumulation of frames first + k rendered with cams[k], into acc."""
    orc = orc or pyoracle.Oracle(cfg)
    if acc is None:
        acc = np.zeros((cfg.height, cfg.width, 4), F)
    f = orc.frame
    f.max_bounce_depth = cfg.max_depth if depth is None else depth
    for k, cam in enumerate(np.asarray(cams, F).reshape(-1, 4, 3)):
        f.eye[:], f.lower_left[:], f.horizontal[:], f.vertical[:] = (list(map(float, r)) for r in cam)
        _, st = orc.render(first + k, 1, accum=acc)
        assert st["stack_overflow"] == 0
    return acc


def load(pt, cfg, mode=TRAVERSE_ZCULL, depth=None):
    pt.upload_scene(cfg.packed)
    for slot, (px, w, h, ch) in enumerate(cfg.textures):
        pt.upload_texture(slot, px, w, h, ch)
    pt.upload_env(cfg.env_rgb, cfg.env_table)
    pt.set_frame(cfg.width, cfg.height, cfg.camera, cfg.max_depth if depth is None else depth)
    pt.set_options(mode)
    pt.enable_moments(False)
    pt.reset_accum()


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


# ---- 1. identical cameras: pnrt_render's image ----------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_identical_cameras_give_render(pt, mode):
    cfg = scene("c1", 37, 19)                        # partial tiles in both directions
    load(pt, cfg, mode)
    pt.render(0, 5)
    ref = pt.read_accum()
    assert ref[..., :3].any()
    pt.reset_accum()
    pt.render_cameras(0, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (5, 1)))
    same(pt.read_accum(), ref, f"identical cameras, mode {mode}")
    pt.reset_accum()
    pt.render_cameras(0, np.tile(np.asarray(cfg.camera, F).reshape(1, 4, 3), (5, 1, 1)))      # the (n, 4, 3) form
    same(pt.read_accum(), ref, f"identical cameras (n, 4, 3), mode {mode}")


# ---- 2. the sequence against the oracle ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sequence_reference(name, W, Hh, depth):
    cfg = scene(name, W, Hh)
    cams = lens_cameras(cfg, 0, 6)
    ref = oracle_cameras(cfg, 0, cams, depth)
    pin = oracle_cameras(cfg, 0, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (6, 1)), depth)
    assert np.isfinite(ref).all()
    ref.setflags(write=False)
    pin.setflags(write=False)
    return cams, ref, pin


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth", [0, 1, 4])
@pytest.mark.parametrize("name,W,Hh", [("c1", 40, 24), ("c2", 48, 32), ("c2wide", 48, 32)])
def test_sequence_matches_oracle(pt, name, W, Hh, depth, mode):
    """The cameras matter: the image differs from the pinhole image in more than half the
    pixels, so ignoring the table cannot pass.  At depth 0 a pixel is the emission of what
    its camera ray hits -- exactly 0 on every surface that does not emit, whatever the
    camera -- so there the count is taken over the pixels that are lit in either image
    (the light, and in c2wide the environment behind the rays that miss)."""
    cfg = scene(name, W, Hh)
    cams, ref, pin = sequence_reference(name, W, Hh, depth)
    if depth == 0:
        lit = int(np.count_nonzero(ref[..., :3].any(axis=-1) | pin[..., :3].any(axis=-1)))
        need = lit // 2
        assert lit > 0
    else:
        need = W * Hh // 2
    assert n_differ(ref, pin) > need, (n_differ(ref, pin), need)
    load(pt, cfg, mode, depth)
    pt.render_cameras(0, cams)
    got = pt.read_accum()
    same(got, ref, f"{name} depth {depth} mode {mode}")
    assert n_differ(got, pin) > need


def test_environment_follows_each_frames_direction():
    """c2wide has camera rays that miss: their colour is the environment along the frame's
    own direction (depth 0: nothing else in the image moves a miss pixel)."""
    _, ref, pin = sequence_reference("c2wide", 48, 32, 0)
    shown = pin[..., :3].any(axis=-1)                # depth 0: lit pixels are misses (and the few of the light)
    assert shown.sum() > 300
    assert np.count_nonzero(np.any(bits(ref)[..., :3] != bits(pin)[..., :3], axis=-1) & shown) > shown.sum() // 2


# ---- 3. frame index against array index ---------------------------------------------------------
def test_high_first_frame_uses_array_index(pt):
    cfg = scene("c1", 40, 24)
    first = 0xFFFFFF - 2                             # (float)(frame + 1) stops being exact inside the call
    cams = lens_cameras(cfg, first, 6)
    ref = oracle_cameras(cfg, first, cams)
    load(pt, cfg)
    pt.render_cameras(first, cams)
    same(pt.read_accum(), ref, "first_frame 0xFFFFFF - 2")
    # (had the library indexed the array by frame number, or the sequence by array index, these would be equal)
    assert not np.array_equal(bits(cams), bits(lens_cameras(cfg, 0, 6)))


# ---- 4. two batches -----------------------------------------------------------------------------
def test_second_batch_starts_at_its_own_cameras(pt):
    cfg = scene("c1", 16, 8)
    cams = lens_cameras(cfg, 0, 130)
    load(pt, cfg)
    plan = pt.cameras_batch_plan(130)
    assert (plan["frames_per_batch"], plan["n_batches"]) == (128, 2)
    ref = oracle_cameras(cfg, 0, cams)
    pt.profile_enable(True)
    pt.render_cameras(0, cams)
    got = pt.read_accum()
    launches = {k: v[1] for k, v in pt.profile_read().items()}
    pt.profile_enable(False)
    same(got, ref, "130 frames in two batches")
    # one camera-ray launch, one gen and one blend per batch; no setup / v1 class
    assert (launches["primary"], launches["gen"], launches["blend"]) == (2, 2, 2), launches
    assert launches["trace"] == launches["shade"] == 2 * cfg.max_depth and launches["setup"] == launches["v1"] == 0


# ---- 5. a capped context ------------------------------------------------------------------------
@contextlib.contextmanager
def capped_tracer(cap):
    """A fresh context created with PNRT_BATCH_BYTES = cap in the environment."""
    os.environ["PNRT_BATCH_BYTES"] = str(cap)
    t = None
    try:
        t = PathTracer(0)
        yield t
    finally:
        del os.environ["PNRT_BATCH_BYTES"]
        if t is not None:
            t.close()


def test_capped_context_plans_by_the_larger_measure(pt):
    cfg = scene("c1", 24, 16)
    load(pt, cfg)
    paths = 3 * 2 * 64                               # 8x8 tiles of 24x16
    by = [0]
    for k in range(1, 7):
        plan, plain = pt.cameras_batch_plan(k), pt.batch_plan(k)
        assert (plan["frames_per_batch"], plan["n_batches"]) == (k, 1)
        assert plan["batch_bytes"] == plain["batch_bytes"] + 48 * paths * k      # the documented per-path bytes
        by.append(plan["batch_bytes"])
    assert all(b > a for a, b in zip(by, by[1:]))
    cap = by[4] + (by[5] - by[4]) // 2               # 4 frames fit, 5 do not: 12 frames = 3 batches
    cams = lens_cameras(cfg, 0, 12)
    ref = oracle_cameras(cfg, 0, cams)
    with capped_tracer(cap) as t:
        load(t, cfg)
        plan = t.cameras_batch_plan(12)
        assert (plan["frames_per_batch"], plan["n_batches"], plan["batch_bytes"]) == (4, 3, by[4])
        # the same cap lets pnrt_render, whose paths are 48 bytes smaller, take more frames
        assert t.batch_plan(12)["frames_per_batch"] > 4
        t.profile_enable(True)
        t.render_cameras(0, cams)
        got = t.read_accum()
        launches = {k: v[1] for k, v in t.profile_read().items()}
        same(got, ref, "12 frames under a cap, 3 batches")
        assert (launches["primary"], launches["gen"], launches["blend"]) == (3, 3, 3), launches


# ---- 6. calls in flight, arrays overwritten -----------------------------------------------------
def test_back_to_back_calls_keep_their_own_cameras(pt):
    """A 40-frame call first (it keeps the GPU busy while the host submits the rest: only a
    call behind another one runs on a pipe's worker stream), then three calls with
    different arrays and no synchronisation, each array filled with NaN the moment its call
    returns.  A table read after the call returned, or overwritten by a later call while a
    queued batch still reads it, gives NaN or another frame's camera."""
    cfg = scene("c1", 40, 24)
    sizes = (40, 5, 3, 4)
    all_cams = lens_cameras(cfg, 0, sum(sizes))
    ref = oracle_cameras(cfg, 0, all_cams)
    load(pt, cfg)
    first = 0
    for n in sizes:
        cams = all_cams[first:first + n].copy()
        pt.render_cameras(first, cams)
        cams.fill(np.nan)
        first += n
    got = pt.read_accum()
    assert np.isfinite(got).all()
    same(got, ref, "four calls in flight")


# ---- 7. shards ----------------------------------------------------------------------------------
def test_shards_render_their_rows_only(pt):
    cfg = scene("c1", 40, 24)
    cams = lens_cameras(cfg, 0, 3)
    ref = oracle_cameras(cfg, 0, cams)
    load(pt, cfg)
    y = np.arange(24)
    done = np.zeros(24, bool)
    for shard in range(3):
        pt.render_cameras(0, cams, 4, 3, shard)
        got = pt.read_accum()
        done |= (y // 4) % 3 == shard
        same(got[done], ref[done], f"rows of shards 0..{shard}")
        assert not got[~done].any(), f"shard {shard} touched another shard's rows"
    assert done.all()
    # a shard without rows queues nothing
    before = pt.read_accum()
    pt.render_cameras(3, cams, 24, 3, 1)
    same(pt.read_accum(), before, "a shard without rows")


# ---- 8. scene kinds -----------------------------------------------------------------------------
def with_nodes(cfg, nodes, name=None):
    return dataclasses.replace(cfg, name=name or cfg.name,
                               packed=dataclasses.replace(cfg.packed, nodes=np.ascontiguousarray(nodes, np.float32)))


def tri_boxes(packed):
    """(nt, 2, 3) float32: min and max corner of every triangle's vertex box."""
    idx = packed.triangles[:, 0:3].astype(np.int64)
    P = packed.vertices[idx, 0:3]
    return np.stack([P.min(axis=1), P.max(axis=1)], axis=1).astype(np.float32)


def chain_nodes(packed, depth, axis=0):
    """A chain of `depth` interior nodes over the triangles in array order: node 2i is
    interior over [i, nt), its left child 2i + 1 the leaf [i, i + 1), its right child node
    2i + 2; the last node is the leaf [depth, nt).  Every box is its triangles' union."""
    tb = tri_boxes(packed)
    nt = len(tb)
    assert 1 <= depth < nt

    def box(a, b):
        return np.concatenate([tb[a:b, 0].min(axis=0), tb[a:b, 1].max(axis=0)])

    nd = np.zeros((2 * depth + 1, 12), np.float32)
    for i in range(depth):
        nd[2 * i, 0:6], nd[2 * i, 6:10] = box(i, nt), (axis, 2 * i + 2, i, nt)
        nd[2 * i + 1, 0:6], nd[2 * i + 1, 6:10] = box(i, i + 1), (0, -1, i, i + 1)
    nd[2 * depth, 0:6], nd[2 * depth, 6:10] = box(depth, nt), (0, -1, depth, nt)
    return nd


def root_leaf_scene(W, Hh):
    """An emissive quad facing the camera under a one-node tree, with an environment."""
    sb = H.SceneBuilder()
    sb.add_model(H.mesh_quad(27.5), [H.translate(0.2, 2.8, 0.0), H.rotate(90.0, 1, 0, 0), H.scale(0.04)],
                 H.Material(baseColor=(0.7, 0.6, 0.5), emssive=(5.0, 4.0, 3.0)), "quad")
    rgb = H.synthetic_hdr(16, 8, 11)
    cfg = S.SceneConfig("rootleaf-quad", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1, max_depth=4, env_rgb=rgb,
                        env_table=H.hdr_table(rgb))
    if len(cfg.packed.nodes) != 1:
        tb = tri_boxes(cfg.packed)
        nd = np.zeros((1, 12), np.float32)
        nd[0, 0:6] = np.concatenate([tb[:, 0].min(axis=0), tb[:, 1].max(axis=0)])
        nd[0, 6:10] = (0, -1, 0, len(tb))
        cfg = with_nodes(cfg, nd)
    assert len(cfg.packed.nodes) == 1 and cfg.packed.nodes[0, 7] == -1
    return cfg


def leaf200_scene(W, Hh):
    """189 loose triangles (one model, added first) in the Cornell box under a hand-made tree:
    root -> leaf [0, 1), leaf [1, 201): 200 triangles, past the 127 a leaf ref holds inline."""
    rng = np.random.default_rng(200)
    sb = H.SceneBuilder()
    P = (rng.uniform(-1.8, 1.8, (189, 1, 3)) + rng.normal(0.0, 0.35, (189, 3, 3)) + np.array([0.0, 2.6, 0.0])).astype(np.float32)
    sb.add_model(H.Mesh(P.reshape(-1, 3), None, None, np.arange(567, dtype=np.int32)), [H.scale(1.0)],
                 H.Material(baseColor=(0.3, 0.5, 0.8), roughness=0.4), "loose")
    S._cornell_walls(sb, H.Material(baseColor=(0.65, 0.65, 0.65)))
    cfg = S.SceneConfig("leaf200", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1, max_depth=4)
    assert len(cfg.packed.triangles) == 201
    return with_nodes(cfg, chain_nodes(cfg.packed, 1))


def fan_chain_scene(W, Hh, depth):
    """Cornell walls + a fan of 70 large overlapping triangles, the fan first in the
    triangle array, under a chain of `depth` interior nodes."""
    rng = np.random.default_rng(70)
    sb = H.SceneBuilder()
    S._cornell_walls(sb, H.Material(baseColor=(0.65, 0.65, 0.65)))
    base = np.array([[-2.0, 0.3, 0.0], [2.0, 0.5, 0.0], [0.0, 4.8, 0.0]])
    for k in range(70):
        P = base + np.array([0.0, 0.0, -2.0 + 4.0 * k / 70]) + rng.normal(0.0, 0.05, (3, 3))
        sb.add_model(H.Mesh(P.astype(np.float32), None, None, np.arange(3, dtype=np.int32)), [H.scale(1.0)],
                     H.Material(baseColor=tuple(rng.uniform(0, 1, 3)), roughness=float(rng.uniform(0, 1))), f"fan{k}")
    built = S.SceneConfig("fan", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1, max_depth=4)
    p = built.packed
    mat = p.triangles[:, 3].astype(np.int64)
    fan = np.flatnonzero(mat >= 6)
    assert len(fan) == 70
    perm = np.concatenate([fan[np.argsort(mat[fan], kind="stable")], np.flatnonzero(mat < 6)])
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    lights = p.lights.copy()
    lights[:, 0] = inv[lights[:, 0].astype(np.int64)]
    packed = dataclasses.replace(p, triangles=np.ascontiguousarray(p.triangles[perm]), lights=lights)
    cfg = dataclasses.replace(built, packed=packed)
    return with_nodes(cfg, chain_nodes(packed, depth), f"fan-chain-{depth}")


@pytest.mark.parametrize("kind", ["root-leaf", "leaf200", "chain"])
def test_scene_kinds(pt, kind):
    W, Hh = 16, 8
    if kind == "root-leaf":
        cfg, want = root_leaf_scene(W, Hh), {"root_is_leaf": 1, "n_interior": 0}
    elif kind == "leaf200":
        cfg, want = leaf200_scene(W, Hh), {"has_leaf_table": 1, "n_interior": 1}
    else:
        pt.upload_scene(scene("c1", W, Hh).packed)
        D = pt.device_info()["stack_limit"] - 2
        cfg, want = fan_chain_scene(W, Hh, D), {"max_depth": D, "n_interior": D}
    cams = lens_cameras(cfg, 0, 3, radius=0.1)
    ref = oracle_cameras(cfg, 0, cams)
    assert ref[..., :3].any()
    for mode in MODES:
        load(pt, cfg, mode)
        info = pt.device_info()
        assert {k: info[k] for k in want} == want
        pt.render_cameras(0, cams)
        same(pt.read_accum(), ref, f"{cfg.name} mode {mode}")


# ---- 9. moments ---------------------------------------------------------------------------------
def test_moments_follow_the_frames_colours(pt):
    """Frames 0, 1, 3, 7: the blend weights are powers of two, so one oracle frame rendered
    into a zeroed image is colour * a exactly and the colour is recovered exactly
    (moments_common.anchor's argument; the replay below asserts the premise)."""
    cfg = scene("c2", 40, 24)
    frames = (0, 1, 3, 7)
    cams = {f: lens_cameras(cfg, f, 1)[0] for f in frames}
    orc = pyoracle.Oracle(cfg)
    colors = []
    for f in frames:
        img = oracle_cameras(cfg, f, cams[f][None], orc=orc)
        rgb = img[..., :3]
        assert not ((rgb != 0) & (np.abs(rgb) < np.finfo(F).tiny)).any()
        colors.append((rgb * F(f + 1)).astype(F))
    acc = np.zeros((24, 40, 4), F)
    for f in frames:
        oracle_cameras(cfg, f, cams[f][None], acc=acc, orc=orc)
    assert np.array_equal(bits(MR.blend(np.zeros((24, 40, 4), F), colors, frames)[..., :3]), bits(acc[..., :3]))
    mom = MR.update(MR.zeros(24, 40), colors, frames)
    load(pt, cfg)
    pt.enable_moments(True)
    pt.reset_accum()
    pt.render_cameras(0, np.stack([cams[0], cams[1]]))
    pt.render_cameras(3, cams[3][None])
    pt.render_cameras(7, cams[7][None])
    same(pt.read_accum(), acc, "accumulation with moments enabled")
    assert np.array_equal(bits(pt.read_moments()), bits(mom))
    # the moments cover the accumulation: an adaptive call is accepted
    st = pt.render_adaptive(8, 1, 0.0, 0xFFFFFFFF)
    assert st["n_active_pixels"] == 40 * 24
    # ... and frames rendered here without the moments break the cover, as pnrt_render's do
    pt.enable_moments(False)
    pt.render_cameras(9, cams[0][None])
    pt.enable_moments(True)
    with pytest.raises(PnrtError) as e:
        pt.render_adaptive(10, 1, 0.0, 2)
    assert e.value.code == -3
    pt.enable_moments(False)


# ---- 10. pnrt_render and the guides afterwards ------------------------------------------------------
def test_render_and_guides_keep_the_pinhole_records(pt):
    cfg = scene("c2", 40, 24)
    cams = lens_cameras(cfg, 2, 3)
    pin = np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (2, 1))
    orc = pyoracle.Oracle(cfg)
    ref = oracle_cameras(cfg, 0, pin, orc=orc)
    oracle_cameras(cfg, 2, cams, acc=ref, orc=orc)
    oracle_cameras(cfg, 5, pin, acc=ref, orc=orc)
    load(pt, cfg)
    pt.profile_enable(True)
    pt.render(0, 2)
    pt.synchronize()
    pt.render_guides()
    guides = [pt.read_aov(k) for k in ("position", "normal", "albedo")]
    n0 = pt.profile_read()["primary"][1]
    pt.render_cameras(2, cams)
    pt.synchronize()
    n1 = pt.profile_read()["primary"][1]
    pt.render(5, 2)                                  # its kept per-pixel records: no camera-ray launch
    got = pt.read_accum()
    n2 = pt.profile_read()["primary"][1]
    pt.profile_enable(False)
    same(got, ref, "render, render_cameras, render")
    assert (n1 - n0, n2 - n1) == (1, 0), (n0, n1, n2)
    pt.render_guides()
    for k, g in zip(("position", "normal", "albedo"), guides):
        assert np.array_equal(bits(pt.read_aov(k)), bits(g)), k


# ---- 11. refusals -------------------------------------------------------------------------------
def test_refusals_leave_the_accumulation(pt):
    cfg = scene("c1", 16, 8)
    cams = lens_cameras(cfg, 0, 4)
    with PathTracer(0) as fresh:
        for step in ("nothing", "scene only"):
            with pytest.raises(PnrtError) as e:
                fresh.render_cameras(0, cams)
            assert e.value.code == -3, step          # PNRT_E_STATE
            fresh.upload_scene(cfg.packed)
    load(pt, cfg)
    pt.render_cameras(0, cams)
    before = pt.read_accum()
    assert before[..., :3].any()

    def refused(code, *args, needle=None):
        with pytest.raises(PnrtError) as e:
            pt.render_cameras(*args)
        assert e.value.code == code, str(e.value)
        if needle:
            assert needle in str(e.value), str(e.value)
        same(pt.read_accum(), before, f"after the refusal of {args[2:]}")

    for sel in ((0, 1, 0), (1, 0, 0), (1, 2, 2), (1, 2, -1)):
        refused(-1, 4, cams, *sel)
    refused(-1, 0xFFFFFFFF - 3, cams)                # first + 4 = 2^32 > 0xFFFFFFFF
    for i in (0, 17, 47):
        for v in (np.nan, np.inf, -np.inf):
            bad = cams.copy()
            bad.reshape(-1)[i] = v
            refused(-1, 5, bad, needle=f"frame {5 + i // 12}")
    # cameras == NULL with n_frames > 0: only through the C entry point
    import ctypes
    rc = pt._lib.pnrt_render_cameras(pt._ctx, 4, 2, None, 1, 1, 0)
    assert rc == -1
    same(pt.read_accum(), before, "after cameras == NULL")
    # n_frames == 0 queues nothing, with or without an array
    assert pt._lib.pnrt_render_cameras(pt._ctx, 4, 0, None, 1, 1, 0) == 0
    pt.render_cameras(4, np.zeros((0, 12), F))
    same(pt.read_accum(), before, "after n_frames == 0")
    # PNRT_KERNEL_V1 renders the pnrt_set_frame camera only
    pt.set_options(TRAVERSE_ZCULL | KERNEL_V1)
    refused(-3, 4, cams)
    pt.set_options(TRAVERSE_ZCULL)
    del ctypes
    # the Python layer's own checks
    for bad in (cams.astype(np.float64), cams.reshape(-1), cams[:, :11], np.zeros((2, 3, 4), F)):
        with pytest.raises(ValueError):
            pt.render_cameras(4, bad)
    with pytest.raises(ValueError):
        pt.render_cameras(2 ** 32, cams)
    same(pt.read_accum(), before, "after the Python layer's refusals")


# ---- 12. the interactive session ----------------------------------------------------------------
def run_session(pt, cfg, lens):
    """still, still, drag, drag, still, still, still: the accumulation after every frame
    against the oracle replayed with the same cameras."""
    W, Hh = cfg.width, cfg.height
    cam = CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, F(W) / F(Hh))
    orc = pyoracle.Oracle(cfg)
    acc = np.zeros((Hh, W, 4), F)
    load(pt, cfg)
    sess = InteractiveSession(pt, W, Hh, cam)
    focus = None
    if lens:
        assert sess.focus_on(W // 2, Hh // 3)
        rec = sess.pick(W // 2, Hh // 3)
        s = cam.state
        focus = float(np.dot(np.asarray(rec["position"], np.float64) - np.array(list(s.eye), np.float64),
                             -np.array(list(s.w), np.float64)))
        assert 1.0 < focus < 20.0
        sess.set_lens(aa_width=1.0, lens_radius=0.08)            # keeps focus_on's distance
        assert sess._lens == (1.0, 0.08, focus)
    for step, redraw in enumerate([False, False, True, True, False, False, False]):
        if redraw:
            cam.rotate(3.0, -1.0)
        fc_before = sess.frame_count
        depth, _ = sess.frame(redraw)
        u = cam.uniforms()
        if redraw or not lens:
            cams, fc = u.reshape(1, 12), 0 if redraw else fc_before
        else:
            cams, fc = H.camera_sequence(u, W, Hh, fc_before, 1, 1.0, 0.08, focus), fc_before
            assert not np.array_equal(bits(cams), bits(u.reshape(1, 12)))
        oracle_cameras(cfg, fc, cams, depth, acc=acc, orc=orc)
        same(pt.read_accum(), acc, f"frame {step} (redraw={redraw}, lens={lens})")
    assert sess.frame_count == 3
    if lens:                                          # frame_counted goes through render_cameras too
        st = sess.frame_counted(2)
        assert st["n_active_pixels"] == W * Hh and sess.frame_count == 5
        oracle_cameras(cfg, 3, H.camera_sequence(cam.uniforms(), W, Hh, 3, 2, 1.0, 0.08, focus), acc=acc, orc=orc)
        same(pt.read_accum(), acc, "frame_counted with a lens")
        pt.enable_moments(False)
    return acc


def test_session_with_and_without_a_lens(pt):
    cfg = scene("c2", 40, 24)
    plain = run_session(pt, cfg, False).copy()
    lens = run_session(pt, cfg, True)
    assert n_differ(plain, lens) > 40 * 24 // 2


def test_focus_on_a_miss_changes_nothing(pt):
    cfg = scene("c2wide", 48, 32)
    load(pt, cfg)
    cam = CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 100.0, F(48) / F(32))
    sess = InteractiveSession(pt, 48, 32, cam)
    assert not sess.pick(0, 0)["hit"]
    assert sess.focus_on(0, 0) is False and sess._lens is None
    sess.set_lens(0.5, 0.0)
    assert sess.focus_on(0, 0) is False and sess._lens == (0.5, 0.0, None)
    with pytest.raises(ValueError):
        sess.set_lens(1.0, 0.1)                      # a lens without a focus distance


# ---- the compiled C caller ----------------------------------------------------------------------
def test_compiled_c_caller_renders_like_python(pt, tmp_path):
    assert os.path.exists(EXE), "tests/abi/c_abi_cameras not built (python -c 'import __graft_entry__ as g; g.build()')"
    src = open(os.path.join(HERE, "abi", "c_abi_cameras.c")).read()
    assert "_Static_assert(sizeof(pnrt_lens_params) == 16" in src
    cfg = scene("c2", 40, 24)
    path, out = str(tmp_path / "s.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    r = subprocess.run([EXE, path, "3", "5", "1.0", "0.125", "6.5", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("expected error:") == 3 and "reserved" in r.stdout and "frame 7" in r.stdout
    load(pt, cfg)
    plan, plain = pt.cameras_batch_plan(5), pt.batch_plan(5)
    assert r.stdout.split("plan")[1].split()[:4] == [str(v) for v in (plan["frames_per_batch"], plan["n_batches"],
                                                                     plan["batch_bytes"], plain["batch_bytes"])]
    pt.render_cameras(3, H.camera_sequence(cfg.camera, 40, 24, 3, 5, 1.0, 0.125, 6.5))
    same(np.fromfile(out, F).reshape(24, 40, 4), pt.read_accum(), "the C caller's image")


# ---- every index checked ------------------------------------------------------------------------
def test_sequence_on_bounds_checked_library():
    """Partial tiles, misses, the three scene kinds and a two-batch call on the `bounds`
    diagnostic library: every fetch and store index of the camera-ray, gen, trace and shade
    kernels is checked against its array, and a violation is an error (PNRT_E_TRACE)."""
    from pnraytracing_amd import build
    lib = build.variant_path("bounds")
    assert os.path.exists(lib), "variants/libpnrt_bounds.so not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(HERE, "cameras_worker.py")], env=dict(os.environ, PNRT_DEVICE_LIB=lib),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CAMERAS-WORKER-DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIAGNOSTIC BUILD" in r.stdout and r.stdout.count(": ok") == 12
