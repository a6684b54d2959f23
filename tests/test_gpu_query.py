"""Ray queries (pnrt_query_rays, pt_query.h) against the CPU oracle's intersection
routines, record by record, bit for bit (tolerance 0: both sides evaluate the same
IEEE operations) -- over every ray, nothing sampled or left out.

The truth is pyoracle.Oracle(cfg).intersect(rays, kind, 0): BVHIntersect /
BVHIntersectP under the GLSL's rules, which tests/test_isect_pin.py pins to the
reference's own CPU code on the ray families of tests/isect_rays.py.  Those very
families go through the GPU's traversal step here, which closes the chain GPU =
oracle = reference CPU code on the traversal itself.

Words 0-12 of a record are the oracle's; word 13 (the accepted triangle) is checked by
intersecting that one triangle (oracle kind 2), words 14-15 as pnrt.h states them.
"""
import functools
import types

import numpy as np
import pytest

import isect_rays
import pyoracle
from guides_common import bits, camera_rays, scene
from pnraytracing_amd.session import InteractiveSession
from pnraytracing_amd.tracer import TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer, PnrtError, decode_hits

pytestmark = pytest.mark.gpu
F = np.float32
MODES = (TRAVERSE_ZCULL, TRAVERSE_EXACT)
W, Hh = 67, 45
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def prepare(pt, cfg, mode):
    """A query needs the scene and the traversal mode only (no set_frame)."""
    pt.upload_scene(cfg.packed)
    pt.set_options(mode)


def oracle(cfg, rays, any_hit):
    return pyoracle.Oracle(cfg).intersect(rays, 1 if any_hit else 0, 0)


def check(rec, ref, rays, any_hit, what):
    """Words 0-12 are the oracle's; 13 is -1 exactly without a hit; 14, 15 are zero."""
    assert rec.shape == (len(rays), 16) and rec.dtype == np.uint32
    bad = np.flatnonzero(np.any(rec[:, :13] != ref, axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(rays)} records differ, first {bad[:5].tolist()}: ray " \
                          f"{rays[bad[0]].tolist()} gpu {rec[bad[0]].tolist()} oracle {ref[bad[0]].tolist()}"
    assert np.array_equal(rec[:, 13] == NONE, rec[:, 0] == 0), what
    assert not rec[:, 14:].any(), what
    if any_hit:
        assert not rec[:, 1:12].any(), what


def check_triangles(cfg, rays, rec, what):
    """The closest-hit records' triangle index names the accepted triangle in the caller's
    order: that triangle alone, at the ray's original tMax, reproduces words 0-11."""
    hit = rec[:, 0] != 0
    tri = rec[hit, 13].view(np.int32)
    assert ((tri >= 0) & (tri < len(cfg.packed.triangles))).all(), what
    one = pyoracle.Oracle(cfg).intersect(rays[hit], 2, 0, tri)
    assert np.array_equal(one[:, :12], rec[hit, :12]), what


def both_kinds_both_modes(pt, cfg, rays, what):
    """Every mode and kind against the oracle; returns the closest-hit records."""
    ref = {any_hit: oracle(cfg, rays, any_hit) for any_hit in (False, True)}
    first = {}
    for mode in MODES:
        prepare(pt, cfg, mode)
        for any_hit in (False, True):
            rec = pt.query_rays(rays, any_hit)
            check(rec, ref[any_hit], rays, any_hit, f"{what} mode {mode} any_hit {any_hit}")
            if any_hit in first:                      # the two modes' records equal each other, word for word
                assert np.array_equal(rec, first[any_hit]), f"{what} any_hit {any_hit}: the modes differ"
            first.setdefault(any_hit, rec)
    check_triangles(cfg, rays, first[False], what)
    # an any-hit ray is occluded iff it has a closest hit, and the triangle that ended it is one the ray hits
    assert np.array_equal(first[True][:, 0], first[False][:, 0]), what
    hit = first[True][:, 0] != 0
    one = pyoracle.Oracle(cfg).intersect(rays[hit], 3, 0, first[True][hit, 13].view(np.int32))
    assert (one[:, 0] == 1).all(), what
    return first[False]


# ---- the pinned ray families ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family_rays(name):
    cfg = scene(name, W, Hh)
    return np.concatenate([isect_rays.make_rays(cfg.packed, cfg.camera, fam, 4096, 7) for fam in isect_rays.FAMILIES])


@pytest.mark.parametrize("name", ["c1", "c2", "c3"])
def test_families_bitwise(pt, name):
    cfg, rays = scene(name, W, Hh), family_rays(name)
    assert rays.shape == (7 * 4096, 7)
    rec = both_kinds_both_modes(pt, cfg, rays, name)
    per_family = (rec[:, 0] != 0).reshape(7, 4096).sum(axis=1)
    assert (per_family > 0).all() and (per_family < 4096).any(), per_family       # hits in every family, and misses


def far_rays(cfg, n, seed):
    """Origins at log-uniform distances 1e3 .. 1e8 from the scene centre -- both sides of
    make_ray's 1e6 culling switch --, aimed at random points of the scene's box, half of the
    directions normalised; tMax from values on both sides of every comparison."""
    rng = np.random.default_rng(seed)
    lo, hi = cfg.packed.nodes[0, 0:3].astype(F), cfg.packed.nodes[0, 3:6].astype(F)
    c = ((lo + hi) * F(0.5)).astype(F)
    dist = (10.0 ** rng.uniform(3.0, 8.0, n)).astype(F)
    o = (c + isect_rays._unit(rng, n) * dist[:, None]).astype(F)
    tgt = (lo + rng.random((n, 3)).astype(F) * (hi - lo)).astype(F)
    d = (tgt - o).astype(F)
    norm = rng.random(n) < 0.5
    d[norm] = (d[norm] / np.sqrt((d[norm] * d[norm]).sum(1, dtype=F))[:, None]).astype(F)
    rays = np.zeros((n, 7), F)
    rays[:, 0:3], rays[:, 3:6] = o, d
    rays[:, 6] = rng.choice(np.array([0.0, -1.0, 1e-30, 1.0 - 1e-4, 1e7, 3.4e38], F), n)
    assert np.isfinite(rays).all() and (np.abs(o).max(axis=1) < 1e6).any() and (np.abs(o).max(axis=1) >= 1e6).any()
    return rays


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_far_family_bitwise(pt, name):
    cfg = scene(name, W, Hh)
    rays = far_rays(cfg, 4096, 11)
    rec = both_kinds_both_modes(pt, cfg, rays, f"{name} far")
    assert 0 < (rec[:, 0] != 0).sum() < len(rays)


# ---- trees at the limits ---------------------------------------------------------------------------
def limit_rays(cfg, n=512):
    return np.concatenate([camera_rays(cfg)] + [isect_rays.make_rays(cfg.packed, cfg.camera, fam, n, 3)
                                                for fam in ("camera", "shadow", "axis", "wide")])


def test_root_leaf_of_130_tied_triangles_last_one_wins(pt):
    """The leaf-table instantiation; the 130 triangles coincide, so every hit is a 130-way
    tie.  Under the `>` rule a later triangle at an equal distance wins: the winner is the
    LAST triangle wherever the tie is exact in float32 -- after the first acceptance tMax =
    tScaled * (1 / det), and the next copy is accepted iff tScaled <= tMax * det, which
    rounding makes false for a few rays, where triangle 0 then keeps the hit.  The expected
    index is the oracle's own: its one-triangle test applied to the leaf's triangles in
    order, each at the tMax the one before left.  An any-hit ray ends at the first."""
    from test_gpu_limits import root_leaf_scene
    cfg = root_leaf_scene("coincident130", 9, 8, False)
    rays = limit_rays(cfg)
    prepare(pt, cfg, TRAVERSE_ZCULL)
    assert pt.device_info()["has_leaf_table"] == 1 and pt.device_info()["root_is_leaf"] == 1
    rec = both_kinds_both_modes(pt, cfg, rays, cfg.name)
    hit = rec[:, 0] != 0
    o, r, win = pyoracle.Oracle(cfg), rays.copy(), np.full(len(rays), -1, np.int32)
    for k in range(130):
        one = o.intersect(r, 2, 0, np.full(len(r), k, np.int32))
        win[one[:, 0] != 0] = k
        r[:, 6] = one[:, 12].view(F)
    assert np.array_equal(rec[:, 13].view(np.int32), win)
    assert hit.any() and set(win[hit]) <= {0, 129} and (win[hit] == 129).sum() > hit.sum() // 2
    assert (pt.query_rays(rays, any_hit=True)[hit, 13] == 0).all()


def test_root_leaf_of_one_triangle(pt):
    from test_gpu_limits import root_leaf_scene
    cfg = root_leaf_scene("triangle", 9, 8, False)
    rec = both_kinds_both_modes(pt, cfg, limit_rays(cfg), cfg.name)
    assert pt.device_info()["has_leaf_table"] == 0 and pt.device_info()["root_is_leaf"] == 1
    assert (rec[rec[:, 0] != 0, 13] == 0).all() and (rec[:, 0] != 0).any()


def test_empty_leaf(pt):
    from test_gpu_limits import empty_leaf_c1
    cfg, plain = empty_leaf_c1()
    rays = limit_rays(cfg)
    rec = both_kinds_both_modes(pt, cfg, rays, cfg.name)
    assert np.array_equal(rec[:, :13], oracle(plain, rays, False))


def test_chain_at_the_stack_limit_uses_the_spill_area(pt):
    from test_gpu_limits import FAN_ROT, PT_STACK, chain_config
    cfg = chain_config("leafleft", 0, FAN_ROT)
    rays = limit_rays(cfg)
    both_kinds_both_modes(pt, cfg, rays, cfg.name)
    info = pt.device_info()
    assert info["max_depth"] == PT_STACK - 2 == info["stack_limit"] - 2


def test_queries_on_the_bounds_checked_library():
    """The families, the limit trees and invalid rays on the `bounds` diagnostic library:
    every index of the query kernel checked against its array (a violation is an error)."""
    import os
    import subprocess
    import sys
    from pnraytracing_amd import build
    lib = build.variant_path("bounds")
    assert os.path.exists(lib), "variants/libpnrt_bounds.so not built (__graft_entry__.build())"
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "query_worker.py")], env=dict(os.environ, PNRT_DEVICE_LIB=lib),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "QUERY-WORKER-DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIAGNOSTIC BUILD" in r.stdout and r.stdout.count(": ok") == 4


# ---- chunk edges -----------------------------------------------------------------------------------
def test_chunk_edges(pt):
    cfg = scene("c2", W, Hh)
    rays = family_rays("c2").reshape(7, 4096, 7)[:, :40].reshape(-1, 7)       # 280 rays, 40 of every family
    ref = {a: oracle(cfg, rays, a) for a in (False, True)}
    prepare(pt, cfg, TRAVERSE_ZCULL)
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        for any_hit in (False, True):
            rec = pt.query_rays(rays[:n], any_hit)
            check(rec, ref[any_hit][:n], rays[:n], any_hit, f"n = {n} any_hit {any_hit}")


def test_more_than_one_grid_sweep(pt):
    """2^20 + 257 rays: more blocks than the grid holds, a partial last block and wave."""
    cfg = scene("c2", W, Hh)
    n = (1 << 20) + 257
    rays = np.concatenate([isect_rays.make_rays(cfg.packed, cfg.camera, "camera", n // 2, 5),
                           isect_rays.make_rays(cfg.packed, cfg.camera, "wide", n - n // 2, 5)])
    prepare(pt, cfg, TRAVERSE_ZCULL)
    rec = pt.query_rays(rays)
    check(rec, oracle(cfg, rays, False), rays, False, "2^20 + 257 rays")


# ---- the guide images are the camera rays' records --------------------------------------------------
@pytest.mark.parametrize("name", ["c3", "c2wide"])
def test_camera_rays_equal_the_guide_images(pt, name):
    cfg = scene(name, W, Hh)
    pt.load(cfg)
    pt.render_guides()
    pos, nrm, alb = (pt.read_aov(k).reshape(-1, 4) for k in ("position", "normal", "albedo"))
    rays = camera_rays(cfg)
    rec = pt.query_rays(rays)
    check(rec, oracle(cfg, rays, False), rays, False, name)
    d = decode_hits(rec)
    hit = d["hit"]
    assert np.array_equal(hit, pos[:, 3] == 1.0) and np.array_equal(~hit, pos[:, 3] == 0.0)      # misses agree
    if name == "c2wide":
        assert (~hit).any()
    assert hit.any()
    assert np.array_equal(bits(d["position"][hit]), bits(pos[hit, :3]))
    assert np.array_equal(bits(d["normal"][hit]), bits(nrm[hit, :3]))
    assert np.array_equal(d["material_id"][hit].astype(F), nrm[hit, 3])
    assert np.array_equal(d["texture_id"][hit].astype(F), alb[hit, 3])
    if name == "c3":
        assert (d["texture_id"][hit] >= 0).any()
    assert (nrm[~hit, 3] == -1.0).all()
    s = InteractiveSession(pt, W, Hh, types.SimpleNamespace(uniforms=lambda: cfg.camera))
    some_hit = int(np.flatnonzero(hit)[len(np.flatnonzero(hit)) // 2])
    for i in (0, W * Hh - 1, some_hit):
        got = s.pick(i % W, i // W)
        for k, v in d.items():
            assert np.asarray(got[k]).tobytes() == np.asarray(v[i]).tobytes(), (i, k)
    assert s.pick(some_hit % W, some_hit // W)["material_id"] == int(nrm[some_hit, 3])


# ---- invalid rays -------------------------------------------------------------------------------------
def test_invalid_rays_are_flagged_and_not_traced(pt):
    """One wave: four invalid rays between valid ones.  Their records are the specified
    ones (nothing is traversed for them), their neighbours' the oracle's."""
    cfg = scene("c2", W, Hh)
    good = family_rays("c2").reshape(7, 4096, 7)[6, :64].copy()          # the wide family
    rays = good.copy()
    rays[3, 1] = np.nan                         # a NaN origin
    rays[17, 4] = np.inf                        # an infinite direction
    rays[30, 6] = np.inf                        # an infinite tMax
    rays[31, 3:6] = (0.0, -0.0, 0.0)            # no direction (either sign of zero)
    rays[63, 0] = -np.inf
    invalid = np.zeros(64, bool)
    invalid[[3, 17, 30, 31, 63]] = True
    prepare(pt, cfg, TRAVERSE_ZCULL)
    for any_hit in (False, True):
        rec = pt.query_rays(rays, any_hit)
        want = np.zeros(16, np.uint32)
        want[13], want[14] = NONE, 1
        assert (rec[invalid] == want).all(), rec[invalid]
        check(rec[~invalid], oracle(cfg, good, any_hit)[~invalid], good[~invalid], any_hit, f"neighbours any_hit {any_hit}")
        d = decode_hits(rec)
        assert np.array_equal(d["invalid"], invalid) and not d["hit"][invalid].any()
    # zero components and one-zero directions are rays like any other
    ok = good.copy()
    ok[:, 3], ok[::2, 4] = 0.0, -0.0
    ok[ok[:, 5] == 0, 5] = 1.0
    check(pt.query_rays(ok), oracle(cfg, ok, False), ok, False, "zero direction components")


# ---- a query changes nothing ------------------------------------------------------------------------
def test_query_leaves_the_images_alone_and_follows_the_scene(pt):
    cfg = scene("c2", W, Hh)
    rays = family_rays("c2")[::16]
    ref = oracle(cfg, rays, False)
    pt.load(cfg)
    pt.reset_accum()
    pt.render(0, 6)
    want = pt.read_accum()
    pt.render_guides()
    pt.reset_accum()
    pt.render(0, 3)
    check(pt.query_rays(rays), ref, rays, False, "between two render calls")
    check(pt.query_rays(rays, True), oracle(cfg, rays, True), rays, True, "between two render calls")
    pt.render(3, 3)
    assert np.array_equal(bits(pt.read_accum()), bits(want)), "3 frames, a query, 3 frames != 6 frames"
    pt.denoise()                                # the guide images are not stale: no PNRT_E_STATE
    pt.synchronize()
    # materials: the geometry a query sees does not depend on them
    mats = cfg.packed.materials.copy()
    mats[:, 3:6] = 0.25
    pt.update_materials(0, mats)
    check(pt.query_rays(rays), ref, rays, False, "after update_materials")
    # a new scene: the next query sees it
    other = scene("c1", W, Hh)
    pt.upload_scene(other.packed)
    rec = pt.query_rays(rays)
    check(rec, oracle(other, rays, False), rays, False, "after a second upload_scene")
    assert not np.array_equal(rec[:, :13], ref)


# ---- the device form -----------------------------------------------------------------------------------
def test_device_form_equals_host_form(pt):
    import torch
    cfg = scene("c3", W, Hh)
    rays = family_rays("c3")[: 4096 + 77]
    prepare(pt, cfg, TRAVERSE_ZCULL)
    stream = torch.cuda.ExternalStream(pt.stream_handle())
    for any_hit in (False, True):
        host = pt.query_rays(rays, any_hit)
        with torch.cuda.stream(stream):
            r = torch.from_numpy(rays).to("cuda")
            out = torch.full((len(rays), 16), -7, dtype=torch.int32, device="cuda")
            pt.query_rays_device(r.data_ptr(), len(rays), out.data_ptr(), any_hit)
            got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, host), f"any_hit {any_hit}"
    with torch.cuda.stream(stream):
        with pytest.raises(PnrtError, match=r"\(-1\)"):          # records not 16-byte aligned
            pt.query_rays_device(r.data_ptr(), 8, out.data_ptr() + 4)
        stream.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == got).all()


# ---- errors ---------------------------------------------------------------------------------------------
def test_errors_queue_nothing():
    import ctypes
    from pnraytracing_amd import _native as N
    cfg = scene("c1", W, Hh)
    rays = family_rays("c1")[:100].copy()
    out = np.full((100, 16), 0xABABABAB, np.uint32)
    rp, op = N.fptr(rays), out.ctypes.data_as(ctypes.POINTER(N.Hit))
    with PathTracer(0) as t:
        lib, ctx = t._lib, t._ctx
        t.profile_enable()
        with pytest.raises(PnrtError, match=r"\(-3\).*upload_scene first") as e:         # PNRT_E_STATE
            t.query_rays(rays)
        assert e.value.code == -3
        with pytest.raises(PnrtError, match=r"\(-3\)"):
            t.query_rays_device(16, 1, 16)
        t.upload_scene(cfg.packed)
        assert lib.pnrt_query_rays(ctx, rp, 100, 2, op) == -1                             # PNRT_E_ARG: kind
        assert lib.pnrt_query_rays(ctx, rp, 100, -1, op) == -1
        assert lib.pnrt_query_rays(ctx, rp, -1, 0, op) == -1                              # n < 0
        assert lib.pnrt_query_rays(ctx, None, 100, 0, op) == -1                           # NULL with n > 0
        assert lib.pnrt_query_rays(ctx, rp, 100, 0, None) == -1
        assert lib.pnrt_query_rays_device(ctx, None, 100, 0, None) == -1
        assert lib.pnrt_query_rays_device(ctx, None, -5, 1, None) == -1
        assert lib.pnrt_query_rays_device(ctx, None, 5, 3, None) == -1
        assert lib.pnrt_query_rays(ctx, None, 0, 0, None) == 0                            # n == 0: PNRT_OK, nothing queued
        assert lib.pnrt_query_rays_device(ctx, None, 0, 1, None) == 0
        assert t.query_rays(rays[:0]).shape == (0, 16)
        assert (out == 0xABABABAB).all()
        assert t.profile_read()["primary"][1] == 0, "a refused or empty query launched a kernel"
        assert lib.pnrt_query_rays(ctx, rp, 100, 0, op) == 0
        check(out, oracle(cfg, rays, False), rays, False, "after the refused calls")
        assert t.profile_read()["primary"][1] == 1                                        # timed as PNRT_K_PRIMARY
