"""Temporal reprojection (pnrt_reproject, pt_reproject.h) against tests/reproject_ref.py,
the numpy restatement of DESIGN.md section 25, fed the GPU's own accumulation, moments and
guide images; the statistics against the CPU replay's table; continuation, what the call
leaves alone, and every refusal of the contract.

Tolerance: 0 ulp everywhere (uint32 views and integers compared)."""
import ctypes
import dataclasses
import math

import numpy as np
import pytest

import adaptive_ref as A
import moments_ref as R
import pyoracle
import reproject_common as C
import reproject_ref as RP
from guides_common import SHAPES, bits, scene
from pnraytracing_amd import _native as N
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_ZCULL, PathTracer, PnrtError
from test_reproject_ref import IDENTITY_BOUND

pytestmark = pytest.mark.gpu

F = np.float32
W, H = C.W, C.H
E_ARG, E_STATE = -1, -3
ALL = 0xFFFFFFFF                                     # min_frames: every pixel active
AOVS = ("position", "normal", "albedo")


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


def code_of(call, *a, **kw):
    with pytest.raises(PnrtError) as e:
        call(*a, **kw)
    return e.value.code


def guides(pt):
    return tuple(pt.read_aov(k) for k in AOVS)


def fresh_guides(name, cam, w, h):
    """The guide images of a context that did nothing but render them at `cam`."""
    cfg = scene(name, w, h)
    with PathTracer(0) as t:
        t.load(cfg)
        t.set_frame(w, h, cam, cfg.max_depth)
        t.render_guides()
        return guides(t)


def move_and_reproject(pt, name, move, w, h, guides_first, **params):
    """The anchor sequence at camera A, then set_frame(B) and reproject(A).  With
    guides_first the guide images of A are current when the call comes (their key matches
    `from`); without, the call renders them itself.  -> (stats, what reproject_ref makes
    of the GPU's own images: accumulation, moments, stats; the images before the call)."""
    cfg = scene(name, w, h)
    cam_a, cam_b = C.camera_a(name, w, h), C.camera_b(name, move, w, h)
    C.run_state(pt, name, w, h)
    acc, mom = pt.read_accum(), pt.read_moments()
    if guides_first:
        pt.render_guides()
        pos_a, nrm_a, _ = guides(pt)
    else:
        pos_a, nrm_a, _ = fresh_guides(name, cam_a, w, h)
    pt.set_frame(w, h, cam_b, cfg.max_depth)
    st = pt.reproject(cam_a, **params)
    pos_b, nrm_b, _ = guides(pt)
    want = RP.reproject(acc, mom, pos_a, nrm_a, pos_b, nrm_b, cam_a, w, h, params)
    return st, want, (acc, mom)


def check(pt, st, want, what):
    acc, mom, wst = want
    print(what, st)
    assert st == wst, what
    same(pt.read_accum(), acc, what + ": accumulation")
    same(pt.read_moments(), mom, what + ": moments")


# ---- 1. the replay cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,move", sorted(C.REPLAY))
def test_replay(pt, name, move):
    guides_first = move in ("rotate", "zoom")
    st, want, _ = move_and_reproject(pt, name, move, W, H, guides_first)
    assert C.stats_tuple(st) == C.REPLAY[(name, move)], "the statistics of the CPU replay"
    assert st["n_pixels"] == W * H
    check(pt, st, want, f"{name} {move}")
    after = guides(pt)
    for k, got, fresh in zip(AOVS, after, fresh_guides(name, C.camera_b(name, move, W, H), W, H)):
        same(got, fresh, f"{name} {move}: the {k} image is the one of a fresh render_guides at the new camera")
    # the GPU's images were the CPU replay's inputs and results
    same(pt.read_accum(), C.replay(name, move)[0], f"{name} {move}: accumulation vs the CPU replay")
    same(pt.read_moments(), C.replay(name, move)[1], f"{name} {move}: moments vs the CPU replay")


# ---- 2. identity and turn-away at every shape ----------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", C.SCENES)
def test_identity(pt, name, shape):
    w, h = shape
    st, want, (acc, mom) = move_and_reproject(pt, name, "identity", w, h, guides_first=(w == 8))
    check(pt, st, want, f"{name} {w}x{h} identity")
    hit = pt.read_aov("position")[..., 3] == 1
    assert (st["n_reprojected"], st["n_disoccluded"], st["n_missed"]) == (int(hit.sum()), 0, int((~hit).sum()))
    out, n0, n1 = pt.read_accum(), R.frames_of(mom), R.frames_of(pt.read_moments())
    assert (n1[hit] >= 1).all() and (n1[hit] <= n0[hit]).all() and not n1[~hit].any()
    diff = np.abs(out[..., :3].astype(np.float64) - acc[..., :3])[hit]
    print(name, shape, "identity: max |colour difference|", float(diff.max()) if diff.size else 0.0)
    assert not diff.size or diff.max() <= IDENTITY_BOUND


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", C.SCENES)
def test_turn_away(pt, name, shape):
    w, h = shape
    st, want, _ = move_and_reproject(pt, name, "away", w, h, guides_first=(w == 8))
    check(pt, st, want, f"{name} {w}x{h} away")
    hit = pt.read_aov("position")[..., 3] == 1
    assert (st["n_reprojected"], st["n_disoccluded"], st["n_missed"], st["sum_frames"], st["max_frames"]) == \
        (0, int(hit.sum()), int((~hit).sum()), 0, 0)
    assert not bits(pt.read_accum()).any() and not bits(pt.read_moments()).any()


def test_zero_camera(pt):
    """A `from` camera of twelve zeros is finite: accepted, and every hit is disoccluded."""
    C.run_state(pt, "c2wide", W, H)
    st = pt.reproject(np.zeros((4, 3), F))
    hit = pt.read_aov("position")[..., 3] == 1
    assert 30 <= hit.sum() <= W * H - 30
    assert C.stats_tuple(st) == (0, int(hit.sum()), int((~hit).sum()), 0, 0)
    assert not bits(pt.read_accum()).any() and not bits(pt.read_moments()).any()


# ---- 3. parameters --------------------------------------------------------------------------------------
def test_max_history_and_explicit_defaults(pt):
    st, want, _ = move_and_reproject(pt, "c3", "rotate", W, H, True)
    check(pt, st, want, "defaults")
    acc, mom = pt.read_accum(), pt.read_moments()
    assert st["max_frames"] == 5
    st2, want2, _ = move_and_reproject(pt, "c3", "rotate", W, H, True, normal_min=0.9, position_tolerance=0.02, max_history=32)
    check(pt, st2, want2, "the defaults, spelled out")
    assert st2 == st
    same(pt.read_accum(), acc, "explicit defaults vs NULL: accumulation")
    same(pt.read_moments(), mom, "explicit defaults vs NULL: moments")
    st3, want3, _ = move_and_reproject(pt, "c3", "rotate", W, H, False, max_history=3)
    check(pt, st3, want3, "max_history = 3")
    n = R.frames_of(pt.read_moments())
    assert st3["max_frames"] == 3 and np.array_equal(n, np.minimum(R.frames_of(mom), 3))
    assert st3["sum_frames"] == int(n.sum()) < st["sum_frames"]
    same(pt.read_accum(), acc, "the colour does not depend on the cap")
    st4, want4, _ = move_and_reproject(pt, "c3", "translate", W, H, True, normal_min=-1.0, position_tolerance=0.5, max_history=1)
    check(pt, st4, want4, "loose tests, max_history = 1")
    assert st4["n_reprojected"] > C.REPLAY[("c3", "translate")][0] and st4["max_frames"] == 1
    assert not pt.read_moments()[..., 1].any()       # n' = 1: M2' = s2 * 0


# ---- 4. continuation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1", "c3"])
def test_continuation(pt, name):
    st, want, _ = move_and_reproject(pt, name, "translate", W, H, False)
    check(pt, st, want, f"{name} translate")
    cfg_b = dataclasses.replace(scene(name, W, H), camera=C.camera_b(name, "translate", W, H))
    # frame 31 at camera B from the oracle: 31 + 1 is a power of two (tests/moments_common.py)
    o = pyoracle.Oracle(cfg_b)
    img, ost = o.render(31, 1)
    assert ost["stack_overflow"] == 0
    rgb = img[..., :3]
    assert not ((rgb != 0) & (np.abs(rgb) < np.finfo(F).tiny)).any(), "a subnormal component: the colour is not recoverable"
    c = (rgb * F(32)).astype(F)
    assert np.array_equal(bits((c * (F(1) / F(32))).astype(F)), bits(rgb)), "round trip of the colour"
    acc, mom, ast = A.render(want[0], want[1], [c], [31], 0.0, ALL)
    got = pt.render_adaptive(31, 1, 0.0, ALL)
    assert got == ast and got["n_active_pixels"] == W * H
    same(pt.read_accum(), acc, f"{name}: accumulation after the frame that follows")
    same(pt.read_moments(), mom, f"{name}: moments after the frame that follows")
    n0, n1 = R.frames_of(want[1]), R.frames_of(mom)
    assert np.array_equal(n1, n0 + 1)
    fresh = n0 == 0                                  # disoccluded and missed pixels hold that frame alone
    assert fresh.sum() >= 30
    same(acc[fresh][:, :3], c[fresh], f"{name}: a pixel without history takes the new frame whole")


# ---- 5. what the call leaves alone ----------------------------------------------------------------------
def test_leaves_alone(pt):
    name = "c2wide"
    cfg = scene(name, W, H)
    cam_a, cam_b = C.camera_a(name, W, H), C.camera_b(name, "rotate", W, H)
    C.run_state(pt, name, W, H)
    pt.render_guides()
    ptrs = (pt.accum_ptr(), pt.moments_ptr(), *(pt.aov_ptr(k) for k in AOVS))
    assert all(ptrs)
    pt.set_frame(W, H, cam_b, cfg.max_depth)
    pt.profile_enable(True)
    st = pt.reproject(cam_a)
    prof = pt.profile_read()
    pt.profile_enable(False)
    assert C.stats_tuple(st) == C.REPLAY[(name, "rotate")]
    launches = {k: v[1] for k, v in prof.items()}
    print(launches)
    assert launches["primary"] >= 1 and launches["blend"] == 3       # the history copies, the kernel, the copies back
    assert not any(v for k, v in launches.items() if k not in ("primary", "blend"))
    assert ptrs == (pt.accum_ptr(), pt.moments_ptr(), *(pt.aov_ptr(k) for k in AOVS))
    # the guide images are valid for the new camera: both previews run without pnrt_render_guides
    pt.denoise()
    pt.denoise_variance()
    assert pt.read_denoised().shape == (H, W, 4)
    # the moments still cover the accumulation
    assert pt.render_adaptive(31, 0, 0.5, 2)["n_pixels"] == W * H
    # a second move chains: from B back to A
    pt.set_frame(W, H, cam_a, cfg.max_depth)
    assert pt.reproject(cam_b)["n_reprojected"] > 0
    # a later pnrt_render at B is the oracle's
    pt.set_frame(W, H, cam_b, cfg.max_depth)
    pt.render(0, 2)
    acc = np.zeros((H, W, 4), F)
    pyoracle.Oracle(dataclasses.replace(cfg, camera=cam_b)).render(0, 2, accum=acc)
    same(pt.read_accum(), acc, "pnrt_render(0, 2) at the new camera after a reprojection")


# ---- 6. refusals -----------------------------------------------------------------------------------------
def raw(pt, cam, params=None):
    """pnrt_reproject through ctypes alone (a NULL camera, a reserved word)."""
    c = None
    if cam is not None:
        c = N.Camera()
        c.eye[:], c.lower_left[:], c.horizontal[:], c.vertical[:] = (list(map(float, r)) for r in np.asarray(cam, F).reshape(4, 3))
        c = ctypes.byref(c)
    return pt._lib.pnrt_reproject(pt._ctx, c, None if params is None else ctypes.byref(params), None)


def test_refusals(pt):
    name = "c1"
    cfg = scene(name, W, H)
    cam_a, cam_b = C.camera_a(name, W, H), C.camera_b(name, "rotate", W, H)
    assert code_of(pt.reproject, cam_a) == E_STATE                   # no scene, no frame
    pt.upload_scene(cfg.packed)
    assert code_of(pt.reproject, cam_a) == E_STATE                   # no frame
    pt.load(cfg)

    def untouched(call, code, what, moments=True):
        acc, g = pt.read_accum(), guides(pt)
        mom = pt.read_moments() if moments else None
        got = call()
        assert got == code, f"{what}: {got}"
        same(pt.read_accum(), acc, what + ": accumulation untouched")
        for k, a, b in zip(AOVS, guides(pt), g):
            same(a, b, what + f": {k} image untouched")
        if moments:
            same(pt.read_moments(), mom, what + ": moments untouched")

    pt.render(0, 2)
    pt.render_guides()
    pt.set_frame(W, H, cam_b, cfg.max_depth)
    untouched(lambda: code_of(pt.reproject, cam_a), E_STATE, "moments never enabled", moments=False)
    pt.enable_moments()
    pt.enable_moments(False)
    pt.set_frame(W, H, cam_a, cfg.max_depth)
    pt.render(0, 2)                                  # frames the moments do not count
    pt.render_guides()
    pt.set_frame(W, H, cam_b, cfg.max_depth)
    untouched(lambda: code_of(pt.reproject, cam_a), E_STATE, "moments disabled")
    pt.enable_moments()
    untouched(lambda: code_of(pt.reproject, cam_a), E_STATE, "the moments do not cover the accumulation")
    pt.set_frame(W, H, cam_a, cfg.max_depth)
    pt.reset_accum()
    pt.render(0, 2)
    pt.render_adaptive(3, 1, 0.5, 2)
    pt.render_guides()
    pt.set_frame(W, H, cam_b, cfg.max_depth)
    pt.enable_moments(False)
    untouched(lambda: code_of(pt.reproject, cam_a), E_STATE, "moments disabled, covering")
    pt.enable_moments()                              # off and on without a render in between: still covered
    pt.set_options(TRAVERSE_ZCULL | KERNEL_V1)
    untouched(lambda: code_of(pt.reproject, cam_a), E_STATE, "PNRT_KERNEL_V1")
    pt.set_options(TRAVERSE_ZCULL)

    untouched(lambda: raw(pt, None), E_ARG, "from NULL")
    for k in range(12):
        for v in (math.nan, math.inf, -math.inf)[:3 if k in (0, 11) else 1]:
            bad = cam_a.copy().reshape(-1)
            bad[k] = v
            untouched(lambda: code_of(pt.reproject, bad), E_ARG, f"camera float {k} = {v}")
    for v in (math.nan, math.inf, 1.5, -1.5):
        untouched(lambda: code_of(pt.reproject, cam_a, normal_min=v), E_ARG, f"normal_min {v}")
    for v in (math.nan, math.inf, 0.0, -0.02):
        untouched(lambda: code_of(pt.reproject, cam_a, position_tolerance=v), E_ARG, f"position_tolerance {v}")
    untouched(lambda: code_of(pt.reproject, cam_a, max_history=0), E_ARG, "max_history 0")
    untouched(lambda: raw(pt, cam_a, N.ReprojectParams(0.9, 0.02, 32, 1)), E_ARG, "reserved 1")
    assert "reserved" in pt._lib.pnrt_last_error(pt._ctx).decode()
    # the boundary values are accepted, and after all the refusals the call does what it does
    assert raw(pt, cam_a, N.ReprojectParams(-1.0, 1e-30, 1, 0)) == 0
    pt.set_frame(W, H, cam_a, cfg.max_depth)
    pt.reset_accum()
    st, want, _ = move_and_reproject(pt, name, "rotate", W, H, True, normal_min=1.0)
    check(pt, st, want, "normal_min = 1")
