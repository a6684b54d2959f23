"""Temporal reprojection under the camera models (pnrt_reproject_view, pt_reproject_view.h)
against tests/reproject_view_ref.py, the numpy restatement of DESIGN.md section 31, fed the
GPU's own accumulation, moments and guide images; the statistics against the CPU replay's
table; the seam, identity, continuation, what the call leaves alone, and every refusal.

Tolerance: 0 ulp everywhere (uint32 views and integers compared)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import adaptive_ref as A
import moments_ref as MR
import pyoracle
import rays_ref as R
import reproject_common as C
import reproject_view_common as VC
import reproject_view_ref as VR
from guides_common import SHAPES, bits, scene
from pnraytracing_amd import _native as N
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_ZCULL, PathTracer, PnrtError
from test_reproject_ref import IDENTITY_BOUND

pytestmark = pytest.mark.gpu

F = np.float32
W, H = VC.W, VC.Hh
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


@functools.lru_cache(maxsize=None)
def fresh_guides(name, spec, w, h):
    """The guide images of a context that did nothing but make the centre rays of a view and render their guides."""
    model, cam, fov = VC.view_of(name, spec, w, h)
    with PathTracer(0) as t:
        t.load(scene(name, w, h))
        t.render_guides_rays(t.make_rays(model, cam, 0, 1, fov_deg=fov))
        out = guides(t)
    for a in out:
        a.setflags(write=False)
    return out


def move_and_reproject(pt, name, a, b, w, h, **params):
    """The anchor sequence (reproject_common.run_state), then reproject_view(a, b), views as specs of
    reproject_view_common.  -> (stats, what reproject_view_ref makes of the GPU's own images:
    accumulation, moments, stats, valid taps; the images before the call)."""
    C.run_state(pt, name, w, h)
    acc, mom = pt.read_accum(), pt.read_moments()
    pos_a, nrm_a, _ = fresh_guides(name, a, w, h)
    va, vb = VC.view_of(name, a, w, h), VC.view_of(name, b, w, h)
    st = pt.reproject_view(va, vb, **params)
    pos_b, nrm_b, _ = guides(pt)
    want = VR.reproject(acc, mom, pos_a, nrm_a, pos_b, nrm_b, va, w, h, params)
    return st, want, (acc, mom)


def check(pt, st, want, what):
    acc, mom, wst, _ = want
    print(what, st)
    assert st == wst, what
    same(pt.read_accum(), acc, what + ": accumulation")
    same(pt.read_moments(), mom, what + ": moments")


# ---- 1. two pinhole views are pnrt_reproject ------------------------------------------------------------------
@pytest.mark.parametrize("name,move", [("c1", "rotate"), ("c2wide", "translate")])
def test_pinhole_equals_reproject(pt, name, move):
    cfg = scene(name, W, H)
    cam_a, cam_b = C.camera_a(name, W, H), C.camera_b(name, move, W, H)
    C.run_state(pt, name, W, H)
    st = pt.reproject_view(("pinhole", cam_a, 180.0), ("pinhole", cam_b, 180.0))
    with PathTracer(0) as other:
        C.run_state(other, name, W, H)
        other.set_frame(W, H, cam_b, cfg.max_depth)
        want = other.reproject(cam_a)
        assert st == want and C.stats_tuple(st) == C.REPLAY[(name, move)]
        same(pt.read_accum(), other.read_accum(), "accumulation")
        same(pt.read_moments(), other.read_moments(), "moments")
        for k, got, ref in zip(AOVS, guides(pt), guides(other)):
            same(got, ref, f"the {k} image")


# ---- 2. every case of the table, the seam among them -------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(VC.CASES))
def test_table(pt, case):
    name, a, b, params = VC.CASES[case]
    params = dict(params)
    st, want, _ = move_and_reproject(pt, name, a, b, W, H, **params)
    assert C.stats_tuple(st) == VC.TABLE[case], "the statistics of the CPU replay"
    assert st["n_pixels"] == W * H
    check(pt, st, want, case)
    for k, got, fresh in zip(AOVS, guides(pt), fresh_guides(name, b, W, H)):
        same(got, fresh, f"{case}: the {k} image is the one of make_rays + render_guides_rays of the new view in a fresh context")
    # the GPU's images were the CPU replay's inputs and results
    same(pt.read_accum(), VC.replay(case)[0], f"{case}: accumulation vs the CPU replay")
    same(pt.read_moments(), VC.replay(case)[1], f"{case}: moments vs the CPU replay")
    pt.denoise()                                     # the guides are valid: no further call


def test_seam(pt):
    """The seam case on the GPU's own images: pixels reprojected from columns W - 1 and 0 at once."""
    name, a, b, params = VC.CASES["seam"]
    params = dict(params)
    st, want, (acc, mom) = move_and_reproject(pt, name, a, b, W, H, **params)
    check(pt, st, want, "seam")
    pos_a, nrm_a, _ = fresh_guides(name, a, W, H)
    pos_b, nrm_b, _ = guides(pt)
    _, valid, _, index = VR.tap_table(acc, mom, pos_a, nrm_a, pos_b, nrm_b, VC.view_of(name, a, W, H), W, H, params)
    col = index % W
    both = (valid & (col == W - 1)).any(axis=-1) & (valid & (col == 0)).any(axis=-1)
    print("seam: pixels with valid taps in columns W - 1 and 0:", int(both.sum()))
    assert both.sum() >= 30
    out = pt.read_accum()
    assert (out[both][:, 3] == 1).all() and (MR.frames_of(pt.read_moments())[both] >= 1).all()


# ---- 3. identity at every shape ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("model", R.MODELS)
def test_identity(pt, model, shape):
    w, h = shape
    name, spec = "c1", (model, "identity", 180.0)
    st, want, (acc, mom) = move_and_reproject(pt, name, spec, spec, w, h)
    check(pt, st, want, f"{model} {w}x{h} identity")
    hit = pt.read_aov("position")[..., 3] == 1
    assert (st["n_reprojected"], st["n_disoccluded"], st["n_missed"]) == (int(hit.sum()), 0, int((~hit).sum()))
    if shape == (1, 1) and model == "fisheye":
        assert st["n_missed"] == 1                   # rho > 1: no ray
    out, n0, n1 = pt.read_accum(), MR.frames_of(mom), MR.frames_of(pt.read_moments())
    assert (n1[hit] >= 1).all() and (n1[hit] <= n0[hit]).all() and not n1[~hit].any()
    diff = np.abs(out[..., :3].astype(np.float64) - acc[..., :3])[hit]
    print(model, shape, "identity: hits", int(hit.sum()), "max |colour difference|", float(diff.max()) if diff.size else 0.0)
    assert not diff.size or diff.max() <= IDENTITY_BOUND


# ---- 4. the sample fields are checked and ignored ---------------------------------------------------------------
def test_sample_fields_are_ignored(pt):
    name, a, b, _ = VC.CASES["fisheye-c1-rotate"]
    st, want, _ = move_and_reproject(pt, name, a, b, W, H)
    acc, mom, g = pt.read_accum(), pt.read_moments(), guides(pt)
    C.run_state(pt, name, W, H)
    va, vb = (PathTracer.ray_camera(m, cam, fov_deg=fov, aa_width=1.0, per_pixel=1)
              for m, cam, fov in (VC.view_of(name, a, W, H), VC.view_of(name, b, W, H)))
    st2 = pt.reproject_view(va, vb)
    assert st2 == st
    same(pt.read_accum(), acc, "aa_width 1, per_pixel 1: accumulation")
    same(pt.read_moments(), mom, "aa_width 1, per_pixel 1: moments")
    for k, got, ref in zip(AOVS, guides(pt), g):
        same(got, ref, f"aa_width 1, per_pixel 1: the {k} image")
    # a pinhole view's lens as well
    C.run_state(pt, "c1", W, H)
    cam_a, cam_b = C.camera_a("c1", W, H), C.camera_b("c1", "rotate", W, H)
    lens = dict(aa_width=2.0, lens_radius=0.2, focus_distance=6.0)
    st3 = pt.reproject_view(PathTracer.ray_camera("pinhole", cam_a, **lens), PathTracer.ray_camera("pinhole", cam_b, **lens))
    assert C.stats_tuple(st3) == C.REPLAY[("c1", "rotate")]
    same(pt.read_accum(), C.replay("c1", "rotate")[0], "a lens in both pinhole views: accumulation")


# ---- 5. continuation -----------------------------------------------------------------------------------------------
def test_continuation(pt):
    name, a, b, _ = VC.CASES["fisheye-c1-translate"]
    st, want, _ = move_and_reproject(pt, name, a, b, W, H)
    check(pt, st, want, "fisheye translate")
    model, cam_b, fov = VC.view_of(name, b, W, H)
    # frame 31 of the new view's rays alone, in a fresh context: 31 + 1 is a power of two (tests/moments_common.py)
    with PathTracer(0) as t:
        t.load(scene(name, W, H))
        t.render_rays(31, 1, t.make_rays(model, cam_b, 31, 1, fov_deg=fov))
        rgb = t.read_accum()[..., :3]
    assert not ((rgb != 0) & (np.abs(rgb) < np.finfo(F).tiny)).any(), "a subnormal component: the colour is not recoverable"
    c = (rgb * F(32)).astype(F)
    assert np.array_equal(bits((c * (F(1) / F(32))).astype(F)), bits(rgb)), "round trip of the colour"
    acc, mom, ast = A.render(want[0], want[1], [c], [31], 0.0, ALL)
    rays = pt.make_rays(model, cam_b, 31, 1, fov_deg=fov)
    got = pt.render_rays_adaptive(31, 1, rays, 0, 0.0, ALL)
    assert got["n_active_pixels"] == got["n_pixels"] == W * H == ast["n_active_pixels"]
    same(pt.read_accum(), acc, "accumulation after the frame that follows")
    same(pt.read_moments(), mom, "moments after the frame that follows")
    n0, n1 = MR.frames_of(want[1]), MR.frames_of(mom)
    assert np.array_equal(n1, n0 + 1)
    fresh = n0 == 0                                  # disoccluded and missed pixels hold that frame alone
    assert fresh.sum() >= 30
    same(acc[fresh][:, :3], c[fresh], "a pixel without history takes the new frame whole")


# ---- 6. what the call leaves alone ----------------------------------------------------------------------------------
def test_leaves_alone(pt):
    name, a, b, _ = VC.CASES["fisheye-c2wide-rotate"]
    cfg = scene(name, W, H)
    va, vb = VC.view_of(name, a, W, H), VC.view_of(name, b, W, H)
    C.run_state(pt, name, W, H)
    pt.render_guides()
    ptrs = (pt.accum_ptr(), pt.moments_ptr(), *(pt.aov_ptr(k) for k in AOVS))
    assert all(ptrs)
    pt.profile_enable(True)
    st = pt.reproject_view(va, vb)
    prof = pt.profile_read()
    pt.profile_enable(False)
    assert C.stats_tuple(st) == VC.TABLE["fisheye-c2wide-rotate"]
    launches = {k: v[1] for k, v in prof.items()}
    print(launches)
    # two guide traces; two pnrt_make_rays launches, the history copies, the kernel, the copies back
    assert launches["primary"] == 2 and launches["blend"] == 5
    assert not any(v for k, v in launches.items() if k not in ("primary", "blend"))
    assert ptrs == (pt.accum_ptr(), pt.moments_ptr(), *(pt.aov_ptr(k) for k in AOVS))
    # the guide images are valid: both previews run without another guides call
    pt.denoise()
    pt.denoise_variance()
    assert pt.read_denoised().shape == (H, W, 4)
    # the moments still cover the accumulation
    assert pt.render_adaptive(31, 0, 0.5, 2)["n_pixels"] == W * H
    # a second move chains: from B back to A, and on into another model
    assert pt.reproject_view(vb, va)["n_reprojected"] > 0
    assert pt.reproject_view(va, ("equirect", va[1], 180.0), position_tolerance=0.13)["n_reprojected"] > 0
    # the pnrt_set_frame camera stayed current: a later pnrt_render is the oracle's
    pt.render(0, 2)
    acc = np.zeros((H, W, 4), F)
    pyoracle.Oracle(cfg).render(0, 2, accum=acc)
    same(pt.read_accum(), acc, "pnrt_render(0, 2) after a reprojection")


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def raw(pt, a, b, params=None):
    """pnrt_reproject_view through ctypes alone (NULL views, reserved words)."""
    ra = None if a is None else ctypes.byref(a)
    rb = None if b is None else ctypes.byref(b)
    return pt._lib.pnrt_reproject_view(pt._ctx, ra, rb, None if params is None else ctypes.byref(params), None)


def test_refusals(pt):
    name = "c1"
    cfg = scene(name, W, H)
    cam_a, cam_b = C.camera_a(name, W, H), C.camera_b(name, "rotate", W, H)
    va, vb = ("fisheye", cam_a, 200.0), ("equirect", cam_b, 180.0)
    assert code_of(pt.reproject_view, va, vb) == E_STATE             # no scene, no frame
    pt.upload_scene(cfg.packed)
    assert code_of(pt.reproject_view, va, vb) == E_STATE             # no frame
    pt.load(cfg)

    def untouched(call, code, what, moments=True):
        acc, g = pt.read_accum(), guides(pt)
        mom = pt.read_moments() if moments else None
        got = call()
        assert got == code, f"{what}: {got}"
        same(pt.read_accum(), acc, what + ": accumulation untouched")
        for k, x, y in zip(AOVS, guides(pt), g):
            same(x, y, what + f": {k} image untouched")
        if moments:
            same(pt.read_moments(), mom, what + ": moments untouched")

    pt.render(0, 2)
    pt.render_guides()
    untouched(lambda: code_of(pt.reproject_view, va, vb), E_STATE, "moments never enabled", moments=False)
    pt.enable_moments()
    pt.enable_moments(False)
    pt.render(0, 2)                                  # frames the moments do not count
    untouched(lambda: code_of(pt.reproject_view, va, vb), E_STATE, "moments disabled")
    pt.enable_moments()
    untouched(lambda: code_of(pt.reproject_view, va, vb), E_STATE, "the moments do not cover the accumulation")
    pt.reset_accum()
    pt.render(0, 2)
    pt.render_adaptive(3, 1, 0.5, 2)
    pt.enable_moments(False)
    untouched(lambda: code_of(pt.reproject_view, va, vb), E_STATE, "moments disabled, covering")
    pt.enable_moments()                              # off and on without a render in between: still covered
    pt.set_options(TRAVERSE_ZCULL | KERNEL_V1)
    untouched(lambda: code_of(pt.reproject_view, va, vb), E_STATE, "PNRT_KERNEL_V1")
    pt.set_options(TRAVERSE_ZCULL)

    def err():
        return pt._lib.pnrt_last_error(pt._ctx).decode()

    good = PathTracer.ray_camera(*va)
    untouched(lambda: raw(pt, None, good), E_ARG, "from NULL")
    assert "from" in err()
    untouched(lambda: raw(pt, good, None), E_ARG, "to NULL")
    assert "to " in err()
    # every argument rule of pnrt_make_rays, in each of the two views, named in the message
    bad_cams = []
    for k in range(12):
        for v in (math.nan, math.inf, -math.inf)[:3 if k in (0, 11) else 1]:
            cam = cam_a.copy().reshape(-1)
            cam[k] = v
            bad_cams.append((f"camera float {k} = {v}", dict(model="pinhole", camera=cam)))
    bad = bad_cams + [
        ("model -1", dict(model=-1)), ("model 4", dict(model=4)),
        ("fov_deg nan", dict(fov_deg=math.nan)), ("focus_distance inf", dict(model="pinhole", focus_distance=math.inf)),
        ("fisheye fov 0", dict(model="fisheye", fov_deg=0.0)), ("fisheye fov 361", dict(model="fisheye", fov_deg=361.0)),
        ("fisheye fov -10", dict(model="fisheye", fov_deg=-10.0)),
        ("aa_width -1", dict(aa_width=-1.0)), ("aa_width nan", dict(aa_width=math.nan)),
        ("lens_radius -1", dict(model="pinhole", lens_radius=-1.0)), ("lens_radius inf", dict(model="pinhole", lens_radius=math.inf)),
        ("a lens under ortho", dict(model="ortho", lens_radius=0.1, focus_distance=3.0)),
        ("a lens without focus", dict(model="pinhole", lens_radius=0.1, focus_distance=0.0)),
        ("per_pixel 2", dict(per_pixel=2)), ("reserved 1", dict(reserved=1))]
    for what, fields in bad:
        kw = dict(model="equirect", camera=cam_a)
        kw.update(fields)
        rc = N.RayCamera()                           # (built by hand: an unknown model number has no name)
        m = kw.pop("model")
        ok = PathTracer.ray_camera("pinhole" if not isinstance(m, str) else m, **kw)
        ctypes.memmove(ctypes.byref(rc), ctypes.byref(ok), ctypes.sizeof(rc))
        if not isinstance(m, str):
            rc.model = m
        untouched(lambda: raw(pt, rc, good), E_ARG, what + " in from")
        assert "reproject_view: from:" in err(), err()
        untouched(lambda: raw(pt, good, rc), E_ARG, what + " in to")
        assert "reproject_view: to:" in err(), err()
    for v in (math.nan, math.inf, 1.5, -1.5):
        untouched(lambda: code_of(pt.reproject_view, va, vb, normal_min=v), E_ARG, f"normal_min {v}")
    for v in (math.nan, math.inf, 0.0, -0.02):
        untouched(lambda: code_of(pt.reproject_view, va, vb, position_tolerance=v), E_ARG, f"position_tolerance {v}")
    untouched(lambda: code_of(pt.reproject_view, va, vb, max_history=0), E_ARG, "max_history 0")
    untouched(lambda: raw(pt, good, good, N.ReprojectParams(0.9, 0.02, 32, 1)), E_ARG, "reserved 1")
    assert "reserved" in err()
    # the boundary values are accepted, and after all the refusals the call does what it does
    assert raw(pt, PathTracer.ray_camera("fisheye", cam_a, fov_deg=360.0), good, N.ReprojectParams(-1.0, 1e-30, 1, 0)) == 0
    st, want, _ = move_and_reproject(pt, name, ("fisheye", "identity", VC.FISHEYE_FOV), ("fisheye", "rotate", VC.FISHEYE_FOV), W, H,
                                     normal_min=1.0)
    check(pt, st, want, "normal_min = 1")


@pytest.mark.parametrize("model", R.MODELS)
def test_zero_camera(pt, model):
    """A `from` camera of twelve zeros is finite: accepted, and every hit is disoccluded."""
    C.run_state(pt, "c2wide", W, H)
    to = ("pinhole", C.camera_a("c2wide", W, H), 180.0)
    st = pt.reproject_view((model, np.zeros((4, 3), F), 180.0), to)
    hit = pt.read_aov("position")[..., 3] == 1
    assert 30 <= hit.sum() <= W * H - 30
    assert C.stats_tuple(st) == (0, int(hit.sum()), int((~hit).sum()), 0, 0)
    assert not bits(pt.read_accum()).any() and not bits(pt.read_moments()).any()
