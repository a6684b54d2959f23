"""Self-checks of tests/reproject_view_ref.py on the CPU: the pinhole
view is reproject_ref's, bit for bit; every model's inverse returns the pixel its centre
ray came from; the equirectangular seam; the replay table the GPU tests compare the
library's statistics with; identity per model (no GPU needed)."""
import numpy as np
import pytest

import moments_ref as MR
import rays_ref as R
import reproject_common as C
import reproject_ref as RP
import reproject_view_common as VC
import reproject_view_ref as VR
from guides_common import SHAPES, bits
from test_reproject_ref import IDENTITY_BOUND

F, U = np.float32, np.uint32
W, H = VC.W, VC.Hh

# The round trip's bound, a condition and no measurement: 1/64 pixel shifts a bilinear weight by
# 1/64 -- far below what moves a tap, far above float noise.
ROUND_TRIP = 2.0 ** -6
# PN-libm's own worst case over test_round_trip's cases, as measured on the restatement: 6.83e-4 pixel (the
# 360-degree fisheye at 67x45, next to the rim); 1.73e-5 at 8x8 (the orthographic view).


# ---- 1. a pinhole view is pnrt_reproject's ----------------------------------------------------------------
@pytest.mark.parametrize("name,move", [("c1", "rotate"), ("c2wide", "translate"), ("c3", "zoom"), ("c1", "away")])
def test_pinhole_is_reproject_ref(name, move):
    acc, mom = C.state(name, W, H)
    pa, na = C.oracle_guides(name, "identity", W, H)
    pb, nb = C.oracle_guides(name, move, W, H)
    cam = C.camera_a(name, W, H)
    view = ("pinhole", cam, 180.0)
    for got, want in zip(VR.project(pb, view, W, H), RP.project(pb, cam, W, H)):
        assert got.dtype == want.dtype
        assert np.array_equal(got.view(U) if got.dtype == F else got, want.view(U) if want.dtype == F else want)
    for params in ({}, {"normal_min": 0.5, "position_tolerance": 0.1, "max_history": 3}):
        for got, want in zip(VR.tap_table(acc, mom, pa, na, pb, nb, view, W, H, params),
                             RP.tap_table(acc, mom, pa, na, pb, nb, cam, W, H, params)):
            assert np.array_equal(bits(got) if got.dtype == F else got, bits(want) if want.dtype == F else want)
        a, m, st, nv = VR.reproject(acc, mom, pa, na, pb, nb, view, W, H, params)
        wa, wm, wst = RP.reproject(acc, mom, pa, na, pb, nb, cam, W, H, params)
        assert st == wst and np.array_equal(bits(a), bits(wa)) and np.array_equal(bits(m), bits(wm))
        if not params:
            assert np.array_equal(nv, C.replay(name, move)[3])


# ---- 2. the inverse returns the pixel ----------------------------------------------------------------------
def _round_trip_cases():
    for model in R.MODELS:
        for fov in (VC.FISHEYE_FOVS if model == "fisheye" else (180.0,)):
            yield model, fov


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("model,fov", list(_round_trip_cases()))
def test_round_trip(model, fov, shape):
    w, h = shape
    worst = 0.0
    for cam in (C.camera_a("c1", w, h), VC.oblique(w, h)):
        rays = R.make_set(model, cam, w, h, 0, fov_deg=fov)
        O, D = rays[:, 0:3], rays[:, 4:7]
        p = np.arange(w * h)
        x, y = (p % w).astype(np.float64), (p // w).astype(np.float64)
        # left out, and nothing else: where the inverse is not defined
        out = np.zeros(w * h, bool)
        if model == "equirect":
            out = p // w == 0                        # the pole: every column of row 0 is one direction
        if model == "fisheye":
            rho = R.fisheye_rho(w, h)
            out = rho > 1                            # no ray
            if fov == 360.0:
                out |= rho == 1                      # the rim is the single direction -f
            assert np.array_equal(rho > 1, ~D.any(axis=1))
        assert np.isfinite(rays).all() and D[~out].any(axis=1).all()
        for dist in (0.5, 3.0, 50.0):
            P = O + F(dist) * D
            assert P.dtype == F
            fx, fy, front, _ = VR.inverse(P, (model, cam, fov), w, h)
            assert front[~out].all() and np.isfinite(fx[~out]).all() and np.isfinite(fy[~out]).all()
            ex = np.abs(fx.astype(np.float64) - x)
            if model == "equirect":
                ex = np.minimum(ex, w - ex)          # modulo W
            ey = np.abs(fy.astype(np.float64) - y)
            if (~out).any():
                worst = max(worst, float(ex[~out].max()), float(ey[~out].max()))
            assert (ex[~out] <= ROUND_TRIP).all() and (ey[~out] <= ROUND_TRIP).all(), (model, fov, shape, dist)
    print(f"round trip {model} fov {fov} {w}x{h}: worst |error| {worst:.3g} px")


# ---- 3. the seam of an equirectangular view ------------------------------------------------------------------
def test_seam_synthetic(monkeypatch):
    """A wall two units in front of the seam of an equirectangular view A at the origin: a hit
    whose fx lies in (W - 1, W) takes its taps from columns W - 1 and 0, and so does one whose fx
    lies in (-1, 0) -- which the inverse itself reaches only by rounding (phi / 2 pi + 0.5 is in
    [0, 1]), so that one is fed to the tap table in the inverse's place."""
    w, h = 16, 8
    cam = np.array([[0, 0, 0], [-1, -1, -1], [2, 0, 0], [0, 2, 0]], F)       # r = +x, u = +y, f = -z
    view = ("equirect", cam, 180.0)
    r, u, f = R.basis(cam)
    assert np.array_equal(f, np.array([0, 0, -1], F))
    n = w * h
    posA, nrmA = np.zeros((n, 4), F), np.zeros((n, 4), F)
    posA[:, 3], nrmA[:, 2], nrmA[:, 3] = 1, -1, 7                          # every pixel of A hit material 7, facing -z
    acc, mom = np.ones((n, 4), F), np.zeros((n, 4), F)
    acc[:, 0] = np.arange(n)
    mom[:, 3].view(U)[:] = 4
    # B: hits on the wall z = 2 (behind A: the seam), on the middle rows, either side of x = 0
    posB, nrmB = np.zeros((h, w, 4), F), np.zeros((h, w, 4), F)
    xs = np.array([0.05, -0.05, 0.1, -0.1], F)
    posB[4, :4, 0], posB[4, :4, 1], posB[4, :4, 2], posB[4, :4, 3] = xs, 0.1, 2.0, 1
    nrmB[..., 2], nrmB[..., 3] = -1, 7
    nrmB[posB[..., 3] == 0, 3] = -1
    fx, fy, _, _ = VR.inverse(posB[4, :4], view, w, h)
    print("seam fx", fx, "fy", fy)
    assert (fx[[0, 2]] > w - 1).all() and (fx[[0, 2]] < w).all()               # +x behind the camera: phi just below pi
    assert (fx[[1, 3]] > 0).all() and (fx[[1, 3]] < 1).all()                   # -x: phi just above -pi, columns 0 and 1
    assert (fy > 4).all() and (fy < 5).all()
    params = {"position_tolerance": 1e9}

    def check(ks):
        hit, valid, wgt, index = VR.tap_table(acc, mom, posA, nrmA, posB, nrmB, view, w, h, params)
        for k in ks:
            cols, rows = index[4, k] % w, index[4, k] // w
            # the left taps (i = 0, 2) are column W - 1, the right ones column 0, on either side of the seam
            assert cols.tolist() == [w - 1, 0, w - 1, 0] and rows.tolist() == [4, 4, 5, 5]
            assert valid[4, k].all() and abs(float(wgt[4, k].sum()) - 1) < 1e-6
        a, m, st, nv = VR.reproject(acc, mom, posA, nrmA, posB, nrmB, view, w, h, params)
        assert st["n_reprojected"] == 4 and st["n_disoccluded"] == 0 and (nv[4, ks] == 4).all()
        for k in ks:                                 # the blend of both columns' colours (acc.x is the pixel index)
            lo, hi = sorted(acc[index[4, k], 0].tolist())[::3]
            assert lo < a[4, k, 0] < hi and hi - lo > w - 2
    check([0, 2])
    # rows do not wrap: a hit straight below A lands on row 0 and takes nothing from row H - 1
    posB2 = np.zeros((h, w, 4), F)
    posB2[0, 0] = (0.3, -5.0, -0.2, 1)
    nrmB2 = nrmB.copy()
    nrmB2[0, 0, 3] = 7
    _, valid2, _, index2 = VR.tap_table(acc, mom, posA, nrmA, posB2, nrmB2, view, w, h, params)
    assert valid2[0, 0].any() and (index2[0, 0][valid2[0, 0]] // w <= 1).all()
    # fx in (-1, 0), and fx == W exactly (its range test is <=: the tap of weight 1 is column 0)
    real = VR.inverse

    def shifted(P, v, ww, hh):
        fx, fy, front, dd = real(P, v, ww, hh)
        fx = fx.copy()
        fx[4, 0], fx[4, 1], fx[4, 2], fx[4, 3] = F(-0.25), F(-0.75), F(-0.5), F(w)
        return fx, fy, front, dd
    monkeypatch.setattr(VR, "inverse", shifted)
    check([0, 1, 2])
    hit, valid, wgt, index = VR.tap_table(acc, mom, posA, nrmA, posB, nrmB, view, w, h, params)
    assert (index[4, 3] % w).tolist()[0::2] == [0, 0] and valid[4, 3].tolist() == [True, False, True, False]


# ---- 4. the replay table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(VC.CASES))
def test_replay_table(case):
    st = VC.replay(case)[2]
    print(repr(case), C.stats_tuple(st))
    assert C.stats_tuple(st) == VC.TABLE[case]
    assert st["n_reprojected"] + st["n_disoccluded"] + st["n_missed"] == st["n_pixels"] == W * H


def test_table_covers_every_class():
    """From the replay, not from the GPU: an input for which this fails is a test error."""
    assert sorted(VC.TABLE) == sorted(VC.CASES)
    for model in R.MODELS:
        for name in ("c1", "c2wide"):
            for move in ("rotate", "translate"):
                _, a, b, _ = VC.CASES[f"{model}-{name}-{move}"]
                assert a[0] == b[0] == model and a[1] == "identity" and b[1] == move and move in C.MOVES
    assert [v[0] for v in VC.CASES["pinhole-to-fisheye"][1:3]] == ["pinhole", "fisheye"]
    assert [v[0] for v in VC.CASES["fisheye-to-equirect"][1:3]] == ["fisheye", "equirect"]
    for model in R.MODELS:                           # a case belongs to the model of its `from` view: the kernel it runs
        four = some = none = 0
        for case, (_, a, _, _) in VC.CASES.items():
            if a[0] != model:
                continue
            nv = VC.replay(case)[3]
            four += int((nv == 4).sum())
            some += int(((nv >= 1) & (nv <= 3)).sum())
            none += int((nv == 0).sum())
        print(model, "four valid taps", four, "one to three", some, "disoccluded", none)
        assert min(four, some, none) >= 30, (model, four, some, none)


def test_seam_case_reprojects_across_the_seam():
    """The `from` camera of the seam case looks away from the box's back wall, so the seam faces it."""
    name, a, b, params = VC.CASES["seam"]
    acc, mom = C.state(name, W, H)
    pa, na = VC.oracle_guides(name, a, W, H)
    pb, nb = VC.oracle_guides(name, b, W, H)
    view = VC.view_of(name, a, W, H)
    _, _, f = R.basis(view[1])
    assert f[2] > 0.99                               # looking along +z, out of the open front
    hit, valid, _, index = VR.tap_table(acc, mom, pa, na, pb, nb, view, W, H, dict(params))
    col = index % W
    both = (valid & (col == W - 1)).any(axis=-1) & (valid & (col == 0)).any(axis=-1)
    print("seam: pixels with valid taps in columns W - 1 and 0:", int(both.sum()))
    assert both.sum() >= 30


# ---- 5. identity per model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("name", ["c1", "c2wide"])
def test_identity(name, model, shape):
    w, h = shape
    spec = (model, "identity", 180.0)
    acc, mom = C.state(name, w, h)
    out, mo, st, nv = VC.replay_views(name, spec, spec, w, h)
    pa, _ = VC.oracle_guides(name, spec, w, h)
    hit = pa[..., 3] == 1
    assert (nv[hit] >= 1).all() and (nv[~hit] == -1).all()
    assert C.stats_tuple(st)[:3] == (int(hit.sum()), 0, int((~hit).sum()))
    if model == "fisheye" and shape == (1, 1):
        assert st["n_missed"] == 1                   # rho > 1: no ray
    assert not bits(out[~hit]).any() and not bits(mo[~hit]).any()
    n, n1 = MR.frames_of(mom), MR.frames_of(mo)
    assert (n1[hit] >= 1).all() and (n1[hit] <= n[hit]).all()
    diff = np.abs(out[..., :3].astype(np.float64) - acc[..., :3])[hit]
    worst = float(diff.max()) if diff.size else 0.0
    print(name, model, shape, "identity: hits", int(hit.sum()), "max |colour difference|", worst)
    assert worst <= IDENTITY_BOUND
