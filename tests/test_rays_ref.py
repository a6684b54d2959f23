"""tests/rays_ref.py, the numpy restatement of pnrt_make_rays, checked
for the properties the camera models promise, and the refusals of the Python layer that
need no device (no GPU needed)."""
import numpy as np
import pytest

import cameras_ref
import rays_ref as R
from pnraytracing_amd import host as H
from pnraytracing_amd import session, tracer

F = np.float32
# a camera that is not axis-aligned: every basis vector has three non-zero components
CAM = np.asarray(H.camera_update((1.5, 3.1, 6.0), (0.2, 2.5, -0.4), (0.1, 1.0, 0.05), 50.0, F(67) / F(45)), F).reshape(4, 3)
# an axis-aligned one: r = x, u = y, f = -z exactly
AXIS = np.array([[0, 1, 5], [-2, -0.5, 3], [4, 0, 0], [0, 3, 0]], F)


def ulps(a, b):
    """|a - b| in units of the last place of 1.0 (unit vectors' components and lengths)."""
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.finfo(F).eps


def test_samples_are_exact_and_extend_the_per_frame_sequence():
    for frame in (0, 1, 7, 0xFFFFFF - 2, 0xFFFFFFFE, 0xFFFFFFFF):
        u = R.u_samples(frame, np.zeros((4, 1), np.uint32))[:, 0]
        assert np.array_equal(u.view(np.uint32), cameras_ref.u4(frame).view(np.uint32)), frame
        n = (frame + 1) & 0xFFFFFFFF
        for i, a in enumerate(R.A):
            h = 0x9E3779B9 + i
            want = (((n * a + h) & 0xFFFFFFFF) >> 8) / 2.0 ** 24        # exact in binary64, and in binary32: 24 bits
            got = R.u_samples(frame, np.full((4, 1), h, np.uint32))[i, 0]
            assert got.dtype == F and float(got) == want and 0.0 <= want < 1.0
    # wang_hash against the shader's own statement (ray_tracing.comp:499-507) on one seed, by hand
    s = 12345
    s = (s ^ 61) ^ (s >> 16); s = (s * 9) & 0xFFFFFFFF; s ^= s >> 4; s = (s * 0x27d4eb2d) & 0xFFFFFFFF; s ^= s >> 15   # noqa: E702
    assert int(R.wang_hash(np.array([12345]))[0]) == s


def test_per_pixel_hashes_differ_between_neighbours():
    W, Hh = 67, 45
    h = R.hashes(W, Hh, 1).reshape(4, Hh, W)
    assert not R.hashes(W, Hh, 0).any()
    for i in range(4):
        assert (h[i, :, 1:] != h[i, :, :-1]).all() and (h[i, 1:] != h[i, :-1]).all()
    assert len({tuple(c) for c in h.reshape(4, -1).T.tolist()}) == W * Hh       # every pixel its own rotation
    # ... so neighbouring pixels' lens samples differ where the per-frame ones are equal
    a = R.make_set("pinhole", CAM, W, Hh, 3, aa_width=1.0, lens_radius=0.2, focus_distance=6.0, per_pixel=1).reshape(Hh, W, 8)
    b = R.make_set("pinhole", CAM, W, Hh, 3, aa_width=1.0, lens_radius=0.2, focus_distance=6.0, per_pixel=0).reshape(Hh, W, 8)
    assert (np.abs(b[:, 1:, 0:3] - b[:, :-1, 0:3]) == 0).all()                  # one lens point per frame
    assert (np.any(a[:, 1:, 0:3] != a[:, :-1, 0:3], axis=-1)).all()             # one per pixel


@pytest.mark.parametrize("params", [{}, {"aa_width": 1.0}, {"aa_width": 1.5, "per_pixel": 1}])
@pytest.mark.parametrize("model", R.MODELS)
def test_directions_are_unit_within_2_ulp(model, params):
    for cam in (CAM, AXIS):
        rays = R.make_set(model, cam, 67, 45, 5, fov_deg=200.0, **params)
        d = rays[:, 4:7].astype(np.float64)
        length = np.sqrt((d * d).sum(axis=1))
        is_ray = rays[:, 4:7].any(axis=1)
        assert is_ray.sum() > 67 * 45 // 2
        assert ulps(length[is_ray], 1.0).max() <= 2.0
        assert not rays[~is_ray].any()                   # no ray: six zeros (and the reserved floats)
        assert not rays[:, 3].any() and not rays[:, 7].any() and np.isfinite(rays).all()
    lens = R.make_set("pinhole", CAM, 67, 45, 5, aa_width=1.0, lens_radius=0.3, focus_distance=5.0, per_pixel=1)
    d = lens[:, 4:7].astype(np.float64)
    assert ulps(np.sqrt((d * d).sum(axis=1)), 1.0).max() <= 2.0


def test_pinhole_is_camera_dir():
    """Without samples the pinhole direction is CameraGetRay's (the host library's pixel ray), bit for bit."""
    W, Hh = 37, 19
    rays = R.make_set("pinhole", CAM, W, Hh, 9).reshape(Hh, W, 8)
    for px, py in ((0, 0), (36, 18), (5, 11), (20, 3)):
        want = np.asarray(H.camera_pixel_ray(CAM, px, py, W, Hh), F).reshape(-1)[:6]
        got = np.concatenate([rays[py, px, 0:3], rays[py, px, 4:7]])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (px, py)
    # frames differ only through samples
    assert np.array_equal(rays.reshape(-1, 8), R.make_set("pinhole", CAM, W, Hh, 0))


def test_equirect_centre_is_f_and_the_set_covers_the_sphere():
    W, Hh = 64, 32
    for cam in (CAM, AXIS):
        rays = R.make_set("equirect", cam, W, Hh, 0).reshape(Hh, W, 8)
        r, u, f = R.basis(cam)
        centre = rays[Hh // 2, W // 2]                   # s = t = 0.5 exactly
        assert np.array_equal(centre[0:3], cam[0])
        assert ulps(centre[4:7], f).max() <= 2.0         # normalize(0 r + 0 u + 1 f): f up to its renormalisation
        d = rays[..., 4:7].reshape(-1, 3).astype(np.float64)
        comps = np.stack([d @ r.astype(np.float64), d @ u.astype(np.float64), d @ f.astype(np.float64)], axis=1)
        octants = {tuple(row) for row in (comps > 0).tolist() if True}
        strict = np.all(np.abs(comps) > 1e-3, axis=1)
        assert len({tuple(row) for row in (comps[strict] > 0).tolist()}) == 8 and len(octants) == 8
    rays = R.make_set("equirect", AXIS, W, Hh, 0).reshape(Hh, W, 8)
    assert np.array_equal(rays[Hh // 2, W // 2, 4:7], np.array([0, 0, -1], F))      # axis-aligned: f itself
    # the seam: s = 0 looks backwards
    assert ulps(rays[Hh // 2, 0, 4:7], np.array([0, 0, 1], F)).max() <= 2.0


@pytest.mark.parametrize("W,Hh", [(67, 45), (8, 8), (1, 1), (64, 32)])
def test_fisheye_is_no_ray_exactly_outside_the_circle(W, Hh):
    rays = R.make_set("fisheye", CAM, W, Hh, 0, fov_deg=180.0)
    rho = R.fisheye_rho(W, Hh)
    no_ray = ~rays[:, 4:7].any(axis=1)
    assert np.array_equal(no_ray, rho > 1)
    assert not rays[no_ray].any()
    if (W, Hh) != (1, 1):
        assert no_ray.any() and (~no_ray).any()
    if W % 2 == 0 and Hh % 2 == 0:                       # the centre pixel has rho == 0: f, not 0 / 0
        c = (Hh // 2) * W + W // 2
        assert rho[c] == 0 and np.array_equal(rays[c, 4:7], R.basis(CAM)[2])
    # at 180 degrees the rim looks sideways: cos(theta) ~ 0 at rho ~ 1
    _, _, f = R.basis(CAM)
    rim = (~no_ray) & (rho > 0.97)
    if rim.any():
        assert np.abs(rays[rim, 4:7].astype(np.float64) @ f.astype(np.float64)).max() < 0.06


def test_ortho_directions_are_all_equal_and_origins_span_the_plane():
    W, Hh = 67, 45
    rays = R.make_set("ortho", CAM, W, Hh, 2, aa_width=1.0, per_pixel=1).reshape(Hh, W, 8)
    f = R.basis(CAM)[2]
    assert (rays[..., 4:7].view(np.uint32) == f.view(np.uint32)).all()
    plain = R.make_set("ortho", CAM, W, Hh, 2).reshape(Hh, W, 8)
    assert np.array_equal(plain[0, 0, 0:3], CAM[1])      # s = t = 0: lower_left + 0 + 0
    assert np.any(plain[0, 1, 0:3] != plain[0, 0, 0:3]) and np.any(plain[1, 0, 0:3] != plain[0, 0, 0:3])


def test_make_rays_layout():
    W, Hh, n, stride = 8, 8, 3, 8 * 8 + 5
    buf = R.make_rays("fisheye", CAM, W, Hh, 4, n, stride, fill=7.0, aa_width=1.0)
    assert buf.shape == ((n - 1) * stride + 64, 8)
    for k in range(n):
        assert np.array_equal(buf[k * stride:k * stride + 64], R.make_set("fisheye", CAM, W, Hh, 4 + k, aa_width=1.0))
    assert (buf[64:stride] == 7.0).all() and (buf[stride + 64:2 * stride] == 7.0).all()      # gap records untouched
    one = R.make_rays("fisheye", CAM, W, Hh, 4, n, 0, aa_width=1.0)
    assert np.array_equal(one, R.make_set("fisheye", CAM, W, Hh, 4, aa_width=1.0))


# ---- the refusals Python makes itself ------------------------------------------------------------
def _bare_tracer():
    pt = object.__new__(tracer.PathTracer)               # no context: the checks below come before any library call
    pt._ctx, pt.width, pt.height = None, 8, 8
    return pt


def test_python_refuses_bad_arguments_without_a_device():
    torch = pytest.importorskip("torch")
    pt = _bare_tracer()
    cpu = torch.zeros((64, 8), dtype=torch.float32)
    for bad in ((-1, 1), (0, -1), (2 ** 32, 1), (0, 2 ** 32)):
        with pytest.raises(ValueError):
            pt.render_rays(bad[0], bad[1], 4096)
    with pytest.raises(ValueError):
        pt.render_rays(0, 1, 4096, frame_stride=2 ** 63)
    with pytest.raises(ValueError):
        pt.render_rays(0, 1, cpu)                        # host memory
    with pytest.raises(ValueError):
        pt.render_rays(0, 1, np.zeros((64, 8), F))       # neither a tensor nor a pointer
    with pytest.raises(ValueError):
        pt.render_guides_rays(cpu)
    with pytest.raises(ValueError):
        pt.render_guides_rays("rays")
    with pytest.raises(ValueError):
        pt.make_rays("pinhole", CAM, -1, 1, out=4096)
    with pytest.raises(ValueError):
        pt.make_rays("pinhole", CAM, 0, 2 ** 32, out=4096)
    with pytest.raises(ValueError):
        pt.make_rays("panorama", CAM, 0, 1, out=4096)    # an unknown model
    with pytest.raises(ValueError):
        pt.make_rays("pinhole", CAM, 0, 1, out=cpu)
    with pytest.raises(ValueError):
        tracer.PathTracer.ray_camera("cube", CAM)
    with pytest.raises(ValueError):
        tracer.PathTracer.ray_camera("pinhole", np.zeros(11, F))       # not twelve floats
    rc = tracer.PathTracer.ray_camera("fisheye", CAM, fov_deg=220.0, aa_width=1.0, per_pixel=1)
    assert (rc.model, rc.per_pixel, rc.reserved) == (3, 1, 0) and rc.fov_deg == 220.0 and list(rc.camera.eye) == list(CAM[0])


def test_session_refuses_a_lens_with_another_model():
    cam = session.CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, 1.0)
    s = session.InteractiveSession(object(), 8, 8, cam)
    with pytest.raises(ValueError):
        s.set_camera_model("cube")
    s.set_lens(1.0, 0.1, focus_distance=3.0)
    with pytest.raises(ValueError):
        s.set_camera_model("fisheye")
    s.set_camera_model("pinhole", per_pixel=True)
    assert s._model == ("pinhole", 180.0, 1)
