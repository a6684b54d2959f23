"""pnrt_camera_sequence (libpnrt_host.so) against tests/cameras_ref.py, the numpy restatement
of include/pnrt_host.h's definition, and the properties that make the sequence a pixel
filter and a thin lens (no GPU needed).

Tolerances: the sequence numbers and every output without a lens are compared bitwise.
With a lens each component may differ from the restatement by 1 float ulp: the two
sides call different double sin / cos, whose last bit may differ and can move a
rounding to float by one step."""
import numpy as np
import pytest

import cameras_ref as R
from pnraytracing_amd import host as H

W, HGT = 40, 24
CAM = H.camera_update((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, np.float32(W) / np.float32(HGT)).reshape(12)
# a camera off every axis, so no component is trivially zero
CAM2 = H.camera_update((1.5, 3.1, 6.2), (-0.3, 2.2, -0.7), (0.1, 1, 0.05), 38.0, np.float32(W) / np.float32(HGT)).reshape(12)
FIRSTS = (0, 7, 0xFFFFFF - 2, 0xFFFFFFF0)
UNIT = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0], np.float32)     # eye above the unit square


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulps(a, b):
    """Distance in float32 steps between same-signed finite values (0 for +-0 pairs)."""
    def key(x):
        i = bits(x).astype(np.int64)
        return np.where(i & 0x80000000, 0x80000000 - i, i)
    return np.abs(key(a) - key(b))


def test_sequence_numbers_are_exact():
    """u_k through the library: a 1 x 1 frame with hor = (1, 0, 0), ver = (0, 1, 0), ll = 0 and
    aa_width = 1 has ll' = (u1 - 0.5, u2 - 0.5, 0), every step exact."""
    cam = UNIT
    for first in FIRSTS:
        got = H.camera_sequence(cam, 1, 1, first, 12, aa_width=1.0)
        for k in range(12):
            u = R.u4(first + k)
            assert 0.0 <= u.min() and u.max() < 1.0
            assert np.array_equal(bits(got[k, 3:5]), bits(u[:2] - np.float32(0.5)))
    # the definition itself, spelled out once: frame 0 -> n = 1 -> A_k >> 8
    assert np.array_equal(R.u4(0), np.array([a >> 8 for a in R.A], np.float32) * np.float32(2.0 ** -24))
    # n = f + 1 wraps in 32 bits
    assert np.array_equal(R.u4(0xFFFFFFFF), np.zeros(4, np.float32))


@pytest.mark.parametrize("cam", [CAM, CAM2], ids=["cornell", "oblique"])
@pytest.mark.parametrize("aa", [0.0, 0.5, 1.0, 2.0])
def test_pinhole_outputs_are_bitwise(cam, aa):
    for first in FIRSTS:
        got = H.camera_sequence(cam, W, HGT, first, 16, aa_width=aa)
        ref = R.camera_sequence(cam, W, HGT, first, 16, aa_width=aa)
        assert np.array_equal(bits(got), bits(ref))
        # eye, horizontal and vertical are copies
        assert np.array_equal(bits(got[:, [0, 1, 2, 6, 7, 8, 9, 10, 11]]), np.tile(bits(cam[[0, 1, 2, 6, 7, 8, 9, 10, 11]]), (16, 1)))
        if aa == 0.0:
            assert np.array_equal(bits(got), np.tile(bits(cam), (16, 1)))       # the input camera, every frame
        else:
            assert (bits(got[:, 3:6]) != bits(cam[3:6])).any()


def test_zero_zero_returns_negative_zero_and_odd_bits_untouched():
    cam = CAM2.copy()
    cam[4] = np.float32(-0.0)
    got = H.camera_sequence(cam, W, HGT, 3, 5, aa_width=0.0, lens_radius=0.0, focus_distance=0.0)
    assert np.array_equal(bits(got), np.tile(bits(cam), (5, 1)))


@pytest.mark.parametrize("cam", [CAM, CAM2], ids=["cornell", "oblique"])
@pytest.mark.parametrize("aa", [0.0, 1.0])
def test_lens_outputs_within_one_ulp(cam, aa):
    for first in FIRSTS:
        got = H.camera_sequence(cam, W, HGT, first, 32, aa_width=aa, lens_radius=0.11, focus_distance=6.5)
        ref = R.camera_sequence(cam, W, HGT, first, 32, aa_width=aa, lens_radius=0.11, focus_distance=6.5)
        d = ulps(got, ref)
        print(f"first {first:#x} aa {aa}: max {d.max()} ulp, {np.count_nonzero(d)} of {d.size} components differ")
        assert d.max() <= 1
        # horizontal, vertical (no sin / cos in them) are bitwise
        assert np.array_equal(bits(got[:, 6:]), bits(ref[:, 6:]))


def cells(u, v):
    c = np.zeros((4, 4), int)
    for a, b in zip(u, v):
        c[int(a * 4), int(b * 4)] += 1
    return c


def test_stratification():
    """Cell counts of a 4 x 4 grid over (u1, u2) and (u3, u4), from the library's output:
    (u1, u2) read back from the pixel shift as above, (u3, u4) from the lens point's polar
    coordinates in the (hor, ver) plane (to ~1e-6, far from a cell edge's effect on the bounds)."""
    cam = UNIT
    got = H.camera_sequence(cam, 1, 1, 0, 256, aa_width=1.0)
    u1, u2 = got[:, 3].astype(np.float64) + 0.5, got[:, 4].astype(np.float64) + 0.5
    ref = np.array([R.u4(f) for f in range(256)])
    assert np.array_equal(u1.astype(np.float32), ref[:, 0]) and np.array_equal(u2.astype(np.float32), ref[:, 1])
    c64, c256 = cells(u1[:64], u2[:64]), cells(u1, u2)
    assert 2 <= c64.min() and c64.max() <= 6, c64
    assert 13 <= c256.min() and c256.max() <= 19, c256
    # the lens dimensions: eye' - eye = r (cos phi, sin phi) in the unit (hor, ver) frame, r = R sqrt(u3), phi = 2 pi u4
    lens = H.camera_sequence(cam, 1, 1, 0, 256, aa_width=0.0, lens_radius=0.5, focus_distance=1.0)
    dx, dy = lens[:, 0].astype(np.float64) - 0.0, lens[:, 1].astype(np.float64) - 0.0
    u3 = (dx * dx + dy * dy) / 0.25
    u4 = (np.arctan2(dy, dx) / (2 * np.pi)) % 1.0
    assert np.abs(u3 - ref[:, 2]).max() < 1e-5
    d4 = np.abs(u4 - ref[:, 3])
    assert np.minimum(d4, 1 - d4).max() < 1e-4
    c64, c256 = cells(ref[:64, 2], ref[:64, 3]), cells(ref[:, 2], ref[:, 3])
    assert 3 <= c64.min() and c64.max() <= 5, c64
    assert 12 <= c256.min() and c256.max() <= 18, c256


@pytest.mark.parametrize("cam", [CAM, CAM2], ids=["cornell", "oblique"])
def test_lens_points_lie_on_the_disc(cam):
    radius = 0.2
    got = H.camera_sequence(cam, W, HGT, 0, 128, aa_width=1.0, lens_radius=radius, focus_distance=5.0).astype(np.float64)
    c = cam.astype(np.float64)
    eye, hor, ver = c[0:3], c[6:9], c[9:12]
    d = got[:, 0:3] - eye
    assert (np.linalg.norm(d, axis=1) <= radius * (1 + 1e-6)).all()
    assert (np.linalg.norm(d, axis=1) > 0).all() and len(np.unique(bits(got[:, 0:3].astype(np.float32)), axis=0)) == 128
    n = np.cross(hor, ver)
    n /= np.linalg.norm(n)
    assert np.abs(d @ n).max() < 1e-6                # in the plane spanned by hor and ver


@pytest.mark.parametrize("cam", [CAM, CAM2], ids=["cornell", "oblique"])
def test_focal_plane_centre_stays_put(cam):
    """The point at the focus distance on the view axis projects to the same (s, t) in
    every frame's camera (aa_width = 0: no pixel shift on top): P = ll' + s hor' + t ver'
    on the frame's own image plane, which holds P itself."""
    focus = 6.5
    got = H.camera_sequence(cam, W, HGT, 0, 64, aa_width=0.0, lens_radius=0.3, focus_distance=focus).astype(np.float64)
    c = cam.astype(np.float64)
    eye, ll, hor, ver = c[0:3], c[3:6], c[6:9], c[9:12]
    centre = ll + 0.5 * hor + 0.5 * ver - eye
    P = eye + centre * (focus / np.linalg.norm(centre))
    for row in got:
        e, l, h, v = row[0:3], row[3:6], row[6:9], row[9:12]
        # the ray from e through P meets the frame's image plane l + s h + t v
        n = np.cross(h, v)
        tt = ((l - e) @ n) / ((P - e) @ n)
        q = e + (P - e) * tt - l
        s, t = (q @ h) / (h @ h), (q @ v) / (v @ v)
        assert abs(s - 0.5) < 1e-5 and abs(t - 0.5) < 1e-5, (s, t)
        assert abs(tt - 1.0) < 1e-5                  # the image plane IS the plane in focus


def test_refusals():
    ok = dict(aa_width=1.0, lens_radius=0.1, focus_distance=5.0)
    H.camera_sequence(CAM, W, HGT, 0, 2, **ok)
    bad = [dict(ok, aa_width=-1.0), dict(ok, aa_width=float("nan")), dict(ok, aa_width=float("inf")),
           dict(ok, lens_radius=-0.1), dict(ok, lens_radius=float("nan")), dict(ok, lens_radius=float("inf")),
           dict(ok, focus_distance=0.0), dict(ok, focus_distance=-2.0), dict(ok, focus_distance=float("nan")),
           dict(ok, focus_distance=float("inf"))]
    for kw in bad:
        with pytest.raises(H.HostError):
            H.camera_sequence(CAM, W, HGT, 0, 2, **kw)
    # the focus distance is not looked at without a lens
    H.camera_sequence(CAM, W, HGT, 0, 2, aa_width=1.0, lens_radius=0.0, focus_distance=float("nan"))
    for w, h in ((0, HGT), (W, 0), (-3, HGT)):
        with pytest.raises(H.HostError):
            H.camera_sequence(CAM, w, h, 0, 2, **ok)
    # a degenerate plane: zero horizontal, zero vertical, the eye on the plane's centre, a non-finite component
    for i, v in ((slice(6, 9), 0.0), (slice(9, 12), 0.0), (0, float("nan")), (7, float("inf"))):
        cam = CAM.copy()
        cam[i] = v
        with pytest.raises(H.HostError):
            H.camera_sequence(cam, W, HGT, 0, 2, **ok)
    cam = UNIT.copy()
    cam[0:3] = (0.5, 0.5, 0.0)                       # the eye in the plane's centre: |c| = 0
    with pytest.raises(H.HostError):
        H.camera_sequence(cam, W, HGT, 0, 2, **ok)


def test_refusals_of_the_c_entry_point():
    import ctypes
    from pnraytracing_amd import _native as N
    lib = N.host_lib()
    out = np.zeros(24, np.float32)
    p = N.LensParams(1.0, 0.0, 0.0, 0)
    assert lib.pnrt_camera_sequence(N.fptr(CAM), W, HGT, ctypes.byref(p), 0, 2, N.fptr(out)) == 0
    assert lib.pnrt_camera_sequence(None, W, HGT, ctypes.byref(p), 0, 2, N.fptr(out)) == -1
    assert lib.pnrt_camera_sequence(N.fptr(CAM), W, HGT, None, 0, 2, N.fptr(out)) == -1
    assert lib.pnrt_camera_sequence(N.fptr(CAM), W, HGT, ctypes.byref(p), 0, 2, None) == -1
    p.reserved = 1
    assert lib.pnrt_camera_sequence(N.fptr(CAM), W, HGT, ctypes.byref(p), 0, 2, N.fptr(out)) == -1
    assert b"reserved" in lib.pnrt_host_last_error()
