"""A numpy restatement of pnrt_make_rays (include/pnrt.h), independent
of the library: binary32 arithmetic, every product and sum rounded on its own, in the
documented order; sine and cosine are PN-libm's through the oracle (pyoracle.math_eval);
division and sqrt are IEEE (numpy's)."""
import numpy as np

import pyoracle

F = np.float32
A = (0xDB4F0B91, 0xBBE05633, 0xA0F2EC77, 0x89E18285)
MODELS = ("pinhole", "ortho", "equirect", "fisheye")
TWO_PI, PI, DEG = F(6.2831855), F(3.1415927), F(0.017453292)
HALF, ONE, TWO = F(0.5), F(1.0), F(2.0)


def wang_hash(seed):
    """pt_common.h's wang_hash of uint32 seeds (ray_tracing.comp:499-507): the value returned."""
    s = np.asarray(seed, np.uint64) & 0xFFFFFFFF
    s = (s ^ 61) ^ (s >> 16)
    s = (s * 9) & 0xFFFFFFFF
    s = s ^ (s >> 4)
    s = (s * 0x27d4eb2d) & 0xFFFFFFFF
    s = s ^ (s >> 15)
    return s.astype(np.uint32)


def hashes(width, height, per_pixel):
    """h_i of every pixel: (4, height * width) uint32 -- zeros, or wang_hash(4 * (y * width + x) + i)."""
    p = np.arange(width * height, dtype=np.uint64)
    if not per_pixel:
        return np.zeros((4, len(p)), np.uint32)
    return np.stack([wang_hash(4 * p + i) for i in range(4)])


def u_samples(frame, h):
    """u_i = (float)(((n * A_i + h_i) & 0xFFFFFFFF) >> 8) * 2^-24, n = frame + 1: h (4, ...) uint32 -> (4, ...) float32."""
    n = (frame + 1) & 0xFFFFFFFF
    h = np.asarray(h, np.uint64)
    out = [(((n * a + h[i]) & 0xFFFFFFFF) >> 8).astype(F) * F(2.0 ** -24) for i, a in enumerate(A)]
    return np.stack(out).astype(F)


def sincos(x):
    x = np.ascontiguousarray(x, F)
    return pyoracle.math_eval(0, x.ravel()).reshape(x.shape), pyoracle.math_eval(1, x.ravel()).reshape(x.shape)


# ---- GLSL vectors over (..., 3) float32 arrays, the library's operation order (pt_common.h) ----
def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)


def normalize(a):
    return a / np.sqrt(dot(a, a))[..., None]


def smul(s, a):
    return np.asarray(s, F)[..., None] * a


def basis(cam):
    """r, u, f of a (4, 3) camera."""
    hor, ver = cam[2], cam[3]
    return normalize(hor), normalize(ver), normalize(cross(ver, hor))


def make_set(model, cam12, width, height, frame, fov_deg=180.0, aa_width=0.0, lens_radius=0.0, focus_distance=0.0,
             per_pixel=0):
    """One set: (height * width, 8) float32 records (origin, 0, direction, 0) of frame `frame`."""
    model = MODELS.index(model) if isinstance(model, str) else int(model)
    cam = np.asarray(cam12, F).reshape(4, 3)
    E, L, Hh, Vv = cam
    aa, radius, focus, fov = F(aa_width), F(lens_radius), F(focus_distance), F(fov_deg)
    npix = width * height
    p = np.arange(npix)
    x, y = (p % width).astype(F), (p // width).astype(F)
    u = u_samples(frame, hashes(width, height, per_pixel))
    s, t = x / F(width), y / F(height)
    if aa > 0:
        s = s + ((u[0] - HALF) * aa) / F(width)
        t = t + ((u[1] - HALF) * aa) / F(height)
    O = np.broadcast_to(E, (npix, 3)).astype(F).copy()
    D = np.zeros((npix, 3), F)
    with np.errstate(invalid="ignore", divide="ignore"):
        if model == 0:
            Lc, Hc, Vc = L, Hh, Vv
            if radius > 0:
                c = ((L + HALF * Hh) + HALF * Vv) - E
                sc = focus / np.sqrt(dot(c, c))
                r = radius * np.sqrt(u[2])
                sn, cs = sincos(TWO_PI * u[3])
                a, b = r * cs, r * sn
                O = (E + smul(a, Hh / np.sqrt(dot(Hh, Hh)))) + smul(b, Vv / np.sqrt(dot(Vv, Vv)))
                Lc, Hc, Vc = E + (L - E) * sc, Hh * sc, Vv * sc
            D = normalize(((Lc + smul(s, Hc)) + smul(t, Vc)) - O)
        else:
            rr, uu, f = basis(cam)
            if model == 1:
                O = (L + smul(s, Hh)) + smul(t, Vv)
                D = np.broadcast_to(f, (npix, 3)).astype(F).copy()
            elif model == 2:
                sp, cp = sincos((s - HALF) * TWO_PI)
                st, ct = sincos((t - HALF) * PI)
                D = normalize((smul(ct * sp, rr) + smul(st, uu)) + smul(ct * cp, f))
            elif model == 3:
                a, b = TWO * s - ONE, TWO * t - ONE
                rho = np.sqrt(a * a + b * b)
                st, ct = sincos(rho * ((fov * DEG) * HALF))
                q = smul(a / rho, rr) + smul(b / rho, uu)
                D = normalize(smul(st, q) + smul(ct, f))
                D[rho == 0] = f
                D[rho > 1] = 0
                O[rho > 1] = 0
            else:
                raise ValueError(f"unknown model {model}")
    out = np.zeros((npix, 8), F)
    out[:, 0:3], out[:, 4:7] = O, D
    return out


def make_rays(model, cam12, width, height, first_frame, n_sets, frame_stride=None, fill=None, **params):
    """pnrt_make_rays' buffer: ((n_sets - 1) * frame_stride + width * height, 8) float32; gap records
    hold `fill` (the buffer's content before the call).  frame_stride 0: the set of first_frame."""
    npix = width * height
    if frame_stride is None:
        frame_stride = npix if n_sets > 1 else 0
    if frame_stride == 0:
        return make_set(model, cam12, width, height, first_frame, **params)
    out = np.full(((n_sets - 1) * frame_stride + npix, 8), np.nan if fill is None else fill, F)
    for k in range(n_sets):
        out[k * frame_stride:k * frame_stride + npix] = make_set(model, cam12, width, height, (first_frame + k) & 0xFFFFFFFF, **params)
    return out


def fisheye_rho(width, height):
    """rho of every pixel of an un-jittered fisheye set, (height * width,) float32."""
    p = np.arange(width * height)
    a = TWO * ((p % width).astype(F) / F(width)) - ONE
    b = TWO * ((p // width).astype(F) / F(height)) - ONE
    return np.sqrt(a * a + b * b)
