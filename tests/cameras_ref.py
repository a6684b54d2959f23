"""A numpy restatement of pnrt_camera_sequence (include/pnrt_host.h), independent of the
host library: float64 arithmetic on the float32 inputs in the documented order, one
rounding to float32 per output component."""
import numpy as np

A = (0xDB4F0B91, 0xBBE05633, 0xA0F2EC77, 0x89E18285)


def u4(frame: int) -> np.ndarray:
    """The frame's four sequence numbers, (4,) float32 (exact)."""
    n = (frame + 1) & 0xFFFFFFFF
    return np.array([np.float32(((n * a) & 0xFFFFFFFF) >> 8) * np.float32(2.0 ** -24) for a in A], np.float32)


def _len(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def camera_sequence(cam12, width, height, first_frame, n_frames, aa_width=1.0, lens_radius=0.0, focus_distance=0.0):
    cam = np.asarray(cam12, np.float32).reshape(4, 3)
    eye, ll, hor, ver = (cam[i].astype(np.float64) for i in range(4))
    aa, radius, focus = (np.float64(np.float32(v)) for v in (aa_width, lens_radius, focus_distance))
    out = np.zeros((n_frames, 4, 3), np.float32)
    for k in range(n_frames):
        u = u4(first_frame + k).astype(np.float64)
        if radius > 0:
            c = ((ll + 0.5 * hor) + 0.5 * ver) - eye
            s = focus / _len(c)
            r = radius * np.sqrt(u[2])
            phi = (2.0 * np.pi) * u[3]
            a, b = r * np.cos(phi), r * np.sin(phi)
            out[k, 0] = ((eye + a * (hor / _len(hor))) + b * (ver / _len(ver))).astype(np.float32)
            llf, h2, v2 = eye + (ll - eye) * s, hor * s, ver * s
            out[k, 2], out[k, 3] = h2.astype(np.float32), v2.astype(np.float32)
        else:
            out[k, 0], out[k, 2], out[k, 3] = cam[0], cam[2], cam[3]
            llf, h2, v2 = ll, hor, ver
        if aa > 0:
            jx, jy = (u[0] - 0.5) * aa, (u[1] - 0.5) * aa
            out[k, 1] = ((llf + (jx / width) * h2) + (jy / height) * v2).astype(np.float32)
        elif radius > 0:
            out[k, 1] = llf.astype(np.float32)
        else:
            out[k, 1] = cam[1]
    return out.reshape(n_frames, 12)
