"""TEST INFRASTRUCTURE: a model's placement restated in numpy, independent of the host
library (pnrt_normal_matrix, pnrt_scene_add_mesh) and of the device kernel (pt_place.h).

Every operation is a float32 one, rounded on its own (numpy float32 arrays and scalars
never contract a product into a sum).  Matrices are the 16 column-major floats
pnrt_model_matrix writes: m[c, r] below is column c, row r.

    N = transpose(inverse(M)), the inverse in glm 0.9.9.8's compute_inverse<4, 4>
        expression order (func_matrix.inl)
    pos[r]    = (M[0][r] * p.x + M[1][r] * p.y) + (M[2][r] * p.z + M[3][r] * 1)
    normal[r] = (N[0][r] * n.x + N[1][r] * n.y) + (N[2][r] * n.z + N[3][r] * 1)
    uv copied"""
import numpy as np

F = np.float32


def inverse(M16) -> np.ndarray:
    """glm::inverse(mat4), (4, 4) indexed [column, row]."""
    m = np.ascontiguousarray(M16, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        c00 = m[2, 2] * m[3, 3] - m[3, 2] * m[2, 3]
        c02 = m[1, 2] * m[3, 3] - m[3, 2] * m[1, 3]
        c03 = m[1, 2] * m[2, 3] - m[2, 2] * m[1, 3]
        c04 = m[2, 1] * m[3, 3] - m[3, 1] * m[2, 3]
        c06 = m[1, 1] * m[3, 3] - m[3, 1] * m[1, 3]
        c07 = m[1, 1] * m[2, 3] - m[2, 1] * m[1, 3]
        c08 = m[2, 1] * m[3, 2] - m[3, 1] * m[2, 2]
        c10 = m[1, 1] * m[3, 2] - m[3, 1] * m[1, 2]
        c11 = m[1, 1] * m[2, 2] - m[2, 1] * m[1, 2]
        c12 = m[2, 0] * m[3, 3] - m[3, 0] * m[2, 3]
        c14 = m[1, 0] * m[3, 3] - m[3, 0] * m[1, 3]
        c15 = m[1, 0] * m[2, 3] - m[2, 0] * m[1, 3]
        c16 = m[2, 0] * m[3, 2] - m[3, 0] * m[2, 2]
        c18 = m[1, 0] * m[3, 2] - m[3, 0] * m[1, 2]
        c19 = m[1, 0] * m[2, 2] - m[2, 0] * m[1, 2]
        c20 = m[2, 0] * m[3, 1] - m[3, 0] * m[2, 1]
        c22 = m[1, 0] * m[3, 1] - m[3, 0] * m[1, 1]
        c23 = m[1, 0] * m[2, 1] - m[2, 0] * m[1, 1]
        v4 = lambda *a: np.array(a, F)  # noqa: E731
        fac0, fac1, fac2 = v4(c00, c00, c02, c03), v4(c04, c04, c06, c07), v4(c08, c08, c10, c11)
        fac3, fac4, fac5 = v4(c12, c12, c14, c15), v4(c16, c16, c18, c19), v4(c20, c20, c22, c23)
        vec0 = v4(m[1, 0], m[0, 0], m[0, 0], m[0, 0])
        vec1 = v4(m[1, 1], m[0, 1], m[0, 1], m[0, 1])
        vec2 = v4(m[1, 2], m[0, 2], m[0, 2], m[0, 2])
        vec3 = v4(m[1, 3], m[0, 3], m[0, 3], m[0, 3])
        inv0 = (vec1 * fac0 - vec2 * fac1) + vec3 * fac2
        inv1 = (vec0 * fac0 - vec2 * fac3) + vec3 * fac4
        inv2 = (vec0 * fac1 - vec1 * fac3) + vec3 * fac5
        inv3 = (vec0 * fac2 - vec1 * fac4) + vec2 * fac5
        sa, sb = v4(1, -1, 1, -1), v4(-1, 1, -1, 1)
        inv = np.stack([inv0 * sa, inv1 * sb, inv2 * sa, inv3 * sb]).astype(F)
        dot0 = m[0] * inv[:, 0]
        dot1 = (dot0[0] + dot0[1]) + (dot0[2] + dot0[3])
        one = F(1.0) / dot1
        out = inv * one
    assert out.dtype == F
    return out


def normal_matrix(M16) -> np.ndarray:
    """transpose(inverse(M)) as 16 column-major floats."""
    return np.ascontiguousarray(inverse(M16).T).reshape(16)


def _through(m, x, y, z):
    """Rows 0-2 of glm's mat4 * vec4(x, y, z, 1) for (n,) coordinate arrays: (n, 3)."""
    with np.errstate(all="ignore"):
        out = np.stack([(m[0, r] * x + m[1, r] * y) + (m[2, r] * z + m[3, r] * F(1.0)) for r in range(3)], axis=1)
    assert out.dtype == F
    return out


def place_ref(model8, M16) -> np.ndarray:
    """The (n, 8) world-space records of the (n, 8) model-space records under M."""
    rec = np.ascontiguousarray(model8, F).reshape(-1, 8)
    M = np.ascontiguousarray(M16, F).reshape(4, 4)
    Nm = normal_matrix(M16).reshape(4, 4)
    out = np.empty_like(rec)
    out[:, 0:3] = _through(M, rec[:, 0], rec[:, 1], rec[:, 2])
    out[:, 3:6] = _through(Nm, rec[:, 3], rec[:, 4], rec[:, 5])
    out[:, 6:8] = rec[:, 6:8]
    return out


def words8(vertices15) -> np.ndarray:
    """Floats 0-5 and 12-13 of (n, 15) packed records: what the device keeps of a vertex."""
    V = np.ascontiguousarray(vertices15, F).reshape(-1, 15)
    return np.ascontiguousarray(V[:, [0, 1, 2, 3, 4, 5, 12, 13]])


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F).view(np.uint32)
