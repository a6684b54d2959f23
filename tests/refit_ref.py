"""TEST INFRASTRUCTURE: the BVH refit rule restated in numpy, independent of the
host library (pnrt_bvh_refit_cpu) and of the device kernels (pt_refit.h).

A loop over the pre-order ids, descending -- every child's id is above its
parent's -- with the two comparisons of the reference's Bound::Union as the host
library's min and max evaluate them:

    min(x, y) = y if y < x else x        max(x, y) = y if x < y else x

so on a tie (-0 against +0) the earlier operand stays, and a NaN never enters a
box.  A non-empty leaf is the fold of its triangles in ascending order, vertices
p0, p1, p2, from (FLT_MAX, -FLT_MAX); an interior node is fold(left box, right
box); an empty leaf keeps its box."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(F).max


def fmin(x, y):
    return np.where(y < x, y, x)


def fmax(x, y):
    return np.where(x < y, y, x)


def refit_ref(vertices, triangles, nodes) -> np.ndarray:
    """A copy of the (nn, 12) node array with floats 0-5 of every node refit."""
    V = np.ascontiguousarray(vertices, F).reshape(-1, 15)
    T = np.ascontiguousarray(triangles, F).reshape(-1, 6)
    out = np.array(nodes, F, order="C").reshape(-1, 12)
    idx = T[:, 0:3].astype(np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(len(out) - 1, -1, -1):
            rc, s0, e0 = (int(out[i, k]) for k in (7, 8, 9))
            if rc == -1:
                if s0 == e0:
                    continue
                lo, hi = np.full(3, FLT_MAX, F), np.full(3, -FLT_MAX, F)
                for p in V[idx[s0:e0].reshape(-1), 0:3]:      # p0, p1, p2 of each triangle in turn
                    lo, hi = fmin(lo, p), fmax(hi, p)
            else:
                lo, hi = fmin(out[i + 1, 0:3], out[rc, 0:3]), fmax(out[i + 1, 3:6], out[rc, 3:6])
            out[i, 0:3], out[i, 3:6] = lo, hi
    return out


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, F).view(np.uint32)


def signed_zero_scene():
    """A hand-made two-leaf scene whose minimal and maximal coordinates tie as -0 and +0,
    in both orders: (vertices (12, 15), triangles (4, 6), nodes (3, 12), materials (1, 18)).

    Inside a leaf: leaf [0, 2) lies in x <= 0 and meets its maximal x as -0 first, +0
    second (the box keeps -0); leaf [2, 4) lies in x >= 0 and meets its minimal x as +0
    first, -0 second (keeps +0).  Between the leaves, at the root: min.y is +0 on the left
    and -0 on the right (the root keeps +0, where a minimum that orders the zeros would
    say -0), min.z is -0 on the left and +0 on the right (keeps -0)."""
    nz, pz = F(-0.0), F(0.0)
    P = np.array([
        # leaf 0: x in [-1, 0], y in [0, 1], z in [0, 0.5]
        [-1, pz, nz], [nz, 1, 0.5], [-1, 1, 0.5],
        [-1, nz, pz], [pz, 1, 0.5], [-1, 1, 0.25],
        # leaf 1: x in [0, 1], y in [0, 1], z in [0, 0.5]
        [pz, nz, pz], [1, 1, 0.5], [1, pz, 0.5],
        [nz, pz, nz], [1, 1, 0.5], [1, pz, 0.25],
    ], F)
    V = np.zeros((12, 15), F)
    V[:, 0:3] = P
    V[:, 5] = 1.0                                            # normal +z
    T = np.zeros((4, 6), F)
    T[:, 0:3] = np.arange(12, dtype=F).reshape(4, 3)
    T[:, 4] = -1
    M = np.zeros((1, 18), F)
    M[0, 3:6] = 0.7
    M[0, 10], M[0, 16] = 0.5, 1.0
    nodes = np.zeros((3, 12), F)
    nodes[0, 6:10] = (0, 2, 0, 4)
    nodes[1, 6:10] = (0, -1, 0, 2)
    nodes[2, 6:10] = (0, -1, 2, 4)
    return V, T, nodes, M
