"""tests/place_ref.py -- the numpy restatement of a model's placement -- against the host
library: its normal matrix equals pnrt_normal_matrix, and its records equal floats 0-5
and 12-13 of host.model_vertices, the ModelOutput path tests/test_host_arrays.py pins to
the reference's model.hpp; bit for bit (no GPU needed)."""
import functools

import numpy as np
import pytest

import place_ref as P
import refit_common as C
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S

BUNNY = functools.partial(H.mesh_displaced_sphere, 24, 12, S.BUNNY_RADIUS, S.BUNNY_CENTER, 0.12, 0x5EED)
# (mesh, ops) of refit_common.edit and of refit_common.same_model_unmoved, and a matrix with a shear
# (a rotation between two unequal scales) and a negative scale
CASES = {
    "C2-edit": (BUNNY, [H.translate(0.9, 0.3, -1.6), H.scale(8)]),
    "C4-edit": (H.mesh_teapot, [H.rotate(40.0, 0, 1, 0), H.scale(0.2)]),
    "C1-edit": (functools.partial(H.mesh_quad, 27.5), [H.translate(0, 5.0, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.035)]),
    "C2-unmoved": (BUNNY, [H.translate(0, 0, -2), H.scale(8)]),
    "C4-unmoved": (H.mesh_teapot, [H.scale(0.2)]),
    "C1-unmoved": (functools.partial(H.mesh_quad, 27.5), [H.translate(0, 5.54, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.02)]),
    "shear-mirror": (BUNNY, [H.translate(-0.4, 1.1, 0.3), H.scale(1.5, 0.5, 1.0), H.rotate(33.0, 1, 2, 3), H.scale(-1.25, 2.0, 0.75)]),
}


def same(got, ref, what):
    bad = np.argwhere(P.bits(got) != P.bits(ref))
    assert len(bad) == 0, f"{what}: {len(bad)} words differ, first {bad[:5].tolist()}"


def test_the_cases_are_the_edits_of_refit_common():
    for name in ("C1", "C2", "C4"):
        for kind, fn in (("edit", C.edit), ("unmoved", C.same_model_unmoved)):
            mesh, ops = CASES[f"{name}-{kind}"]
            same(H.model_vertices(mesh(), ops), fn(name)[1], f"{name}-{kind}")


@pytest.mark.parametrize("case", list(CASES))
def test_normal_matrix_is_the_host_librarys(case):
    M = H.model_matrix(CASES[case][1])
    Nm = P.normal_matrix(M)
    assert Nm.dtype == np.float32 and np.isfinite(Nm).all()
    same(Nm, H.normal_matrix(M), case)


@pytest.mark.parametrize("case", list(CASES))
def test_records_are_model_outputs(case):
    mesh, ops = CASES[case]
    mesh = mesh()
    got = P.place_ref(H.model_records(mesh), H.model_matrix(ops))
    ref = P.words8(H.model_vertices(mesh, ops))
    same(got, ref, case)
    assert got.dtype == np.float32 and len(got) == len(mesh.positions)


def test_the_shear_is_one():
    """Its normal matrix is not a multiple of the matrix's upper 3x3, and it mirrors."""
    M = H.model_matrix(CASES["shear-mirror"][1]).reshape(4, 4)[:3, :3].astype(np.float64)
    Nm = H.normal_matrix(H.model_matrix(CASES["shear-mirror"][1])).reshape(4, 4)[:3, :3].astype(np.float64)
    assert np.linalg.det(M) < 0
    ratio = Nm / M
    assert ratio.max() - ratio.min() > 0.1


def test_singular_matrix_has_no_finite_normal_matrix():
    M = H.model_matrix([H.scale(0)])
    assert not np.isfinite(P.normal_matrix(M)).all() and not np.isfinite(H.normal_matrix(M)).all()


def test_negative_zero_and_nan_go_through_unchanged_in_kind():
    """A coordinate of -0 under a positive scale stays -0 in the product, and a NaN
    coordinate makes the position's three words NaN; the host library says the same."""
    mesh = H.Mesh(np.array([[-0.0, -0.0, -0.0], [np.nan, 1.0, 2.0], [1.0, 2.0, 3.0]], np.float32),
                  np.array([[-0.0, 1.0, -0.0], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]], np.float32),
                  np.array([[-0.0, 0.5], [np.nan, 1.0], [0.25, 0.75]], np.float32), np.arange(3, dtype=np.int32))
    ops = [H.scale(2.0)]
    got = P.place_ref(H.model_records(mesh), H.model_matrix(ops))
    ref = P.words8(H.model_vertices(mesh, ops))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = ~np.isnan(ref)
    assert np.array_equal(P.bits(got)[fin], P.bits(ref)[fin])
    # scale(2) of (-0, -0, -0): (-0 + -0) + (-0 + 0 * 1) = +0, as IEEE addition has it -- and as the host library has it;
    # the texcoord is copied: -0 stays -0
    assert P.bits(got[0, 6]) == P.bits(np.float32(-0.0))
    assert np.isnan(got[1, 0:3]).all() and np.isnan(got[1, 3:6]).all() and np.isnan(got[1, 6])
    assert not np.isnan(got[2]).any() and not np.isnan(got[0]).any()
    # under a matrix whose last column is -0 the position's -0 survives the sums
    M = H.model_matrix(ops).copy()
    M[12:15] = np.float32(-0.0)
    got = P.place_ref(H.model_records(mesh), M)
    assert np.array_equal(P.bits(got[0, 0:3]), P.bits(np.full(3, -0.0, np.float32)))
