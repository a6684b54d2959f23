"""The BVH refit rule (tests/refit_ref.py) against the builder and against the host
library, bit for bit (no GPU needed):

* refit_ref on the unchanged C1, C2 (nu=24, nv=12) and C4 returns BuildBVH's own node
  array -- so "a refit with unchanged vertices changes no bit" is a test, and a refit
  tree is the node array the reference's shader would be handed for that topology;
* pnrt_bvh_refit_cpu equals refit_ref after the bunny was translated, the teapot rotated
  and C1's light scaled, and on the hand-made scene whose extremes tie as -0 / +0;
* pnrt_scene_relight reproduces the packed areas, light list and lights_sum_area."""
import numpy as np
import pytest

import refit_common as C
import refit_ref as R
from pnraytracing_amd import host as H

SCENES = ["C1", "C2", "C4"]


@pytest.mark.parametrize("name", SCENES)
def test_ref_on_unchanged_scene_is_the_builders_tree(name):
    p = C.scene(name).packed
    got = R.refit_ref(p.vertices, p.triangles, p.nodes)
    assert np.array_equal(R.bits(got), R.bits(p.nodes)), name
    assert {"C1": (12, 9), "C2": (588, 559), "C4": (5636, 5663)}[name] == (len(p.triangles), len(p.nodes))


@pytest.mark.parametrize("name", SCENES)
def test_host_library_on_unchanged_scene_is_the_builders_tree(name):
    p = C.scene(name).packed
    assert np.array_equal(R.bits(H.bvh_refit_cpu(p.vertices, p.triangles, p.nodes)), R.bits(p.nodes)), name


@pytest.mark.parametrize("name", SCENES)
def test_host_library_equals_ref_after_an_edit(name):
    p = C.scene(name).packed
    first, rec = C.edit(name)
    f0, same = C.same_model_unmoved(name)
    assert f0 == first and same.shape == rec.shape
    assert np.array_equal(R.bits(same), R.bits(p.vertices[first:first + len(rec)])), "the range is the model's"
    assert not np.array_equal(rec[:, 0:3], same[:, 0:3])
    new = H.refit_packed(p, first, rec)
    want = R.refit_ref(new.vertices, new.triangles, p.nodes)
    assert np.array_equal(R.bits(new.nodes), R.bits(want)), name
    assert not np.array_equal(R.bits(new.nodes[:, 0:6]), R.bits(p.nodes[:, 0:6])), "the edit moves boxes"
    assert np.array_equal(R.bits(new.nodes[:, 6:]), R.bits(p.nodes[:, 6:])), "topology untouched"
    assert np.array_equal(new.vertices[first:first + len(rec)], rec)
    assert np.array_equal(R.bits(p.vertices), R.bits(C.scene(name).packed.vertices)), "the input is not modified"
    # every triangle's vertices are inside its leaf's box and the root's
    idx = new.triangles[:, 0:3].astype(int)
    P = new.vertices[idx.reshape(-1), 0:3]
    assert (P >= new.nodes[0, 0:3]).all() and (P <= new.nodes[0, 3:6]).all()


def test_signed_zero_ties_keep_the_first():
    V, T, nodes, _ = R.signed_zero_scene()
    want = R.refit_ref(V, T, nodes)
    got = H.bvh_refit_cpu(V, T, nodes)
    assert np.array_equal(R.bits(got), R.bits(want))
    nz, pz = R.bits(np.float32(-0.0)), R.bits(np.float32(0.0))
    b = R.bits(want)
    assert b[1, 3] == nz and b[2, 0] == pz, "inside a leaf: max.x met as -0, +0 and min.x met as +0, -0"
    assert (b[1, 1], b[2, 1], b[0, 1]) == (pz, nz, pz), "min.y: the root keeps the left leaf's +0"
    assert (b[1, 2], b[2, 2], b[0, 2]) == (nz, pz, nz), "min.z: the root keeps the left leaf's -0"
    # the other order of the leaves: the root keeps the other sign
    swapped = nodes.copy()
    swapped[1, 8:10], swapped[2, 8:10] = (2, 4), (0, 2)
    want2 = R.refit_ref(V, T, swapped)
    assert np.array_equal(R.bits(H.bvh_refit_cpu(V, T, swapped)), R.bits(want2))
    assert (R.bits(want2)[0, 1], R.bits(want2)[0, 2]) == (nz, pz)


def test_nan_never_enters_a_box_and_empty_leaves_keep_theirs():
    V, T, nodes, _ = R.signed_zero_scene()
    V = V.copy()
    V[4, 0] = np.nan
    nd = np.zeros((5, 12), np.float32)          # root -> (interior over both leaves, empty leaf)
    nd[0, 6:10] = (0, 4, 0, 4)
    nd[1:4] = nodes
    nd[1, 7] = 3
    nd[4, 0:6] = (-9, -9, -9, 9, np.inf, 9)
    nd[4, 6:10] = (0, -1, 4, 4)
    want = R.refit_ref(V, T, nd)
    got = H.bvh_refit_cpu(V, T, nd)
    assert np.array_equal(R.bits(got), R.bits(want))
    assert not np.isnan(got[:, 0:6]).any()
    assert np.array_equal(R.bits(got[4]), R.bits(nd[4])) and got[0, 0] == -9 and got[0, 4] == np.inf


@pytest.mark.parametrize("name", SCENES)
def test_relight_reproduces_the_packed_scene(name):
    p = C.scene(name).packed
    T, L, sa = H.scene_relight(p.vertices, p.triangles, p.materials)
    assert np.array_equal(R.bits(T), R.bits(p.triangles)), "areas as ModelOutput computes them"
    assert np.array_equal(R.bits(L), R.bits(p.lights)) and len(L) > 0
    assert np.float32(sa) == np.float32(p.lights_sum_area)


def test_relight_after_scaling_the_light():
    p = C.scene("C1").packed
    first, rec = C.edit("C1")
    new = H.refit_packed(p, first, rec)
    assert np.array_equal(new.lights[:, 0], p.lights[:, 0])
    ratio = new.lights_sum_area / p.lights_sum_area
    assert abs(ratio - (0.035 / 0.02) ** 2) < 1e-4
    assert np.float32(new.lights[-1, 1]) == np.float32(new.lights_sum_area)


def test_argument_errors():
    p = C.scene("C1").packed
    with pytest.raises(H.HostError):
        H.bvh_refit_cpu(p.vertices[:3], p.triangles, p.nodes)           # a vertex index out of range
    bad = p.nodes.copy()
    bad[0, 7] = len(bad)
    with pytest.raises(H.HostError):
        H.bvh_refit_cpu(p.vertices, p.triangles, bad)
    with pytest.raises(H.HostError):
        H.scene_relight(p.vertices, p.triangles, p.materials[:1])
    with pytest.raises(ValueError):
        H.refit_packed(p, len(p.vertices) - 1, p.vertices[:2])
