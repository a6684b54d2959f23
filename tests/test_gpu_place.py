"""pnrt_define_model / pnrt_place_models: models moved on the device by a matrix.

The records the device holds afterwards (pnrt_read_vertices) equal the host library's
ModelOutput path (host.model_vertices) and the numpy restatement tests/place_ref.py, the
boxes pnrt_bvh_refit_cpu and tests/refit_ref.py, every image the CPU oracle rendering
host.refit_packed's scene -- all bit for bit, as tests/test_gpu_refit.py has them for
pnrt_update_vertices.  Frames are 48x32 or smaller at 1 spp."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest

import place_ref as P
import pyoracle
import refit_common as C
import refit_ref as R
from test_gpu_refit import camera, check_boxes, edited, oracle_sequence, same
from pnraytracing_amd import _native as N
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.session import InteractiveSession
from pnraytracing_amd.tracer import TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

MODES = (TRAVERSE_ZCULL, TRAVERSE_EXACT)
E_ARG, E_STATE = -1, -3
LIGHT_OPS = [H.translate(0, 5.54, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.02)]
# the model refit_common.edit moves: (mesh, the scene's own matrix, the edit's matrix)
MODELS = {
    "C2": (functools.partial(H.mesh_displaced_sphere, 24, 12, S.BUNNY_RADIUS, S.BUNNY_CENTER, 0.12, 0x5EED),
           [H.translate(0, 0, -2), H.scale(8)], [H.translate(0.9, 0.3, -1.6), H.scale(8)]),
    "C4": (H.mesh_teapot, [H.scale(0.2)], [H.rotate(40.0, 0, 1, 0), H.scale(0.2)]),
    "C1": (functools.partial(H.mesh_quad, 27.5), LIGHT_OPS, [H.translate(0, 5.0, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.035)]),
}


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


@functools.lru_cache(maxsize=None)
def model(name):
    """(first vertex, mesh, own matrix, edit's matrix) -- checked to be refit_common's model."""
    mesh, own, ops = MODELS[name]
    mesh = mesh()
    first, rec = C.edit(name)
    assert len(rec) == len(mesh.positions) and C.same_model_unmoved(name)[0] == first
    return first, mesh, H.model_matrix(own), H.model_matrix(ops)


def two_frames(pt):
    pt.reset_accum()
    pt.render(0, 2)
    return pt.read_accum()


def same_records(got, ref15, what):
    same(got, P.words8(ref15), what)


# ---- 1 unmoved ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C2", "C4"])
def test_own_matrix_changes_no_bit(pt, name):
    cfg = C.scene(name)
    p = cfg.packed
    first, mesh, own, _ = model(name)
    n = len(mesh.positions)
    pt.load(cfg)
    before = two_frames(pt)
    same_records(pt.read_vertices(0, len(p.vertices)), p.vertices, "records as uploaded")
    mid = pt.define_model(first, H.model_records(mesh))
    assert mid == 0
    same_records(pt.read_vertices(0, len(p.vertices)), p.vertices, "a definition changes nothing")
    pt.place_models([(mid, own)])
    same_records(pt.read_vertices(first, n), p.vertices[first:first + n], "the model's records under the scene's own matrix")
    same_records(pt.read_vertices(0, len(p.vertices)), p.vertices, "every record")
    same(pt.read_bvh_boxes(p.nodes), p.nodes, "boxes")
    same(two_frames(pt), before, f"{name}: two frames after the placement vs two frames before")
    assert before[..., :3].any()
    pt.place_models([(mid, own)], relight=True)           # the areas come back as the builder has them
    same(two_frames(pt), before, f"{name}: ... and with the areas recomputed")


# ---- 2 moved --------------------------------------------------------------------------------------------
def run_sequence(pt, name, mode, relight):
    """The material test's sequence: two still frames, the edit, the redraw, three still frames."""
    cfg = C.scene(name)
    first, rec = C.edit(name)
    _, mesh, _, _ = model(name)
    new = edited(cfg, first, rec)
    redraw, final = oracle_sequence(name)
    pt.load(cfg, mode)
    pt.reset_accum()
    sess = InteractiveSession(pt, C.W, C.Hh, camera(name))
    mid = sess.define_model(first, mesh)
    for _ in range(2):
        sess.frame(False)
    assert sess.move_model(mid, MODELS[name][2], relight=relight) == (1, 0)
    same(pt.read_accum(), redraw, f"{name} mode {mode}: the redraw frame after the placement")
    for _ in range(3):
        sess.frame(False)
    same(pt.read_accum(), final, f"{name} mode {mode}: still frames after the placement")
    same_records(pt.read_vertices(first, len(rec)), rec, "records vs host.model_vertices")
    same(pt.read_vertices(first, len(rec)), P.place_ref(H.model_records(mesh), model(name)[3]), "records vs place_ref")
    return check_boxes(pt, cfg.packed, new.packed)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["C2", "C4"])
def test_moved_model_matches_oracle(pt, name, mode):
    run_sequence(pt, name, mode, relight=False)


@pytest.mark.parametrize("name", ["C2", "C4"])
def test_moved_model_equals_update_vertices(pt, name):
    cfg = C.scene(name)
    first, rec = C.edit(name)
    boxes = run_sequence(pt, name, TRAVERSE_ZCULL, relight=False)
    img = pt.read_accum()
    with PathTracer(0) as other:
        other.load(cfg, TRAVERSE_ZCULL)
        other.reset_accum()
        sess = InteractiveSession(other, C.W, C.Hh, camera(name))
        for _ in range(2):
            sess.frame(False)
        sess.edit_vertices(first, rec)
        for _ in range(3):
            sess.frame(False)
        same(other.read_accum(), img, "images of the two contexts")
        same(other.read_bvh_boxes(cfg.packed.nodes), boxes, "boxes of the two contexts")
        same(other.read_vertices(first, len(rec)), pt.read_vertices(first, len(rec)), "records of the two contexts")


# ---- 3 no drift -----------------------------------------------------------------------------------------
def test_a_placement_is_defined_from_the_model_space_copy(pt):
    cfg = C.scene("C4")
    p = cfg.packed
    first, mesh, own, m2 = model("C4")
    n = len(mesh.positions)
    m1 = H.model_matrix([H.translate(0.3, 0.2, -0.1), H.rotate(77.0, 1, 1, 0), H.scale(0.17, 0.23, 0.2)])
    pt.load(cfg)
    mid = pt.define_model(first, H.model_records(mesh))
    pt.place_models([(mid, m2)])
    want, boxes = pt.read_vertices(0, len(p.vertices)), pt.read_bvh_boxes(p.nodes)
    pt.load(cfg)
    mid = pt.define_model(first, H.model_records(mesh))
    pt.place_models([(mid, m1)])
    assert np.any(P.bits(pt.read_vertices(first, n)) != P.bits(want[first:first + n]))
    pt.place_models([(mid, m2)])
    same(pt.read_vertices(0, len(p.vertices)), want, "M1 then M2 vs M2 alone")
    same(pt.read_bvh_boxes(p.nodes), boxes, "boxes, M1 then M2 vs M2 alone")
    # an update_vertices on the range in between is legal, and the next placement overwrites it
    pt.place_models([(mid, m1)])
    squashed = p.vertices[first:first + n].copy()
    squashed[:, 0:3] *= np.float32(0.5)
    pt.update_vertices(first, squashed)
    same_records(pt.read_vertices(first, n), squashed, "update_vertices on a defined model's range")
    pt.place_models([(mid, m2)])
    same(pt.read_vertices(0, len(p.vertices)), want, "M1, update_vertices, M2 vs M2 alone")
    same(pt.read_bvh_boxes(p.nodes), boxes, "boxes, M1, update_vertices, M2 vs M2 alone")


# ---- 4 several models in one call ------------------------------------------------------------------------
def test_two_models_in_one_call_equal_two_calls_and_the_oracle(pt):
    cfg = C.scene("C2")
    p = cfg.packed
    first, bunny, _, m_bunny = model("C2")
    nb = len(bunny.positions)
    quad = H.mesh_quad(27.5)
    wall_first = nb + 6                                   # the front wall: the second quad after the bunny
    wall_own = [H.translate(0, 2.75, -2.75), H.rotate(90.0, 1, 0, 0), H.scale(0.1)]
    same_records(P.words8(p.vertices[wall_first:wall_first + 6]), H.model_vertices(quad, wall_own), "the front wall is there")
    wall_ops = [H.translate(0.2, 2.75, -3.1), H.rotate(80.0, 1, 0, 0), H.scale(0.1)]
    m_wall = H.model_matrix(wall_ops)
    new = H.refit_packed(H.refit_packed(p, first, H.model_vertices(bunny, MODELS["C2"][2])), wall_first,
                         H.model_vertices(quad, wall_ops))
    ref, _ = pyoracle.Oracle(dataclasses.replace(cfg, packed=new)).render(0, 2)
    got = []
    for calls in ("one", "two", "two, the other order"):
        pt.load(cfg)
        a, b = pt.define_model(first, H.model_records(bunny)), pt.define_model(wall_first, H.model_records(quad))
        assert (a, b) == (0, 1)
        if calls == "one":
            pt.place_models([(b, m_wall), (a, m_bunny)])      # (the table's order is the call's, not the array's)
        elif calls == "two":
            pt.place_models([(a, m_bunny)])
            pt.place_models([(b, m_wall)])
        else:
            pt.place_models([(b, m_wall)])
            pt.place_models([(a, m_bunny)])
        same_records(pt.read_vertices(0, len(p.vertices)), new.vertices, f"{calls}: every record")
        check_boxes(pt, p, new)
        same(two_frames(pt), ref, f"{calls}: two frames vs the oracle")


@functools.lru_cache(maxsize=None)
def strips_scene():
    """C1 with an extra quad and a sphere strip, whose vertex ranges make three models of 1, 65 and 300
    vertices: concatenated, the prefix boundaries 1 and 66 fall inside the first wave and the 366
    vertices end inside the second block."""
    sb = H.SceneBuilder()
    S._cornell_walls(sb, H.Material(baseColor=(0.65, 0.65, 0.65)))
    quad = H.mesh_quad(27.5)
    strip = H.mesh_displaced_sphere(12, 7, 0.6, (0.0, 0.0, 0.0), 0.1, 0xBEEF)
    first_quad = 36
    sb.add_model(quad, [H.translate(0, 1.0, 0), H.scale(0.03)], H.Material(baseColor=(0.2, 0.4, 0.8)), "plate")
    sb.add_model(strip, [H.translate(0.5, 2.0, -0.5), H.scale(1.0)], H.Material(baseColor=(0.8, 0.4, 0.2)), "strip")
    cfg = S.SceneConfig("strips", sb.build(), S._cornell_camera(24, 16), 24, 16, 1, max_depth=4)
    assert len(strip.positions) >= 365 and len(cfg.packed.vertices) == first_quad + 6 + len(strip.positions)
    rq, rs = H.model_records(quad), H.model_records(strip)
    models = [(first_quad + 2, rq[2:3]), (first_quad + 6, rs[0:65]), (first_quad + 6 + 65, rs[65:365])]
    return cfg, models


def test_three_models_whose_boundaries_fall_inside_a_wave(pt):
    cfg, models = strips_scene()
    p = cfg.packed
    assert [len(r) for _, r in models] == [1, 65, 300]
    mats = [H.model_matrix([H.translate(0.1, 1.2, 0.3), H.scale(0.05)]),
            H.model_matrix([H.translate(0.4, 2.1, -0.4), H.rotate(20.0, 0, 1, 0), H.scale(1.1, 0.9, 1.0)]),
            H.model_matrix([H.translate(0.6, 1.9, -0.6), H.rotate(-35.0, 1, 0, 1), H.scale(-0.9, 1.0, 1.2)])]
    want = P.words8(p.vertices)
    for (first, rec), m in zip(models, mats):
        want[first:first + len(rec)] = P.place_ref(rec, m)
    V = p.vertices.copy()
    V[:, [0, 1, 2, 3, 4, 5, 12, 13]] = want
    for order in ((0, 1, 2), (2, 0, 1)):
        pt.load(cfg)
        ids = [pt.define_model(first, rec) for first, rec in models]
        assert ids == [0, 1, 2]
        pt.place_models([(ids[k], mats[k]) for k in order])
        same(pt.read_vertices(0, len(p.vertices)), want, f"order {order}: every record vs place_ref, vertex by vertex")
        got = pt.read_bvh_boxes(p.nodes)
        same(got, R.refit_ref(V, p.triangles, p.nodes), "boxes vs refit_ref")
        same(got, H.bvh_refit_cpu(V, p.triangles, p.nodes), "boxes vs pnrt_bvh_refit_cpu")


# ---- 5 relight ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_scaled_and_lowered_light_with_relight_matches_oracle(pt, mode):
    run_sequence(pt, "C1", mode, relight=True)
    cfg = C.scene("C1")
    new = edited(cfg, *C.edit("C1"))
    assert new.packed.lights_sum_area != cfg.packed.lights_sum_area
    # a later material edit uploads spans of the library's host copy of the light records: the copy is in step
    pt.update_materials(0, cfg.packed.materials)
    same(two_frames(pt), pyoracle.Oracle(new).render(0, 2)[0], "after update_materials")


def test_relight_false_keeps_the_areas_as_lights_none_does(pt):
    cfg = C.scene("C1")
    first, rec = C.edit("C1")
    _, mesh, _, m = model("C1")
    pt.load(cfg)
    mid = pt.define_model(first, H.model_records(mesh))
    pt.place_models([(mid, m)], relight=False)
    img = two_frames(pt)
    with PathTracer(0) as other:
        other.load(cfg)
        other.update_vertices(first, rec, lights=None)
        same(two_frames(other), img, "relight=False vs update_vertices(lights=None)")
    assert np.any(P.bits(img) != P.bits(pyoracle.Oracle(edited(cfg, first, rec)).render(0, 2)[0]))   # the areas matter
    pt.update_materials(0, cfg.packed.materials)
    same(two_frames(pt), img, "after update_materials")
    pt.place_models([(mid, m)], relight=True)
    same(two_frames(pt), pyoracle.Oracle(edited(cfg, first, rec)).render(0, 2)[0], "relight=True afterwards")


# ---- 6 the device form ----------------------------------------------------------------------------------
def test_model_defined_from_device_memory(pt):
    import torch
    cfg = C.scene("C4")
    first, rec = C.edit("C4")
    _, mesh, _, m = model("C4")
    pt.load(cfg)
    t = torch.from_numpy(H.model_records(mesh)).to("cuda")
    torch.cuda.synchronize()
    mid = ctypes.c_int(-5)
    rc = pt._lib.pnrt_define_model_device(pt._ctx, first, len(rec), ctypes.c_void_p(t.data_ptr() + 2), ctypes.byref(mid))
    assert rc == E_ARG and mid.value == -5 and b"4-byte aligned" in pt._lib.pnrt_last_error(pt._ctx)
    rc = pt._lib.pnrt_define_model_device(pt._ctx, first, len(rec), None, ctypes.byref(mid))
    assert rc == E_ARG and mid.value == -5 and b"NULL" in pt._lib.pnrt_last_error(pt._ctx)
    assert pt.define_model(first, t) == 0                 # nothing was kept by the refused calls
    del t
    pt.place_models([(0, m)])
    same_records(pt.read_vertices(first, len(rec)), rec, "records of a model defined from a device tensor")
    check_boxes(pt, cfg.packed, edited(cfg, first, rec).packed)


# ---- 7 refusals -----------------------------------------------------------------------------------------
def test_refusals_change_nothing(pt):
    cfg = C.scene("C1")
    p = cfg.packed
    nv = len(p.vertices)
    first, mesh, own, m = model("C1")
    rec8 = H.model_records(mesh)
    pt.load(cfg)
    before = two_frames(pt)
    assert pt.define_model(first, rec8) == 0
    lib, ctx = pt._lib, pt._ctx

    def refused(call, text, code=E_ARG):
        with pytest.raises(PnrtError, match=text) as e:
            call()
        assert e.value.code == code
        same_records(pt.read_vertices(0, nv), p.vertices, f"records after the refused call ({text})")
        same(pt.read_bvh_boxes(p.nodes), p.nodes, f"boxes after the refused call ({text})")

    def raw(entries, n=None, relight=0):
        arr = (N.Placement * max(len(entries), 1))()
        for k, (mid, mat, reserved) in enumerate(entries):
            arr[k].model, arr[k].reserved = mid, reserved
            arr[k].matrix[:] = np.asarray(mat, np.float32).tolist()
        pt._ck(lib.pnrt_place_models(ctx, arr, len(entries) if n is None else n, relight), "p")

    refused(lambda: pt.define_model(first + 2, rec8[:2]), "overlap model 0")           # an overlapping definition
    refused(lambda: pt.define_model(first - 3, rec8), "overlap model 0")
    refused(lambda: pt.define_model(nv - 2, rec8[:3]), "vertex range")                  # past the end
    refused(lambda: pt.define_model(-1, rec8[:2]), "vertex range")
    refused(lambda: pt.define_model(0, rec8[:0]), "at least one vertex")                # count < 1
    refused(lambda: pt._ck(lib.pnrt_define_model(ctx, 0, 2, None, ctypes.byref(ctypes.c_int())), "d"), "NULL")
    assert pt.define_model(0, rec8) == 1                   # the refused definitions kept nothing: the next id is 1
    inf = m.copy()
    inf[5] = np.inf
    nan = m.copy()
    nan[12] = np.nan
    refused(lambda: pt.place_models([(2, m)]), "placement 0 names the unknown model 2")
    refused(lambda: pt.place_models([(-1, m)]), "placement 0 names the unknown model -1")
    refused(lambda: pt.place_models([(0, m), (1, own), (0, own)]), "placement 2 names model 0 a second time")
    refused(lambda: pt.place_models([]), "placements a call")                           # n = 0
    refused(lambda: raw([(0, m, 0)], n=-1), "placements a call")
    refused(lambda: raw([(0, m, 0)], n=1025), "placements a call")                      # (refused before the array is read)
    refused(lambda: pt._ck(lib.pnrt_place_models(ctx, None, 1, 0), "p"), "NULL")
    refused(lambda: pt.place_models([(1, own), (0, inf)]), "placement 1: matrix float 5 is not finite")
    refused(lambda: pt.place_models([(0, nan)]), "placement 0: matrix float 12 is not finite")
    refused(lambda: pt.place_models([(0, H.model_matrix([H.scale(0)]))]), "placement 0: the matrix is singular")
    refused(lambda: raw([(0, m, 0), (1, own, 1)]), "placement 1: reserved")
    refused(lambda: raw([(0, m, 0)], relight=2), "relight is 0 or 1")
    refused(lambda: pt.place_models([(0, m)], relight=2), "relight is 0 or 1")
    refused(lambda: pt.read_vertices(nv - 1, 2), "vertex range")
    refused(lambda: pt.read_vertices(-1, 2), "vertex range")
    same(two_frames(pt), before, "the next image after every refused call")
    with PathTracer(0) as fresh:                          # before upload_scene
        for call in (lambda: fresh.define_model(0, rec8), lambda: fresh.place_models([(0, m)]), lambda: fresh.read_vertices(0, 1)):
            with pytest.raises(PnrtError, match="upload_scene first") as e:
                call()
            assert e.value.code == E_STATE
    pt.upload_scene(p)                                    # forgets every model
    refused(lambda: pt.place_models([(0, m)]), "placement 0 names the unknown model 0")
    assert pt.define_model(first, rec8) == 0
    pt.place_models([(0, own)])
    same(two_frames(pt), before, "and a placement under the scene's own matrix")


# ---- 8 non-finite positions ------------------------------------------------------------------------------
def test_non_finite_model_coordinates(pt):
    """As tests/test_gpu_refit.py's infinite box: an infinite coordinate switches the culling mode to the
    exact traversal, a NaN one reaches the record and enters no box; both images are the oracle's."""
    cfg = C.scene("C1")
    quad = H.mesh_quad(27.5)
    floor_ops = [H.scale(0.1)]
    same_records(P.words8(cfg.packed.vertices[0:6]), H.model_vertices(quad, floor_ops), "the floor is the first model")
    bad = H.Mesh(quad.positions.copy(), quad.normals, quad.texcoords, quad.indices)
    bad.positions[0, 0], bad.positions[1, 1] = np.inf, np.nan
    rec = H.model_vertices(bad, floor_ops)
    new = edited(cfg, 0, rec)
    assert np.isinf(new.packed.nodes[0, 3]) and not np.isnan(new.packed.nodes[:, 0:6]).any()
    assert np.isnan(rec[1, 0:3]).all() and np.isinf(rec[0, 0])
    ref, _ = pyoracle.Oracle(new).render(0, 2)
    for mode in MODES:
        pt.load(cfg, mode)
        mid = pt.define_model(0, H.model_records(bad))
        pt.place_models([(mid, H.model_matrix(floor_ops))])
        got, want = pt.read_vertices(0, 6), P.words8(rec)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any()
        assert np.array_equal(P.bits(got)[~np.isnan(want)], P.bits(want)[~np.isnan(want)])
        check_boxes(pt, cfg.packed, new.packed)
        same(two_frames(pt), ref, f"mode {mode}")


# ---- 9 staleness -----------------------------------------------------------------------------------------
def test_kept_records_and_guides_go_stale(pt):
    cfg = C.scene("C2")
    first, rec = C.edit("C2")
    _, mesh, _, m = model("C2")
    new = edited(cfg, first, rec)
    pt.load(cfg)
    mid = pt.define_model(first, H.model_records(mesh))
    pt.reset_accum()
    pt.render(0, 1)
    same(pt.read_accum(), pyoracle.Oracle(cfg).render(0, 1)[0], "frame 0 before")
    pt.render_guides()
    pt.denoise()
    pt.place_models([(mid, m)])
    with pytest.raises(PnrtError) as e:
        pt.denoise()
    assert e.value.code == E_STATE
    pt.reset_accum()
    pt.render(0, 1)                            # frame 0, the same camera: the primary records are not reused
    same(pt.read_accum(), pyoracle.Oracle(new).render(0, 1)[0], "frame 0 after")
    pt.render_guides()
    pt.denoise()
    from guides_common import camera_rays
    rays = camera_rays(cfg)
    ref = pyoracle.Oracle(new).intersect(rays, 0, 0)
    assert np.array_equal(pt.query_rays(rays)[:, :13], ref)
    assert np.any(ref != pyoracle.Oracle(cfg).intersect(rays, 0, 0))
