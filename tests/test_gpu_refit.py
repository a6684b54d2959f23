"""pnrt_update_vertices: in-place geometry edits with the BVH refit on the device.

The boxes the device holds (pnrt_read_bvh_boxes) equal pnrt_bvh_refit_cpu and the numpy
restatement tests/refit_ref.py bit for bit; every image equals the CPU oracle rendering
the edited scene -- host.refit_packed: the new vertices, areas and lights under the REFIT
node array, which is the contract (a rebuilt tree may render other bits) -- bit for bit.
Frames are 48x32 or smaller at 1 spp."""
import dataclasses
import functools

import numpy as np
import pytest

import pyoracle
import refit_common as C
import refit_ref as R
from test_gpu_limits import chain_config, empty_leaf_c1, root_leaf_scene, with_nodes, chain_nodes
from pnraytracing_amd import _native as N
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.session import CameraController, InteractiveSession
from pnraytracing_amd.tracer import TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

MODES = (TRAVERSE_ZCULL, TRAVERSE_EXACT)
E_ARG, E_STATE = -1, -3
CAMERAS = {"C1": ((0, 2.8, 7), (0, 2.8, 0)), "C2": ((0, 2.8, 7), (0, 2.8, 0)), "C4": ((0, 5, 5), (0, 0, 0))}


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def same(got, ref, what):
    bad = np.argwhere(np.any(R.bits(got) != R.bits(ref), axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first {bad[:5].tolist()}"


def edited(cfg, first, rec):
    return dataclasses.replace(cfg, packed=H.refit_packed(cfg.packed, first, rec))


def check_boxes(pt, old, new):
    """Device boxes == pnrt_bvh_refit_cpu (new.nodes) == refit_ref; floats 6-11 are the caller's."""
    got = pt.read_bvh_boxes(old.nodes)
    same(got, new.nodes, "device boxes vs pnrt_bvh_refit_cpu")
    same(got, R.refit_ref(new.vertices, new.triangles, old.nodes), "device boxes vs refit_ref")
    return got


def camera(name):
    eye, centre = CAMERAS[name]
    return CameraController(eye, centre, (0, 1, 0), 45.0, np.float32(C.W) / np.float32(C.Hh))


def set_oracle_frame(orc, cam, depth):
    f = orc.frame
    f.eye[:], f.lower_left[:], f.horizontal[:], f.vertical[:] = (list(map(float, r)) for r in cam.uniforms())
    f.max_bounce_depth = depth


@functools.lru_cache(maxsize=None)
def oracle_sequence(name):
    """The material test's sequence on the oracle: two still frames of the old scene, the
    edit with its depth-1 redraw, three still frames.  (image after the redraw, at the end)"""
    cfg = C.scene(name)
    new = edited(cfg, *C.edit(name))
    cam = camera(name)
    acc = np.zeros((C.Hh, C.W, 4), np.float32)
    orc_old, orc_new = pyoracle.Oracle(cfg), pyoracle.Oracle(new)
    for fc in range(2):
        set_oracle_frame(orc_old, cam, 4)
        orc_old.render(fc, 1, accum=acc)
    set_oracle_frame(orc_new, cam, 1)
    orc_new.render(0, 1, accum=acc)
    redraw = acc.copy()
    for fc in range(3):
        set_oracle_frame(orc_new, cam, 4)
        orc_new.render(fc, 1, accum=acc)
    assert np.any(R.bits(redraw) != R.bits(acc))
    return redraw, acc.copy()


def run_sequence(pt, name, mode, form, lights):
    cfg = C.scene(name)
    first, rec = C.edit(name)
    new = edited(cfg, first, rec)
    redraw, final = oracle_sequence(name)
    pt.load(cfg, mode)
    pt.reset_accum()
    sess = InteractiveSession(pt, C.W, C.Hh, camera(name))
    for _ in range(2):
        sess.frame(False)
    kw = {"lights": new.packed.lights, "lights_sum_area": new.packed.lights_sum_area} if lights else {}
    if form == "host":
        assert sess.edit_vertices(first, rec, **kw) == (1, 0)
    else:
        import torch
        t = torch.from_numpy(np.ascontiguousarray(rec)).to("cuda")
        torch.cuda.synchronize()
        pt.update_vertices_device(first, len(rec), t.data_ptr(), **kw)
        sess.frame(True)
    same(pt.read_accum(), redraw, f"{name} mode {mode} {form}: the redraw frame after the edit")
    for _ in range(3):
        sess.frame(False)
    same(pt.read_accum(), final, f"{name} mode {mode} {form}: still frames after the edit")
    check_boxes(pt, cfg.packed, new.packed)


# ---- unchanged vertices --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C1", "C2", "C4"])
def test_unchanged_vertices_change_no_bit(pt, name):
    cfg = C.scene(name)
    p = cfg.packed
    pt.load(cfg)
    pt.reset_accum()
    pt.render(0, 2)
    before = pt.read_accum()
    same(pt.read_bvh_boxes(p.nodes), p.nodes, "boxes as uploaded")
    pt.update_vertices(0, p.vertices)
    same(pt.read_bvh_boxes(p.nodes), p.nodes, "boxes after a refit with unchanged vertices")
    pt.update_vertices(0, p.vertices, lights=p.lights, lights_sum_area=p.lights_sum_area)
    same(pt.read_bvh_boxes(p.nodes), p.nodes, "... and with the uploaded lights")
    pt.reset_accum()
    pt.render(0, 2)
    same(pt.read_accum(), before, f"{name}: two frames after the refit vs two frames before")
    assert before[..., :3].any()


# ---- moving models --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["C2", "C4"])
def test_moved_model_matches_oracle(pt, name, mode):
    """The bunny translated in C2, the teapot rotated in C4; lights=None: no light moved."""
    run_sequence(pt, name, mode, "host", lights=False)


@pytest.mark.parametrize("name", ["C2", "C4"])
def test_moved_model_from_device_memory(pt, name):
    run_sequence(pt, name, TRAVERSE_ZCULL, "device", lights=False)


# ---- the light's area changes ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_scaled_and_lowered_light_matches_oracle(pt, mode):
    run_sequence(pt, "C1", mode, "host", lights=True)
    cfg = C.scene("C1")
    new = edited(cfg, *C.edit("C1"))
    assert new.packed.lights_sum_area != cfg.packed.lights_sum_area

    def two_frames():
        pt.reset_accum()
        pt.render(0, 2)
        return pt.read_accum()

    # a later material edit uploads spans of the library's host copy of the light records,
    # which hold the light triangles' vertices: the copy is in step
    pt.update_materials(0, cfg.packed.materials)
    same(two_frames(), pyoracle.Oracle(new).render(0, 2)[0], "after update_materials")
    before, boxes = two_frames(), pt.read_bvh_boxes(cfg.packed.nodes)
    bad = new.packed.lights.copy()
    bad[1, 0] = bad[0, 0]
    with pytest.raises(PnrtError, match=r"lights entry 1 ") as e:
        pt.update_vertices(0, cfg.packed.vertices, lights=bad)
    assert e.value.code == E_ARG
    same(pt.read_bvh_boxes(cfg.packed.nodes), boxes, "nothing changed")
    same(two_frames(), before, "the next render after a refused edit")


# ---- shapes at the edges --------------------------------------------------------------------------------
def deformed(packed, scale=0.9, shift=(0.15, 0.1, -0.2)):
    """Every vertex position scaled about the scene's centre and shifted (float32 steps)."""
    V = packed.vertices.copy()
    mid = ((V[:, 0:3].min(axis=0) + V[:, 0:3].max(axis=0)) * np.float32(0.5)).astype(np.float32)
    V[:, 0:3] = ((V[:, 0:3] - mid) * np.float32(scale) + mid + np.asarray(shift, np.float32)).astype(np.float32)
    return V


def edit_and_render(pt, cfg, first, rec, n_frames=2, info=None, modes=MODES):
    """Upload cfg, edit, compare boxes and n_frames frames with the oracle of the refit scene."""
    new = edited(cfg, first, rec)
    ref, st = pyoracle.Oracle(new).render(0, n_frames)
    assert st["stack_overflow"] == 0
    for mode in modes:
        pt.load(cfg, mode)
        for k, v in (info or {}).items():
            assert pt.device_info()[k] == v, k
        pt.update_vertices(first, rec, lights=new.packed.lights, lights_sum_area=new.packed.lights_sum_area)
        got = check_boxes(pt, cfg.packed, new.packed)
        pt.reset_accum()
        pt.render(0, n_frames)
        same(pt.read_accum(), ref, f"{cfg.name} mode {mode}")
    return new, got, ref


@pytest.mark.parametrize("what", ["quad", "coincident130"])
def test_root_leaf_has_only_the_root_box(pt, what):
    cfg = root_leaf_scene(what, 9, 8, True)
    new, got, ref = edit_and_render(pt, cfg, 0, deformed(cfg.packed, 0.7), 3,
                                    {"root_is_leaf": 1, "n_interior": 0, "has_leaf_table": int(what == "coincident130")})
    assert len(got) == 1 and not np.array_equal(got[0, 0:6], cfg.packed.nodes[0, 0:6]) and ref[..., :3].any()


def test_empty_leaf_keeps_its_uploaded_box(pt):
    cfg, _ = empty_leaf_c1()
    first, rec = C.edit("C1")
    new, got, _ = edit_and_render(pt, cfg, first, rec)
    same(got[-1], cfg.packed.nodes[-1], "the empty leaf's box")
    # (the light moves inside the box: the scene's box stays, the light's leaf follows)
    assert got[-1, 8] == got[-1, 9] and not np.array_equal(got[:, 0:6], cfg.packed.nodes[:, 0:6])


@functools.lru_cache(maxsize=None)
def leaf200_scene():
    """189 loose triangles (one model, added first) in the Cornell box under a hand-made tree:
    root -> leaf [0, 1), leaf [1, 201): 200 triangles, past the 127 a leaf ref holds inline."""
    rng = np.random.default_rng(200)
    sb = H.SceneBuilder()
    P = (rng.uniform(-1.8, 1.8, (189, 1, 3)) + rng.normal(0.0, 0.35, (189, 3, 3)) + np.array([0.0, 2.6, 0.0])).astype(np.float32)
    mesh = H.Mesh(P.reshape(-1, 3), None, None, np.arange(567, dtype=np.int32))
    sb.add_model(mesh, [H.scale(1.0)], H.Material(baseColor=(0.3, 0.5, 0.8), roughness=0.4), "loose")
    S._cornell_walls(sb, H.Material(baseColor=(0.65, 0.65, 0.65)))
    cfg = S.SceneConfig("leaf200", sb.build(), S._cornell_camera(24, 16), 24, 16, 1, max_depth=4)
    assert len(cfg.packed.triangles) == 201
    return with_nodes(cfg, chain_nodes(cfg.packed, "leafleft", 0, 1)), mesh


def test_leaf_of_200_triangles_through_the_leaf_table(pt):
    cfg, mesh = leaf200_scene()
    assert cfg.packed.nodes[2, 9] - cfg.packed.nodes[2, 8] == 200
    rec = H.model_vertices(mesh, [H.translate(0.3, -0.4, 0.2), H.rotate(25.0, 0, 0, 1), H.scale(0.8)])
    edit_and_render(pt, cfg, 0, rec, 2, {"has_leaf_table": 1, "n_interior": 1})


@pytest.mark.parametrize("kind,axis", [("leafleft", 0), ("interiorleft", 2)])
def test_chain_at_the_stack_limit_runs_the_longest_level_loop(pt, kind, axis):
    D = pt.device_info()["stack_limit"] - 2
    cfg = chain_config(kind, axis, 0, D)
    edit_and_render(pt, cfg, 0, deformed(cfg.packed), 2, {"max_depth": D, "n_interior": D})


def zero_scene(V, T, nodes, M):
    packed = H.PackedScene(V, M, T, nodes, np.zeros((0, 3), np.float32), 0.0, 1)
    return S.SceneConfig("signed-zero", packed, S._cornell_camera(8, 8), 8, 8, 1, max_depth=1)


@pytest.mark.parametrize("swap", [False, True])
def test_signed_zero_ties_keep_the_first(pt, swap):
    V, T, nodes, M = R.signed_zero_scene()
    if swap:                                  # the other order of the leaves at the root
        nodes[1, 8:10], nodes[2, 8:10] = (2, 4), (0, 2)
    away = V.copy()
    away[:, 0:3] += np.float32(1.5)
    start = zero_scene(away, T, R.refit_ref(away, T, nodes), M)
    want = R.refit_ref(V, T, nodes)
    ys, xs = np.meshgrid(np.linspace(-0.25, 1.25, 13, dtype=np.float32), np.linspace(-1.25, 1.25, 21, dtype=np.float32))
    rays = np.zeros((xs.size, 7), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2], rays[:, 6] = xs.reshape(-1), ys.reshape(-1), 3.0, 1e7
    d = np.array([0.01, 0.02, -1.0])
    rays[:, 3:6] = (d / np.linalg.norm(d)).astype(np.float32)
    end = zero_scene(V, T, want, M)
    ref = pyoracle.Oracle(end).intersect(rays, 0, 0)
    assert 0 < (ref[:, 0] != 0).sum() < len(rays)
    for mode in MODES:
        pt.upload_scene(start.packed)
        pt.set_options(mode)
        pt.update_vertices(0, V)
        got = pt.read_bvh_boxes(start.packed.nodes)
        same(got, want, "boxes, the zeros' signs included")
        same(got, H.bvh_refit_cpu(V, T, start.packed.nodes), "pnrt_bvh_refit_cpu")
        rec = pt.query_rays(rays)
        assert np.array_equal(rec[:, :13], ref), f"mode {mode}"
    b = R.bits(got)
    nz, pz = R.bits(np.float32(-0.0)), R.bits(np.float32(0.0))
    assert (b[0, 1], b[0, 2]) == ((nz, pz) if swap else (pz, nz))


def test_infinite_box_falls_back_to_the_exact_traversal(pt):
    """boxes_finite is re-evaluated from the refit boxes: with a vertex at +inf the culling
    mode renders what the exact mode renders, which is the oracle's image; a NaN coordinate
    enters no box."""
    cfg = C.scene("C1")
    V = cfg.packed.vertices.copy()
    V[0, 0], V[1, 1] = np.inf, np.nan
    new = edited(cfg, 0, V)
    assert np.isinf(new.packed.nodes[0, 3]) and not np.isnan(new.packed.nodes[:, 0:6]).any()
    ref, _ = pyoracle.Oracle(new).render(0, 2)
    for mode in MODES:
        pt.load(cfg, mode)
        pt.update_vertices(0, V)
        check_boxes(pt, cfg.packed, new.packed)
        pt.reset_accum()
        pt.render(0, 2)
        same(pt.read_accum(), ref, f"mode {mode}")
    pt.update_vertices(0, cfg.packed.vertices)         # and back: finite again, the plain image
    same(pt.read_bvh_boxes(cfg.packed.nodes), cfg.packed.nodes, "boxes after moving back")
    pt.reset_accum()
    pt.render(0, 2)
    same(pt.read_accum(), pyoracle.Oracle(cfg).render(0, 2)[0], "C1 after moving back")


# ---- staleness ------------------------------------------------------------------------------------------
def test_kept_records_and_guides_go_stale(pt):
    cfg = C.scene("C2")
    first, rec = C.edit("C2")
    new = edited(cfg, first, rec)
    pt.load(cfg)
    pt.reset_accum()
    pt.render(0, 1)
    same(pt.read_accum(), pyoracle.Oracle(cfg).render(0, 1)[0], "frame 0 before")
    pt.render_guides()
    pt.denoise()
    pt.update_vertices(first, rec)
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


# ---- errors ---------------------------------------------------------------------------------------------
def test_errors_change_nothing(pt):
    cfg = C.scene("C1")
    p = cfg.packed
    nv = len(p.vertices)
    pt.load(cfg)
    moved = deformed(p)
    lib, ctx = pt._lib, pt._ctx

    def refused(call, text):
        with pytest.raises(PnrtError, match=text) as e:
            call()
        assert e.value.code == E_ARG
        same(pt.read_bvh_boxes(p.nodes), p.nodes, f"boxes after the refused call ({text})")

    refused(lambda: pt.update_vertices(1, moved), "vertex range")                       # past the array
    refused(lambda: pt.update_vertices(nv, moved[:1]), "vertex range")
    refused(lambda: pt.update_vertices(-1, moved[:2]), "vertex range")                  # negative first
    refused(lambda: pt._ck(lib.pnrt_update_vertices(ctx, 0, -1, N.fptr(moved), None, 0.0), "u"), "vertex range")
    refused(lambda: pt._ck(lib.pnrt_update_vertices(ctx, 0, 2, None, None, 0.0), "u"), "NULL")     # NULL with count > 0
    refused(lambda: pt.update_vertices_device(0, 2, 0), "NULL")
    import torch
    t = torch.from_numpy(moved).to("cuda")
    torch.cuda.synchronize()
    refused(lambda: pt.update_vertices_device(0, 2, t.data_ptr() + 2), "4-byte aligned")
    pt.update_vertices(3, moved[:0])                                                    # count == 0, lights NULL: nothing
    same(pt.read_bvh_boxes(p.nodes), p.nodes, "count == 0")
    # read_bvh_boxes wants the uploaded topology
    other = C.scene("C2").packed.nodes
    for nodes, text in ((other, "interior nodes"), (p.nodes[:1], "not the uploaded tree")):
        with pytest.raises(PnrtError, match=text) as e:
            pt.read_bvh_boxes(nodes)
        assert e.value.code == E_ARG
    # the same interior count in another shape: a chain to the left and one to the right (C1's tree is
    # at most one of them); a child is a leaf in one tree and interior in the other
    k = int((p.nodes[:, 7] != -1).sum())
    assert len(p.nodes) == 2 * k + 1
    left, right = np.zeros((2 * k + 1, 12), np.float32), np.zeros((2 * k + 1, 12), np.float32)
    left[:, 7] = right[:, 7] = -1
    for i in range(k):
        left[i, 7] = 2 * k - i
        right[2 * i, 7] = 2 * i + 2
    shapes = [t for t in (left, right) if not np.array_equal(t[:, 7] == -1, p.nodes[:, 7] == -1)]
    assert shapes
    for t in shapes:
        with pytest.raises(PnrtError, match="is a leaf in one tree") as e:
            pt.read_bvh_boxes(t)
        assert e.value.code == E_ARG
    with PathTracer(0) as fresh:
        for call in (lambda: fresh.update_vertices(0, moved), lambda: fresh.read_bvh_boxes(p.nodes)):
            with pytest.raises(PnrtError, match="upload_scene first") as e:
                call()
            assert e.value.code == E_STATE
    pt.reset_accum()
    pt.render(0, 2)
    same(pt.read_accum(), pyoracle.Oracle(cfg).render(0, 2)[0], "C1 after every refused call")
