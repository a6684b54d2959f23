"""Light lists longer than PT_LIGHT_SCAN (8): GetLightIndex's binary search and its tables.

Up to eight light triangles with non-decreasing prefix areas, pt_wf.h light_entry scans a copy
of the areas held in the kernel arguments; every other scene of the suite stays below that.
Here the list has 9 .. 1002 entries (tests/lamps_common.py: an emissive triangle soup in the
Cornell box), or is short but not monotone, so that the search over `lights` in memory, the
light records past entry 8, the fallback entry n_lights, pt_refit_lights_kernel over more than
one block, pnrt_place_models' relight prefix over hundreds of entries and pnrt_update_materials'
span of light records all run -- everything bit for bit against the CPU oracle.

Every case asserts ON THE ORACLE that it bites: a list cut to its first eight entries renders
another image, GetLightIndex returns more than eight triangles, the fallback index is returned.
Frames are 32x24 at 1 spp."""
import dataclasses
import functools

import numpy as np
import pytest

import lamps_common as L
import pyoracle
import shader_pin as SP
import test_gpu_cameras as T          # its helpers; nothing runs on import
from test_gpu_refit import check_boxes, same
from pnraytracing_amd import host as H
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer

pytestmark = pytest.mark.gpu

F = np.float32
MODES3 = (TRAVERSE_ZCULL, TRAVERSE_EXACT, TRAVERSE_ZCULL | KERNEL_V1)
MODES = (TRAVERSE_ZCULL, TRAVERSE_EXACT)
CALLS = ((0, 3), (5, 2))
ALL = 0xFFFFFFFF                        # min_frames: every pixel active
SCAN = 8                                # PT_LIGHT_SCAN
U = np.random.default_rng(SP.SEED).random(4000).astype(F)


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def n_differ(a, b):
    return int(np.count_nonzero(np.any(T.bits(a) != T.bits(b), axis=-1)))


def with_packed(cfg, **kw):
    return dataclasses.replace(cfg, packed=dataclasses.replace(cfg.packed, **kw))


def light_indices(cfg):
    """The oracle's GetLightIndex over the 4000 seeded u."""
    return SP.oracle_fn(pyoracle.Oracle(cfg), 14, SP.fw(U))[:, 0]


def oracle_calls(cfg):
    orc = pyoracle.Oracle(cfg)
    out = []
    for first, n in CALLS:
        img, st = orc.render(first, n)
        assert st["stack_overflow"] == 0
        out.append(img)
    return out


def gpu_equals_oracle(pt, cfg, modes=MODES3, refs=None):
    refs = refs or oracle_calls(cfg)
    for mode in modes:
        pt.load(cfg, mode)
        for (first, n), ref in zip(CALLS, refs):
            pt.reset_accum()
            pt.render(first, n)
            same(pt.read_accum(), ref, f"{cfg.name} ({len(cfg.packed.lights)} lights) mode {mode:#x} frames {first}+{n}")
    return refs


# ---- 1 list lengths -------------------------------------------------------------------------------------
# (soup triangles, the ceiling light, an environment) -> 8, 9, 16, 17, 64, 65, 300 and 1002 entries; then 17 entries
# with an environment, and 65 whose entry 0 is a lamp triangle
LENGTHS = [(6, True, False), (7, True, False), (14, True, False), (15, True, False), (62, True, False), (63, True, False),
           (298, True, False), (1000, True, False), (15, True, True), (65, False, False)]


@pytest.mark.parametrize("n,walls_light,env", LENGTHS,
                         ids=[f"{n + 2 * w}{'' if w else '-lamp-only'}{'-env' if e else ''}" for n, w, e in LENGTHS])
def test_list_length(pt, n, walls_light, env):
    cfg = L.lamp_scene(n, walls_light, env)
    p = cfg.packed
    nl = len(p.lights)
    assert nl == n + 2 * walls_light and np.all(np.diff(p.lights[:, 1]) >= 0)
    assert len(set(L.light_materials(p).tolist())) == 1 + walls_light and (cfg.env_rgb is not None) == env
    refs = oracle_calls(cfg)
    if nl > SCAN:
        # a scan of the first eight entries cannot pass: it renders another image, and the search returns other triangles
        cut, _ = pyoracle.Oracle(with_packed(cfg, lights=p.lights[:SCAN].copy())).render(*CALLS[0])
        d = n_differ(cut, refs[0])
        distinct = len(np.unique(light_indices(cfg)))
        print(f"{nl} lights: {d} of {cfg.width * cfg.height} pixels differ from the list cut to {SCAN}; {distinct} distinct triangles")
        assert 10 * d >= cfg.width * cfg.height
        assert distinct > SCAN
    gpu_equals_oracle(pt, cfg, refs=refs)


# ---- 2 short lists the scan must not take, and the fallback ----------------------------------------------
def unscannable(kind):
    cfg = L.lamp_scene(63 if kind == "sum63" else 5)
    p = cfg.packed
    lights = p.lights.copy()
    if kind == "swapped":
        lights[[2, 4], 1] = lights[[4, 2], 1]
        assert np.any(np.diff(lights[:, 1]) < 0)
        return cfg, with_packed(cfg, lights=lights)
    if kind == "nan":
        lights[3, 1] = np.nan
        return cfg, with_packed(cfg, lights=lights)
    return cfg, with_packed(cfg, lights_sum_area=float(F(1.5) * F(lights[-1, 1])))


@pytest.mark.parametrize("kind", ["swapped", "nan", "sum7", "sum63"])
def test_list_the_scan_must_not_take(pt, kind):
    plain, cfg = unscannable(kind)
    p = cfg.packed
    assert len(p.lights) == (65 if kind == "sum63" else 7)
    refs = oracle_calls(cfg)
    d = n_differ(refs[0], oracle_calls(plain)[0])
    print(f"{kind}: {d} of {cfg.width * cfg.height} pixels differ from the plain scene's image")
    if kind != "nan":
        assert d > 0
    if kind.startswith("sum"):
        # u * sum beyond the last prefix area: GetLightIndex's fallback, triangle 0, which is no light
        got = light_indices(cfg)
        assert 0 not in p.lights[:, 0] and (got == 0).any() and (got != 0).any()
        assert not (light_indices(plain) == 0).any()
    gpu_equals_oracle(pt, cfg, refs=refs)


# ---- 3 every entry point that instantiates the setup kernels ---------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_entry_point(pt, mode):
    """(The ray buffer is a torch tensor, as in tests/test_gpu_rays.py: run alone, the first case pays torch's
    start-up on the device, about ten seconds; in the suite the process has paid it before.)"""
    cfg = L.lamp_scene(63)
    W, Hh = cfg.width, cfg.height
    refs = oracle_calls(cfg)
    cam = np.asarray(cfg.camera, F).reshape(1, 12)
    for (first, n), ref in zip(CALLS, refs):
        T.load(pt, cfg, mode)
        pt.render(first, n)
        same(pt.read_accum(), ref, f"render {first}+{n}")
        pt.reset_accum()
        pt.render_cameras(first, np.tile(cam, (n, 1)))
        same(pt.read_accum(), ref, f"render_cameras {first}+{n}")
        pt.reset_accum()
        rays = pt.make_rays("pinhole", cfg.camera)
        pt.render_rays(first, n, rays)
        same(pt.read_accum(), ref, f"render_rays {first}+{n}")
    # the adaptive calls fold a frame at the weight of the pixel's own count, which is pnrt_render's weight
    # where the frames follow one another from 0: frames 0..2, then 3..4, then the second call's 5..6
    ref7, st = pyoracle.Oracle(cfg).render(0, 7)
    assert st["stack_overflow"] == 0
    T.load(pt, cfg, mode)
    pt.render(0, 7)
    same(pt.read_accum(), ref7, "render 0+7")
    rays = pt.make_rays("pinhole", cfg.camera)
    tiles = (W // 8) * (Hh // 8)
    for name, call in (("render_adaptive", lambda first, n: pt.render_adaptive(first, n, 0.0, ALL)),
                       ("render_rays_adaptive", lambda first, n: pt.render_rays_adaptive(first, n, rays, 0, 0.0, ALL))):
        pt.enable_moments(True)
        pt.reset_accum()
        for first, n in ((0, 3), (3, 2), (5, 2)):
            assert call(first, n) == {"n_pixels": W * Hh, "n_active_pixels": W * Hh, "n_tiles": tiles, "n_active_tiles": tiles,
                                      "frames_per_batch": n, "n_batches": 1}
            if first == 0:
                same(pt.read_accum(), refs[0], f"{name} 0+3")
        same(pt.read_accum(), ref7, f"{name} 0+3, 3+2, 5+2")
        pt.enable_moments(False)


# ---- 4 geometry edits with 300 lights --------------------------------------------------------------------
NA, NB = 150, 148
MAT_A, MAT_B = 6, 7


@functools.lru_cache(maxsize=None)
def moved_lamps():
    """(scene, lamp A's mesh, its records under the new matrix, the refit scene, its oracle's two frames)"""
    cfg = L.two_lamps_scene(NA, NB)
    p = cfg.packed
    mesh = L.soup(NA, 11, (0, 3, 0))
    same(H.model_vertices(mesh, L.LAMP_A_OPS), p.vertices[L.LAMP_FIRST_VERTEX:L.LAMP_FIRST_VERTEX + 3 * NA], "lamp A where it is said to be")
    mats = L.light_materials(p)
    changes = int(np.count_nonzero(np.diff(mats)))
    assert len(mats) == 300 and set(mats.tolist()) == {5, MAT_A, MAT_B} and changes >= 100, changes
    rec = H.model_vertices(mesh, L.LAMP_A_MOVED)
    new = dataclasses.replace(cfg, packed=H.refit_packed(p, L.LAMP_FIRST_VERTEX, rec))
    assert new.packed.lights_sum_area != p.lights_sum_area
    ref, st = pyoracle.Oracle(new).render(0, 2)
    assert st["stack_overflow"] == 0 and n_differ(ref, pyoracle.Oracle(cfg).render(0, 2)[0]) > 0
    ref.setflags(write=False)
    return cfg, mesh, rec, new, ref


def two_frames(pt):
    pt.reset_accum()
    pt.render(0, 2)
    return pt.read_accum()


def place_lamp_a(pt, mode, relight):
    cfg, mesh, rec, new, _ = moved_lamps()
    pt.load(cfg, mode)
    mid = pt.define_model(L.LAMP_FIRST_VERTEX, H.model_records(mesh))
    pt.place_models([(mid, H.model_matrix(L.LAMP_A_MOVED))], relight=relight)
    return cfg, new


@pytest.mark.parametrize("mode", MODES)
def test_lamp_moved_by_update_vertices_and_by_place_models(pt, mode):
    cfg, mesh, rec, new, ref = moved_lamps()
    pt.load(cfg, mode)
    pt.update_vertices(L.LAMP_FIRST_VERTEX, rec, lights=new.packed.lights, lights_sum_area=new.packed.lights_sum_area)
    check_boxes(pt, cfg.packed, new.packed)
    edited = two_frames(pt)
    same(edited, ref, f"mode {mode}: update_vertices with the new areas vs the oracle")
    place_lamp_a(pt, mode, relight=True)
    check_boxes(pt, cfg.packed, new.packed)
    placed = two_frames(pt)
    same(placed, ref, f"mode {mode}: place_models(relight=True) vs the oracle")
    same(placed, edited, "the two paths")


def test_relight_false_keeps_300_areas_as_lights_none_does(pt):
    cfg, mesh, rec, new, ref = moved_lamps()
    place_lamp_a(pt, TRAVERSE_ZCULL, relight=False)
    img = two_frames(pt)
    with PathTracer(0) as other:
        other.load(cfg)
        other.update_vertices(L.LAMP_FIRST_VERTEX, rec, lights=None)
        same(two_frames(other), img, "relight=False vs update_vertices(lights=None)")
    assert n_differ(img, ref) > 0                                               # the areas matter
    # ... which is the oracle's image of the new vertices under the old list
    old_list = with_packed(new, lights=cfg.packed.lights, lights_sum_area=cfg.packed.lights_sum_area)
    same(img, pyoracle.Oracle(old_list).render(0, 2)[0], "the old areas with the new vertices vs the oracle")


# ---- 5 material edits with 300 lights --------------------------------------------------------------------
def test_material_edits_patch_interleaved_spans(pt):
    """After a placement, so that the library's host copy of the light records is the one read back
    from the device.  Lamp B's entries lie among lamp A's: every span uploaded holds entries of
    another material, which must keep their emission."""
    cfg, new = place_lamp_a(pt, TRAVERSE_ZCULL, relight=True)
    mats = new.packed.materials.copy()
    seen = [pyoracle.Oracle(new).render(0, 2)[0]]

    def edit(first, count, what):
        pt.update_materials(first, mats[first:first + count])
        ref, _ = pyoracle.Oracle(with_packed(new, materials=mats.copy())).render(0, 2)
        assert all(n_differ(ref, s) > 0 for s in seen), f"{what}: the edit shows in the oracle's image"
        seen.append(ref)
        same(two_frames(pt), ref, what)

    same(two_frames(pt), seen[0], "before any edit")
    mats[MAT_B, 0:3] = (9.0, 0.5, 2.0)
    edit(MAT_B, 1, "lamp B's emission alone")
    mats[MAT_A, 0:3] = (0.5, 7.0, 3.0)
    edit(MAT_A, 1, "lamp A's emission alone")
    mats[MAT_A, 0:3] = (2.0, 2.0, 11.0)
    mats[MAT_B, 0:3] = (12.0, 3.0, 1.0)
    edit(MAT_A, 2, "both lamps in one call")
    mats[MAT_A, 0:3] = 0.0                                                      # the list stays, as in the reference
    edit(MAT_A, 1, "lamp A's emission set to zero")
    mats[5, 0:3] = (20.0, 30.0, 40.0)
    mats[MAT_B, 0:3] = 0.0
    edit(0, len(mats), "every material in one call")
