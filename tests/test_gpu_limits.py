"""Scenes, trees and frames at the limits the C ABI accepts, GPU vs CPU oracle,
bit for bit (tolerance 0 ulp: both sides evaluate the same IEEE operations).

pnrt_upload_scene / pnrt_set_frame / pnrt_render accept more than the
SceneBuilder scenes of the other modules reach.  Driven here:

* trees at the stack limit: hand-built chains of depth stack_limit - 2 (the
  deepest the validator admits) over a fan of 70 overlapping triangles, in two
  row orders (fan_scene: in the second the topmost stack entry holds the closest
  hit); depth stack_limit - 1 is rejected.  tests/test_limits_model.py shows on
  the CPU that rays really hold stack_limit - 2 deferred siblings;
* a leaf as the root (inline and leaf-table), an empty leaf;
* frames smaller than one 8x8 tile and one 256-entry segment, down to 1x1;
* camera rays lying exactly in box faces and triangle planes (0 * inf slabs);
* shard selectors with band_rows up to INT_MAX and more shards than bands;
* the last texture slot, an unbound slot, and texture ids outside -1..19.

The scene builders are module-level so tests/coop_worker.py renders the same
cases on the bounds-checked diagnostic library (test_limits_on_bounds_checked_library).
"""
import dataclasses
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pyoracle
from pnraytracing_amd import build
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer, PnrtError, shard_rows

pytestmark = pytest.mark.gpu          # (the CPU-only checks of these scenes are in tests/test_limits_model.py)
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = (TRAVERSE_ZCULL, TRAVERSE_EXACT, TRAVERSE_ZCULL | KERNEL_V1)
with open(os.path.join(os.path.dirname(HERE), "pnraytracing_amd", "csrc", "pt_common.h")) as _f:
    # the library's stack limit, from its source: the chain depth, FAN_ROT, limit_cases() and the CPU model
    # all follow it (the GPU tests also require device_info()["stack_limit"] to say the same)
    PT_STACK = int(re.search(r"^#define PT_STACK (\d+)", _f.read(), re.M).group(1))
N_FAN = 70


def assert_bitwise(got, ref, what):
    g, r = got.view(np.uint32), ref.view(np.uint32)
    bad = np.argwhere(np.any(g != r, axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {bad[:5].tolist()} " \
                          f"gpu={got[tuple(bad[0])]} oracle={ref[tuple(bad[0])]}"


def with_nodes(cfg, nodes, name=None):
    return dataclasses.replace(cfg, name=name or cfg.name,
                               packed=dataclasses.replace(cfg.packed, nodes=np.ascontiguousarray(nodes, np.float32)))


def oracle_render(cfg, first, n):
    ref, st = pyoracle.Oracle(cfg).render(first, n)
    assert st["stack_overflow"] == 0, cfg.name
    return ref


def load(pt, cfg, mode):
    """PathTracer.load, except that a texture entry of width 0 leaves its slot
    unbound (the oracle takes such an entry as an unbound sampler too)."""
    pt.upload_scene(cfg.packed)
    for slot, (px, w, h, ch) in enumerate(cfg.textures):
        if w > 0:
            pt.upload_texture(slot, px, w, h, ch)
    pt.upload_env(cfg.env_rgb, cfg.env_table)
    pt.set_frame(cfg.width, cfg.height, cfg.camera, cfg.max_depth)
    pt.set_options(mode)


def gpu_render(pt, cfg, first, n, mode, shard=(1, 1, 0)):
    load(pt, cfg, mode)
    pt.reset_accum()
    pt.render(first, n, *shard)
    return pt.read_accum()


def check_modes(pt, cfg, first, n, ref=None, modes=MODES):
    ref = oracle_render(cfg, first, n) if ref is None else ref
    for mode in modes:
        assert_bitwise(gpu_render(pt, cfg, first, n, mode), ref, f"{cfg.name} mode {mode:#x} frames {first}+{n}")
    return ref


# ---- section 2: trees at the stack limit ------------------------------------------------------
def tri_boxes(packed):
    """(nt, 2, 3) float32: min and max corner of every triangle's vertex box."""
    idx = packed.triangles[:, 0:3].astype(np.int64)
    P = packed.vertices[idx, 0:3]                       # (nt, 3 corners, xyz)
    return np.stack([P.min(axis=1), P.max(axis=1)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fan_scene(rot=0):
    """Cornell walls + a fan of 70 large overlapping triangles (one model each),
    24x16, depth 4; the packed triangle rows permuted so the fan comes first,
    triangle i being fan triangle (i + rot) % 70 (the builder's tree no longer
    fits the arrays: every use puts a chain in).  Returns (config with permuted
    rows, builder's config).

    rot = 0 is the plain order.  With rot = 70 - D = 8 the chains' deepest single
    leaf, [D - 1, D), holds fan triangle 69, the one nearest the Cornell camera,
    and the last leaf [D, nt) only the eight farthest and the walls: the sibling
    deferred LAST -- the topmost stack entry -- then holds the closest hit of
    every ray through the fan, so an entry lost or overwritten at the very top of
    the stack changes the picture (in the plain order the last leaf holds the
    nearest triangles and hides every deferred one from the camera)."""
    rng = np.random.default_rng(70)
    sb = H.SceneBuilder()
    S._cornell_walls(sb, H.Material(baseColor=(0.65, 0.65, 0.65)))
    n_wall_mats = 6
    base = np.array([[-2.0, 0.3, 0.0], [2.0, 0.5, 0.0], [0.0, 4.8, 0.0]])
    for k in range(N_FAN):
        P = base + np.array([0.0, 0.0, -2.0 + 4.0 * k / N_FAN]) + rng.normal(0.0, 0.05, (3, 3))
        mesh = H.Mesh(P.astype(np.float32), None, None, np.arange(3, dtype=np.int32))
        sb.add_model(mesh, [H.scale(1.0)], H.Material(baseColor=tuple(rng.uniform(0, 1, 3)),
                                                     roughness=float(rng.uniform(0, 1))), f"fan{k}")
    W, Hh = 24, 16
    built = S.SceneConfig("fan-builder", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1, max_depth=4)
    p = built.packed
    mat = p.triangles[:, 3].astype(np.int64)
    fan = np.flatnonzero(mat >= n_wall_mats)
    assert len(fan) == N_FAN and len(set(mat[fan])) == N_FAN
    perm = np.concatenate([np.roll(fan[np.argsort(mat[fan], kind="stable")], -rot), np.flatnonzero(mat < n_wall_mats)])
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    lights = p.lights.copy()
    lights[:, 0] = inv[lights[:, 0].astype(np.int64)]
    packed = dataclasses.replace(p, triangles=np.ascontiguousarray(p.triangles[perm]), lights=lights)
    return dataclasses.replace(built, name=f"fan-rot{rot}", packed=packed), built


def chain_nodes(packed, kind, axis, depth):
    """A chain of `depth` interior nodes over the triangles in array order, every
    box the union of its triangles' vertex boxes.

    "leafleft": node 2i is interior over [i, nt), its left child 2i+1 the leaf
    [i, i+1), its right child node 2i+2; the last node is the leaf [depth, nt).
    "interiorleft": the mirror -- interior nodes 0..depth-1 nested to the left,
    node depth the leaf [depth, nt), node i's right child the leaf [i, i+1) at
    index 2*depth - i."""
    tb = tri_boxes(packed)
    nt = len(tb)
    assert 1 <= depth < nt

    def box(a, b):
        return np.concatenate([tb[a:b, 0].min(axis=0), tb[a:b, 1].max(axis=0)])

    nd = np.zeros((2 * depth + 1, 12), np.float32)

    def leaf(i, a, b):
        nd[i, 0:6], nd[i, 6:10] = box(a, b), (0, -1, a, b)

    def interior(i, a, right):
        nd[i, 0:6], nd[i, 6:10] = box(a, nt), (axis, right, a, nt)

    for i in range(depth):
        if kind == "leafleft":
            interior(2 * i, i, 2 * i + 2)
            leaf(2 * i + 1, i, i + 1)
        else:
            interior(i, i, 2 * depth - i)
            leaf(2 * depth - i, i, i + 1)
    leaf(2 * depth if kind == "leafleft" else depth, depth, nt)
    return nd


def primary_rays(cfg):
    """Origins and unnormalised float64 directions of the camera rays (s = x / W,
    t = y / H, no jitter: CameraGetRay)."""
    cam = np.asarray(cfg.camera, np.float64).reshape(4, 3)
    y, x = np.mgrid[0:cfg.height, 0:cfg.width]
    s, t = (x / cfg.width).reshape(-1, 1), (y / cfg.height).reshape(-1, 1)
    d = cam[1] + s * cam[2] + t * cam[3] - cam[0]
    return cam[0], d


def peak_deferred(nodes, origin, dirs):
    """Model of a near-first traversal that tests both child boxes at the parent
    and defers the far child only when its box is hit: per ray, the peak number
    of deferred siblings held at once.  float64 slabs; the near child is the
    right one when dir[axis] < 0 (pn_oracle.c BVHIntersect), else the left."""
    nodes = np.asarray(nodes, np.float64)
    lo, hi = nodes[:, 0:3], nodes[:, 3:6]
    axis, right = nodes[:, 6].astype(int), nodes[:, 7].astype(int)
    peaks = np.zeros(len(dirs), int)
    for k, d in enumerate(dirs):
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / d
            t0, t1 = (lo - origin) * inv, (hi - origin) * inv
        tn = np.fmax.reduce(np.fmin(t0, t1), axis=1)
        tf = np.fmin.reduce(np.fmax(t0, t1), axis=1)
        hit = (tn <= tf) & (tf >= 0.0)
        stack, peak, cur = [], 0, 0 if hit[0] else -1
        while cur >= 0:
            if right[cur] != -1:
                near, far = (right[cur], cur + 1) if d[axis[cur]] < 0 else (cur + 1, right[cur])
                if hit[near] and hit[far]:
                    stack.append(far)
                    peak = max(peak, len(stack))
                    cur = near
                    continue
                if hit[near] or hit[far]:
                    cur = near if hit[near] else far
                    continue
            cur = stack.pop() if stack else -1
        peaks[k] = peak
    return peaks


FAN_ROT = N_FAN - (PT_STACK - 2)
CHAINS = [(kind, axis, rot) for kind in ("leafleft", "interiorleft") for axis in (0, 2) for rot in (0, FAN_ROT)]


def chain_config(kind, axis, rot=0, depth=PT_STACK - 2):
    cfg, _ = fan_scene(rot)
    return with_nodes(cfg, chain_nodes(cfg.packed, kind, axis, depth), f"{cfg.name}-{kind}-axis{axis}-depth{depth}")


@functools.lru_cache(maxsize=None)
def fan_reference():
    """The builder tree's oracle image of frames 0..1 (unpermuted rows)."""
    return oracle_render(fan_scene()[1], 0, 2)


# ---- section 3: root leaves, empty leaves -----------------------------------------------------
def _single_leaf(cfg):
    """The scene under a one-node tree: the root is a leaf over every triangle."""
    tb = tri_boxes(cfg.packed)
    nd = np.zeros((1, 12), np.float32)
    nd[0, 0:6] = np.concatenate([tb[:, 0].min(axis=0), tb[:, 1].max(axis=0)])
    nd[0, 6:10] = (0, -1, 0, len(tb))
    return with_nodes(cfg, nd)


def root_leaf_scene(what, W, Hh, env):
    sb = H.SceneBuilder()
    if what == "quad":         # an emissive quad facing the camera: 2 lights
        sb.add_model(H.mesh_quad(27.5), [H.translate(0.2, 2.8, 0.0), H.rotate(90.0, 1, 0, 0), H.scale(0.04)],
                     H.Material(baseColor=(0.7, 0.6, 0.5), emssive=(5.0, 4.0, 3.0)), "quad")
    else:
        tri = np.array([[-1.5, 1.2, -1.0], [1.8, 1.4, -0.5], [0.1, 4.5, -1.2]], np.float32)
        n = 1 if what == "triangle" else 130
        mesh = H.Mesh(np.tile(tri, (n, 1)), None, None, np.arange(3 * n, dtype=np.int32))
        sb.add_model(mesh, [H.scale(1.0)], H.Material(baseColor=(0.3, 0.6, 0.8), roughness=0.4), what)
    rgb = tab = None
    if env:
        rgb = H.synthetic_hdr(16, 8, 11)
        tab = H.hdr_table(rgb)
    cfg = S.SceneConfig(f"rootleaf-{what}-{W}x{Hh}-env{int(env)}", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1,
                        max_depth=4, env_rgb=rgb, env_table=tab)
    if len(cfg.packed.nodes) != 1:
        cfg = _single_leaf(cfg)
    assert len(cfg.packed.nodes) == 1 and cfg.packed.nodes[0, 7] == -1
    assert len(cfg.packed.lights) == (2 if what == "quad" else 0)
    return cfg


ROOT_LEAVES = [(what, W, Hh, env) for what in ("quad", "triangle", "coincident130")
               for (W, Hh) in ((9, 8), (7, 3)) for env in (False, True)]


def empty_leaf_c1():
    """C1 16x12 under a new root: left subtree the old tree (rightChild + 1),
    right child a leaf with start == end and the scene's box."""
    c = S.cornell_c1(16, 12)
    old = c.packed.nodes
    nd = np.zeros((len(old) + 2, 12), np.float32)
    nd[1:-1] = old
    inner = nd[1:-1, 7] != -1
    nd[1:-1][inner, 7] += 1
    nd[0, 0:6], nd[0, 6:10] = old[0, 0:6], (0, len(old) + 1, 0, len(c.packed.triangles))
    nd[-1, 0:6], nd[-1, 6:10] = old[0, 0:6], (0, -1, 0, 0)
    return with_nodes(c, nd, "C1-empty-leaf"), c


# ---- section 4: frames smaller than a tile and a segment ---------------------------------------
SMALL_SIZES = [(1, 1), (1, 5), (5, 1), (7, 3), (8, 8), (9, 8), (3, 70)]
SMALL_SCENES = ["C1", "fuzz3", "fuzz4"]      # fuzz seeds 3 (environment) and 4 (environment + textures)


def small_frame(scene, W, Hh):
    if scene == "C1":
        c = S.cornell_c1(W, Hh)
        return dataclasses.replace(c, name=f"C1-{W}x{Hh}")
    from test_gpu_fuzz import random_scene
    seed = int(scene[4:])
    c, _ = random_scene(seed)
    assert c.env_rgb is not None
    if seed == 4:      # (seed 3 has an environment but no texture; seed 4 has both, and uses slot 0)
        assert len(c.textures) == 2 and 0 in set(c.packed.triangles[:, 4].astype(int))
    return dataclasses.replace(c, name=f"{scene}-{W}x{Hh}", width=W, height=Hh)   # (camera vectors as they are)


# ---- section 5: rays in box faces and triangle planes -----------------------------------------
PLANE_CAMERAS = {"right-wall": ((2.75, 2.8, 7), (0, 0, -1)), "left-wall": ((-2.75, 2.8, 7), (0, 0, -1)),
                 "ceiling": ((0, 5.54, 7), (0, 0, -1)), "floor": ((0, 0, 7), (0, 0, -1)),
                 "open-face": ((0, 2.8, 2.75), (0, 0, -1)), "front-wall+x": ((0, 2.8, -2.75), (1, 0, 0))}


def plane_camera(name):
    """C1 at 16x12 with the eye in a wall / ceiling / floor / box-face plane and the
    centre pixel (x = 8, y = 6: s = t = 0.5 exactly) looking along an axis."""
    eye, look = PLANE_CAMERAS[name]
    c = S.cornell_c1(16, 12)
    centre = tuple(np.float32(e) + np.float32(d) for e, d in zip(eye, look))
    cam = H.camera_update(eye, centre, (0, 1, 0), 45.0, np.float32(16) / np.float32(12))
    return dataclasses.replace(c, name=f"C1-plane-{name}", camera=cam)


def centre_direction(cfg):
    """The centre pixel's unnormalised direction in CameraGetRay's float32 order."""
    eye, llc, hor, ver = np.asarray(cfg.camera, np.float32).reshape(4, 3)
    s, t = np.float32(cfg.width // 2) / np.float32(cfg.width), np.float32(cfg.height // 2) / np.float32(cfg.height)
    assert s == 0.5 and t == 0.5
    return ((llc + s * hor) + t * ver) - eye


# ---- the cases the bounds-checked diagnostic library renders (tests/coop_worker.py "limits") ----
def limit_cases():
    """(name, config, first frame, frames) of sections 2-5, one or two of each kind."""
    out = [(c.name, c, 0, 1) for c in (chain_config(*ch) for ch in CHAINS)]
    out += [(c.name, c, 0, 2) for c in (root_leaf_scene(*a) for a in ROOT_LEAVES if a[1:3] == (9, 8) or a[3])]
    out.append(("C1-empty-leaf", empty_leaf_c1()[0], 0, 2))
    for scene in SMALL_SCENES:
        for W, Hh in SMALL_SIZES:
            out.append((f"{scene}-{W}x{Hh}", small_frame(scene, W, Hh), 5, 3))
    out.append(("C1-1x1-140", small_frame("C1", 1, 1), 0, 140))
    out += [(f"plane-{k}", plane_camera(k), 0, 2) for k in PLANE_CAMERAS]
    return out


# ================================================================================================
@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def test_limits_on_bounds_checked_library():
    """Sections 2-5 on the `coop` diagnostic library (every fetch, store and stack
    index bounds-checked, a violation reported as an error; every ray handed to the
    cooperative finish), culling and exact mode, against the oracle.  Rays with
    spilled stack entries (`deep`) must have occurred."""
    lib = build.variant_path("coop")
    assert os.path.exists(lib), "variants/libpnrt_coop.so not built (__graft_entry__.build())"
    env = dict(os.environ, PNRT_DEVICE_LIB=lib)
    r = subprocess.run([sys.executable, os.path.join(HERE, "coop_worker.py"), "limits"], env=env,
                       capture_output=True, text=True, timeout=400)
    assert r.returncode == 0 and "COOP-WORKER-DONE" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "DIAGNOSTIC BUILD" in r.stdout
    deep = sum(int(m.group(1)) for m in re.finditer(r"\[coop\] bounce \d+ n=\d+ .* deep=(\d+)", r.stderr))
    print(f"coop limits: {r.stdout.count(': ok')} renders, rays with spilled stack entries {deep}")
    assert deep > 0


# ---- section 2 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,axis,rot", CHAINS)
def test_chain_at_stack_limit_bitwise(pt, kind, axis, rot):
    D = pt.device_info()["stack_limit"] - 2
    assert D == PT_STACK - 2
    cfg = chain_config(kind, axis, rot, D)
    ref = oracle_render(cfg, 0, 2)
    for mode in MODES:
        got = gpu_render(pt, cfg, 0, 2, mode)
        info = pt.device_info()
        assert info["max_depth"] == D and info["n_interior"] == D and info["root_is_leaf"] == 0
        assert_bitwise(got, ref, f"{cfg.name} mode {mode:#x}")


@pytest.mark.parametrize("kind,axis", [(kind, axis) for kind, axis, rot in CHAINS if rot == 0])
def test_chain_past_stack_limit_rejected(kind, axis):
    """One level deeper: PNRT_E_SCENE at upload (host-only, nothing is rendered)."""
    with PathTracer(0) as t:
        D = t.device_info()["stack_limit"] - 2
        cfg = chain_config(kind, axis, 0, D + 1)
        with pytest.raises(PnrtError, match=rf"\(-4\): BVH depth {D + 1} exceeds the kernel stack"):
            t.upload_scene(cfg.packed)


# ---- section 3 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("what,W,Hh,env", ROOT_LEAVES)
def test_root_leaf_bitwise(pt, what, W, Hh, env):
    cfg = root_leaf_scene(what, W, Hh, env)
    ref = oracle_render(cfg, 0, 3)
    if env or what == "quad":
        assert ref[..., :3].any(), "the scene shows nothing"
    for mode in MODES:
        got = gpu_render(pt, cfg, 0, 3, mode)
        info = pt.device_info()
        assert info["root_is_leaf"] == 1 and info["n_interior"] == 0 and info["max_depth"] == 0
        assert info["has_leaf_table"] == (1 if what == "coincident130" else 0)
        assert_bitwise(got, ref, f"{cfg.name} mode {mode:#x}")


def test_empty_leaf_bitwise(pt):
    cfg, plain = empty_leaf_c1()
    ref = check_modes(pt, cfg, 0, 3)
    assert_bitwise(oracle_render(plain, 0, 3), ref, "oracle: plain C1 vs C1 with an empty leaf")
    assert_bitwise(gpu_render(pt, plain, 0, 3, TRAVERSE_ZCULL), ref, "plain C1 vs C1 with an empty leaf")


# ---- section 4 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", SMALL_SIZES)
@pytest.mark.parametrize("scene", SMALL_SCENES)
def test_small_frames_bitwise(pt, scene, W, Hh):
    cfg = small_frame(scene, W, Hh)
    for first, n in ((0, 1), (5, 3)):
        check_modes(pt, cfg, first, n)


@pytest.mark.parametrize("scene", SMALL_SCENES)
def test_one_pixel_many_frames_and_calls(pt, scene):
    """1x1: one call of 140 frames (two batches, every frame a single padded
    tile) and six back-to-back calls of 2 frames (the pipes rotate)."""
    cfg = small_frame(scene, 1, 1)
    ref140, ref12 = oracle_render(cfg, 0, 140), oracle_render(cfg, 0, 12)
    for mode in MODES:
        assert_bitwise(gpu_render(pt, cfg, 0, 140, mode), ref140, f"{cfg.name} render(0, 140) mode {mode:#x}")
        if not mode & KERNEL_V1:
            assert pt.batch_plan(140)["n_batches"] == 2
        pt.reset_accum()
        for k in range(6):
            pt.render(2 * k, 2)
        assert_bitwise(pt.read_accum(), ref12, f"{cfg.name} 6 x render(2k, 2) mode {mode:#x}")


# ---- section 5 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PLANE_CAMERAS))
def test_rays_in_box_faces_and_triangle_planes(pt, name):
    cfg = plane_camera(name)
    d = centre_direction(cfg)
    assert int((d == 0).sum()) == 2, d
    eye, look = PLANE_CAMERAS[name]
    assert np.sign(d[np.flatnonzero(d)[0]]) == sum(look) and np.array_equal(cfg.camera[0], np.float32(eye))
    ref = check_modes(pt, cfg, 0, 3)
    if look == (0, 0, -1):
        assert np.isfinite(ref).all()


# ---- section 6 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", [(80, 5), (40, 21)])
def test_oversized_bands(pt, W, Hh):
    import torch
    cfg = S.cornell_c1(W, Hh)
    ref = oracle_render(cfg, 0, 2)
    for mode in MODES:
        full = gpu_render(pt, cfg, 0, 2, mode)
        assert_bitwise(full, ref, f"C1 {W}x{Hh} mode {mode:#x}")
        plan_full = pt.batch_plan(2)
        for band in (Hh, Hh + 1, 1 << 30, 2**31 - 1):
            for nsh in (1, 2, 4):
                what = f"mode {mode:#x} band {band} shards {nsh}"
                pt.reset_accum()
                pt.render(0, 2, band, nsh, 0)
                assert_bitwise(pt.read_accum(), full, f"{what} shard 0 vs (1, 1, 0)")
                assert pt.batch_plan(2, band, nsh, 0) == plan_full
                for sh in range(1, nsh):
                    pt.render(2, 2, band, nsh, sh)            # OK, and no rows: the bits stay
                    assert pt.batch_plan(2, band, nsh, sh) == {"frames_per_batch": 0, "n_batches": 0, "batch_bytes": 0}
                    one = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
                    pt.pack_rows(one.data_ptr(), band, nsh, sh)
                    pt.synchronize()
                    assert (one.cpu().numpy() == 7.0).all()
                    assert_bitwise(pt.read_accum(), full, f"{what} shard {sh}: accumulation touched")
        whole = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
        pt.pack_rows(whole.data_ptr(), 2**31 - 1, 4, 0)
        pt.synchronize()
        assert_bitwise(whole.cpu().numpy(), full, f"mode {mode:#x}: pack_rows of the one band")


# (band_rows, n_shards) at 40x21: more shards than bands (one band each, the last partial, four empty
# shards); shards of three bands each, one ending in a one-row band; a shard count of INT_MAX
SHARD_SPLITS = [(8, 7), (4, 2), (8, 2**31 - 1)]


@pytest.mark.parametrize("band,nsh", SHARD_SPLITS)
def test_more_shards_than_bands(pt, band, nsh):
    """The union of the shards equals the full render and the oracle's image in
    every mode (the v1 kernel maps rows in its own code, pt_path.h), and
    pack_rows + unpack_rows restore the image."""
    import torch
    W, Hh = 40, 21
    cfg = S.cornell_c1(W, Hh)
    ref = oracle_render(cfg, 0, 2)
    shards = list(range(nsh)) if nsh < 100 else [0, 1, 2, 3, nsh - 1]      # (every shard that has rows, and empty ones)
    assert sum(len(shard_rows(Hh, band, nsh, sh)) for sh in shards) == Hh
    for mode in MODES:
        full = gpu_render(pt, cfg, 0, 2, mode)
        assert_bitwise(full, ref, f"C1 40x21 mode {mode:#x}")
        pt.reset_accum()
        for sh in shards:
            pt.render(0, 2, band, nsh, sh)
            rows = len(shard_rows(Hh, band, nsh, sh))
            assert (pt.batch_plan(2, band, nsh, sh)["n_batches"] > 0) == (rows > 0)
        assert_bitwise(pt.read_accum(), ref, f"mode {mode:#x}: union of the shards ({band}-row bands, {nsh} shards)")
        image = torch.zeros((Hh, W, 4), dtype=torch.float32, device="cuda")
        for sh in shards:
            rows = shard_rows(Hh, band, nsh, sh)
            packed = torch.full((max(len(rows), 1), W, 4), -1.0, dtype=torch.float32, device="cuda")
            pt.pack_rows(packed.data_ptr(), band, nsh, sh)
            pt.synchronize()
            if len(rows):
                np.testing.assert_array_equal(packed.cpu().numpy().view(np.uint32), full[rows].view(np.uint32))
            else:
                assert (packed.cpu().numpy() == -1.0).all()
            pt.unpack_rows(packed.data_ptr(), image.data_ptr(), band, nsh, sh)
        pt.synchronize()
        assert_bitwise(image.cpu().numpy(), full, f"mode {mode:#x}: pack_rows + unpack_rows over the shards")


# ---- section 7 ---------------------------------------------------------------------------------
def texture_slot_scene(last):
    """Cornell walls + a soup textured from slot 19 (uv in -1..2) + a soup whose
    texture id names slot 7, which nobody uploads."""
    rng = np.random.default_rng(19)
    sb = H.SceneBuilder()
    S._cornell_walls(sb, H.Material(baseColor=(0.65, 0.65, 0.65)))
    for k, tex in enumerate((19, 7)):
        n = 30
        base = rng.uniform(-1.5, 1.5, (n, 1, 3)) + np.array([0, 2.5, 0])
        P = (base + rng.normal(0, 0.5, (n, 3, 3))).reshape(-1, 3).astype(np.float32)
        uv = rng.uniform(-1, 2, (3 * n, 2)).astype(np.float32)
        sb.add_model(H.Mesh(P, None, uv, np.arange(3 * n, dtype=np.int32)), [H.scale(1.0)],
                     H.Material(baseColor=(0.9, 0.8, 0.2), roughness=0.6), f"soup{k}", texture_ids=[tex])
    unbound = (np.zeros(0, np.uint8), 0, 0, 3)
    W, Hh = 24, 16
    cfg = S.SceneConfig("texture-slot-19", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1, max_depth=3,
                        textures=[unbound] * 19 + [last])
    assert set(cfg.packed.triangles[:, 4].astype(int)) == {-1, 7, 19}
    return cfg


@pytest.mark.parametrize("tex", ["rgb1x1", "grey3x2"])
def test_last_and_unbound_texture_slots(tex):
    last = (np.array([200, 40, 90], np.uint8), 1, 1, 3) if tex == "rgb1x1" else \
           (np.array([10, 250, 60, 130, 0, 255], np.uint8), 3, 2, 1)
    cfg = texture_slot_scene(last)
    ref, st = pyoracle.Oracle(cfg).render(0, 3)
    assert st["stack_overflow"] == 0 and st["albedo_bytes"] > 0
    with PathTracer(0) as t:                  # a fresh context: slot 7 was never bound
        for mode in MODES:
            assert_bitwise(gpu_render(t, cfg, 0, 3, mode), ref, f"{cfg.name} {tex} mode {mode:#x}")


@pytest.mark.parametrize("tex", [20, 255, 256, -2])
def test_texture_id_out_of_range_rejected(tex):
    """Host-only: the wavefront records keep texture id + 1 in 8 bits, so 255 would
    shade as untextured and 256 as slot 0; upload refuses ids outside -1..19."""
    c = S.cornell_c1(16, 12)
    tri = c.packed.triangles.copy()
    tri[5, 4] = tex
    with PathTracer(0) as t:
        with pytest.raises(PnrtError, match=r"\(-4\): triangle 5 has an out-of-range texture id"):
            t.upload_scene(dataclasses.replace(c.packed, triangles=tri))
        for ok in (-1, 0, 19):
            tri[5, 4] = ok
            t.upload_scene(dataclasses.replace(c.packed, triangles=tri))
