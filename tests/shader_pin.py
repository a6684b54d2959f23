"""Cases and plumbing for pinning the oracle to the reference's shader text.

TEST INFRASTRUCTURE shared by tests/golden/make_shader_golden.py (which runs
oracle/_ref/shader_driver -- shaders/ray_tracing.comp translated to C++ -- and
commits what it wrote), tests/test_shader_pin.py (oracle vs driver / fixtures)
and tests/test_gpu_shader_pin.py (GPU vs the committed driver images).

Every input is float32 / uint32 numpy data from seeded PCG64 streams, so the
driver, the oracle and the fixtures see identical bits.
"""
from __future__ import annotations

import dataclasses
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, HERE)

import isect_rays as IR  # noqa: E402
import lamps_common as LAMPS  # noqa: E402
import pyoracle  # noqa: E402
from pnraytracing_amd import host as H  # noqa: E402
from pnraytracing_amd import scenes as S  # noqa: E402

DRIVER = os.path.join(REPO, "oracle", "_ref", "shader_driver")
GOLD = os.path.join(HERE, "golden")
F = np.float32
U = np.uint32
SEED = 20261021
SAMPLE = 64                      # records of every function case kept in full


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- the driver ---------------------------------------------------------------
def scene_blob(cfg) -> bytes:
    p = cfg.packed
    parts = [b"PNSH"]
    for a, per in ((p.vertices, 15), (p.materials, 18), (p.triangles, 6), (p.nodes, 12), (p.lights, 3)):
        a = np.ascontiguousarray(a, "<f4").reshape(-1, per)
        parts += [struct.pack("<i", len(a)), a.tobytes()]
    parts.append(struct.pack("<f", p.lights_sum_area))
    parts.append(struct.pack("<i", len(cfg.textures)))
    for px, w, h, ch in cfg.textures:
        parts += [struct.pack("<iii", w, h, ch), pyoracle.gl_unpacked(px, w, h, ch).tobytes()]
    if cfg.env_rgb is not None:
        h, w = cfg.env_rgb.shape[:2]
        parts += [struct.pack("<iii", 1, w, h), np.ascontiguousarray(cfg.env_rgb, "<f4").tobytes(),
                  np.ascontiguousarray(cfg.env_table, "<f4").tobytes()]
    else:
        parts.append(struct.pack("<iii", 0, 0, 0))
    parts += [np.ascontiguousarray(cfg.camera, "<f4").tobytes(), struct.pack("<iii", cfg.width, cfg.height, cfg.max_depth)]
    return b"".join(parts)


def _run(driver, data: bytes):
    res = subprocess.run([driver], input=data, capture_output=True)
    if res.returncode != 0:
        raise RuntimeError(f"{os.path.basename(driver)} failed ({res.returncode}): {res.stderr.decode(errors='replace')[-400:]}")
    return res


def driver_image(cfg, first: int, n: int, driver: str = DRIVER, blob: bytes | None = None) -> np.ndarray:
    res = _run(driver, (blob or scene_blob(cfg)) + b"IMAG" + struct.pack("<IIii", first, n, 0, cfg.height))
    return np.frombuffer(res.stdout, "<f4").reshape(cfg.height, cfg.width, 4).copy()


def driver_fn(cfg, fn: int, words: np.ndarray, driver: str = DRIVER, blob: bytes | None = None) -> np.ndarray:
    words = np.ascontiguousarray(words, "<u4")
    res = _run(driver, (blob or scene_blob(cfg)) + b"FUNC" + struct.pack("<iii", fn, len(words), words.shape[1]) + words.tobytes())
    return np.frombuffer(res.stdout, "<u4").reshape(len(words), -1).copy()


# ---- scenes ---------------------------------------------------------------------
def coincident_scene(copies: int = 130, W: int = 40, Hh: int = 30):
    """tests/test_gpu_fuzz.py's coincident-triangle scene: one leaf of `copies`
    identical triangles in three materials, exact t ties everywhere."""
    rng = np.random.default_rng(copies)
    sb = H.SceneBuilder()
    S._cornell_walls(sb, H.Material(baseColor=(0.6, 0.6, 0.6)))
    tri = np.array([[-1.0, 0.5, -1.0], [1.5, 0.7, -0.5], [0.0, 3.0, -1.2]], F)
    for k in range(3):
        P = np.tile(tri, (copies // 3, 1))
        mesh = H.Mesh(P, None, None, np.arange(len(P), dtype=np.int32))
        sb.add_model(mesh, [H.scale(1.0)], H.Material(baseColor=tuple(rng.uniform(0, 1, 3)), metallic=0.3 * k), f"stack{k}")
    return S.SceneConfig("coincident", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1, max_depth=3)


def fuzz_scene(seed: int):
    import test_gpu_fuzz
    cfg, rng = test_gpu_fuzz.random_scene(seed)
    return cfg, int(rng.integers(0, 20)), int(rng.integers(1, 10))


def fuzz_properties(cfg) -> set:
    """What a fuzz scene exercises, read off its arrays."""
    p = cfg.packed
    props = set()
    n_emissive = int(np.any(p.materials[:, 0:3] > 0, axis=1).sum())
    props.add("no light" if len(p.lights) == 0 else "light")
    if n_emissive >= 2 and len(p.lights) >= 4:
        props.add("several lights")
    props.add("environment" if cfg.env_rgb is not None else "no environment")
    used = np.unique(p.triangles[:, 0:3].astype(np.int64))
    if np.any(np.all(p.vertices[used, 3:6] == 0, axis=1)):
        props.add("zero vertex normal")
    used_m = np.unique(p.triangles[:, 3].astype(np.int64))
    if np.any(p.materials[used_m, 10] == 0):
        props.add("roughness 0")
    for t in np.unique(p.triangles[:, 4].astype(np.int64)):
        if t >= 0:
            props.add(f"texture {cfg.textures[t][3]} channels")
    return props


# the eight fuzz seeds and what each is there for (asserted by test_fuzz_seeds_cover)
FUZZ_SEEDS = (14, 2, 17, 16, 4, 5, 7, 23)
FUZZ_NEED = ("no light", "several lights", "environment", "no environment", "zero vertex normal", "roughness 0",
             "texture 1 channels", "texture 3 channels", "texture 4 channels")
GPU_FUZZ_SEEDS = FUZZ_SEEDS[:4]


def extreme_scene(seed: int, exp10: int):
    """tests/test_gpu_fuzz.py test_random_scene_extreme_emission's scene."""
    cfg, first, _ = fuzz_scene(seed)
    mats = cfg.packed.materials.copy()
    mats[:, 0:3] = (mats[:, 0:3].astype(np.float64) * 10.0 ** exp10).astype(F)
    cfg = dataclasses.replace(cfg, packed=dataclasses.replace(cfg.packed, materials=mats), max_depth=4)
    return cfg, first, 3


def image_cases():
    """name -> (build() -> (cfg, first frame, frames), used by the GPU test)."""
    cases = {}
    for depth in range(5):
        for first, n in ((0, 1), (0, 4), (7, 3)):
            def c1(depth=depth, first=first, n=n):
                return dataclasses.replace(S.cornell_c1(64, 48), max_depth=depth), first, n
            cases[f"C1/d{depth}/f{first}x{n}"] = (c1, depth == 4 and first == 0 and n == 4)
    cases["C1/d4/f255x2"] = (lambda: (S.cornell_c1(64, 48), 255, 2), True)       # crosses a Gray-code top bit
    cases["C3/f0x2"] = (lambda: (S.marry_c3(96, 54), 0, 2), True)
    cases["C4/f0x2"] = (lambda: (S.teapot_c4(96, 54), 0, 2), True)
    for seed in FUZZ_SEEDS:
        cases[f"fuzz{seed}"] = (lambda seed=seed: fuzz_scene(seed), seed in GPU_FUZZ_SEEDS)
    cases["coincident130"] = (lambda: (coincident_scene(130), 0, 3), True)
    cases["emission1e-30"] = (lambda: extreme_scene(206, -30), False)
    cases["emission1e25"] = (lambda: extreme_scene(205, 25), False)
    cases["lamp65/f0x3"] = (lambda: (LAMPS.lamp_scene(63), 0, 3), True)           # 65 lights: GetLightIndex's search, not a scan
    return cases


# ---- function inputs ------------------------------------------------------------
def fw(*cols) -> np.ndarray:
    """Columns (float32 -> bits, integers as they are) side by side as u32 words."""
    out = []
    for c in cols:
        c = np.asarray(c)
        c = c.reshape(len(c), -1)
        out.append(c.astype(F).view(U) if c.dtype.kind == "f" else c.astype(np.int64).astype(U))
    return np.ascontiguousarray(np.concatenate(out, axis=1), U)


def unit(rng, n):
    v = rng.standard_normal((n, 3)).astype(F)
    return (v / np.sqrt((v * v).sum(1, dtype=F))[:, None]).astype(F)


def frames(n_):
    """Tangent frames the way BuildTangentSpace makes them (any float32 rounding will do: inputs)."""
    t = np.cross(n_, np.array([0, 0, 1], F)).astype(F)
    ln = np.sqrt((t * t).sum(1, dtype=F))
    bad = ~(ln > 0)
    ln[bad] = 1
    t = (t / ln[:, None]).astype(F)
    t[bad] = (1, 0, 0)
    return t, np.cross(n_, t).astype(F)


def materials(rng, n):
    """Material records (18 floats, struct order): every parameter at 0, at 1 and at random."""
    m = rng.random((n, 18)).astype(F)
    m[:, 0:3] *= F(20)
    pick = rng.integers(0, 3, (n, 15))
    body = m[:, 3:]
    body[pick == 0] = 0
    body[pick == 1] = 1
    k = n // 16
    m[:k, 3:6] = 0                       # black base colour: Cdlum = 0
    m[k:2 * k, 3:] = 0                   # every parameter 0
    m[2 * k:3 * k, 3:] = 1               # every parameter 1
    return m


def inv_wang_hash(h: int) -> int:
    """The seed whose wang_hash value is h (every step is a bijection of u32)."""
    M = 0xFFFFFFFF

    def unshift(x, k):
        r = x
        for _ in range(32 // k + 1):
            r = x ^ (r >> k)
        return r
    s = unshift(h, 15)
    s = (s * pow(0x27d4eb2d, -1, 1 << 32)) & M
    s = unshift(s, 4)
    s = (s * pow(9, -1, 1 << 32)) & M
    return unshift(s, 16) ^ 61


def _brdf_inputs(rng, n):
    N = unit(rng, n)
    V = unit(rng, n)
    L = unit(rng, n)
    flipv = (V * N).sum(1) < 0
    V[flipv & (rng.random(n) < 0.8)] *= -1          # most V, L in the upper hemisphere; some below (NdotV < 0)
    flipl = (L * N).sum(1) < 0
    L[flipl & (rng.random(n) < 0.8)] *= -1
    k = n // 10
    L[:k] = -V[:k]                                   # L = -V: H = normalize(0)
    N[k:3 * k] = (0, 0, 1)                           # N = +z: in-plane vectors have N.x exactly 0
    L[k:2 * k, 2] = 0                                # NdotL exactly 0
    V[2 * k:3 * k, 2] = 0                            # NdotV exactly 0
    V[2 * k:2 * k + k // 4, :] = L[2 * k:2 * k + k // 4, :] * (1, 1, 0)   # both 0
    T, B = frames(N)
    return V, N, L, T, B


def fn_cases(cfgs):
    """name -> (fn, scene key, words).  cfgs: scene key -> cfg (for the sizes the inputs need)."""
    rng = np.random.default_rng(SEED)
    n = 4000
    cases = {}
    V, N, L, T, B = _brdf_inputs(rng, n)
    cases["DisneyBRDF"] = (0, "fuzz", fw(V, N, L, T, B, materials(rng, n)))

    # SampleDisneyBRDF: every lobe, and r exactly on both thresholds
    V, N, L, T, B = _brdf_inputs(rng, n)
    seeds = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    mats = materials(rng, n)
    r12 = rng.random((n, 2)).astype(F)
    edge = []
    # metallic 0, clearcoat 0: pDiffuse = 0.5, pDiffuse + pSpecular = 1; metallic 1, clearcoat 1: 0 and 0.8f
    half = [(1 << 31) - 200, (1 << 31) - 64, 1 << 31, (1 << 31) + 128, (1 << 31) + 129, (1 << 31) + 400]
    top = [(1 << 32) - 1, (1 << 32) - 128, (1 << 32) - 129, (1 << 32) - 300]
    p8 = int(F(1) / F(1.25) * F(4294967296.0))
    eight = [p8 - 300, p8 - 128, p8, p8 + 128, p8 + 129, p8 + 300, 0, 1]
    for hs, met, cc in ((half, 0.0, 0.0), (top, 0.0, 0.0), (eight, 1.0, 1.0)):
        for h in hs:
            edge.append((inv_wang_hash(h), met, cc))
    for i, (sd, met, cc) in enumerate(edge):
        seeds[i] = sd
        mats[i, 7] = met
        mats[i, 14] = cc
    r12[len(edge):len(edge) + 40, 1] = np.tile(np.array([0, 1], F), 20)
    cases["SampleDisneyBRDF"] = (1, "fuzz", fw(seeds, V, N, T, B, mats, r12))

    for name, fn in (("SampleGTR1", 2), ("SampleGTR2", 3)):
        Nn = unit(rng, n)
        Tt, Bb = frames(Nn)
        v = unit(rng, n)
        r = rng.random((n, 2)).astype(F)
        r[:200, 1] = np.tile(np.array([0, 1], F), 100)
        r[200:300, 0] = np.tile(np.array([0, 1], F), 50)
        alpha = rng.choice(np.array([0.001, 0.1, 0.5, 1.0], F), n)
        alpha[n // 2:] = rng.random(n - n // 2).astype(F)
        cases[name] = (fn, "fuzz", fw(Nn, Tt, Bb, v, r, alpha))

    Nn = unit(rng, n)
    Tt, Bb = frames(Nn)
    cases["SampleCosineHemisphere"] = (4, "fuzz", fw(rng.integers(0, 1 << 32, n, dtype=np.uint64), Nn, Tt, Bb))

    Nn = unit(rng, n)
    thr = F(0.9999995)
    zs = [np.nextafter(thr, F(0)), thr, np.nextafter(thr, F(2)), F(1), F(-1), F(0.99999), np.nextafter(F(1), F(0))]
    for i, z in enumerate(zs):
        s = np.sqrt(max(0.0, 1.0 - float(z) ** 2))
        Nn[i] = (s, 0, z)
        Nn[i + len(zs)] = (0, s, z)
    Nn[2 * len(zs)] = (0, 0, 1)
    Nn[2 * len(zs) + 1] = (0, 0, -1)
    Nn[2 * len(zs) + 2] = (-0.0, 0.0, 1)
    cases["BuildTangentSpace"] = (5, "fuzz", fw(Nn))

    nh = (rng.random(n) * 2 - 1).astype(F)
    nh[:8] = (0, 1, -1, 0.5, 1, 0, -0.0, 1)
    a = rng.random(n).astype(F)
    a[:200] = rng.choice(np.array([1.0, 1.5, 0.001, 0.1, 0.0, 2.0], F), 200)
    cases["GTR1"] = (6, "fuzz", fw(nh, a))
    cases["GTR2"] = (7, "fuzz", fw(nh, np.where(rng.random(n) < 0.1, F(0.001), rng.random(n).astype(F))))
    d = (rng.random((n, 3)) * 2 - 1).astype(F)
    ax = np.maximum(F(0.001), rng.random((n, 2)).astype(F) ** 2).astype(F)
    ax[:100] = F(0.001)
    cases["GTR2_aniso"] = (8, "fuzz", fw(d, ax))
    nv = rng.random(n).astype(F)
    nv[:4] = (0, 1, 0.5, -0.0)
    cases["smithG_GGX"] = (9, "fuzz", fw(nv, np.where(rng.random(n) < 0.3, F(0.25), rng.random(n).astype(F))))
    cases["smithG_GGX_aniso"] = (10, "fuzz", fw(nv, (rng.random((n, 2)) * 2 - 1).astype(F), ax))

    v = unit(rng, n)
    poles = [(0, 1, 0), (0, -1, 0), (-1, 0, 0.0), (-1, 0, -0.0), (-0.5, 0.5, 0.0), (-0.5, 0.5, -0.0), (1, 0, 0), (0, 0, 1),
             (0, 0, -1), (0.0, 0.0, 0.0), (-1e-20, 0, 1e-30), (-1e-20, 0, -1e-30), (0, np.nextafter(F(1), F(0)), 0)]
    v[:len(poles)] = np.array(poles, F)
    cases["toSphericalCoord"] = (11, "fuzz", fw(v))
    cases["GetHDRImageColor"] = (12, "fuzz", fw(v))
    cases["GetHDRImageColor/1k"] = (12, "C4", fw(v[:1000]))
    sd = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    cases["SampleHDRImage"] = (13, "fuzz", fw(sd))
    cases["SampleHDRImage/1k"] = (13, "C4", fw(sd[:1000]))

    u = rng.random(600).astype(F)
    u[:8] = (0, 1, 1 / 3, 2 / 3, 0.5, np.nextafter(F(1 / 3), F(1)), np.nextafter(F(2 / 3), F(0)), 1e-30)
    for key in ("lights0", "lights1", "lights5", "fuzz"):
        cases[f"GetLightIndex/{key}"] = (14, key, fw(u))

    for key in ("fuzz", "C1"):
        nt = len(cfgs[key].packed.triangles)
        ti = rng.integers(0, nt, n)
        uu = rng.random((n, 2)).astype(F)
        uu[:6] = ((0, 0), (1, 0), (0, 1), (1, 1), (0.25, 0.5), (0, 0.5))
        if key == "fuzz":
            p = cfgs[key].packed
            zero = np.flatnonzero(np.all(p.vertices[p.triangles[:, 0:3].astype(np.int64), 3:6] == 0, axis=2).any(axis=1))
            assert len(zero), "the fuzz scene of the function cases needs a zero vertex normal"
            ti[:200] = rng.choice(zero, 200)
        cases[f"TriangleSample/{key}"] = (15, key, fw(ti, uu))
    uu = rng.random((n, 2)).astype(F)
    uu[:4] = ((0, 0), (1, 1), (0, 1), (1, 0))
    cases["UniformSampleTriangle"] = (16, "fuzz", fw(uu))

    i = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    i[:12] = (0, 1, 2, 255, 256, 257, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, (1 << 32) - 1, 1 << 30, 3 << 30)
    cases["sobolVec2"] = (17, "fuzz", fw(i, rng.integers(0, 4, n)))

    c = cfgs["fuzz"]
    p2 = rng.random((n, 2)).astype(F)
    p2[:6] = ((0, 0), (1, 1), (1, 0), (0.5, 1), (np.nextafter(F(1), F(0)),) * 2, (1e-8, 1e-8))
    cases["CranleyPattersonRotation"] = (18, "fuzz", fw(rng.integers(0, c.width, n), rng.integers(0, c.height, n), p2))
    s = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    s[:4] = (0, 1, (1 << 32) - 1, 61)
    cases["wang_hash"] = (19, "fuzz", fw(s))
    st = rng.random((n, 2)).astype(F)
    st[:4] = ((0, 0), (1, 1), (0, 1), (0.5, 0.5))
    cases["CameraGetRay"] = (20, "fuzz", fw(st))
    for key in ("fuzz", "C3"):
        cases[f"GetMaterial/{key}"] = (21, key, fw(np.arange(-1, len(cfgs[key].packed.materials) + 1)))

    # the intersection routines under the GLSL's own rules (sem 0), on the ray families of isect_rays
    for key in ("C1", "fuzz", "coincident"):
        cfg = cfgs[key]
        for fam in IR.FAMILIES:
            rays = IR.make_rays(cfg.packed, cfg.camera, fam, 2000, SEED)
            cases[f"BVHIntersect/{key}/{fam}"] = (25, key, fw(rays))
            cases[f"BVHIntersectP/{key}/{fam}"] = (26, key, fw(rays))
        rays, idx = IR.make_pairs(cfg.packed, 6000, SEED, "tri")          # a share aimed at edges and vertices
        cases[f"TriangleIntersect/{key}"] = (23, key, fw(rays, idx))
        cases[f"TriangleIntersectP/{key}"] = (24, key, fw(rays, idx))
        rays, idx = IR.make_pairs(cfg.packed, 6000, SEED, "box")
        cases[f"BoundIntersect/{key}"] = (22, key, fw(rays, idx))

    # a list of 300: the u of the short lists, then every prefix area over the sum and its float neighbours
    # (ties and boundaries of the search); no draw from rng, which the cases above share
    p = cfgs["lamp300"].packed
    edge = (p.lights[:, 1].astype(F) / F(p.lights_sum_area)).astype(F)
    ul = np.concatenate([u, edge, np.nextafter(edge, F(0)), np.nextafter(edge, F(2))]).astype(F)
    cases["GetLightIndex/lamp300"] = (14, "lamp300", fw(ul))
    return cases


FN_SCENE_SEED = 4        # the fuzz scene of the function cases: environment, lights, textures, a zero vertex normal


def fn_scenes():
    fuzz = fuzz_scene(FN_SCENE_SEED)[0]
    c1 = S.cornell_c1(64, 48)
    idx = c1.packed.lights[:, 0] if len(c1.packed.lights) else np.zeros(1, F)

    def with_lights(rows):
        L = np.array(rows, F).reshape(-1, 3)
        total = float(L[-1, 1]) if len(L) else 0.0
        return dataclasses.replace(c1, packed=dataclasses.replace(c1.packed, lights=L, lights_sum_area=total))
    i0, i1 = float(idx[0]), float(idx[-1])
    return {"fuzz": fuzz, "C1": c1, "C3": S.marry_c3(96, 54), "C4": S.teapot_c4(96, 54), "coincident": coincident_scene(130),
            "lamp300": LAMPS.lamp_scene(298), "lights0": with_lights([]), "lights1": with_lights([(i0, 2.5, 0)]),
            # equal prefix areas: entries 1 and 3 repeat their predecessor's (zero-area lights)
            "lights5": with_lights([(i0, 1, 0), (i1, 1, 0), (3, 2, 0), (4, 2, 0), (5, 3, 0)])}


INT_COLUMNS = {1: [4], 4: [3], 13: [7], 14: [0], 15: [8, 9], 17: [], 19: [0, 1], 22: [0], 23: [0, 9, 10], 24: [0, 9, 10],
               25: [0, 9, 10], 26: [0, 9, 10]}


def differing(fn: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Mask of differing words; two NaNs in a float column count as equal."""
    d = a != b
    fa, fb_ = a.view(F), b.view(F)
    both_nan = np.isnan(fa) & np.isnan(fb_)
    both_nan[:, INT_COLUMNS.get(fn, [])] = False
    return d & ~both_nan


def canonical(fn: int, words: np.ndarray) -> np.ndarray:
    """The words with every NaN of a float column as 0x7fc00000, so that hashes
    follow the same rule (fn -1: an image, every column a float)."""
    w = np.array(words, U, copy=True)
    nan = np.isnan(w.view(F))
    nan[:, INT_COLUMNS.get(fn, [])] = False
    w[nan] = 0x7FC00000
    return w


def oracle_fn(oracle, fn: int, words: np.ndarray) -> np.ndarray:
    """The oracle's side of a function case: pno_shade_eval, or pno_intersect under the GLSL's rules."""
    if fn < 22:
        return oracle.shade_eval(fn, words)
    kind = {22: 4, 23: 2, 24: 3, 25: 0, 26: 1}[fn]
    rays = words[:, :7].view(F)
    idx = words[:, 7].astype(np.int32) if words.shape[1] == 8 else None
    return oracle.intersect(rays, kind, 0, idx)
