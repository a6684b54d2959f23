"""The oracle's shading half, and its intersection code under the GLSL's own
rules, pinned to the reference's shader TEXT.

oracle/_ref/shader_driver is shaders/ray_tracing.comp itself, translated to C++
by text surgery (oracle/shader/translate.py) and compiled against a shim that
supplies only what the text does not define (oracle/shader/glsl_shim.hpp: the
oracle's libm, vector forms, min/max, samplers; DESIGN.md 7 lists them).  Every
comparison is on raw 32-bit words, no tolerance; two NaNs count as equal.

  * per function: pno_shade_eval / pno_intersect(sem 0) -- the very functions
    pno_render runs -- against the shader's function of the same name, on a few
    thousand seeded inputs plus the edges (tests/shader_pin.py fn_cases);
  * whole images: pyoracle.Oracle.render against the translated main() run per
    pixel and frame (tests/shader_pin.py image_cases).

The *_fixture cases check the oracle against what the driver wrote when
tests/golden/make_shader_golden.py ran (tests/golden/shader_fixtures.json,
shader_samples.npz) and never skip; the *_live cases run where the driver is
built, compare word by word, and check that the fixtures are what the driver
produces now.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import shader_pin as SP  # noqa: E402
import pyoracle  # noqa: E402

FIX = json.load(open(os.path.join(SP.GOLD, "shader_fixtures.json")))
SAMPLES = np.load(os.path.join(SP.GOLD, "shader_samples.npz"))
live = pytest.mark.skipif(not os.path.exists(SP.DRIVER), reason="oracle/_ref/shader_driver is built only beside the reference tree")
U = np.uint32


@pytest.fixture(scope="module")
def fn_world():
    cfgs = SP.fn_scenes()
    return {"cfgs": cfgs, "cases": SP.fn_cases(cfgs), "oracles": {k: pyoracle.Oracle(c) for k, c in cfgs.items()},
            "blobs": {}}


def oracle_words(world, name):
    fn, key, words = world["cases"][name]
    return fn, key, words, SP.oracle_fn(world["oracles"][key], fn, words)


def check_properties(name, fn, words, out):
    """The edges a case is there for are present in what it computed."""
    if fn >= 22:
        hits = int(out[:, 0].sum())
        assert 0 < hits < len(out), f"{name}: {hits} hits of {len(out)}"
    if name == "SampleDisneyBRDF":
        # the seed afterwards: one draw on the specular / clearcoat lobes, three on the diffuse lobe
        s1 = wang_hash_np(words[:, 0])
        s3 = wang_hash_np(wang_hash_np(s1))
        one, three = out[:, 4] == s1, out[:, 4] == s3
        assert one.any() and three.any() and (one | three).all()
        # all three lobes, by the thresholds in double precision with a margin
        with np.errstate(invalid="ignore"):
            f = words.view(np.float32).astype(np.float64)
        rd, rc = 1.0 - f[:, 20], 0.25 * f[:, 27]
        r = s1.astype(np.float64) / 2.0 ** 32
        p_d, p_ds = rd / (rd + 1.0 + rc), (rd + 1.0) / (rd + 1.0 + rc)
        assert (r < p_d - 1e-3).any() and ((r > p_d + 1e-3) & (r < p_ds - 1e-3)).any() and (r > p_ds + 1e-3).any()
        assert three[r < p_d - 1e-3].all() and one[r > p_d + 1e-3].all()
    if name.startswith("SampleHDRImage"):
        sin_theta = out[:, 4].view(np.float32)
        assert (sin_theta <= 1e-10).any() and (sin_theta > 1e-10).any(), "both sides of max(1e-10, sin theta)"
    if name == "GetLightIndex/lights0":
        assert (out == 0xFFFFFFFF).all()
    if name == "GetLightIndex/lights5":
        assert len(np.unique(out)) >= 3
    if name == "GetLightIndex/lamp300":
        assert len(np.unique(out)) > 200
    if name == "GTR1":
        assert (words[:, 1].view(np.float32) >= 1).any()


def wang_hash_np(s):
    s = np.asarray(s, np.uint64)
    M = np.uint64(0xFFFFFFFF)
    s = ((s ^ np.uint64(61)) ^ (s >> np.uint64(16))) & M
    s = (s * np.uint64(9)) & M
    s = s ^ (s >> np.uint64(4))
    s = (s * np.uint64(0x27d4eb2d)) & M
    s = s ^ (s >> np.uint64(15))
    return s.astype(U)


def test_inverse_hash_and_fuzz_seeds_cover():
    """The helpers the cases rest on: the seeds aimed at the lobe thresholds hash to
    their targets, and the eight fuzz scenes together have every property asked for."""
    for h in (0, 1, 1 << 31, (1 << 32) - 1, 0x12345678):
        assert int(wang_hash_np([SP.inv_wang_hash(h)])[0]) == h
    have = set()
    for seed in SP.FUZZ_SEEDS:
        have |= SP.fuzz_properties(SP.fuzz_scene(seed)[0])
    for need in SP.FUZZ_NEED:
        assert need in have, f"no fuzz seed of {SP.FUZZ_SEEDS} has: {need}"
    assert SP.fuzz_properties(SP.fuzz_scene(SP.FN_SCENE_SEED)[0]) >= {"environment", "light", "zero vertex normal"}


def test_fixture_lists_every_case(fn_world):
    assert set(FIX["functions"]) == set(fn_world["cases"])
    assert set(FIX["images"]) == set(SP.image_cases())


@pytest.mark.parametrize("name", list(FIX["functions"]))
def test_function_fixture(fn_world, name):
    fn, key, words, got = oracle_words(fn_world, name)
    fx = FIX["functions"][name]
    assert SP.sha(words) == fx["in_sha256"], f"{name}: input generator drifted"
    check_properties(name, fn, words, got)
    got = SP.canonical(fn, got)
    ref = SAMPLES[f"fn/{name}"]
    bad = np.nonzero(np.any(got[:len(ref)] != ref, axis=1))[0]
    assert not len(bad), f"{name}: record {bad[0]}: oracle {got[bad[0]].tolist()} shader text {ref[bad[0]].tolist()}"
    assert SP.sha(got) == fx["out_sha256"], f"{name}: oracle != shader text beyond the {len(ref)} sampled records"
    print(f"{name}: {got.size} words compared, 0 differ")


@live
@pytest.mark.parametrize("name", list(FIX["functions"]))
def test_function_live(fn_world, name):
    fn, key, words, got = oracle_words(fn_world, name)
    if key not in fn_world["blobs"]:
        fn_world["blobs"][key] = SP.scene_blob(fn_world["cfgs"][key])
    ref = SP.driver_fn(fn_world["cfgs"][key], fn, words, blob=fn_world["blobs"][key])
    d = SP.differing(fn, got, ref)
    print(f"{name}: {ref.size} words compared, {int(d.sum())} differ")
    rows = np.flatnonzero(d.any(axis=1))
    assert not len(rows), (f"{name}: {int(d.sum())} of {ref.size} words differ; first record {rows[0]}: input "
                           f"{words[rows[0]].tolist()} oracle {got[rows[0]].tolist()} shader text {ref[rows[0]].tolist()}")
    assert SP.sha(SP.canonical(fn, ref)) == FIX["functions"][name]["out_sha256"], f"{name}: the fixture is stale"


def image_words(img):
    return SP.canonical(-1, np.ascontiguousarray(img, np.float32).view(U).reshape(-1, 4))


@pytest.mark.parametrize("name", list(FIX["images"]))
def test_image_fixture(name):
    cfg, first, n = SP.image_cases()[name][0]()
    fx = FIX["images"][name]
    assert (cfg.width, cfg.height, cfg.max_depth, first, n) == (fx["width"], fx["height"], fx["depth"], fx["first"], fx["frames"])
    got, _ = pyoracle.Oracle(cfg).render(first, n)
    ref = SAMPLES[f"img/{name}"]
    part = got[..., :3] if fx["full"] else got[::4, :, :3]
    d = SP.differing(-1, np.ascontiguousarray(part).view(U).reshape(-1, 3), ref.view(U).reshape(-1, 3))
    assert not d.any(), f"{name}: {int(d.sum())} of {d.size} recorded words differ from the shader text's image"
    assert SP.sha(image_words(got)) == fx["sha256"], f"{name}: oracle image != shader text's outside the recorded rows"
    print(f"{name}: {got.size} words compared, 0 differ")


@live
@pytest.mark.parametrize("name", list(FIX["images"]))
def test_image_live(name):
    cfg, first, n = SP.image_cases()[name][0]()
    got, _ = pyoracle.Oracle(cfg).render(first, n)
    ref = SP.driver_image(cfg, first, n)
    d = SP.differing(-1, got.view(U).reshape(-1, 4), ref.view(U).reshape(-1, 4))
    print(f"{name}: {ref.size} words compared, {int(d.sum())} differ")
    px = np.flatnonzero(d.any(axis=1))
    assert not len(px), (f"{name}: {len(px)} of {len(d)} pixels differ; first (x {px[0] % cfg.width}, y {px[0] // cfg.width}): "
                         f"oracle {got.reshape(-1, 4)[px[0]].tolist()} shader text {ref.reshape(-1, 4)[px[0]].tolist()}")
    assert SP.sha(image_words(ref)) == FIX["images"][name]["sha256"], f"{name}: the fixture is stale"


# ---- the translator's own rules, on made-up text ---------------------------------
def _translator():
    sys.path.insert(0, os.path.join(SP.REPO, "oracle", "shader"))
    import translate
    return translate


TOY = """#version 450 core
layout(local_size_x = 8) in;
uniform int N;
uint state;
float draw() { state = state * 3u + 1u; return float(state) * 0.5; }
float two(float a, float b) { return a - b; }
void fill(out vec3 v, in float s) { v = vec3(s).rgb; }
void main() { vec2 p = vec2(draw(), draw()); %s }
"""


def test_translator_orders_side_effects():
    T = _translator()
    out, info = T.translate(TOY % "")
    assert "vec2{draw(), draw()}" in out and info["braced"] == 1
    assert "0.5f" in out and "3u" in out and "uniform" not in out and "layout" not in out
    assert "vec3& v, float s" in out and ".rgb()" in out and "shader_main" in out
    for bad in ("float d = two(draw(), draw());", "float d = draw() - draw();"):
        with pytest.raises(T.TranslateError):
            T.translate(TOY % bad)
    T.translate(TOY % "float a = draw(), b = draw(); float d = two(draw(), 1.0);")
