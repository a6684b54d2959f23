"""The GPU against the reference's shader text, with the oracle out of the loop.

tests/golden/shader_samples.npz holds the accumulation images that
shaders/ray_tracing.comp itself, compiled as C++ (oracle/shader/), wrote when
tests/golden/make_shader_golden.py ran.  The library's read_accum must equal
them bit for bit in every traversal mode.  Only tests/golden/ is read: neither
the reference tree nor the driver.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import shader_pin as SP  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = json.load(open(os.path.join(SP.GOLD, "shader_fixtures.json")))
CASES = [name for name, fx in FIX["images"].items() if fx["full"]]


@pytest.fixture(scope="module")
def pt():
    from pnraytracing_amd.tracer import PathTracer
    with PathTracer(0) as t:
        yield t


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(SP.GOLD, "shader_samples.npz"))


def test_cases_are_the_ones_asked_for():
    want = {"C1/d4/f0x4", "C1/d4/f255x2", "C3/f0x2", "C4/f0x2", "coincident130", "lamp65/f0x3"} | {f"fuzz{s}" for s in SP.GPU_FUZZ_SEEDS}
    assert set(CASES) == want and len(SP.GPU_FUZZ_SEEDS) == 4


@pytest.mark.parametrize("name", CASES)
def test_gpu_equals_shader_text(pt, golden, name):
    from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_EXACT, TRAVERSE_ZCULL
    cfg, first, n = SP.image_cases()[name][0]()
    fx = FIX["images"][name]
    assert (cfg.width, cfg.height, cfg.max_depth, first, n) == (fx["width"], fx["height"], fx["depth"], fx["first"], fx["frames"])
    ref = np.ones((cfg.height, cfg.width, 4), np.float32)
    ref[..., :3] = golden[f"img/{name}"]
    assert SP.sha(SP.canonical(-1, ref.view(np.uint32).reshape(-1, 4))) == fx["sha256"]
    for mode in (TRAVERSE_ZCULL, TRAVERSE_EXACT, TRAVERSE_ZCULL | KERNEL_V1):
        pt.load(cfg, mode)
        pt.reset_accum()
        pt.render(first, n)
        got = pt.read_accum()
        d = SP.differing(-1, got.view(np.uint32).reshape(-1, 4), ref.view(np.uint32).reshape(-1, 4))
        print(f"{name} mode {mode:#x}: {d.size} words compared, {int(d.sum())} differ")
        assert not d.any(), f"{name} mode {mode:#x}: {int(d.any(axis=1).sum())} of {len(d)} pixels differ from the shader text's image"
