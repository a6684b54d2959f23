"""The frame-number domain of pnrt_render against the CPU oracle.

A still view accumulates until the camera moves: frame 2^16 after half a
minute, 2^24 after two hours.  Everything that depends on the frame number --
the per-batch Sobol table of pt_wf_gen_setup (grayCode(frame + 1): bits 8..31),
gen's own bounce-0 Sobol pair, the v1 kernel's frame loop, the seed product
frame * 26699 (wraps from frame 160 871 on) and the blend weight
1 / (float)(frame + 1) (uint -> float rounds above 2^24) -- is rendered here on
both sides of bit 8, 16, 24 and 31 and up to the last frame number,
0xFFFFFFFE, on a Cornell box and on the env + bunny scene, by the wavefront
and the v1 kernel.  The accumulation starts from zero at `first`, so pixel
values are of order 1 / first: fine for a bitwise comparison, and the oracle
image is required to be finite and non-zero so it cannot be a degenerate one.

Past the end (first + n > 0xFFFFFFFF: frame 0xFFFFFFFF has the weight 1 / 0)
pnrt_render refuses the call, queues nothing and leaves the accumulation as it
was; PathTracer.render refuses what a uint32 cannot hold.

Tolerance: 0 ulp (uint32 views compared)."""
import numpy as np
import pytest

import pyoracle
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import KERNEL_V1, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

CASES = [(0xFF - 2, 6),            # Sobol table entries on both sides of bit 8
         (0xFFFF - 2, 6),          # bit 16; the seed product has not wrapped yet
         (0xFFFFFF - 2, 6),        # bit 24; blend weights at 2^24 - 1 .. 2^24 + 4 (ties to even)
         (0x1000000 - 70, 140),    # two batches (128 + 12), the second starting above 2^24
         (0x7FFFFFFF - 2, 6),      # across 2^31 (signed / unsigned)
         (0xFFFFFFFF - 6, 6)]      # up to frame 0xFFFFFFFE, weight 1 / (float)0xFFFFFFFF
F24 = 0xFFFFFF - 2

_scenes, _refs = {}, {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = S.cornell_c1(64, 48) if name == "C1" else S.CONFIGS["C2"](width=80, height=48, spp=4)
        assert _scenes[name].max_depth == 4
    return _scenes[name]


def oracle(name, first, n):
    """The oracle's image of frames first .. first + n - 1 (computed once, shared, read-only)."""
    key = (name, first, n)
    if key not in _refs:
        ref, st = pyoracle.Oracle(scene(name)).render(first, n)
        assert st["stack_overflow"] == 0
        assert np.isfinite(ref).all() and (ref[..., :3] > 0).any(), "degenerate oracle image"
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


def assert_bitwise(got, ref, what):
    g, r = got.view(np.uint32), ref.view(np.uint32)
    bad = np.argwhere(np.any(g != r, axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {bad[:5].tolist()} " \
                          f"gpu={got[tuple(bad[0])]} oracle={ref[tuple(bad[0])]}"


@pytest.mark.parametrize("mode", [TRAVERSE_ZCULL, TRAVERSE_ZCULL | KERNEL_V1], ids=["wavefront", "v1"])
@pytest.mark.parametrize("first,n", CASES, ids=[f"{f:#x}+{n}" for f, n in CASES])
@pytest.mark.parametrize("name", ["C1", "C2"])
def test_high_frame_numbers_vs_oracle(pt, name, first, n, mode):
    ref = oracle(name, first, n)
    pt.load(scene(name), mode)
    pt.reset_accum()
    pt.render(first, n)
    assert_bitwise(pt.read_accum(), ref, f"{name} mode {mode:#x} frames {first:#x}+{n}")


@pytest.mark.parametrize("name", ["C1", "C2"])
def test_pipelined_calls_across_2_24(pt, name):
    """Three back-to-back two-frame calls, no synchronisation, across frame 2^24:
    every call's own Sobol table and blend weights (first_frame + k per batch)."""
    ref = oracle(name, F24, 6)
    pt.load(scene(name), TRAVERSE_ZCULL)
    pt.reset_accum()
    for k in range(3):
        pt.render(F24 + 2 * k, 2)
    assert_bitwise(pt.read_accum(), ref, f"{name}: 3 x render({F24:#x} + 2k, 2)")


WRAPS = [(0xFFFFFFFD, 4),          # names frame 0xFFFFFFFF and wraps to 0
         (0xFFFFFFFF, 1),          # frame 0xFFFFFFFF alone: weight 1 / (float)0
         (0xFFFFFFFA, 6),          # ends on frame 0xFFFFFFFF
         (1, 0xFFFFFFFF)]


@pytest.mark.parametrize("mode", [TRAVERSE_ZCULL, TRAVERSE_ZCULL | KERNEL_V1], ids=["wavefront", "v1"])
def test_render_past_last_frame_is_refused(pt, mode):
    """first + n > 0xFFFFFFFF: PNRT_E_ARG with a message, no kernel launched, the
    accumulation bit for bit what it was -- and the context renders on afterwards."""
    c = scene("C1")
    pt.load(c, mode)
    pt.reset_accum()
    pt.render(5, 3)
    before = pt.read_accum()
    pt.profile_enable(True)
    try:
        for first, n in WRAPS:
            with pytest.raises(PnrtError, match="0xFFFFFFFF"):
                pt.render(first, n)
        pt.render(0xFFFFFFFF, 0)                       # no frames: nothing to refuse
        assert all(launches == 0 for _, launches in pt.profile_read().values())
    finally:
        pt.profile_enable(False)
    assert np.array_equal(pt.read_accum().view(np.uint32), before.view(np.uint32))
    pt.render(8, 1)
    assert_bitwise(pt.read_accum(), oracle("C1", 5, 4), "frames 5..8 around refused calls")


def test_python_render_refuses_what_uint32_truncates(pt):
    """2**32 + 5 must not become frame 5 on its way through ctypes."""
    pt.load(scene("C1"))
    pt.reset_accum()
    pt.render(5, 3)
    before = pt.read_accum()
    for first, n in [(2**32 + 5, 1), (2**32, 1), (-1, 1), (0, 2**32), (0, -1)]:
        with pytest.raises(ValueError):
            pt.render(first, n)
    assert np.array_equal(pt.read_accum().view(np.uint32), before.view(np.uint32))
