"""The batch plan of pnrt_render (pnrt_batch_plan, PNRT_BATCH_BYTES) and
multi-batch, growing and leaf-table calls issued while other calls are in
flight, against the CPU oracle.

Plan: an uncapped context reports bytes(k), the cap's own measure of a batch of
k frames; a context capped between bytes(4) and bytes(5) must plan 4 frames
per batch (the largest that fits -- halving 40 -> 20 -> 10 -> 5 -> 3 would
skip it), launch exactly the planned number of gen and blend kernels, and
render the oracle's image.  PNRT_BATCH_BYTES is read when the context is
created and parsed strictly.

In flight: a call with nothing in flight runs on the caller's stream; only a
call issued behind another one runs on a pipe's worker stream, where the wait
that keeps batch k + 1 from overwriting the colours batch k's blend still
reads (render_wavefront: `if (f0 && w != c->stream)`), the reallocation of a
pipe's buffers under calls in flight (grow) and the staggered start are.  Each
of these tests therefore first issues a call that keeps the GPU busy for at
least ten times as long as the host needs to submit the calls that follow (the
measured times are in each test's docstring), then the calls under test with
no synchronisation in between.  The first call's frames are part of the
compared sequence.  A missing dependency is a race and need not show on every
run: these tests are necessary, not sufficient.

Tolerance: 0 ulp (uint32 views compared)."""
import contextlib
import os

import numpy as np
import pytest

import pyoracle
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer, PnrtError

pytestmark = pytest.mark.gpu

_cache = {}


def cfg(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = S.CONFIGS[name](**kw)
    return _cache[key]


@pytest.fixture(scope="module")
def pt():
    t = PathTracer(0)
    yield t
    t.close()


@contextlib.contextmanager
def capped_tracer(cap):
    """A fresh context created with PNRT_BATCH_BYTES = cap in the environment."""
    os.environ["PNRT_BATCH_BYTES"] = str(cap)
    t = None
    try:
        t = PathTracer(0)
        yield t
    finally:
        del os.environ["PNRT_BATCH_BYTES"]
        if t is not None:
            t.close()


def assert_bitwise(got, ref, what):
    g, r = got.view(np.uint32), ref.view(np.uint32)
    bad = np.argwhere(np.any(g != r, axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} of {g.shape[0] * g.shape[1]} pixels differ, first {bad[:5].tolist()}"


def batch_bytes(pt, n):
    """bytes(k), k = 1..n, from an uncapped context: plan(k) is one batch of k frames."""
    plans = [pt.batch_plan(k) for k in range(1, n + 1)]
    assert [p["frames_per_batch"] for p in plans] == list(range(1, n + 1))
    assert all(p["n_batches"] == 1 for p in plans)
    by = [0] + [p["batch_bytes"] for p in plans]         # by[k] = bytes(k)
    assert all(b > a for a, b in zip(by, by[1:])), "bytes(k) must be strictly increasing"
    return by


def cap_for(by, k):
    """A cap that k frames fit and k + 1 do not, half way between the two."""
    return by[k] + (by[k + 1] - by[k]) // 2


def launches(pt):
    p = pt.profile_read()
    return {k: v[1] for k, v in p.items()}


def oracle_rows(c, frames, step, offset):
    ref = np.zeros((c.height, c.width, 4), np.float32)
    _, st = pyoracle.Oracle(c).render(0, frames, rows=(offset, c.height), y_step=step, accum=ref)
    assert st["stack_overflow"] == 0
    return ref, np.arange(offset, c.height, step)


# ---- the plan ---------------------------------------------------------------------------------
N40 = 40


@pytest.fixture(scope="module")
def c1():
    return S.cornell_c1(96, 64)


@pytest.fixture(scope="module")
def c1_ref(c1):
    ref, _ = pyoracle.Oracle(c1).render(0, N40)
    assert np.isfinite(ref).all() and (ref[..., :3] > 0).any()
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def c1_bytes(pt, c1):
    pt.load(c1)
    return batch_bytes(pt, N40)


def render_counted(t, c, n):
    t.load(c)
    t.reset_accum()
    t.profile_enable(True)
    t.render(0, n)
    got = t.read_accum()
    n_launch = launches(t)
    t.profile_enable(False)
    return got, n_launch


def test_plan_uncapped(pt, c1, c1_bytes, c1_ref):
    """One batch of up to 128 frames; two for 140; zeros for no frames and for a shard
    without rows; PNRT_E_STATE before set_frame; one gen and one blend launch."""
    pt.load(c1)
    assert pt.batch_plan(N40) == {"frames_per_batch": 40, "n_batches": 1, "batch_bytes": c1_bytes[40]}
    p = pt.batch_plan(140)
    assert (p["frames_per_batch"], p["n_batches"]) == (128, 2)
    zero = {"frames_per_batch": 0, "n_batches": 0, "batch_bytes": 0}
    assert pt.batch_plan(0) == zero
    assert pt.batch_plan(N40, 16, 8, 5) == zero                # 64 rows: bands 0..3, shard 5 has none
    half = pt.batch_plan(N40, 16, 2, 1)                        # a shard's plan measures the shard's rows
    assert half["frames_per_batch"] == 40 and 0 < half["batch_bytes"] < c1_bytes[40]
    with pytest.raises(PnrtError, match="bad shard"):
        pt.batch_plan(N40, 16, 2, 2)
    fresh = PathTracer(0)
    try:
        with pytest.raises(PnrtError, match=r"\(-3\)"):
            fresh.batch_plan(1)
    finally:
        fresh.close()
    got, n_launch = render_counted(pt, c1, N40)
    assert n_launch["gen"] == n_launch["blend"] == 1
    assert_bitwise(got, c1_ref, "uncapped: one batch of 40 frames")


def test_cap_takes_largest_fit(c1, c1_bytes, c1_ref):
    """A cap between bytes(4) and bytes(5): 4 frames per batch, 10 batches, 10 gen and 10
    blend launches, the oracle's image (halving from 40 would settle on 3)."""
    cap = cap_for(c1_bytes, 4)
    with capped_tracer(cap) as t:
        t.load(c1)
        p = t.batch_plan(N40)
        assert (p["frames_per_batch"], p["n_batches"]) == (4, 10)
        assert p["batch_bytes"] == c1_bytes[4] <= cap
        assert t.batch_plan(3) == {"frames_per_batch": 3, "n_batches": 1, "batch_bytes": c1_bytes[3]}
        got, n_launch = render_counted(t, c1, N40)
    assert n_launch["gen"] == n_launch["blend"] == 10
    assert_bitwise(got, c1_ref, "4 frames per batch")


def test_cap_below_one_frame(c1, c1_bytes, c1_ref):
    """A cap not even one frame fits: one frame per batch, 40 gen launches, same image."""
    with capped_tracer(c1_bytes[1] - 1) as t:
        t.load(c1)
        p = t.batch_plan(N40)
        assert (p["frames_per_batch"], p["n_batches"], p["batch_bytes"]) == (1, 40, c1_bytes[1])
        got, n_launch = render_counted(t, c1, N40)
    assert n_launch["gen"] == n_launch["blend"] == 40
    assert_bitwise(got, c1_ref, "1 frame per batch")


@pytest.mark.parametrize("k", [2, 7, 40])
def test_cap_edges(c1, c1_bytes, k):
    """bytes(k) itself fits k frames, one byte less fits k - 1, whatever the call's length."""
    with capped_tracer(c1_bytes[k]) as t:
        t.load(c1)
        assert t.batch_plan(N40)["frames_per_batch"] == k
        assert t.batch_plan(200) == {"frames_per_batch": k, "n_batches": -(-200 // k), "batch_bytes": c1_bytes[k]}
    with capped_tracer(c1_bytes[k] - 1) as t:
        t.load(c1)
        assert t.batch_plan(N40)["frames_per_batch"] == k - 1


def _parent_frames_per_batch(w, h, n):
    """The frame limit of an uncapped call: 128 frames, 2^28 - 1 path slots of 8x8 tiles."""
    per_frame = ((w + 7) // 8) * ((h + 7) // 8) * 64
    return min(n, 128, (2**28 - 1) // per_frame)


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160), (8192, 4320)])
def test_uncapped_plan_is_the_frame_limit(w, h):
    """No cap (none set, 0, or one nothing reaches): the plan at the BASELINE sizes
    (C2-C4 1080p, C5 4K) and at the largest frame the suite renders is the frame
    limit alone, as before there was a plan to ask."""
    for cap in (None, 0, 2**64 - 1):
        with (capped_tracer(cap) if cap is not None else contextlib.closing(PathTracer(0))) as t:
            t.set_frame(w, h, S._cornell_camera(w, h), 4)
            for n in (1, 4, 7, 8, 16, 40, 128, 200):
                p = t.batch_plan(n)
                fpb = _parent_frames_per_batch(w, h, n)
                assert (p["frames_per_batch"], p["n_batches"]) == (fpb, -(-n // fpb)), (cap, n, p)


@pytest.mark.parametrize("text", ["3e9", "abc", "-1", "", "12x", "18446744073709551616"])
def test_misspelt_cap_is_refused(text):
    """strtoull read `3e9` as a 3-byte cap and `abc` as no cap; pnrt_create refuses them."""
    os.environ["PNRT_BATCH_BYTES"] = text
    try:
        with pytest.raises(PnrtError, match="PNRT_BATCH_BYTES"):
            PathTracer(0)
    finally:
        del os.environ["PNRT_BATCH_BYTES"]


# ---- calls behind other calls -----------------------------------------------------------------
def test_multi_batch_calls_behind_another_call(pt):
    """C2 at 1920x1080 under a cap of 3 frames per batch: render(0, 24) (8 batches, on
    the caller's stream), then three 8-frame calls (3 batches each, on worker
    streams, each later batch waiting for the previous one's blend), frames
    0..47 on every 36th row vs the oracle; 17 gen launches as planned.
    Measured: the first call keeps the GPU busy for 31.8 ms after it returns; the
    three calls behind it are submitted in 0.35-0.40 ms (80 times less)."""
    c = cfg("C2")
    pt.load(c)
    cap = cap_for(batch_bytes(pt, 4), 3)
    with capped_tracer(cap) as t:
        t.load(c)
        plans = [t.batch_plan(n) for n in (24, 8, 8, 8)]
        assert [(p["frames_per_batch"], p["n_batches"]) for p in plans] == [(3, 8), (3, 3), (3, 3), (3, 3)]
        t.profile_enable(True)
        t.render(0, 24)
        for k in range(3):
            t.render(24 + 8 * k, 8)
        got = t.read_accum()
        n_launch = launches(t)
    assert n_launch["gen"] == n_launch["blend"] == sum(p["n_batches"] for p in plans) == 17
    ref, rows = oracle_rows(c, 48, 36, 7)
    assert_bitwise(got[rows], ref[rows], "C2 1080p: multi-batch calls on worker streams")


def test_growing_calls_in_flight(pt):
    """C2 at 1920x1080, no cap: an 8-frame call, then calls of 1, 5, 2, 9, 1 and 12
    frames back to back -- calls larger than any their pipe has seen, so its
    buffers are reallocated after a wait for the calls in flight -- frames 0..37
    on every 36th row vs the oracle.
    Measured: the first call keeps the GPU busy for 10.5-10.7 ms after it returns;
    the 1- and the 5-frame call behind it are submitted in 0.16 ms (65 times
    less).  The first reallocation is the 2-frame call's (small calls rotate
    over a third pipe, which the 1-frame call sized): it waits 19 ms for the
    three calls in flight; the 9- and the 12-frame call wait 4 and 13 ms."""
    c = cfg("C2")
    sizes = [8, 1, 5, 2, 9, 1, 12]
    pt.load(c)
    assert all(pt.batch_plan(n)["n_batches"] == 1 for n in sizes)
    pt.reset_accum()
    f = 0
    for n in sizes:
        pt.render(f, n)
        f += n
    got = pt.read_accum()
    ref, rows = oracle_rows(c, f, 36, 11)
    assert_bitwise(got[rows], ref[rows], "C2 1080p: growing calls")


def coincident_scene(copies, W, Hh):
    """tests/test_gpu_fuzz.py's coincident-triangle scene: one leaf of `copies` identical
    triangles, too large for an inline leaf ref (> 127 -> the leaf table)."""
    rng = np.random.default_rng(copies)
    sb = H.SceneBuilder()
    S._cornell_walls(sb, H.Material(baseColor=(0.6, 0.6, 0.6)))
    tri = np.array([[-1.0, 0.5, -1.0], [1.5, 0.7, -0.5], [0.0, 3.0, -1.2]], np.float32)
    for k in range(3):
        P = np.tile(tri, (copies // 3, 1))
        mesh = H.Mesh(P, None, None, np.arange(len(P), dtype=np.int32))
        sb.add_model(mesh, [H.scale(1.0)], H.Material(baseColor=tuple(rng.uniform(0, 1, 3)), metallic=0.3 * k),
                     f"stack{k}")
    return S.SceneConfig("coincident", sb.build(), S._cornell_camera(W, Hh), W, Hh, 1, max_depth=3,
                         env_rgb=None, env_table=None)


def test_leaf_table_scene_pipelined(pt):
    """The leaf-table instantiation of the trace kernels under pipelined calls: the
    130-coincident-triangle scene at 640x360, a 64-frame call, then six 2-frame
    calls back to back, frames 0..75 on every 12th row vs the oracle.
    Measured: the first call keeps the GPU busy for 10.6-10.7 ms after it returns;
    the six calls behind it are submitted in 0.25-0.26 ms (41 times less)."""
    c = coincident_scene(130, 640, 360)
    nd = c.packed.nodes
    leaves = nd[:, 7] == -1
    assert (nd[leaves, 9] - nd[leaves, 8]).max() > 127
    pt.load(c)
    assert pt.device_info()["has_leaf_table"] == 1
    pt.reset_accum()
    pt.render(0, 64)
    for k in range(6):
        pt.render(64 + 2 * k, 2)
    got = pt.read_accum()
    ref, rows = oracle_rows(c, 76, 12, 5)
    assert_bitwise(got[rows], ref[rows], "leaf-table scene: pipelined calls")


def test_staggered_multi_batch_calls(pt):
    """C4 at 1920x1080 under a cap of 8 frames per batch (16.6M paths: staggered calls,
    WF_STAGGER_PATHS = 12M): render(0, 16); render(16, 16) back to back -- two
    batches each, the second call on a worker stream, started from the first
    one's stage event -- equals the same 32 frames as four synchronised 8-frame
    calls, and the oracle on rows 0 and 701.
    Measured: the first call keeps the GPU busy for 12.4-12.5 ms after it returns;
    the second is submitted in 0.12-0.13 ms (94 times less)."""
    c = cfg("C4")
    pt.load(c)
    cap = cap_for(batch_bytes(pt, 9), 8)
    with capped_tracer(cap) as t:
        t.load(c)
        p = t.batch_plan(16)
        assert (p["frames_per_batch"], p["n_batches"]) == (8, 2)
        t.profile_enable(True)
        t.render(0, 16)
        t.render(16, 16)
        got = t.read_accum()
        assert launches(t)["gen"] == 4
        t.profile_enable(False)
        t.reset_accum()
        for k in range(4):
            t.render(8 * k, 8)
            t.synchronize()
        assert_bitwise(got, t.read_accum(), "C4 1080p: two staggered 2-batch calls vs four synchronised calls")
    o = pyoracle.Oracle(c)
    for y in (0, 701):
        ref, _ = o.render(0, 32, rows=(y, y + 1))
        assert_bitwise(got[y:y + 1], ref[y:y + 1], f"C4 1080p, 32 frames, row {y} vs oracle")
