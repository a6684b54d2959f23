"""pnrt_render_adaptive exists in include/pnrt.h, in the ctypes layer, in the built
library and in the Python classes, with one layout; InteractiveSession.
render_adaptive_until against a fake tracer; self-checks of tests/adaptive_ref.py on
synthetic moments; the committed resource-usage listings (no GPU needed)."""
import ctypes
import inspect
import os
import re

import numpy as np

import adaptive_ref as A
import moments_ref as R
from pnraytracing_amd import _native as N
from pnraytracing_amd import session, tracer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "pnrt.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
F, U = np.float32, np.uint32


def test_header_declares_the_entry_point():
    assert re.search(r"int\s+pnrt_render_adaptive\s*\(\s*pnrt_ctx\s*\*\s*\w*\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,"
                     r"\s*float\s+\w+\s*,\s*uint32_t\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*pnrt_adaptive_stats\s*\*\s*\w*\s*\)", CODE)


def test_adaptive_stats_layout_is_the_headers():
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*pnrt_adaptive_stats\s*;", CODE)
    assert m, "pnrt_adaptive_stats not declared"
    fields = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert fields == [("n_pixels", "int64_t"), ("n_active_pixels", "int64_t"), ("n_tiles", "int64_t"),
                      ("n_active_tiles", "int64_t"), ("frames_per_batch", "uint32_t"), ("n_batches", "uint32_t")]
    ctype = {"int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32}
    assert [(n, t) for n, t in N.AdaptiveStats._fields_] == [(n, ctype[t]) for n, t in fields]
    assert ctypes.sizeof(N.AdaptiveStats) == 40
    assert [getattr(N.AdaptiveStats, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 36]


def test_library_exports_the_symbol_typed():
    fn = N.device_lib().pnrt_render_adaptive         # AttributeError: the built library lacks the symbol
    P, INT, U32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32
    assert fn.restype is INT
    assert list(fn.argtypes) == [P, U32, U32, ctypes.c_float, U32, INT, INT, INT, ctypes.POINTER(N.AdaptiveStats)]


def test_device_deps_cover_the_new_header():
    from pnraytracing_amd import build
    assert "pt_adaptive.h" in build.DEVICE_DEPS
    assert os.path.exists(os.path.join(build.CSRC, "pt_adaptive.h"))


def test_python_layer_has_the_methods():
    sig = inspect.signature(tracer.PathTracer.render_adaptive)
    assert list(sig.parameters)[1:] == ["first", "n", "threshold", "min_frames", "band", "n_shards", "shard"]
    assert [sig.parameters[k].default for k in ("min_frames", "band", "n_shards", "shard")] == [8, 1, 1, 0]
    assert sig.parameters["threshold"].default is inspect.Parameter.empty
    sig = inspect.signature(session.InteractiveSession.render_adaptive_until)
    assert list(sig.parameters)[1:] == ["threshold", "max_frames", "frames_per_call", "min_frames"]
    assert [sig.parameters[k].default for k in ("max_frames", "frames_per_call", "min_frames")] == [1024, 8, 8]
    # render_until stays as it is
    sig = inspect.signature(session.InteractiveSession.render_until)
    assert list(sig.parameters)[1:] == ["threshold", "fraction", "max_frames", "check_every"]


# ---- render_adaptive_until against a fake tracer -----------------------------------------------------
class _FakeTracer:
    """`left` pixels stay active until `converge_at` frames were issued."""

    def __init__(self, converge_at, n_pixels=100):
        self.converge_at, self.n_pixels = converge_at, n_pixels
        self.calls, self.enabled, self.frames = [], 0, 0

    def enable_moments(self, on=True):
        self.enabled += 1 if on else 0

    def set_frame(self, *a):
        pass

    def render(self, *a):
        raise AssertionError("render_adaptive_until issues adaptive calls only")

    def render_adaptive(self, first, n, threshold, min_frames=8, band=1, n_shards=1, shard=0):
        assert self.enabled, "render_adaptive_until must enable the moments before the first call"
        self.calls.append((first, n, threshold, min_frames))
        left = 0 if self.frames >= self.converge_at else self.n_pixels - self.frames
        if left:
            self.frames += n
        return {"n_pixels": self.n_pixels, "n_active_pixels": left, "n_tiles": 4, "n_active_tiles": min(left, 4),
                "frames_per_batch": n if left else 0, "n_batches": 1 if left else 0}


class _Cam:
    def uniforms(self):
        return None


def _session(pt):
    return session.InteractiveSession(pt, 4, 4, _Cam())


def test_render_adaptive_until_stops_when_nothing_is_active():
    pt = _FakeTracer(converge_at=20)
    s = _session(pt)
    stats, frames = s.render_adaptive_until(0.125, max_frames=1000)
    # calls of 8 frames at 0, 8, 16; the call at 24 finds nothing active and renders nothing
    assert [c[:2] for c in pt.calls] == [(0, 8), (8, 8), (16, 8), (24, 8)]
    assert all(c[2:] == (0.125, 8) for c in pt.calls)
    assert stats["n_active_pixels"] == 0 and frames == 24 and s.frame_count == 24 and pt.enabled == 1


def test_render_adaptive_until_honours_max_frames_with_a_short_last_call():
    pt = _FakeTracer(converge_at=10**9)
    s = _session(pt)
    stats, frames = s.render_adaptive_until(0.01, max_frames=20, frames_per_call=6, min_frames=3)
    assert [c[:2] for c in pt.calls] == [(0, 6), (6, 6), (12, 6), (18, 2)]
    assert all(c[2:] == (0.01, 3) for c in pt.calls)
    assert frames == 20 and s.frame_count == 20 and stats["n_active_pixels"] > 0
    pt = _FakeTracer(converge_at=10**9)
    assert _session(pt).render_adaptive_until(0.01, max_frames=0) == (None, 0) and pt.calls == []


def test_render_adaptive_until_continues_the_frame_count():
    pt = _FakeTracer(converge_at=10**9)
    s = _session(pt)
    s.frame_count = 5
    assert s.render_adaptive_until(0.1, max_frames=7, frames_per_call=4)[1] == 7
    assert [c[:2] for c in pt.calls] == [(5, 4), (9, 3)] and s.frame_count == 12


# ---- self-checks of adaptive_ref on synthetic moments --------------------------------------------------
def _moments(n, mean=0.5, m2=0.0):
    n = np.asarray(n, U)
    m = np.zeros(n.shape + (4,), F)
    m[..., 0], m[..., 1] = mean, m2
    m[..., 3] = n.view(F)
    return m


def test_ref_predicate_and_min_frames_below_two():
    # n = 0, 1: unmeasured -> active whatever min_frames; n = 2 with zero variance: converged
    n = np.array([[0, 1, 2, 3, 9]], U)
    m = _moments(n)
    for mf in (0, 1, 2):                             # min_frames below 2 acts as 2
        assert A.active(m, 0.5, mf).tolist() == [[True, True, False, False, False]]
    assert A.active(m, 0.5, 3).tolist() == [[True, True, True, False, False]]
    assert A.active(m, 0.5, 0xFFFFFFFF).all()
    # e_c against the threshold: strictly above
    m = _moments(np.full((1, 3), 4, U), mean=1.0, m2=np.array([[0.0, 12.0, 48.0]], F))
    e = R.error(m)                                   # sqrt(m2 / 3 / 4): 0, 1, 2
    assert e.tolist() == [[0.0, 1.0, 2.0]]
    assert A.active(m, 1.0, 2).tolist() == [[False, False, True]]
    assert A.active(m, 0.0, 2).tolist() == [[False, True, True]]
    # a NaN error counts as 65535
    m = _moments(np.full((1, 1), 4, U), mean=1.0, m2=np.nan)
    assert A.active(m, 65534.0, 2).all() and not A.active(m, 65535.0, 2).any()


def test_ref_tile_order_and_ragged_edges():
    mask = np.zeros((45, 67), bool)                  # 9 x 6 tiles, the last column 3 wide, the top row 5 high
    mask[0, 0] = mask[7, 7] = True                   # tile 0: bits 0 and 63
    mask[44, 66] = True                              # tile 53: pixel (2, 4) -> bit 34
    mask[8, 64] = True                               # tile 17: pixel (0, 0)
    mask[9, 15] = True                               # tile 10: pixel (7, 1) -> bit 15
    assert A.tile_list(mask) == [(0, 1 | 1 << 63), (10, 1 << 15), (17, 1), (53, 1 << 34)]
    assert A.tile_list(np.zeros((45, 67), bool)) == []
    full = A.tile_list(np.ones((45, 67), bool))
    assert [t for t, _ in full] == list(range(54))
    assert full[0][1] == (1 << 64) - 1
    assert full[8][1] == sum(0b111 << (8 * r) for r in range(8))         # 3 columns
    assert full[45][1] == (1 << 40) - 1                                  # 5 rows
    assert full[53][1] == sum(0b111 << (8 * r) for r in range(5))
    assert A.tile_list(np.ones((1, 1), bool)) == [(0, 1)]


def test_ref_render_updates_active_pixels_only():
    rng = np.random.default_rng(5)
    h, w = 11, 13
    colors = [rng.random((h, w, 4), dtype=F) for _ in range(5)]
    acc = R.blend(np.zeros((h, w, 4), F), colors[:2], [0, 1])
    mom = R.update(R.zeros(h, w), colors[:2], [0, 1])
    thr = float(np.median(R.error(mom)))
    a1, m1, st = A.render(acc, mom, colors[2:4], [2, 3], thr, 2)
    act = A.active(mom, thr, 2)
    assert 0 < act.sum() < h * w and st["n_active_pixels"] == int(act.sum())
    assert st == {"n_pixels": h * w, "n_active_pixels": int(act.sum()), "n_tiles": 4, "n_active_tiles": 4,
                  "frames_per_batch": 2, "n_batches": 1}
    # inactive: untouched; active: the plain four-frame result (n == frame + 1 throughout)
    assert np.array_equal(a1[~act].view(U), acc[~act].view(U)) and np.array_equal(m1[~act].view(U), mom[~act].view(U))
    full_acc = R.blend(np.zeros((h, w, 4), F), colors[:4], [0, 1, 2, 3])
    full_mom = R.update(R.zeros(h, w), colors[:4], [0, 1, 2, 3])
    assert np.array_equal(a1[act].view(U), full_acc[act].view(U)) and np.array_equal(m1[act].view(U), full_mom[act].view(U))
    # a pixel that skipped frames: the mean of the frames it got, weight 1 / n
    a2, m2, _ = A.render(a1, m1, colors[4:], [9], 0.0, 0xFFFFFFFF)
    n2 = R.frames_of(m2)
    assert (n2[act] == 5).all() and (n2[~act] == 3).all()
    w3 = F(1) / F(3)
    want = ((acc[~act][:, :3] * (F(1) - w3)).astype(F) + (colors[4][~act][:, :3] * w3).astype(F)).astype(F)
    assert np.array_equal(a2[~act][:, :3].view(U), want.view(U))
    # shards: only the selector's rows, tiles over local rows
    a3, m3, st3 = A.render(acc, mom, colors[2:3], [2], 0.0, 0xFFFFFFFF, band=3, n_shards=2, shard=1)
    rows = A.selector_rows(h, 3, 2, 1)
    assert rows.tolist() == [3, 4, 5, 9, 10]
    other = np.setdiff1d(np.arange(h), rows)
    assert np.array_equal(m3[other].view(U), mom[other].view(U)) and (R.frames_of(m3[rows]) == 3).all()
    assert (st3["n_pixels"], st3["n_tiles"], st3["n_active_tiles"]) == (5 * w, 2, 2)
    # nothing to do
    assert A.render(acc, mom, [], [], 0.0, 2)[2]["frames_per_batch"] == 0
    st0 = A.render(acc, mom, colors[2:3], [2], 65535.0, 2)[2]
    assert (st0["n_active_pixels"], st0["n_active_tiles"], st0["frames_per_batch"], st0["n_batches"]) == (0, 0, 0, 0)


def test_ref_plan():
    assert A.plan(54, 12) == (12, 1) and A.plan(54, 300) == (128, 3) and A.plan(0, 5) == (0, 0) and A.plan(3, 0) == (0, 0)
    assert A.plan(54, 12, cap_frames=4) == (4, 3)
    assert A.plan(1 << 20, 16) == (3, 6)             # 2^26 slots per frame: three frames fit 2^28 - 1


# ---- the default instantiations compile to what they compiled to ----------------------------------------
def _listing(name):
    rows = {}
    for line in open(os.path.join(REPO, "profiles", "adaptive", name)):
        if line.startswith("#") or not line.strip():
            continue
        kernel, numbers = line.rsplit("|", 1)
        rows[kernel.strip()] = numbers.split()
    return rows


def test_existing_kernels_keep_their_resources():
    """profiles/adaptive/resource_usage_{parent,this}.txt (tools/resource_usage.py): every
    kernel of the parent commit is in this tree with the same SGPRs, VGPRs, AGPRs, scratch,
    occupancy, spills and LDS."""
    parent, this = _listing("resource_usage_parent.txt"), _listing("resource_usage_this.txt")
    assert len(parent) >= 40
    for kernel, numbers in parent.items():
        assert this.get(kernel) == numbers, kernel
    new = sorted(set(this) - set(parent))
    assert any("pt_blend_adaptive_kernel" in k for k in new) and any("pt_wf_gen_setup<WfAdapt>" in k for k in new)
    for k in new:                                    # the new kernels: no scratch, no spills
        sgpr, vgpr, agpr, scratch, occ, sspill, vspill, lds = (int(v) for v in this[k])
        assert (scratch, sspill, vspill) == (0, 0, 0), k
