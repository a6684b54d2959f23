"""pnrt_denoise_variance against tests/atrous_var_ref.py (the numpy restatement of
DESIGN.md section 24.2), bit for bit, on the accumulation, guide and moments images
of the same context: uniform and non-uniform frame counts, unmeasured pixels,
pass-through pixels, the untouched inputs, stream ordering, the error codes, the
fixed-sigma filter beside it, and the session's preview."""
import numpy as np
import pytest

from atrous_ref import atrous_ref, passthrough
from atrous_var_ref import atrous_var_ref
from guides_common import F, SCENES, SHAPES, bits, scene
from moments_ref import frames_of
from pnraytracing_amd import host as H
from pnraytracing_amd.tracer import PathTracer, PnrtError

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -3
SIGMAS = [{}, {"sigma_variance": 1.5, "sigma_normal": 0.5, "sigma_position": 1.5}]    # the defaults, and another set


def _count(a, b):
    return int(np.count_nonzero(np.any(bits(a) != bits(b), axis=-1)))


def _inputs(pt):
    """What the restatement takes, read from the context."""
    return pt.read_accum(), pt.read_aov("position"), pt.read_aov("normal"), pt.read_aov("albedo")


def _ref(pt, mats, **params):
    accum, pos, nrm, alb = _inputs(pt)
    return atrous_var_ref(accum, pos, nrm, alb, mats, pt.read_moments(), **params)


def _code(fn, *a, **k):
    with pytest.raises(PnrtError) as e:
        fn(*a, **k)
    return e.value.code


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_denoised_image_is_the_restatements(name, shape):
    """4 frames with the moments on, then every level count and sigma set on the same images."""
    w, h = shape
    cfg = scene(name, w, h)
    mats = np.asarray(cfg.packed.materials, F)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        pt.render(0, 4)
        pt.render_guides()
        accum, pos, nrm, alb = _inputs(pt)
        mom = pt.read_moments()
        assert np.all(frames_of(mom) == 4)
        pt_mask = passthrough(pos, nrm, mats)
        pt.denoise(levels=1)
        ptr = pt.denoised_ptr()                    # the image pnrt_denoise gives
        assert ptr != 0
        for levels in (1, 3, 5):
            for sg in SIGMAS:
                pt.denoise_variance(levels=levels, **sg)
                got = pt.read_denoised()
                want = atrous_var_ref(accum, pos, nrm, alb, mats, mom, levels=levels, **sg)
                bad = _count(got, want)
                assert bad == 0, f"levels {levels} sigmas {sg or 'default'}: {bad} of {w * h} pixels differ"
                # pass-through pixels are the accumulation's; the others have alpha 1
                assert _count(got[pt_mask], accum[pt_mask]) == 0
                assert np.all(got[~pt_mask][:, 3] == 1)
                # the same image, whatever the parity of the level count
                assert pt.denoised_ptr() == ptr
        pt.denoise_variance()                      # NULL parameters: the stated defaults
        assert _count(pt.read_denoised(), atrous_var_ref(accum, pos, nrm, alb, mats, mom)) == 0
        # the accumulation and the moments were only read
        assert _count(pt.read_accum(), accum) == 0
        assert _count(pt.read_moments(), mom) == 0
    if name == "c1" and shape == (67, 45):
        assert pt_mask.any() and not pt_mask.all()          # the area light's pixels
        assert _count(got[~pt_mask], accum[~pt_mask]) > 0    # ... and the rest is filtered
    if name == "c2wide" and shape == (67, 45):
        assert (pos[..., 3] == 0).any()                      # misses


def test_non_uniform_frame_counts():
    """An adaptive call over half the pixels: counts of 4 and 8 in one image."""
    w, h = 67, 45
    cfg = scene("c2", w, h)
    mats = np.asarray(cfg.packed.materials, F)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        pt.render(0, 4)
        thr = float(np.median(pt.read_error()))
        pt.render_adaptive(4, 4, threshold=thr, min_frames=2)
        pt.render_guides()
        counts = set(np.unique(frames_of(pt.read_moments())).tolist())
        assert counts == {4, 8}, counts
        for levels, sg in ((5, SIGMAS[0]), (3, SIGMAS[1])):
            pt.denoise_variance(levels=levels, **sg)
            assert _count(pt.read_denoised(), _ref(pt, mats, levels=levels, **sg)) == 0


def test_unmeasured_pixels():
    """n = 1 everywhere; then n = 0 and a black accumulation in the other shard's rows."""
    w, h = 67, 45
    cfg = scene("c3", w, h)
    mats = np.asarray(cfg.packed.materials, F)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        pt.render_guides()
        pt.render(0, 1)
        assert np.all(frames_of(pt.read_moments()) == 1)
        for levels in (1, 5):
            pt.denoise_variance(levels=levels)
            got = pt.read_denoised()
            assert _count(got, _ref(pt, mats, levels=levels)) == 0
        assert np.all(np.isfinite(got))

        pt.reset_accum()
        pt.render(0, 4, band=8, n_shards=2, shard=0)
        n = frames_of(pt.read_moments())
        rows = (np.arange(h) // 8) % 2 == 0
        assert np.all(n[rows] == 4) and np.all(n[~rows] == 0)
        assert np.all(pt.read_accum()[~rows] == 0)
        for levels in (2, 5):
            pt.denoise_variance(levels=levels)
            got = pt.read_denoised()
            assert _count(got, _ref(pt, mats, levels=levels)) == 0
        assert np.all(np.isfinite(got))


def test_ordering_without_host_synchronisation():
    """render; filter; render; filter queued back to back equals the sequence with a wait
    after every call: the filter reads the accumulation and the moments after the blends
    queued before it, and the next call's blend waits for that read."""
    w, h = 67, 45
    cfg = scene("c3", w, h)
    mats = np.asarray(cfg.packed.materials, F)

    def run(sync):
        with PathTracer(0) as pt:
            pt.load(cfg)
            pt.enable_moments()
            pt.render_guides()
            wait = pt.synchronize if sync else (lambda: None)
            wait()
            pt.render(0, 2); wait()
            pt.denoise_variance(levels=4); wait()
            mid = pt.read_denoised() if sync else None
            pt.render(2, 2); wait()
            pt.denoise_variance(levels=4); wait()
            return pt.read_denoised(), pt.read_accum(), pt.read_moments(), _ref(pt, mats, levels=4), mid

    a_den, a_acc, a_mom, a_ref, _ = run(False)
    b_den, b_acc, b_mom, _, mid = run(True)
    assert _count(a_acc, b_acc) == 0
    assert _count(a_mom, b_mom) == 0
    assert _count(a_den, b_den) == 0
    assert _count(a_den, a_ref) == 0
    assert _count(mid, b_den) > 0                  # the second call saw the later frames


def test_state_errors():
    w, h = 67, 45
    cfg = scene("c2", w, h)
    mats = np.asarray(cfg.packed.materials, F)
    moved = H.camera_update((0.5, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, F(w) / F(h))
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.render_guides()
        pt.render(0, 2)
        with pytest.raises(PnrtError, match="never enabled") as e:          # before the moments are enabled
            pt.denoise_variance()
        assert e.value.code == E_STATE
        assert pt.denoised_ptr() == 0                                        # ... and nothing was allocated
        pt.enable_moments()
        pt.reset_accum()
        pt.render(0, 2)
        pt.denoise_variance(levels=2)
        ok = pt.read_denoised()

        pt.enable_moments(False)                                             # disabled, nothing rendered: they still cover
        pt.denoise_variance(levels=2)
        assert _count(pt.read_denoised(), ok) == 0
        pt.render(2, 1)                                                      # a frame the moments do not count
        pt.enable_moments()
        with pytest.raises(PnrtError, match="do not cover") as e:
            pt.denoise_variance(levels=2)
        assert e.value.code == E_STATE
        assert _count(pt.read_denoised(), ok) == 0                           # the image is left as it was
        pt.reset_accum()
        pt.render(0, 2)
        pt.denoise_variance(levels=2)
        assert _count(pt.read_denoised(), ok) == 0                           # the same two frames

        pt.set_frame(w, h, moved, 4)                                         # stale guides
        with pytest.raises(PnrtError, match="render_guides") as e:
            pt.denoise_variance(levels=2)
        assert e.value.code == E_STATE
        pt.set_frame(w, h, cfg.camera, 4)                                    # ... and back: the key matches again
        pt.denoise_variance(levels=2)
        pt.update_materials(0, mats.reshape(-1, 18)[0:1])
        assert _code(pt.denoise_variance) == E_STATE
        pt.render_guides()
        pt.denoise_variance(levels=2)
        assert _count(pt.read_denoised(), ok) == 0

    with PathTracer(0) as pt:                                                # moments, but never guides
        pt.load(cfg)
        pt.enable_moments()
        pt.render(0, 2)
        with pytest.raises(PnrtError, match="render_guides first") as e:
            pt.denoise_variance()
        assert e.value.code == E_STATE


def test_bad_arguments_leave_the_image_alone():
    w, h = 8, 8
    cfg = scene("c1", w, h)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        pt.render(0, 4)
        pt.render_guides()
        pt.denoise_variance(levels=3)
        before = pt.read_denoised()
        for levels in (0, 6, -1):
            assert _code(pt.denoise_variance, levels=levels) == E_ARG
        for name in ("sigma_variance", "sigma_normal", "sigma_position"):
            for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
                assert _code(pt.denoise_variance, **{name: bad}) == E_ARG, (name, bad)
        assert _count(pt.read_denoised(), before) == 0
        pt.denoise_variance(levels=3)                              # and the context still works
        assert _count(pt.read_denoised(), before) == 0


def test_fixed_sigma_filter_is_unaffected():
    """pnrt_denoise after pnrt_denoise_variance on the same context (the same images and
    guide records) still equals its own restatement, and the other way round."""
    w, h = 67, 45
    cfg = scene("c1", w, h)
    mats = np.asarray(cfg.packed.materials, F)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        pt.render(0, 4)
        pt.render_guides()
        accum, pos, nrm, alb = _inputs(pt)
        for levels in (2, 5):                      # both parities of the ping-pong
            pt.denoise_variance(levels=5)
            pt.denoise(levels=levels)
            assert _count(pt.read_denoised(), atrous_ref(accum, pos, nrm, alb, mats, levels=levels)) == 0
            pt.denoise_variance(levels=levels)
            assert _count(pt.read_denoised(), _ref(pt, mats, levels=levels)) == 0
        assert _count(pt.read_denoised(), atrous_ref(accum, pos, nrm, alb, mats, levels=5)) > 0     # two filters, two images


def test_session_preview_variance():
    """InteractiveSession.preview_variance(): guides when the camera moved, then the filter."""
    from pnraytracing_amd.session import CameraController, InteractiveSession
    w, h = 67, 45
    cfg = scene("c2", w, h)
    mats = np.asarray(cfg.packed.materials, F)
    cam = CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, F(w) / F(h))
    with PathTracer(0) as pt:
        pt.load(cfg)
        sess = InteractiveSession(pt, w, h, cam)
        sess.frame()
        with pytest.raises(PnrtError, match="never enabled"):      # the moments error comes through, no guides rendered
            sess.preview_variance(levels=3)
        assert pt.aov_ptr("albedo") == 0
        pt.enable_moments()
        sess.frame(redraw=True)                                    # frame 0 again: the moments restart with it
        for step in range(3):
            sess.frame()
            sess.preview_variance(levels=3)
        assert _count(pt.read_denoised(), _ref(pt, mats, levels=3)) == 0
        cam.rotate(4.0, -1.5)
        sess.frame(redraw=True)
        sess.preview_variance(levels=3)
        assert _count(pt.read_denoised(), _ref(pt, mats, levels=3)) == 0
        assert np.all(frames_of(pt.read_moments()) == 1)           # one frame after the move: the unmeasured branch
