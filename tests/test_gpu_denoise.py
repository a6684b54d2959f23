"""pnrt_denoise against tests/atrous_ref.py (the numpy restatement of DESIGN.md
section 20.2), bit for bit; pass-through pixels, the untouched accumulation
image, stream ordering, staleness of the guides and argument checks."""
import numpy as np
import pytest

from atrous_ref import atrous_ref, passthrough
from guides_common import F, SCENES, SHAPES, bits, scene
from pnraytracing_amd import host as H
from pnraytracing_amd.tracer import TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer, PnrtError

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -3
SIGMAS = [{}, {"sigma_color": 0.75, "sigma_normal": 0.5, "sigma_position": 1.5}]      # the defaults, and another set


def _count(a, b):
    return int(np.count_nonzero(np.any(bits(a) != bits(b), axis=-1)))


def _aovs(pt):
    return pt.read_aov("position"), pt.read_aov("normal"), pt.read_aov("albedo")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", SCENES)
def test_denoised_image_is_the_restatements(name, shape):
    """4 frames, then every level count and sigma set on the same accumulation image."""
    w, h = shape
    cfg = scene(name, w, h)
    mats = np.asarray(cfg.packed.materials, F)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.render(0, 4)
        pt.render_guides()
        accum = pt.read_accum()
        pos, nrm, alb = _aovs(pt)
        pt_mask = passthrough(pos, nrm, mats)
        ptr = None
        for levels in (1, 3, 5):
            for sg in SIGMAS:
                pt.denoise(levels=levels, **sg)
                got = pt.read_denoised()
                want = atrous_ref(accum, pos, nrm, alb, mats, levels=levels, **sg)
                bad = _count(got, want)
                assert bad == 0, f"levels {levels} sigmas {sg or 'default'}: {bad} of {w * h} pixels differ"
                # pass-through pixels are the accumulation's; the others have alpha 1
                assert _count(got[pt_mask], accum[pt_mask]) == 0
                assert np.all(got[~pt_mask][:, 3] == 1)
                # the image stays where it is, whatever the parity of the level count
                ptr = ptr or pt.denoised_ptr()
                assert pt.denoised_ptr() == ptr != 0
        pt.denoise()                               # NULL parameters: the stated defaults
        assert _count(pt.read_denoised(), atrous_ref(accum, pos, nrm, alb, mats)) == 0
        # the accumulation image was only read
        assert _count(pt.read_accum(), accum) == 0
    if name == "c1" and shape == (67, 45):
        assert pt_mask.any() and not pt_mask.all()          # the area light's pixels
        assert _count(got[~pt_mask], accum[~pt_mask]) > 0    # ... and the rest is filtered
    if name == "c2wide" and shape == (67, 45):
        assert (pos[..., 3] == 0).any()                      # misses


def test_ordering_without_host_synchronisation():
    """render; denoise; render; denoise queued back to back equals the sequence with a
    wait after every call: the filter reads the accumulation image after the blends
    queued before it, and the next call's blend waits for that read."""
    w, h = 67, 45
    cfg = scene("c3", w, h)
    mats = np.asarray(cfg.packed.materials, F)

    def run(sync):
        with PathTracer(0) as pt:
            pt.load(cfg)
            pt.render_guides()
            wait = pt.synchronize if sync else (lambda: None)
            wait()
            pt.render(0, 2); wait()
            pt.denoise(levels=4); wait()
            mid = pt.read_denoised() if sync else None
            pt.render(2, 2); wait()
            pt.denoise(levels=4); wait()
            return pt.read_denoised(), pt.read_accum(), _aovs(pt), mid

    a_den, a_acc, aov, _ = run(False)
    b_den, b_acc, _, mid = run(True)
    assert _count(a_acc, b_acc) == 0
    assert _count(a_den, b_den) == 0
    assert _count(a_den, atrous_ref(a_acc, *aov, mats, levels=4)) == 0
    assert _count(mid, b_den) > 0                  # the second denoise saw the later frames


def _code(fn, *a, **k):
    with pytest.raises(PnrtError) as e:
        fn(*a, **k)
    return e.value.code


def test_stale_guides_are_refused():
    w, h = 67, 45
    cfg = scene("c2", w, h)
    moved = H.camera_update((0.5, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, F(w) / F(h))
    with PathTracer(0) as pt:
        pt.load(cfg, TRAVERSE_ZCULL)
        pt.render(0, 2)
        assert _code(pt.denoise) == E_STATE                       # never rendered
        with pytest.raises(PnrtError):
            pt.read_denoised()
        pt.render_guides()
        pt.denoise(levels=2)
        ok = pt.read_denoised()

        pt.set_frame(w, h, cfg.camera, 1)                         # the same camera (another depth): still valid
        pt.denoise(levels=2)
        assert _count(pt.read_denoised(), ok) == 0

        pt.set_frame(w, h, moved, 4)                              # a moved camera
        assert _code(pt.denoise) == E_STATE
        pt.set_frame(w, h, cfg.camera, 4)                         # ... and back: the key matches again
        pt.denoise(levels=2)

        pt.update_materials(0, np.asarray(cfg.packed.materials, F)[0:1])      # even the same record
        assert _code(pt.denoise) == E_STATE
        pt.render_guides(); pt.denoise(levels=2)

        pt.upload_env(cfg.env_rgb, cfg.env_table)
        assert _code(pt.denoise) == E_STATE
        pt.render_guides(); pt.denoise(levels=2)

        pt.set_options(TRAVERSE_EXACT)
        assert _code(pt.denoise) == E_STATE
        pt.render_guides(); pt.denoise(levels=2)

        pt.upload_texture(0, np.zeros(12, np.uint8), 2, 2, 3)      # the albedo image samples the textures
        assert _code(pt.denoise) == E_STATE
        pt.render_guides(); pt.denoise(levels=2)

        pt.upload_scene(cfg.packed)
        assert _code(pt.denoise) == E_STATE
        pt.render_guides(); pt.denoise(levels=2)

        pt.set_frame(w - 1, h, cfg.camera, 4)                     # another size
        assert _code(pt.denoise) == E_STATE
        assert _code(pt.read_denoised) == E_STATE
        assert _code(pt.read_aov, "albedo") == E_STATE


def test_bad_arguments_leave_the_image_alone():
    w, h = 8, 8
    cfg = scene("c1", w, h)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.render(0, 4)
        pt.render_guides()
        pt.denoise(levels=3)
        before = pt.read_denoised()
        for levels in (0, 6, -1):
            assert _code(pt.denoise, levels=levels) == E_ARG
        for name in ("sigma_color", "sigma_normal", "sigma_position"):
            for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
                assert _code(pt.denoise, **{name: bad}) == E_ARG, (name, bad)
        assert _count(pt.read_denoised(), before) == 0
        pt.denoise(levels=3)                                       # and the context still works
        assert _count(pt.read_denoised(), before) == 0


def test_session_preview():
    """InteractiveSession.preview(): guides when the camera moved, then the filter."""
    from pnraytracing_amd.session import CameraController, InteractiveSession
    w, h = 67, 45
    cfg = scene("c2", w, h)
    mats = np.asarray(cfg.packed.materials, F)
    cam = CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, F(w) / F(h))
    with PathTracer(0) as pt:
        pt.load(cfg)
        sess = InteractiveSession(pt, w, h, cam)
        for step in range(3):
            sess.frame()
            sess.preview(levels=3)
        assert _count(pt.read_denoised(), atrous_ref(pt.read_accum(), *_aovs(pt), mats, levels=3)) == 0
        cam.rotate(4.0, -1.5)
        sess.frame(redraw=True)
        sess.preview(levels=3)
        assert _count(pt.read_denoised(), atrous_ref(pt.read_accum(), *_aovs(pt), mats, levels=3)) == 0
