"""pnrt_display and pnrt_luma_histogram_read against tests/display_ref.py (the numpy
restatement of DESIGN.md section 26), byte for byte and count for count: every tone
curve, transfer, row order and source, a crafted external image of edge values, the
PN-libm pow the sRGB branch rests on, stream ordering, the images that must stay
untouched, the display image's lifetime and the argument checks."""
import ctypes

import numpy as np
import pytest

import display_ref as D
from guides_common import F, bits, scene
from pnraytracing_amd import _native as N
from pnraytracing_amd.image import to_display
from pnraytracing_amd.tracer import PathTracer, PnrtError, exposure_from_histogram, merge_histograms, shard_rows

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -3
# 67x45: no multiple of 4 in either direction, several blocks' worth of groups that cross
# row ends; 8x8: whole groups only; 1x1 and 5x3: a last group stored word by word
SHAPES = [(67, 45), (8, 8), (1, 1), (5, 3)]
EXPOSURES = [1.0, 0.37, 6.5]
COMBOS = [(t, x, e, b) for t in D.TONES for x in D.TRANSFERS for e in EXPOSURES for b in (False, True)]


def _diff(a, b):
    return int(np.count_nonzero(np.asarray(a) != np.asarray(b)))


def _same_hist(a, b):
    return a["n_pixels"] == b["n_pixels"] and a["n_counted"] == b["n_counted"] and np.array_equal(a["bins"], b["bins"])


def _check_all(pt, source, img, **kw):
    for tone, transfer, exposure, bottom in COMBOS:
        pt.display(source=source, tone=tone, transfer=transfer, exposure=exposure, white=3.0, bottom_first=bottom, **kw)
        got = pt.read_display()
        want = D.display_ref(img, tone, transfer, exposure, 3.0, bottom)
        bad = _diff(got, want)
        assert bad == 0, f"{source} {tone} {transfer} exposure {exposure} bottom_first {bottom}: {bad} of {got.size} bytes differ"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["c1", "c2wide"])
def test_display_is_the_restatements(name, shape):
    """4 frames, then every tone x transfer x exposure x row order on the accumulation
    image, and on the denoised image after denoise(levels=3)."""
    w, h = shape
    cfg = scene(name, w, h)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.render(0, 4)
        accum = pt.read_accum()
        _check_all(pt, "accum", accum)
        ptr = pt.display_ptr()
        # NULL parameters and the Python defaults: the reference's display plus alpha
        assert pt._lib.pnrt_display(pt._ctx, None) == 0
        null = pt.read_display()
        pt.display()
        assert _diff(null, pt.read_display()) == 0
        assert _diff(null[..., :3], to_display(accum)) == 0 and np.all(null[..., 3] == 255)
        pt.render_guides()
        pt.denoise(levels=3)
        den = pt.read_denoised()
        _check_all(pt, "denoised", den)
        assert pt.display_ptr() == ptr != 0                       # one image, whatever the source
        assert _diff(bits(pt.read_accum()), bits(accum)) == 0     # the sources were only read
        assert _diff(bits(pt.read_denoised()), bits(den)) == 0
        assert _same_hist(pt.luma_histogram("denoised"), D.histogram_ref(den))
    if shape == (67, 45):
        assert _diff(bits(den), bits(accum)) > 0                  # the filter did something
        # (a frame's colour is clamped to [0, 1] by the integrator, as the reference's shader does:
        # values above 1 reach the curves through the exposures above and the external image below)
        assert 0 < accum[..., :3].max() <= 1


def _crafted():
    """64x17 float4: the edge values of the definition, then log-uniform noise."""
    w, h = 64, 17
    one = F(1)
    v = [np.nan, np.inf, -np.inf, -1.0, -1e-30, -0.0, 0.0, 1e-45, 1e-40, 1.1754942e-38, 1e30, 3.4028235e38]
    for c in (F(0.0031308), one, F(65536), F(4.0), F(0.18)):
        v += [np.nextafter(c, F(0)), c, np.nextafter(c, F(np.inf))]
    for k in range(255):
        c = F(F(k + 0.5) / F(255))
        v += [np.nextafter(c, F(0)), c, np.nextafter(c, F(np.inf))]
    v = np.array(v, F)
    assert 3 * 256 <= len(v) <= 13 * w
    rng = np.random.default_rng(26)
    img = np.exp(rng.uniform(np.log(1e-6), np.log(2e5), (h, w, 4))).astype(F)       # (alpha is noise too: it is ignored)
    # 13 rows of grey pixels, r = g = b = one edge value, so that the luminance sees it too
    img[:13].reshape(-1, 4)[:len(v), :3] = v[:, None]
    # 4 rows with three different edge values per pixel
    img[13:].reshape(-1, 4)[:, :3] = v[:3 * 256].reshape(3, 256).T
    return img


def test_external_source_with_edge_values():
    import torch
    img = _crafted()
    h, w = img.shape[:2]
    cfg = scene("c1", w, h)
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    with PathTracer(0) as pt:
        pt.load(cfg)
        _check_all(pt, "external", img, src_ptr=dev.data_ptr())
        pt.display(source="external", src_ptr=dev.data_ptr())      # the defaults: to_display for an image without NaN
        clean = ~np.isnan(img[::-1, :, :3])
        with np.errstate(invalid="ignore"):                        # (to_display leaves NaN to numpy's cast)
            host = to_display(img)
        assert _diff(pt.read_display()[..., :3][clean], host[clean]) == 0
        want = D.histogram_ref(img)
        assert _same_hist(pt.luma_histogram("external", src_ptr=dev.data_ptr()), want)
        assert 0 < want["n_counted"] < want["n_pixels"] and want["bins"][0] > 0 and want["bins"][511] > 0
        parts = [pt.luma_histogram("external", band=2, n_shards=3, shard=s, src_ptr=dev.data_ptr()) for s in range(3)]
        for s, p in enumerate(parts):
            assert _same_hist(p, D.histogram_ref(img, rows=shard_rows(h, 2, 3, s)))
        assert _same_hist(merge_histograms(parts), want)
        assert torch.equal(dev.cpu().view(torch.int32), torch.from_numpy(img).view(torch.int32))   # only read
    del dev


def test_pow_of_the_srgb_branch_is_the_oracles():
    import pyoracle
    t = np.linspace(0.0031308, 1.0, 4096).astype(F)
    t[0], t[-1] = F(0.0031308), F(1.0)
    e = np.full_like(t, D.SRGB_EXPONENT)
    assert e.view(np.uint32)[0] == 0x3ED55555 and D.SRGB_EXPONENT == F(1.0) / F(2.4)
    with PathTracer(0) as pt:
        got = pt.debug_math(5, t, e)
    want = pyoracle.math_eval(5, t, e)
    assert _diff(bits(got), bits(want)) == 0
    assert got[-1] == 1.0 and abs(float(got[0]) - 0.0031308 ** (1 / 2.4)) < 1e-6


def test_histogram_is_the_restatements_and_shards_add_up():
    w, h = 67, 45
    cfg = scene("c2wide", w, h)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.render(0, 4)
        accum = pt.read_accum()
        whole = pt.luma_histogram()
        want = D.histogram_ref(accum)
        assert _same_hist(whole, want)
        assert whole["n_pixels"] == w * h and int(whole["bins"].sum()) == whole["n_counted"] > 0
        assert np.count_nonzero(whole["bins"]) > 16                # spread over more than an octave
        for band, n in ((8, 3), (1, 2)):
            parts = [pt.luma_histogram(band=band, n_shards=n, shard=s) for s in range(n)]
            for s, p in enumerate(parts):
                assert _same_hist(p, D.histogram_ref(accum, rows=shard_rows(h, band, n, s))), (band, n, s)
            assert _same_hist(merge_histograms(parts), whole), (band, n)
        none = pt.luma_histogram(band=h, n_shards=2, shard=1)      # one band: shard 1 has no rows
        assert none["n_pixels"] == 0 and none["n_counted"] == 0 and not none["bins"].any()
        assert _same_hist(pt.luma_histogram(band=h, n_shards=2, shard=0), whole)
        # the exposure from it, and the image it gives
        e = exposure_from_histogram(whole)
        assert F(e) == D.exposure_ref(want)
        pt.display(tone="aces", transfer="srgb", exposure=e)
        assert _diff(pt.read_display(), D.display_ref(accum, "aces", "srgb", e)) == 0
        assert _diff(bits(pt.read_accum()), bits(accum)) == 0


def test_ordering_without_host_synchronisation():
    """render; display; render; display queued back to back equals the sequence with a
    wait after every call: the display reads the accumulation image after the blends
    queued before it, and the next call's blend waits for that read."""
    w, h = 67, 45
    cfg = scene("c2wide", w, h)

    def run(sync):
        with PathTracer(0) as pt:
            pt.load(cfg)
            wait = pt.synchronize if sync else (lambda: None)
            wait()
            pt.render(0, 2); wait()
            pt.display(tone="reinhard", transfer="srgb"); wait()
            mid = pt.read_display() if sync else None
            pt.render(2, 2); wait()
            pt.display(tone="reinhard", transfer="srgb"); wait()
            return pt.read_display(), pt.read_accum(), mid

    a_img, a_acc, _ = run(False)
    b_img, b_acc, mid = run(True)
    assert _diff(bits(a_acc), bits(b_acc)) == 0
    assert _diff(a_img, b_img) == 0
    assert _diff(a_img, D.display_ref(a_acc, "reinhard", "srgb")) == 0
    assert _diff(mid, b_img) > 0                                   # the second display saw the later frames


def _code(fn, *a, **k):
    with pytest.raises(PnrtError) as e:
        fn(*a, **k)
    return e.value.code


def test_state_images_untouched_and_the_display_images_lifetime():
    w, h = 67, 45
    cfg = scene("c2wide", w, h)
    with PathTracer(0) as pt:
        assert pt.display_ptr() == 0
        assert _code(pt.display) == E_STATE                        # before set_frame
        assert _code(pt.luma_histogram) == E_STATE
        pt.width, pt.height = w, h
        assert _code(pt.read_display) == E_STATE                   # before the first display
        pt.load(cfg)
        pt.enable_moments(True)
        pt.render(0, 4)
        assert _code(pt.display, source="denoised") == E_STATE     # no pnrt_denoise* yet
        assert _code(pt.luma_histogram, "denoised") == E_STATE
        assert pt.display_ptr() == 0 and _code(pt.read_display) == E_STATE
        pt.render_guides()
        pt.denoise_variance(levels=2)
        acc, mom, den = pt.read_accum(), pt.read_moments(), pt.read_denoised()
        ptrs = (pt.accum_ptr(), pt.moments_ptr(), pt.denoised_ptr())
        pt.display()
        ptr = pt.display_ptr()
        assert ptr != 0
        for source in ("accum", "denoised"):
            pt.display(source=source, tone="aces", transfer="srgb", exposure=0.5)
            pt.luma_histogram(source)
            assert pt.display_ptr() == ptr
        assert _diff(bits(pt.read_accum()), bits(acc)) == 0
        assert _diff(bits(pt.read_moments()), bits(mom)) == 0
        assert _diff(bits(pt.read_denoised()), bits(den)) == 0
        assert (pt.accum_ptr(), pt.moments_ptr(), pt.denoised_ptr()) == ptrs
        # a resize: the old display image is not this frame's
        pt.set_frame(w - 1, h, cfg.camera, cfg.max_depth)
        assert _code(pt.read_display) == E_STATE
        assert _code(pt.display, source="denoised") == E_STATE     # the denoised image has the old size
        pt.render(0, 1)
        pt.display()
        assert pt.display_ptr() not in (0, ptr)
        assert _diff(pt.read_display()[..., :3], to_display(pt.read_accum())) == 0
        ptr2 = pt.display_ptr()
        pt.display(bottom_first=True)
        assert pt.display_ptr() == ptr2


def test_bad_arguments_leave_the_display_image_alone():
    import torch
    w, h = 8, 8
    cfg = scene("c1", w, h)
    ext = torch.zeros(w * h * 4 + 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.render(0, 4)
        pt.display(tone="aces", transfer="srgb", exposure=2.0)
        before = pt.read_display()
        for field in ("source", "tone", "transfer"):
            for bad in (-1, 2 if field == "transfer" else 3, 77):
                assert _code(pt.display, **{field: bad}) == E_ARG, (field, bad)
        for bad in (-1, 2):
            assert _code(pt.display, bottom_first=bad) == E_ARG
        for field in ("exposure", "white"):
            for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
                assert _code(pt.display, **{field: bad}) == E_ARG, (field, bad)
        assert _code(pt.display, source="external") == E_ARG                       # NULL
        assert _code(pt.display, source="external", src_ptr=ext.data_ptr() + 4) == E_ARG
        assert _code(pt.display, source="denoised") == E_STATE
        assert pt._lib.pnrt_read_display(pt._ctx, None) == E_ARG
        assert _diff(pt.read_display(), before) == 0
        # the histogram's
        for sel in ({"band": 0}, {"n_shards": 0}, {"shard": -1}, {"n_shards": 2, "shard": 2}):
            assert _code(pt.luma_histogram, **sel) == E_ARG, sel
        assert _code(pt.luma_histogram, 3) == E_ARG and _code(pt.luma_histogram, -1) == E_ARG
        assert _code(pt.luma_histogram, "external") == E_ARG
        assert _code(pt.luma_histogram, "external", src_ptr=ext.data_ptr() + 8) == E_ARG
        assert pt._lib.pnrt_luma_histogram_read(pt._ctx, 0, None, 1, 1, 0, None) == E_ARG
        assert _diff(pt.read_display(), before) == 0
        # and the context still works, the external source with a good pointer included
        pt.display(source="external", src_ptr=ext.data_ptr())
        assert _diff(pt.read_display()[..., :3], 0) == 0
        pt.display(tone="aces", transfer="srgb", exposure=2.0)
        assert _diff(pt.read_display(), before) == 0
    del ext


def test_session_show():
    """InteractiveSession.show(): the accumulation or the preview, with the exposure the
    histogram of the shown image gives."""
    from pnraytracing_amd.session import CameraController, InteractiveSession
    w, h = 67, 45
    cfg = scene("c2", w, h)
    cam = CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 100.0, F(w) / F(h))
    with PathTracer(0) as pt:
        pt.load(cfg)
        sess = InteractiveSession(pt, w, h, cam)
        for _ in range(3):
            sess.frame()
        acc = pt.read_accum()
        assert _diff(sess.show()[..., :3], to_display(acc)) == 0
        got = sess.show(auto_exposure=True, tone="aces", transfer="srgb")
        e = D.exposure_ref(D.histogram_ref(acc))
        assert _diff(got, D.display_ref(acc, "aces", "srgb", e)) == 0
        sess.preview(levels=2)
        den = pt.read_denoised()
        got = sess.show(denoised=True, auto_exposure=True, tone="reinhard")
        assert _diff(got, D.display_ref(den, "reinhard", "linear", D.exposure_ref(D.histogram_ref(den)))) == 0
