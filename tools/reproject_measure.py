"""Cost and quality of pnrt_reproject (results in
profiles/reproject/).  Reported, not asserted.

  cost     C2 at 1920x1080 and 512x512: 8 frames at camera A, one drag step to B (a new
           pair of cameras every repetition), then
           pnrt_reproject(A) -- the call's wall time (it is synchronous), the profile's
           PNRT_K_PRIMARY (the guide traces) and PNRT_K_BLEND (the kernel and the four
           copies) sums, the same four device-to-device copies timed alone between HIP
           events (the kernel's time is the blend sum less these), with the guide images
           of A current before the call and without.  Beside it frame(redraw=True) with a
           synchronise, which is what a camera move costs without the call.  The kernel's
           bytes: 32 read and 32 written per pixel, and 64 per unique history pixel its
           taps touch (counted with tests/reproject_ref.py on the images read back).
  quality  C2 at 512x512: 64 frames at A, one drag step to B, then (a) redraw + K frames
           and (b) reproject + frame_counted(K), K = 1, 4, 16: the RMSE of the luminance
           against a 1024-frame render at B, for the accumulation and for
           preview_variance() on top of it, and the shares reprojected / disoccluded /
           missed.

  cost_view     pnrt_reproject_view (results in profiles/reproject_view/):
           the same drag steps with both views one camera model, per model: the call's wall
           time, the PNRT_K_PRIMARY sum (two guide traces) and the PNRT_K_BLEND sum (two
           pnrt_make_rays launches, the kernel, the four copies); pnrt_make_rays timed alone
           the same way, so the kernel's time is the blend sum less the copies and two of
           those.  Beside it pnrt_reproject in the same process.
  quality_view  the quality experiment under the 180-degree fisheye: reproject_view() +
           frame_counted(K) against a redraw + K frames, against a 1024-frame render of
           the new view's rays.

usage: python tools/reproject_measure.py cost|quality|cost_view|quality_view [out.json]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
from pnraytracing_amd import scenes  # noqa: E402
from pnraytracing_amd.session import CameraController, InteractiveSession  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

DRAG = (5.0, 2.0)                # one drag step: the mouse moved 5 pixels right and 2 up (3 and 1.2 degrees)
HBM_PEAK = 8.0e12                # bytes/s


def controller(w, h):
    """C2's camera (main.cpp:199-202) with its controls."""
    return CameraController((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, np.float32(w) / np.float32(h))


def drag(rep):
    """The drag step of repetition `rep`: forth, then nine tenths of it back, so that the
    camera stays near C2's and never returns to one it had."""
    return DRAG if rep % 2 == 0 else (-0.9 * DRAG[0], -0.9 * DRAG[1])


def lum(img):
    c = img[..., :3].astype(np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


# ---- cost ------------------------------------------------------------------------------------------------
def copies_alone_ms(stream, bytes_each, reps=5):
    """Two pairs of device-to-device copies of bytes_each, as the call queues them, between HIP events."""
    hip = ctypes.CDLL("libamdhip64.so")
    P = ctypes.c_void_p
    hip.hipMalloc.argtypes = [ctypes.POINTER(P), ctypes.c_size_t]
    hip.hipFree.argtypes = [P]
    hip.hipEventCreate.argtypes = [ctypes.POINTER(P)]
    hip.hipEventRecord.argtypes = [P, P]
    hip.hipEventSynchronize.argtypes = [P]
    hip.hipEventDestroy.argtypes = [P]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), P, P]
    hip.hipMemcpyAsync.argtypes = [P, P, ctypes.c_size_t, ctypes.c_int, P]

    def ck(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    bufs = [P() for _ in range(4)]
    for b in bufs:
        ck(hip.hipMalloc(ctypes.byref(b), bytes_each))
    e0, e1 = P(), P()
    ck(hip.hipEventCreate(ctypes.byref(e0)))
    ck(hip.hipEventCreate(ctypes.byref(e1)))
    out = []
    for _ in range(reps + 1):
        ck(hip.hipEventRecord(e0, stream))
        for _pair in range(2):
            ck(hip.hipMemcpyAsync(bufs[0], bufs[1], bytes_each, 3, stream))      # hipMemcpyDeviceToDevice
            ck(hip.hipMemcpyAsync(bufs[2], bufs[3], bytes_each, 3, stream))
        ck(hip.hipEventRecord(e1, stream))
        ck(hip.hipEventSynchronize(e1))
        ms = ctypes.c_float()
        ck(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        out.append(ms.value)
    for b in bufs:
        hip.hipFree(b)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return out[1:]                                   # the first one warms up


def kernel_bytes(pt, cam_a, w, h):
    """The bytes the kernel needs once: B's two guide reads and the two writes per pixel, and
    the four history images at every unique pixel a tap of a hit pixel loads."""
    import reproject_ref as RP
    pos_b = pt.read_aov("position")
    with np.errstate(all="ignore"):
        taps, x0, y0, _, _, _ = RP.project(pos_b, cam_a, w, h)
    hit = pos_b[..., 3] != 0
    at = [(np.clip(y0 + (i >> 1), 0, h - 1) * w + np.clip(x0 + (i & 1), 0, w - 1))[hit] for i in range(4)]
    unique = int(len(np.unique(np.concatenate(at)))) if hit.any() else 0
    return {"pixels": w * h, "guide_read": 32 * w * h, "written": 32 * w * h, "unique_history_pixels": unique,
            "history_read": 64 * unique, "total": 64 * w * h + 64 * unique}


def cost_at(w, h, reps=5):
    cfg = scenes.bunny_c2(width=w, height=h, spp=1)
    cam = controller(w, h)
    res = {"size": f"{w}x{h}", "runs": []}
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        for guides_current in (True, False):
            for rep in range(reps + 1):              # the first call allocates: reported apart
                # every repetition moves on by a drag step, so neither view's camera rays are
                # found traced already
                cam_a = cam.uniforms()
                assert cam.rotate(*drag(rep))
                cam_b = cam.uniforms()
                pt.set_frame(w, h, cam_a, cfg.max_depth)
                pt.render(0, 8)
                if guides_current:
                    pt.render_guides()
                pt.synchronize()
                pt.set_frame(w, h, cam_b, cfg.max_depth)
                pt.profile_enable(True)
                t0 = time.perf_counter()
                st = pt.reproject(cam_a)
                wall = (time.perf_counter() - t0) * 1e3
                prof = pt.profile_read()
                pt.profile_enable(False)
                res["runs"].append({"guides_of_A_current": guides_current, "first": rep == 0 and guides_current,
                                    "wall_ms": wall, "primary_ms": prof["primary"][0], "primary_launches": prof["primary"][1],
                                    "blend_ms": prof["blend"][0], "blend_launches": prof["blend"][1]})
        res["stats"] = st
        res["bytes"] = kernel_bytes(pt, cam_a, w, h)
        res["copies_alone_ms"] = copies_alone_ms(pt.stream_handle(), w * h * 16, reps)
        # what a camera move costs without the call: the redraw frame (depth 1, frame 0), waited for
        s = InteractiveSession(pt, w, h, cam, cfg.max_depth)
        redraw = []
        for rep in range(reps + 1):
            assert cam.rotate(*drag(rep))         # a new camera every time
            pt.synchronize()
            t0 = time.perf_counter()
            s.frame(redraw=True)
            pt.synchronize()
            redraw.append((time.perf_counter() - t0) * 1e3)
        res["redraw_wall_ms"] = redraw[1:]
    steady = [r for r in res["runs"] if not r["first"]]
    for cur in (True, False):
        sel = [r for r in steady if r["guides_of_A_current"] == cur]
        key = "guides_current" if cur else "guides_rendered_by_the_call"
        res[key] = {k: statistics.median(r[k] for r in sel) for k in ("wall_ms", "primary_ms", "blend_ms")}
    copies = statistics.median(res["copies_alone_ms"])
    kern = res["guides_current"]["blend_ms"] - copies
    res["summary"] = {"copies_alone_ms": copies, "kernel_ms": kern, "redraw_wall_ms": statistics.median(res["redraw_wall_ms"]),
                      "kernel_bytes_per_s": res["bytes"]["total"] / (kern * 1e-3) if kern > 0 else None,
                      "kernel_share_of_hbm_peak": res["bytes"]["total"] / (kern * 1e-3) / HBM_PEAK if kern > 0 else None}
    return res


# ---- quality ---------------------------------------------------------------------------------------------
def quality(w=512, h=512, frames_a=64, ks=(1, 4, 16), long_frames=1024):
    cfg = scenes.bunny_c2(width=w, height=h, spp=1)
    res = {"size": f"{w}x{h}", "frames_at_A": frames_a, "reference_frames": long_frames, "K": {}}
    with PathTracer(0) as pt:
        pt.load(cfg)
        cam = controller(w, h)
        moved = controller(w, h)
        assert moved.rotate(*DRAG)
        pt.set_frame(w, h, moved.uniforms(), cfg.max_depth)
        pt.render(0, long_frames)
        ref = lum(pt.read_accum())
        res["ref_mean_lum"] = float(ref.mean())

        def rmse(img):
            return float(np.sqrt(np.mean((lum(img) - ref) ** 2)))

        def both(s):
            raw = pt.read_accum()
            s.preview_variance()
            return {"raw": rmse(raw), "preview_variance": rmse(pt.read_denoised())}

        for k in ks:
            row = {}
            # (a) redraw, then K frames
            pt.reset_accum()
            s = InteractiveSession(pt, w, h, controller(w, h), cfg.max_depth)
            s.frame_counted(frames_a)
            s.camera = moved
            s.frame(redraw=True)
            pt.enable_moments(True)
            for _ in range(k):
                s.frame()
            row["redraw"] = both(s)
            # (b) reproject, then K frames at every pixel's own weight
            pt.reset_accum()
            s = InteractiveSession(pt, w, h, controller(w, h), cfg.max_depth)
            s.frame_counted(frames_a)
            s.camera = moved
            st = s.reproject()
            s.frame_counted(k)
            row["reproject"] = both(s)
            row["stats"] = st
            res["K"][str(k)] = row
            print(k, json.dumps(row), flush=True)
        n = st["n_pixels"]
        res["shares"] = {x: st["n_" + x] / n for x in ("reprojected", "disoccluded", "missed")}
        del cam
    return res


# ---- pnrt_reproject_view ---------------------------------------------------------
VIEW_FOV = 180.0                 # the fisheye's


def cost_view_at(w, h, reps=5):
    from pnraytracing_amd import _native as N
    cfg = scenes.bunny_c2(width=w, height=h, spp=1)
    cam = controller(w, h)
    res = {"size": f"{w}x{h}", "models": {}}
    med = statistics.median
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        res["copies_alone_ms"] = med(copies_alone_ms(pt.stream_handle(), w * h * 16, reps))
        for model in N.CAM_MODELS + ("pnrt_reproject",):
            runs, rays_ms = [], []
            for rep in range(reps + 1):              # the first call allocates: left out
                cam_a = cam.uniforms()
                assert cam.rotate(*drag(rep))
                cam_b = cam.uniforms()
                pt.set_frame(w, h, cam_a, cfg.max_depth)
                pt.render(0, 8)
                pt.synchronize()
                pt.profile_enable(True)
                t0 = time.perf_counter()
                if model == "pnrt_reproject":        # the call lent nothing: A's guides rendered by the call
                    pt.set_frame(w, h, cam_b, cfg.max_depth)
                    t0 = time.perf_counter()
                    st = pt.reproject(cam_a)
                else:
                    st = pt.reproject_view((model, cam_a, VIEW_FOV), (model, cam_b, VIEW_FOV))
                wall = (time.perf_counter() - t0) * 1e3
                prof = pt.profile_read()
                pt.profile_enable(False)
                runs.append({"wall_ms": wall, "primary_ms": prof["primary"][0], "primary_launches": prof["primary"][1],
                             "blend_ms": prof["blend"][0], "blend_launches": prof["blend"][1]})
                if model != "pnrt_reproject":
                    pt.profile_enable(True)
                    keep = pt.make_rays(model, cam_b, 0, 1, fov_deg=VIEW_FOV)
                    rays_ms.append(pt.profile_read()["blend"][0])
                    pt.profile_enable(False)
                    del keep
            row = {k: med(r[k] for r in runs[1:]) for k in ("wall_ms", "primary_ms", "blend_ms")}
            row["wall_ms_spread"] = [min(r["wall_ms"] for r in runs[1:]), max(r["wall_ms"] for r in runs[1:])]
            row["blend_launches"], row["primary_launches"] = runs[-1]["blend_launches"], runs[-1]["primary_launches"]
            row["make_rays_alone_ms"] = med(rays_ms[1:]) if rays_ms else 0.0
            row["kernel_ms"] = row["blend_ms"] - res["copies_alone_ms"] - 2 * row["make_rays_alone_ms"]
            row["runs"] = runs
            row["stats"] = st
            res["models"][model] = row
    return res


def quality_view(w=512, h=512, frames_a=64, ks=(1, 4, 16), long_frames=1024, model="fisheye", fov=VIEW_FOV):
    cfg = scenes.bunny_c2(width=w, height=h, spp=1)
    res = {"size": f"{w}x{h}", "model": model, "fov_deg": fov, "frames_at_A": frames_a, "reference_frames": long_frames, "K": {}}
    with PathTracer(0) as pt:
        pt.load(cfg)
        moved = controller(w, h)
        assert moved.rotate(*DRAG)
        pt.set_frame(w, h, moved.uniforms(), cfg.max_depth)
        rays = pt.make_rays(model, moved.uniforms(), 0, 1, fov_deg=fov)
        pt.render_rays(0, long_frames, rays, 0)
        ref = lum(pt.read_accum())
        res["ref_mean_lum"] = float(ref.mean())

        def rmse(img):
            return float(np.sqrt(np.mean((lum(img) - ref) ** 2)))

        def session():
            pt.reset_accum()
            s = InteractiveSession(pt, w, h, controller(w, h), cfg.max_depth)
            s.set_camera_model(model, fov_deg=fov)
            s.frame_counted(frames_a)
            s.camera = moved
            return s

        for k in ks:
            row = {}
            s = session()                            # (a) redraw, then K frames
            s.frame(redraw=True)
            pt.enable_moments(True)
            for _ in range(k):
                s.frame()
            row["redraw"] = {"raw": rmse(pt.read_accum())}
            s = session()                            # (b) reproject_view, then K frames at every pixel's own weight
            st = s.reproject_view()
            s.frame_counted(k)
            row["reproject_view"] = {"raw": rmse(pt.read_accum())}
            row["stats"] = st
            res["K"][str(k)] = row
            print(k, json.dumps(row), flush=True)
        n = st["n_pixels"]
        res["shares"] = {x: st["n_" + x] / n for x in ("reprojected", "disoccluded", "missed")}
    return res


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "cost":
        out = {"cost": [cost_at(1920, 1080), cost_at(512, 512)]}
        for c in out["cost"]:
            print(c["size"], json.dumps({k: c[k] for k in ("guides_current", "guides_rendered_by_the_call", "summary", "bytes", "stats")}))
    elif what == "quality":
        out = {"quality": quality()}
    elif what == "cost_view":
        out = {"cost_view": [cost_view_at(1920, 1080), cost_view_at(512, 512)]}
        for c in out["cost_view"]:
            print(c["size"], "copies alone", c["copies_alone_ms"])
            for m, row in c["models"].items():
                print(" ", m, json.dumps({k: v for k, v in row.items() if k != "runs"}))
    elif what == "quality_view":
        out = {"quality_view": quality_view()}
    else:
        sys.exit(__doc__)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(out, f, indent=1)
