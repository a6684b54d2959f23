"""Cost and quality of pnrt_render_rays (results in profiles/rays/).
Reported, not asserted.

  cost cameras   pnrt_render_cameras with the camera sequence (aa_width 1, a lens of 1 % of the
                 scene's width focused on the bunny): the yardstick.  Runs on any library that
                 has the call (PNRT_DEVICE_LIB: the parent commit's build).
  cost rays      pnrt_render_rays on pinhole rays of the same lens: one set for every frame
                 (frame_stride 0), a set per frame made before the clock starts, and a set per
                 frame with its pnrt_make_rays call inside the clock.
                 Both: C2 at 1920x1080 in 16-frame calls (4 per repetition, pipelined) and at
                 512x512 in one-frame synchronised calls (32 per repetition); two warm-up
                 repetitions, then median, minimum and maximum of five; and from a run of its
                 own the per-class profile.
  quality        C2 at 512x512 with that lens at 4, 16 and 64 frames: luminance RMSE against a
                 long render (4096 frames whose lens and pixel samples are another frame
                 range's, per pixel), lens and pixel-filter samples per frame (per_pixel 0)
                 against per pixel (1), raw and under pnrt_denoise_variance.

  adaptive       pnrt_render_rays_adaptive (results in profiles/rays_adaptive/):
                 C2 at 1920x1080, 16-frame calls of a set per frame with that lens, the moments on,
                 the host clock around a call and the synchronise that ends it.  Every repetition
                 starts from the same state -- 64 frames of pnrt_render_rays on the lens sets, made
                 again outside the clock -- so the mask is the same in every repetition and in both
                 builds.  `yardstick` (any library with pnrt_render_rays and pnrt_render_adaptive:
                 the parent commit's build through PNRT_DEVICE_LIB): pnrt_render_rays, and
                 pnrt_render_adaptive at the thresholds that leave half and a quarter of the tiles
                 active.  `this`: pnrt_render_rays_adaptive with every tile active and at those two
                 thresholds.  Two warm-up repetitions, then median, minimum and maximum of five;
                 `profile`: the per-class profile of one call of each of this tree's variants, alone.

usage: python tools/rays_bench.py cost cameras|rays [out.json] | quality [out.json] |
                                  adaptive yardstick|this|profile [out.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tools")]
from cameras_bench import SCENE_WIDTH, focus_on_bunny, lum  # noqa: E402
from pnraytracing_amd import host as H  # noqa: E402
from pnraytracing_amd import scenes  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

RADIUS = 0.01 * SCENE_WIDTH


def cost_at(which, w, h, frames_per_call, calls_per_rep, sync_each, reps=5, warm=2):
    cfg = scenes.bunny_c2(width=w, height=h, spp=1)
    res = {"size": f"{w}x{h}", "frames_per_call": frames_per_call, "calls_per_repetition": calls_per_rep,
           "synchronised_calls": sync_each}
    pix = w * h
    with PathTracer(0) as pt:
        res["library"] = pt.version()
        pt.load(cfg)
        focus, _ = focus_on_bunny(pt, cfg, w, h)
        pin = np.asarray(cfg.camera, np.float32).reshape(12)
        lens = {"aa_width": 1.0, "lens_radius": RADIUS, "focus_distance": focus}
        variants = ("cameras_sequence",) if which == "cameras" else ("rays_one_set", "rays_sets", "rays_sets_with_make_rays")
        bufs = None
        if which == "rays":
            import torch
            n_sets = frames_per_call
            bufs = [torch.empty(((n_sets - 1) * pix + pix, 8), dtype=torch.float32, device="cuda") for _ in range(calls_per_rep)]
            torch.cuda.synchronize()

        def repetition(variant, first):
            # what is made before the clock starts is not the call's cost
            tables = None
            if variant == "cameras_sequence":
                tables = [H.camera_sequence(pin, w, h, first + i * frames_per_call, frames_per_call, 1.0, RADIUS, focus)
                          for i in range(calls_per_rep)]
            elif variant in ("rays_one_set", "rays_sets"):
                for i in range(calls_per_rep):
                    pt.make_rays("pinhole", cfg.camera, first + i * frames_per_call, 1 if variant == "rays_one_set" else frames_per_call,
                                 pix, out=bufs[i], **lens)
            pt.synchronize()
            t0 = time.perf_counter()
            for i in range(calls_per_rep):
                f = first + i * frames_per_call
                if variant == "cameras_sequence":
                    pt.render_cameras(f, tables[i])
                else:
                    if variant == "rays_sets_with_make_rays":
                        pt.make_rays("pinhole", cfg.camera, f, frames_per_call, pix, out=bufs[i], **lens)
                    pt.render_rays(f, frames_per_call, bufs[i], 0 if variant == "rays_one_set" else pix)
                if sync_each:
                    pt.synchronize()
            pt.synchronize()
            return (time.perf_counter() - t0) * 1e3 / calls_per_rep

        step = frames_per_call * calls_per_rep
        for variant in variants:
            pt.reset_accum()
            ms = [repetition(variant, r * step) for r in range(warm + reps)][warm:]
            res[variant] = {"ms_per_call": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}, "all_ms": ms}
        for variant in variants:                     # the per-class profile: a run of its own
            pt.reset_accum()
            repetition(variant, 0)
            pt.profile_enable(True)
            repetition(variant, step)
            prof = pt.profile_read()
            pt.profile_enable(False)
            res[variant]["profile_ms_per_call"] = {k: v[0] / calls_per_rep for k, v in prof.items() if v[1]}
            res[variant]["profile_launches_per_call"] = {k: v[1] / calls_per_rep for k, v in prof.items() if v[1]}
    return res


def quality(w=512, h=512, counts=(4, 16, 64), long_frames=4096):
    cfg = scenes.bunny_c2(width=w, height=h, spp=1)
    res = {"size": f"{w}x{h}", "long_frames": long_frames}
    pix = w * h
    with PathTracer(0) as pt:
        pt.load(cfg)
        focus, _ = focus_on_bunny(pt, cfg, w, h)
        lens = {"aa_width": 1.0, "lens_radius": RADIUS, "focus_distance": focus}
        res["lens"] = lens
        pt.reset_accum()
        for f in range(0, long_frames, 64):          # frames 0.. (the blend weighs by frame number) with the lens and pixel
            # samples of another frame range: independent of both short renders' samples
            pt.render_rays(f, 64, pt.make_rays("pinhole", cfg.camera, 1000000 + f, 64, pix, per_pixel=1, **lens), pix)
            pt.synchronize()
        ref = lum(pt.read_accum())
        pt.render_guides()                           # the centre view's guides, as the session's preview takes them
        for n in counts:
            for pp in (0, 1):
                pt.enable_moments(True)
                pt.reset_accum()
                rays = pt.make_rays("pinhole", cfg.camera, 0, n, pix, per_pixel=pp, **lens)
                pt.render_rays(0, n, rays, pix)
                raw = lum(pt.read_accum())
                pt.denoise_variance()
                den = lum(pt.read_denoised())
                pt.enable_moments(False)
                res[f"frames_{n}_per_pixel_{pp}"] = {"rmse_raw": float(np.sqrt(np.mean((raw - ref) ** 2))),
                                                     "rmse_denoise_variance": float(np.sqrt(np.mean((den - ref) ** 2)))}
    return res


def adaptive(which, w=1920, h=1080, frames=16, reps=5, warm=2):
    cfg = scenes.bunny_c2(width=w, height=h, spp=1)
    res = {"size": f"{w}x{h}", "frames_per_call": frames, "state_frames": 64}
    pix = w * h
    ALL = 0xFFFFFFFF
    with PathTracer(0) as pt:
        import torch
        res["library"] = pt.version()
        pt.load(cfg)
        focus, _ = focus_on_bunny(pt, cfg, w, h)
        lens = {"aa_width": 1.0, "lens_radius": RADIUS, "focus_distance": focus}
        buf = torch.empty((frames * pix, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        pt.enable_moments(True)

        def restart():
            """64 frames of the lens sets, then the call's own sets (frames 64 ..) in the buffer."""
            pt.reset_accum()
            for f in range(0, 64 + frames, frames):
                pt.make_rays("pinhole", cfg.camera, f, frames, pix, out=buf, **lens)
                if f < 64:
                    pt.render_rays(f, frames, buf, pix)
            pt.synchronize()

        def threshold_for(share):                    # the active-tile share falls with the threshold
            lo, hi = 0.0, 1.0
            for _ in range(14):
                mid = (lo + hi) / 2
                st = pt.render_adaptive(64, 0, mid, 2)
                lo, hi = (mid, hi) if st["n_active_tiles"] / st["n_tiles"] > share else (lo, mid)
            return hi

        restart()
        thr = {"half": threshold_for(0.5), "quarter": threshold_for(0.25)}
        res["thresholds"] = thr
        if which == "yardstick":
            variants = {"render_rays": lambda: pt.render_rays(64, frames, buf, pix),
                        "render_adaptive_half": lambda: pt.render_adaptive(64, frames, thr["half"], 2),
                        "render_adaptive_quarter": lambda: pt.render_adaptive(64, frames, thr["quarter"], 2)}
        else:
            variants = {"rays_adaptive_all": lambda: pt.render_rays_adaptive(64, frames, buf, pix, 0.0, ALL),
                        "rays_adaptive_half": lambda: pt.render_rays_adaptive(64, frames, buf, pix, thr["half"], 2),
                        "rays_adaptive_quarter": lambda: pt.render_rays_adaptive(64, frames, buf, pix, thr["quarter"], 2)}

        def repetition(call):
            restart()
            t0 = time.perf_counter()
            st = call()
            pt.synchronize()
            return (time.perf_counter() - t0) * 1e3, st

        for name, call in variants.items():
            if which == "profile":
                repetition(call)
                restart()
                pt.profile_enable(True)
                st = call()
                pt.synchronize()
                prof = pt.profile_read()
                pt.profile_enable(False)
                res[name] = {"profile_ms": {k: v[0] for k, v in prof.items() if v[1]},
                             "profile_launches": {k: v[1] for k, v in prof.items() if v[1]}, "stats": st}
                continue
            runs = [repetition(call) for _ in range(warm + reps)][warm:]
            ms = [r[0] for r in runs]
            res[name] = {"ms_per_call": {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}, "all_ms": ms,
                         "stats": runs[-1][1]}
    return res


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "cost" and len(sys.argv) > 2 and sys.argv[2] in ("cameras", "rays"):
        out = {"cost": [cost_at(sys.argv[2], 1920, 1080, 16, 4, False), cost_at(sys.argv[2], 512, 512, 1, 32, True)]}
        for c in out["cost"]:
            print(c["size"], json.dumps({v: {k: c[v][k] for k in c[v] if k != "all_ms"} for v in c if isinstance(c[v], dict)}))
        path = sys.argv[3] if len(sys.argv) > 3 else None
    elif what == "adaptive" and len(sys.argv) > 2 and sys.argv[2] in ("yardstick", "this", "profile"):
        out = {"adaptive": adaptive(sys.argv[2])}
        print(json.dumps({k: ({q: v[q] for q in v if q != "all_ms"} if isinstance(v, dict) else v) for k, v in out["adaptive"].items()}))
        path = sys.argv[3] if len(sys.argv) > 3 else None
    elif what == "quality":
        out = {"quality": quality()}
        print(json.dumps(out))
        path = sys.argv[2] if len(sys.argv) > 2 else None
    else:
        sys.exit(__doc__)
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
