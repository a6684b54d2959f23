"""Quality of the two denoised previews against a long render (DESIGN.md section 24.4;
results in profiles/denoise_variance/): C2 and C2 through a 100-degree lens (misses
that show the environment) at 512x512.

  uniform   16 frames for every pixel
  adaptive  8 frames for every pixel, then one adaptive call of 16 frames with the
            median of pnrt_read_error over the filtered pixels as its threshold:
            half of them hold 8 frames, half 24 -- the same budget, non-uniform
            counts

For each: the RMSE of the demodulated luminance, lum(rgb / max(albedo, 1/256)),
over the pixels that are not pass-through, against the same quantity of a long
render, for the raw accumulation image, pnrt_denoise with its defaults and
pnrt_denoise_variance with its defaults.  The long render goes on, 256 frames at a
time, until its own mean_error (pnrt_convergence) is below a tenth of the uniform
16-frame image's; the count is reported.  Reported, not asserted.

usage: python tools/denoise_variance_quality.py [out.json]"""
import dataclasses
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pnraytracing_amd import host as H, scenes  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

W = Hh = 512
ALBEDO_MIN = 1.0 / 256.0


def lum_demod(img, alb):
    c = img[..., :3].astype(np.float64) / np.maximum(alb[..., :3].astype(np.float64), ALBEDO_MIN)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def passthrough(pos, nrm, mats):
    mats = np.asarray(mats, np.float32).reshape(-1, 18)
    mat = nrm[..., 3].astype(np.int64)
    ok = (mat >= 0) & (mat < len(mats))
    return (pos[..., 3] == 0) | (ok & np.any(mats[np.clip(mat, 0, len(mats) - 1), 0:3] != 0, axis=-1))


def three_images(pt):
    raw = pt.read_accum()
    pt.denoise()
    fixed = pt.read_denoised()
    pt.denoise_variance()
    return {"raw": raw, "denoise": fixed, "denoise_variance": pt.read_denoised()}


def run(cfg):
    res = {}
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        pt.render_guides()
        alb = pt.read_aov("albedo")
        keep = ~passthrough(pt.read_aov("position"), pt.read_aov("normal"), cfg.packed.materials)
        res["pixels"], res["pixels_filtered"] = int(keep.size), int(keep.sum())
        pt.render(0, 16)
        e16 = pt.convergence(0.0)["mean_error"]
        uniform = three_images(pt)
        frames = 16
        while True:                              # the long render continues the same sequence
            pt.render(frames, 256)
            frames += 256
            e_long = pt.convergence(0.0)["mean_error"]
            if e_long < 0.1 * e16 or frames >= 16384:
                break
        ref = lum_demod(pt.read_accum(), alb)
        res.update(mean_error_16=e16, long_frames=frames, mean_error_long=e_long)

        pt.reset_accum()
        pt.render(0, 8)
        thr = float(np.median(pt.read_error()[keep]))     # (a miss shows one constant colour: its error is 0)
        st = pt.render_adaptive(8, 16, threshold=thr, min_frames=2)
        n = pt.read_moments()[..., 3].view(np.uint32)
        res["adaptive_counts"] = {str(k): int(v) for k, v in zip(*np.unique(n, return_counts=True))}
        res["adaptive_threshold"], res["adaptive_active_pixels"] = thr, int(st["n_active_pixels"])
        adaptive = three_images(pt)

    def rmse(img):
        return float(np.sqrt(np.mean((lum_demod(img, alb)[keep] - ref[keep]) ** 2)))
    res["rmse_uniform16"] = {k: rmse(v) for k, v in uniform.items()}
    res["rmse_adaptive_8_24"] = {k: rmse(v) for k, v in adaptive.items()}
    res["ref_mean_lum_demod"] = float(ref[keep].mean())
    return res


c2 = scenes.bunny_c2(width=W, height=Hh, spp=1)
wide = dataclasses.replace(c2, name="C2-bunny-wide",
                           camera=H.camera_update((0, 2.8, 7), (0, 2.8, 0), (0, 1, 0), 100.0, np.float32(W) / np.float32(Hh)))
out = {"size": f"{W}x{Hh}", "scenes": {}}
for name, cfg in (("c2", c2), ("c2wide", wide)):
    out["scenes"][name] = run(cfg)
    print(name, json.dumps(out["scenes"][name]))

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
