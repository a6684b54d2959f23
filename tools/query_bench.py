"""Rate of pnrt_query_rays_device on the C2 scene at 1920x1080 (DESIGN.md section 23;
results in profiles/query/): Mrays/s of the camera family (every pixel's camera ray,
closest hit), of `bounce` (closest hit) and of `shadow` (any hit), 2 073 600 rays each,
from the library's own launch timing (class PNRT_K_PRIMARY: HIP events around the launch)
-- warm, RUNS runs of N launches each.

Yardstick for the camera family: the PNRT_K_PRIMARY launch of pnrt_render_guides on a
camera no records exist for, which traces exactly those rays with the same step and
writes 48 B per ray where the query reads 28 B and writes 64 B.  The extra 92 B per ray
are priced with a plain device copy of as many bytes of traffic.

usage: python tools/query_bench.py [out.json]      (PNRT_DEVICE_LIB selects another build)"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import isect_rays  # noqa: E402
from pnraytracing_amd import scenes  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

W, Hh = 1920, 1080
N, RUNS, WARM = 10, 3, 3
F = np.float32


def camera_rays(cfg):
    """CameraGetRay for every pixel, row 0 = bottom (tests/guides_common.py camera_rays)."""
    eye, llc, hor, ver = np.asarray(cfg.camera, F).reshape(4, 3)
    py, px = np.mgrid[0:cfg.height, 0:cfg.width]
    s = (px.astype(F) / F(cfg.width)).reshape(-1, 1)
    t = (py.astype(F) / F(cfg.height)).reshape(-1, 1)
    d = (((llc + s * hor) + t * ver) - eye).astype(F)
    d = (d / np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F))[:, None]).astype(F)
    rays = np.empty((len(d), 7), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = eye, d, F(1e7)
    return rays


def primary_ms(pt, fn):
    """Mean PNRT_K_PRIMARY launch time (ms) of N calls of fn, RUNS times, after WARM calls."""
    for _ in range(WARM):
        fn()
    pt.synchronize()
    runs = []
    for _ in range(RUNS):
        pt.profile_enable(True)
        for _ in range(N):
            fn()
        ms, launches = pt.profile_read()["primary"]
        assert launches == N, launches
        runs.append(ms / launches)
    pt.profile_enable(False)
    return runs


def main():
    cfg = scenes.bunny_c2(width=W, height=Hh, spp=1)
    n = W * Hh
    fam = {"camera": (camera_rays(cfg), False),
           "bounce": (isect_rays.make_rays(cfg.packed, cfg.camera, "bounce", n, 1), False),
           "shadow": (isect_rays.make_rays(cfg.packed, cfg.camera, "shadow", n, 1), True)}
    out = {"scene": cfg.name, "width": W, "height": Hh, "rays": n, "launches_per_run": N, "runs": RUNS, "unit": "ms",
           "families": {}}
    with PathTracer(0) as pt:
        out["version"] = pt.version()
        stream = torch.cuda.ExternalStream(pt.stream_handle())
        torch.cuda.set_stream(stream)
        pt.set_stream(stream.cuda_stream)
        pt.load(cfg)
        pt.profile_select(["primary"])
        rec = torch.empty((n, 16), dtype=torch.int32, device="cuda")
        for name, (rays, any_hit) in fam.items():
            r = torch.from_numpy(rays).to("cuda")
            ms = primary_ms(pt, lambda: pt.query_rays_device(r.data_ptr(), n, rec.data_ptr(), any_hit))
            hits = int((rec[:, 0] != 0).sum().item())
            out["families"][name] = {"any_hit": any_hit, "ms": ms, "mrays_per_s": [n / m / 1e3 for m in ms], "hits": hits}
            print(f"{name:7s} any_hit={int(any_hit)} hits {hits:8d}  ms {['%.4f' % m for m in ms]}  "
                  f"Mrays/s {['%.0f' % (n / m / 1e3) for m in ms]}", flush=True)
        k = [0]

        def guides_traced():      # a camera no records exist for, every time: the guides' own trace launch
            k[0] += 1
            cam = np.array(cfg.camera, F).reshape(4, 3)
            cam[0, 0] += F(1e-6) * k[0]
            pt.set_frame(W, Hh, cam, 4)
            pt.render_guides()
        out["guides_primary_ms"] = primary_ms(pt, guides_traced)
        # the traffic a query adds to the guides' launch: 28 B in + 64 B out against 48 B out = 44 B more,
        # and its whole stream, 92 B per ray: a device copy of 46 B per ray moves 92 B
        for label, per_ray in (("copy_92B_per_ray_ms", 46), ("copy_44B_per_ray_ms", 22)):
            src = torch.empty(n * per_ray, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            ts = []
            for _ in range(WARM):
                dst.copy_(src)
            for _ in range(RUNS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                for _ in range(N):
                    dst.copy_(src)
                b.record(stream)
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) / N)
            out[label] = ts
        torch.cuda.synchronize()
    q, g = min(out["families"]["camera"]["ms"]), min(out["guides_primary_ms"])
    out["camera_over_guides_primary"] = q / g
    print(f"guides' primary launch ms {['%.4f' % m for m in out['guides_primary_ms']]}; query / guides = {q / g:.3f}; "
          f"copy of 92 B/ray ms {['%.4f' % m for m in out['copy_92B_per_ray_ms']]}, of 44 B/ray "
          f"{['%.4f' % m for m in out['copy_44B_per_ray_ms']]}")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
