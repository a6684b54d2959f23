"""Cost of pnrt_render_guides and pnrt_denoise (HIP events on the context stream, warm,
median of N) beside a plain device copy of each pass's compulsory bytes, at 512x512
and 1920x1080 on the C2 scene (results in
profiles/guides_denoise/).  PNRT_DEVICE_LIB selects another build of the library
(e.g. one compiled with -DDN_LDS_MAX_STEP=0 for the A/B).

usage: python tools/denoise_cost.py [out.json]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pnraytracing_amd import host as H, scenes  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

N = 30
out = {"n": N, "unit": "ms", "sizes": {}}


def timed(stream, fn, n=N, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median": statistics.median(ts), "min": ts[0], "p90": ts[int(0.9 * (n - 1))]}


for (W, Hh) in [(512, 512), (1920, 1080)]:
    cfg = scenes.bunny_c2(width=W, height=Hh, spp=1)
    pix = W * Hh
    r = {}
    with PathTracer(0) as pt:
        stream = torch.cuda.ExternalStream(pt.stream_handle())
        torch.cuda.set_stream(stream)
        pt.set_stream(stream.cuda_stream)
        pt.load(cfg)
        pt.render(0, 4)
        pt.synchronize()
        r["guides_borrowed_records"] = timed(stream, pt.render_guides)
        k = [0]

        def guides_traced():      # a camera no records exist for, every time
            k[0] += 1
            cam = H.camera_update((0.001 * k[0], 2.8, 7), (0, 2.8, 0), (0, 1, 0), 45.0, np.float32(W) / np.float32(Hh))
            pt.set_frame(W, Hh, cam, 4)
            pt.render_guides()
        r["guides_own_trace"] = timed(stream, guides_traced)
        pt.set_frame(W, Hh, cfg.camera, 4)
        pt.render_guides()
        for lv in (1, 2, 3, 4, 5):
            r[f"denoise_levels{lv}"] = timed(stream, lambda: pt.denoise(levels=lv))
        # a plain copy of one pass's compulsory bytes: 32 B guide record + 16 B colour read, 16 B written
        # per pixel = 64 B of traffic = a 32-byte-per-pixel device-to-device copy
        src = torch.empty(pix * 32, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        r["copy_64B_per_pixel"] = timed(stream, lambda: dst.copy_(src))
        # the prep kernel's: 4 x 16 B read, 48 B written = 112 B
        src2 = torch.empty(pix * 56, dtype=torch.uint8, device="cuda")
        dst2 = torch.empty_like(src2)
        r["copy_112B_per_pixel"] = timed(stream, lambda: dst2.copy_(src2))
        torch.cuda.synchronize()
    med = {k2: v["median"] for k2, v in r.items()}
    r["per_pass_increment"] = {f"pass{i}_step{1 << i}": med[f"denoise_levels{i + 1}"] - (med[f"denoise_levels{i}"] if i else 0.0)
                               for i in range(5)}
    r["per_pass_increment"]["pass0_step1"] = None      # levels=1 is prep + pass 0
    r["prep_plus_pass0"] = med["denoise_levels1"]
    out["sizes"][f"{W}x{Hh}"] = r
    print(W, Hh, json.dumps({k2: (round(v["median"], 4) if isinstance(v, dict) and "median" in v else v) for k2, v in r.items()}))

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
