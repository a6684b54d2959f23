"""Cost of pnrt_denoise_variance beside pnrt_denoise at the same level count, in one
session on one context (HIP events on the context stream, warm, median of N), at
512x512 and 1920x1080 on the C2 scene (results in
profiles/denoise_variance/).  The sibling of tools/denoise_cost.py, whose timing
loop this is.

usage: python tools/denoise_variance_cost.py [out.json]"""
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pnraytracing_amd import scenes  # noqa: E402
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
    r = {}
    with PathTracer(0) as pt:
        stream = torch.cuda.ExternalStream(pt.stream_handle())
        torch.cuda.set_stream(stream)
        pt.set_stream(stream.cuda_stream)
        pt.load(cfg)
        pt.enable_moments()
        pt.render(0, 4)
        pt.render_guides()
        pt.synchronize()
        for lv in (1, 2, 3, 4, 5):          # the two filters alternate, level by level
            r[f"denoise_levels{lv}"] = timed(stream, lambda: pt.denoise(levels=lv))
            r[f"denoise_variance_levels{lv}"] = timed(stream, lambda: pt.denoise_variance(levels=lv))
        torch.cuda.synchronize()
    med = {k: v["median"] for k, v in r.items()}
    for name in ("denoise", "denoise_variance"):
        inc = {f"pass{i}_step{1 << i}": med[f"{name}_levels{i + 1}"] - med[f"{name}_levels{i}"] for i in range(1, 5)}
        inc["prep_plus_pass0"] = med[f"{name}_levels1"]
        r[f"{name}_per_pass_increment"] = inc
    r["ratio_variance_over_fixed"] = {f"levels{lv}": med[f"denoise_variance_levels{lv}"] / med[f"denoise_levels{lv}"]
                                      for lv in (1, 2, 3, 4, 5)}
    out["sizes"][f"{W}x{Hh}"] = r
    print(W, Hh, json.dumps({k: (round(v["median"], 4) if "median" in v else {a: round(b, 4) for a, b in v.items()})
                             for k, v in r.items()}))

if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
