"""Cost of the sample moments (results in profiles/moments/):

* PNRT_K_BLEND ms per launch (pnrt_profile_read, HIP events around the blend alone)
  with moments off and on, for the two timed shapes -- C2 at 1920x1080 in 16-frame
  calls (bench.py's), and the C2 scene at 512x512 in one-frame calls (bench.py's D2)
  -- calls issued back to back, ROUNDS rounds of CALLS calls, each round's mean;
* pnrt_convergence and pnrt_read_error, host clock around the synchronous call, at
  both sizes.

--tree DIR imports the package from another checkout (e.g. the parent commit's, to
compare the plain blend across commits in one session); a library without
pnrt_enable_moments measures the plain blend only.

usage: python tools/moments_cost.py [--tree DIR] [out.json]"""
import json
import os
import statistics
import sys
import time

argv = sys.argv[1:]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if argv[:1] == ["--tree"]:
    REPO, argv = os.path.abspath(argv[1]), argv[2:]
sys.path.insert(0, REPO)
from pnraytracing_amd import scenes  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

ROUNDS, CALLS, LAT_N = 7, 8, 30
SHAPES = {"C2_1920x1080_16frames": (1920, 1080, 16), "D2_512x512_1frame": (512, 512, 1)}
out = {"tree": REPO, "rounds": ROUNDS, "calls_per_round": CALLS, "unit": "ms", "shapes": {}}


def blend_ms(pt, frames, first):
    """Mean PNRT_K_BLEND ms per launch over CALLS back-to-back calls, per round."""
    rounds = []
    for _ in range(ROUNDS):
        pt.profile_select(["blend"])
        pt.profile_enable(True)
        for _ in range(CALLS):
            pt.render(first, frames)
            first += frames
        ms, n = pt.profile_read()["blend"]
        pt.profile_enable(False)
        assert n == CALLS, (n, CALLS)
        rounds.append(ms / n)
    return {"rounds": [round(v, 5) for v in rounds], "median": statistics.median(rounds), "min": min(rounds),
            "max": max(rounds)}, first


def latency(fn):
    ts = []
    for _ in range(LAT_N + 3):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    ts = sorted(ts[3:])
    return {"median": statistics.median(ts), "min": ts[0], "p90": ts[int(0.9 * (LAT_N - 1))]}


for name, (W, Hh, frames) in SHAPES.items():
    cfg = scenes.bunny_c2(width=W, height=Hh, spp=1)
    r = {}
    with PathTracer(0) as pt:
        pt.load(cfg)
        has = hasattr(pt, "enable_moments")
        pt.render(0, frames)                         # sizes the buffers
        pt.render(frames, frames)
        pt.synchronize()
        f = 2 * frames
        # off, on, off, on: the two alternate inside the session
        for rep in range(2):
            r[f"blend_off_{rep}"], f = blend_ms(pt, frames, f)
            if has:
                pt.enable_moments(True)
                r[f"blend_on_{rep}"], f = blend_ms(pt, frames, f)
                pt.enable_moments(False)
        if has:
            pt.enable_moments(True)
            pt.render(f, frames)
            pt.synchronize()
            r["convergence"] = latency(lambda: pt.convergence(0.05))
            r["read_error"] = latency(pt.read_error)
            r["read_accum_for_scale"] = latency(pt.read_accum)
            off = statistics.median([r["blend_off_0"]["median"], r["blend_off_1"]["median"]])
            on = statistics.median([r["blend_on_0"]["median"], r["blend_on_1"]["median"]])
            r["on_over_off"] = on / off
            r["byte_model_on_over_off"] = (16 * frames + 64) / (16 * frames + 32)
    out["shapes"][name] = r
    print(name, json.dumps({k: (round(v["median"], 5) if isinstance(v, dict) else round(v, 4)) for k, v in r.items()}))

if argv:
    with open(argv[0], "w") as fh:
        json.dump(out, fh, indent=1)
