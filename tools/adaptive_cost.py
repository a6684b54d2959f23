"""Cost and yield of adaptive sampling (results in
profiles/adaptive/): the C2 scene at 1920x1080, 16-frame calls, the caller waiting for
every call (host clock around call + pnrt_synchronize), moments enabled throughout.

* indirection: pnrt_render_adaptive with every pixel active (min_frames = 0xFFFFFFFF)
  against pnrt_render, alternating, ROUNDS rounds of CALLS calls each: wall ms per call,
  and per-class pnrt_profile_read ms per call from a second group of calls per round;
* yield: after 64 plain frames, the thresholds at which about 3/4, 1/2 and 1/4 of the
  tiles are still active (bisection over pnrt_render_adaptive's n_frames = 0 query), and
  at each one successive adaptive 16-frame calls: wall ms beside the active-pixel and
  active-tile shares of each call;
* fixed cost: the n_frames = 0 call (wait, mask, scan, scatter, readback) alone, and
  plain calls issued back to back without a wait against waited ones (what a call loses
  by not pipelining with its predecessor).

usage: python tools/adaptive_cost.py [out.json]"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pnraytracing_amd import scenes  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

W, H, FRAMES = 1920, 1080, 16
ROUNDS, CALLS, LAT_N = 5, 4, 30
ALL = 0xFFFFFFFF
CLASSES = ("primary", "gen", "trace", "shade", "blend")
out = {"shape": f"C2 {W}x{H}, {FRAMES}-frame calls", "rounds": ROUNDS, "calls_per_round": CALLS, "unit": "ms"}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "values": [round(x, 4) for x in v]}


def timed(pt, call):
    t = time.perf_counter()
    st = call()
    pt.synchronize()
    return (time.perf_counter() - t) * 1e3, st


def main():
    cfg = scenes.bunny_c2(width=W, height=H, spp=1)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        f = [0]

        def plain():
            pt.render(f[0], FRAMES)
            f[0] += FRAMES

        def adaptive_all():
            st = pt.render_adaptive(f[0], FRAMES, 0.0, ALL)
            f[0] += FRAMES
            return st

        for call in (plain, adaptive_all, plain, adaptive_all):      # sizes the buffers of both
            timed(pt, call)

        # ---- indirection ----------------------------------------------------------------------
        modes = {"plain": plain, "adaptive_all_active": adaptive_all}
        wall = {k: [] for k in modes}
        prof = {k: {c: [] for c in CLASSES} for k in modes}
        for _ in range(ROUNDS):
            for name, call in modes.items():
                wall[name].append(statistics.mean(timed(pt, call)[0] for _ in range(CALLS)))
                pt.profile_enable(True)
                for _ in range(CALLS):
                    timed(pt, call)
                p = pt.profile_read()
                pt.profile_enable(False)
                for c in CLASSES:
                    prof[name][c].append(p[c][0] / CALLS)
        out["indirection"] = {k: {"wall_ms_per_call": spread(wall[k]),
                                  "class_ms_per_call": {c: spread(prof[k][c]) for c in CLASSES}} for k in modes}
        out["indirection"]["wall_ratio_adaptive_over_plain"] = (statistics.median(wall["adaptive_all_active"]) /
                                                                statistics.median(wall["plain"]))
        print("indirection", json.dumps({k: round(statistics.median(v), 3) for k, v in wall.items()}),
              "ratio", round(out["indirection"]["wall_ratio_adaptive_over_plain"], 4))

        # ---- pipelining: plain calls back to back against waited ones ----------------------------
        b2b = []
        for _ in range(ROUNDS):
            t = time.perf_counter()
            for _ in range(CALLS):
                plain()
            pt.synchronize()
            b2b.append((time.perf_counter() - t) * 1e3 / CALLS)
        out["plain_back_to_back_ms_per_call"] = spread(b2b)
        print("plain back to back", round(statistics.median(b2b), 3))

        # ---- yield ------------------------------------------------------------------------------
        def restart():
            pt.reset_accum()
            for k in range(4):
                pt.render(16 * k, 16)
            pt.synchronize()
            f[0] = 64

        def tiles_at(thr):
            st = pt.render_adaptive(f[0], 0, thr, 2)
            return st["n_active_tiles"] / st["n_tiles"], st

        restart()
        out["convergence_after_64_frames"] = {str(t): pt.convergence(t) for t in (0.01, 0.02, 0.05, 0.1, 0.2)}
        out["yield"] = {}
        for share in (0.75, 0.5, 0.25):
            restart()
            lo, hi = 0.0, 1.0                        # the active share falls with the threshold
            for _ in range(14):
                mid = (lo + hi) / 2
                if tiles_at(mid)[0] > share:
                    lo = mid
                else:
                    hi = mid
            thr = hi
            got, st0 = tiles_at(thr)
            calls = []
            for _ in range(6):
                ms, st = timed(pt, lambda: pt.render_adaptive(f[0], FRAMES, thr, 2))
                f[0] += FRAMES
                calls.append({"ms": round(ms, 4), "pixel_share": st["n_active_pixels"] / st["n_pixels"],
                              "tile_share": st["n_active_tiles"] / st["n_tiles"], "frames_per_batch": st["frames_per_batch"],
                              "n_batches": st["n_batches"]})
            out["yield"][f"tile_share_{share}"] = {"threshold": thr, "before": st0, "calls": calls}
            print("yield", share, "threshold", round(thr, 5), json.dumps(calls[:3]))

        # ---- fixed cost ---------------------------------------------------------------------------
        restart()
        thr = out["yield"]["tile_share_0.5"]["threshold"]
        ts = sorted(timed(pt, lambda: pt.render_adaptive(f[0], 0, thr, 2))[0] for _ in range(LAT_N + 3))[:LAT_N]
        out["mask_step_only_ms"] = {"median": statistics.median(ts), "min": ts[0], "p90": ts[int(0.9 * (LAT_N - 1))]}
        ts = sorted(timed(pt, lambda: pt.render_adaptive(f[0], FRAMES, 65535.0, 2))[0] for _ in range(LAT_N + 3))[:LAT_N]
        out["fully_converged_call_ms"] = {"median": statistics.median(ts), "min": ts[0], "p90": ts[int(0.9 * (LAT_N - 1))]}
        print("mask step only", out["mask_step_only_ms"], "fully converged call", out["fully_converged_call_ms"])

    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
