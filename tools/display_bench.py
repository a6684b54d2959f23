"""Cost of the display transform (results in profiles/display/),
on the C2 scene after 16 frames at 1920x1080 and 512x512, in one session:

  * pnrt_display's kernel, CLAMP + LINEAR and ACES + sRGB: HIP events on the context
    stream (warm, median of N) and the library's own PNRT_K_BLEND class;
  * pnrt_luma_histogram_read: the synchronous call on the host clock and its kernel in
    the BLEND class, for the library as built and for the other LDS layout
    (-DLUMA_HIST_PER_WAVE=1, a variant library that `--build-variant` compiles; each
    layout runs in child processes of its own, alternating);
  * a host-visible 8-bit image per frame: pnrt_display + pnrt_read_display against
    pnrt_read_accum + image.to_display (the only way before pnrt_display; both paths are
    this library's, the second unchanged from the parent commit), on the host clock;
  * D2 (512x512, one frame per call, synchronised) with a displayed image per frame,
    both ways, and without one.

usage: python tools/display_bench.py --build-variant          (no GPU needed)
       python tools/display_bench.py [out.json]"""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pnraytracing_amd import build  # noqa: E402

N = 50
SIZES = [(1920, 1080), (512, 512)]
VARIANT = os.path.join(build.PKG, "variants", "libpnrt_histwave.so")


def build_variant():
    os.makedirs(os.path.dirname(VARIANT), exist_ok=True)
    subprocess.run(build.device_cmd(VARIANT, ["-DLUMA_HIST_PER_WAVE=1"]), check=True)
    print(VARIANT)


def stats(ts):
    ts = sorted(ts)
    return {"median": statistics.median(ts), "min": ts[0], "p90": ts[int(0.9 * (len(ts) - 1))]}


def host_timed(fn, n=N, warm=5):
    """ms per call of a function that ends synchronised."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return stats(ts)


def loaded(W, H):
    from pnraytracing_amd import scenes
    from pnraytracing_amd.tracer import PathTracer
    pt = PathTracer(0)
    pt.load(scenes.bunny_c2(width=W, height=H, spp=1))
    pt.render(0, 16)
    pt.synchronize()
    return pt


def blend_class(pt, fn, n=N):
    """ms per launch of the PNRT_K_BLEND class over n calls."""
    pt.profile_select(["blend"])
    pt.profile_enable(True)
    for _ in range(n):
        fn()
    ms, launches = pt.profile_read()["blend"]
    pt.profile_enable(False)
    pt.profile_select(None)
    return {"ms_per_launch": ms / launches, "launches": launches}


def hist_child():
    """One layout (the library PNRT_DEVICE_LIB names) at both sizes: a JSON line."""
    out = {}
    for W, H in SIZES:
        pt = loaded(W, H)
        r = {"call_host_ms": host_timed(pt.luma_histogram), "kernel": blend_class(pt, pt.luma_histogram)}
        h = pt.luma_histogram()
        r["n_counted"], r["bins_used"], r["largest_bin_share"] = h["n_counted"], int((h["bins"] > 0).sum()), \
            float(h["bins"].max() / max(h["n_counted"], 1))
        r["bins_sha1"] = hashlib.sha1(h["bins"].tobytes()).hexdigest()[:12]      # the layouts count the same
        out[f"{W}x{H}"] = r
        pt.close()
    print("HIST " + json.dumps(out))


def main():
    import torch
    from pnraytracing_amd.image import to_display
    out = {"n": N, "unit": "ms", "sizes": {}, "histogram_layouts": {}}
    for W, H in SIZES:
        pt = loaded(W, H)
        stream = torch.cuda.ExternalStream(pt.stream_handle())
        r = {}

        def timed(fn, n=N, warm=5):
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
            return stats(ts)

        for name, kw in (("clamp_linear", {}), ("aces_srgb", {"tone": "aces", "transfer": "srgb", "exposure": 0.6})):
            r[f"display_{name}_events"] = timed(lambda: pt.display(**kw))
            r[f"display_{name}_blend_class"] = blend_class(pt, lambda: pt.display(**kw))
        # the two ways to a host-visible 8-bit image, alternating
        a, b = [], []
        for rep in range(3):
            a.append(host_timed(lambda: (pt.display(), pt.read_display()), n=N // 2))
            b.append(host_timed(lambda: to_display(pt.read_accum()), n=N // 2))
        r["host_image_display_read_display"] = {k: statistics.median(x[k] for x in a) for k in a[0]}
        r["host_image_read_accum_to_display"] = {k: statistics.median(x[k] for x in b) for k in b[0]}
        r["host_image_read_accum_alone"] = host_timed(pt.read_accum, n=N // 2)
        r["host_image_ratio_parent_over_this"] = (r["host_image_read_accum_to_display"]["median"]
                                                  / r["host_image_display_read_display"]["median"])
        assert (pt.read_display()[..., :3] == to_display(pt.read_accum())).all()
        r["bytes_copied"] = {"display": W * H * 4, "accum": W * H * 16}
        out["sizes"][f"{W}x{H}"] = r
        print(W, H, json.dumps(r), flush=True)
        if (W, H) == (512, 512):
            # D2: one frame per call, synchronised, with a displayed image per frame
            d2 = {}
            frames = 200

            def loop(show):
                pt.reset_accum()
                ts = []
                for f in range(frames):
                    t = time.perf_counter()
                    pt.render(f, 1)
                    show()
                    ts.append((time.perf_counter() - t) * 1e3)
                return stats(ts[20:])
            for rep in range(2):
                for name, show in (("no_image", pt.synchronize), ("display_read_display", lambda: (pt.display(), pt.read_display())),
                                   ("read_accum_to_display", lambda: to_display(pt.read_accum()))):
                    d2.setdefault(name, []).append(loop(show))
            out["d2_512x512_ms_per_frame"] = {k: {m: statistics.median(x[m] for x in v) for m in v[0]} for k, v in d2.items()}
            print("D2", json.dumps(out["d2_512x512_ms_per_frame"]), flush=True)
        pt.close()
    # the histogram's two LDS layouts, each in child processes of its own, alternating
    layouts = {"per_block(built)": None, "per_wave(variant)": VARIANT}
    if not os.path.exists(VARIANT):
        print("no variant library: run --build-variant first", file=sys.stderr)
        layouts.pop("per_wave(variant)")
    for rep in range(2):
        for name, lib in layouts.items():
            env = dict(os.environ)
            if lib:
                env["PNRT_DEVICE_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--hist-child"], env=env, capture_output=True, text=True,
                               timeout=300, check=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("HIST ")][0]
            out["histogram_layouts"].setdefault(name, []).append(json.loads(line[5:]))
            print(name, line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    if "--build-variant" in sys.argv:
        build_variant()
    elif "--hist-child" in sys.argv:
        hist_child()
    else:
        main()
