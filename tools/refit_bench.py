#!/usr/bin/env python3
"""tools/refit_bench.py -- what an in-place geometry edit costs against a re-upload.

For each configuration (C2, C4, C5) the first model -- the bunny stand-in, the teapot,
the 4M-triangle sphere -- is moved by a Cornell-box half-width, and the host clock is
taken around synchronous calls, after a warm-up, in one process:

  1  pnrt_update_vertices of that model's vertex range, and of the whole vertex array;
  2  what the library offered before for the same edit, at its most favourable: the nodes
     already refit on the host, pnrt_upload_scene of the full arrays alone;
  3  the same with a rebuild: SceneBuilder.build() plus the upload.

Median, minimum and maximum of --reps repetitions (3 is slow at C5: --rebuild-reps).
With --quality (C2): Msamples/s of the moved scene under the REFIT tree against the
same scene REBUILT -- how much traversal quality a refit costs after a large move.
One JSON line per configuration on stdout; --out also writes them to a file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from pnraytracing_amd import host as H          # noqa: E402
from pnraytracing_amd import scenes as S        # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

HALF_WIDTH = 2.75


def first_model(name):
    """(mesh, the configuration's own ops) of the model each configuration adds first."""
    if name == "C2":
        return H.mesh_displaced_sphere(264, 132, S.BUNNY_RADIUS, S.BUNNY_CENTER, 0.12, 0x5EED), [H.translate(0, 0, -2), H.scale(8)]
    if name == "C4":
        return H.mesh_teapot(), [H.scale(0.2)]
    if name == "C5":
        return H.mesh_displaced_sphere(2048, 1024, S.BUNNY_RADIUS, S.BUNNY_CENTER, 0.12, 0x5EED), [H.translate(0, 0, -2), H.scale(8)]
    raise KeyError(name)


def moved_builder(name, mesh, ops):
    """The configuration's SceneBuilder with its first model under `ops`."""
    sb = H.SceneBuilder()
    if name == "C4":
        sb.add_model(mesh, ops, H.Material(baseColor=(0.6, 0.7, 0.2), metallic=0.7, roughness=0.3), "teapot")
        sb.add_model(H.mesh_quad(27.5), [H.scale(1.0)], H.Material(baseColor=(0.73, 0.73, 0.73), metallic=0.2, roughness=0.85), "floor")
        sb.add_model(H.mesh_quad(27.5), [H.translate(1.5, 3.0, 1.0), H.rotate(180.0, 0, 0, 1), H.scale(0.02)],
                     H.Material(baseColor=(0.73, 0.73, 0.73), emssive=(8.0, 8.0, 8.0)), "area_light")
    else:
        m = H.Material(baseColor=(0.65, 0.65, 0.65))
        sb.add_model(mesh, ops, m, "model")
        S._cornell_walls(sb, m)
    return sb


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "reps": reps}


def msamples(pt, cfg, calls=5, frames=16):
    pt.reset_accum()
    pt.render(0, frames)
    pt.synchronize()
    t = []
    for k in range(calls):
        t0 = time.perf_counter()
        pt.render(frames * (k + 1), frames)
        pt.synchronize()
        t.append(time.perf_counter() - t0)
    return round(cfg.width * cfg.height * frames / statistics.median(t) / 1e6, 1)


def run(name, args, pt):
    t0 = time.perf_counter()
    cfg = S.CONFIGS[name](env=False) if name != "C4" else S.teapot_c4(env=False)
    mesh, ops = first_model(name)
    nv = len(mesh.positions)
    ops_moved = [H.translate(HALF_WIDTH, 0, 0)] + ops
    sb = moved_builder(name, mesh, ops_moved)
    rebuilt = sb.build()
    rec = np.ascontiguousarray(rebuilt.vertices[:nv])
    p = cfg.packed
    assert np.array_equal(rebuilt.vertices[nv:], p.vertices[nv:]) and not np.array_equal(rec, p.vertices[:nv])
    refit = H.refit_packed(p, 0, rec)
    print(f"# {name}: {len(p.triangles)} triangles, {len(p.nodes)} nodes, scenes ready in {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)
    pt.upload_scene(p)
    levels = pt.device_info()["max_depth"]
    out = {"config": name, "triangles": len(p.triangles), "vertices": len(p.vertices), "model_vertices": nv, "nodes": len(p.nodes),
           "tree_depth": levels, "launches": 4 + max(levels - 1, 1)}
    both = (np.ascontiguousarray(p.vertices[:nv]), rec)
    whole = (np.ascontiguousarray(p.vertices), np.ascontiguousarray(refit.vertices))
    k = [0]

    def upd(pair):
        k[0] += 1
        pt.update_vertices(0, pair[k[0] & 1])        # alternate, so every call moves the model

    out["update_model"] = timed(lambda: upd(both), args.reps)
    out["update_all"] = timed(lambda: upd(whole), args.reps)
    pt.update_vertices(0, rec)
    got = pt.read_bvh_boxes(p.nodes)
    out["boxes_equal_host_refit"] = bool(np.array_equal(got.view(np.uint32), refit.nodes.view(np.uint32)))
    print(f"# {name}: updates timed", file=sys.stderr, flush=True)
    out["upload_refit_on_host"] = timed(lambda: pt.upload_scene(refit), args.reps)
    print(f"# {name}: uploads timed", file=sys.stderr, flush=True)

    def rebuild():
        pt.upload_scene(sb.build())

    out["rebuild_and_upload"] = timed(rebuild, args.rebuild_reps, warmup=1)
    if args.quality and name == "C2":
        pt.upload_env(None, None)
        pt.set_frame(cfg.width, cfg.height, cfg.camera, cfg.max_depth)
        pt.upload_scene(refit)
        a = msamples(pt, cfg)
        pt.upload_scene(rebuilt)
        b = msamples(pt, cfg)
        pt.upload_scene(p)
        out["msamples_per_s"] = {"refit_tree": a, "rebuilt_tree": b, "unmoved": msamples(pt, cfg), "frame": [cfg.width, cfg.height]}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="C2,C4,C5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    lines = []
    with PathTracer(0) as pt:
        for name in args.configs.split(","):
            lines.append(json.dumps(run(name, args, pt)))
            print(lines[-1], flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
