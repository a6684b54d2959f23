#!/usr/bin/env python3
"""tools/place_bench.py -- what moving a model costs by its matrix against by its vertices.

For each configuration (C2, C4, C5) the first model -- the bunny stand-in, the teapot,
the 4M-triangle sphere -- is moved by a Cornell-box half-width and back, and the host
clock is taken around the synchronous calls, after 2 warm-up calls, in one process:

  1  pnrt_place_models of that model (72 bytes go up);
  2  pnrt_update_vertices of its vertex range from host records (60 bytes a vertex go up);
  3  pnrt_update_vertices_device of the same records, already in device memory.

The three run the same regather and refit; they differ in how the world-space records
reach the vertex array.  The host and device records of 2 and 3 are the placement's own
(read back from the device), so the three leave the same scene.  Median, minimum and
maximum of --reps repetitions, and the kernel launches of a call.  --only-update times 2
and 3 alone, with records shifted in numpy: what an older checkout of the library, which
lacks 1, can run.  One JSON line per configuration on stdout; --out also writes them to
a file."""
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


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "reps": reps}


def records15(words8):
    """(n, 15) packed records from the (n, 8) the device keeps (tangent and bitangent: zeros, unread)."""
    rec = np.zeros((len(words8), 15), np.float32)
    rec[:, [0, 1, 2, 3, 4, 5, 12, 13]] = words8
    return rec


def run(name, args, pt):
    import torch
    t0 = time.perf_counter()
    cfg = S.CONFIGS[name](env=False) if name != "C4" else S.teapot_c4(env=False)
    mesh, ops = first_model(name)
    nv = len(mesh.positions)
    p = cfg.packed
    print(f"# {name}: {len(p.triangles)} triangles, {len(p.nodes)} nodes, scene ready in {time.perf_counter() - t0:.1f} s",
          file=sys.stderr, flush=True)
    pt.upload_scene(p)
    levels = pt.device_info()["max_depth"]
    refit_launches = 3 + max(levels - 1, 1)            # gather, lights, leaves, the levels
    out = {"config": name, "triangles": len(p.triangles), "vertices": len(p.vertices), "model_vertices": nv, "nodes": len(p.nodes),
           "tree_depth": levels, "launches": {"place_models": 1 + refit_launches, "update_vertices": 1 + refit_launches,
                                              "update_vertices_device": 1 + refit_launches},
           "bytes_up": {"place_models": 72, "update_vertices": 60 * nv, "update_vertices_device": 0}}
    home = np.ascontiguousarray(p.vertices[:nv])
    k = [0]
    if args.only_update:
        away = home.copy()
        away[:, 0] += np.float32(HALF_WIDTH)
    else:
        mats = (H.model_matrix(ops), H.model_matrix([H.translate(HALF_WIDTH, 0, 0)] + ops))
        mid = pt.define_model(0, H.model_records(mesh))

        def place():
            k[0] += 1
            pt.place_models([(mid, mats[k[0] & 1])])       # alternate, so every call moves the model

        out["place_models"] = timed(place, args.reps)
        pt.place_models([(mid, mats[0])])
        out["home_equals_upload"] = bool(np.array_equal(records15(pt.read_vertices(0, nv))[:, :6].view(np.uint32),
                                                        home[:, :6].view(np.uint32)))
        pt.place_models([(mid, mats[1])])
        away = records15(pt.read_vertices(0, nv))
        boxes = pt.read_bvh_boxes(p.nodes)
        print(f"# {name}: placements timed", file=sys.stderr, flush=True)
    both = (home, away)

    def upd():
        k[0] += 1
        pt.update_vertices(0, both[k[0] & 1])

    out["update_vertices"] = timed(upd, args.reps)
    dev = tuple(torch.from_numpy(a).to("cuda") for a in both)
    torch.cuda.synchronize()

    def upd_dev():
        k[0] += 1
        pt.update_vertices_device(0, nv, dev[k[0] & 1].data_ptr())

    out["update_vertices_device"] = timed(upd_dev, args.reps)
    if not args.only_update:
        pt.update_vertices_device(0, nv, dev[1].data_ptr())
        out["boxes_equal_placement"] = bool(np.array_equal(pt.read_bvh_boxes(p.nodes).view(np.uint32), boxes.view(np.uint32)))
    del dev
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--configs", default="C2,C4,C5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-update", action="store_true")
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
