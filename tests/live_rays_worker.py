"""Child of tests/test_gpu_live_rays.py: renders on the device library named by
PNRT_DEVICE_LIB (a diagnostic variant: its census goes to stderr, a tripped bounds
check is an error) and compares each image with the oracle's, bit for bit.

    live_rays_worker.py c2     the small C2-like scene (Cornell + mesh + env), 64x64, 4 frames, depth 4
    live_rays_worker.py dark   the Cornell box with every emission zeroed, 64x64, 3 frames, depth 4
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import numpy as np

import pyoracle
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer


def config(name):
    if name == "c2":
        return S.bunny_c2(64, 64, spp=1, nu=24, nv=12, env=True), 4
    if name == "dark":
        cfg = S.cornell_c1(64, 64)
        cfg.packed.materials = cfg.packed.materials.copy()
        cfg.packed.materials[:, 0:3] = 0.0
        return cfg, 3
    raise KeyError(name)


def main():
    cfg, frames = config(sys.argv[1])
    with PathTracer(0) as pt:
        print("LIB", pt.version(), flush=True)
        pt.load(cfg)
        pt.reset_accum()
        pt.render(0, frames)
        got = pt.read_accum()
    ref, _ = pyoracle.Oracle(cfg).render(0, frames)
    bad = int(np.count_nonzero(np.any(got.view(np.uint32) != ref.view(np.uint32), axis=-1)))
    print("DIFFERING", bad, flush=True)


if __name__ == "__main__":
    main()
