"""Child process of tests/test_gpu_cameras.py: the camera sequence on the library
PNRT_DEVICE_LIB names -- the `bounds` diagnostic library, which checks every fetch and
store index of the integrator kernels against its array and reports a violation as
PNRT_E_TRACE -- against the oracle, bit for bit.  Prints one "case <name> mode <m>: ok"
line per case and exits non-zero on the first difference or error."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), HERE]

import numpy as np  # noqa: E402

import test_gpu_cameras as T  # noqa: E402  (its scenes and helpers; nothing runs on import)
from pnraytracing_amd.tracer import PathTracer  # noqa: E402


def main():
    with PathTracer(0) as pt:
        print(pt.version())
        pt.upload_scene(T.scene("c1", 16, 8).packed)
        D = pt.device_info()["stack_limit"] - 2
        cases = [(T.scene("c1", 37, 19), 5), (T.scene("c2wide", 48, 32), 3), (T.root_leaf_scene(16, 8), 3),
                 (T.leaf200_scene(16, 8), 3), (T.fan_chain_scene(16, 8, D), 3), (T.scene("c1", 16, 8), 130)]
        for cfg, n in cases:
            cams = T.lens_cameras(cfg, 0, n, radius=0.1)
            ref = T.oracle_cameras(cfg, 0, cams)
            for mode in T.MODES:
                T.load(pt, cfg, mode)
                pt.render_cameras(0, cams)
                T.same(pt.read_accum(), ref, f"{cfg.name} x {n} mode {mode}")
                print(f"case {cfg.name} x {n} mode {mode}: ok")
    print("CAMERAS-WORKER-DONE")


if __name__ == "__main__":
    main()
