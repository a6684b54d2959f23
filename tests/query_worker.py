"""Child process of tests/test_gpu_query.py: ray queries on the library PNRT_DEVICE_LIB
names -- the bounds-checked diagnostic build, where every fetch, store and stack index
of the query kernel goes through PT_CHECK and a violation is reported as PNRT_E_TRACE --
against the oracle, bit for bit.  Prints one "case <name>: ok" line per case and exits
non-zero on the first difference or error.  TEST INFRASTRUCTURE."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), HERE]

import numpy as np  # noqa: E402

import isect_rays  # noqa: E402
import pyoracle  # noqa: E402
from guides_common import camera_rays, scene  # noqa: E402
from pnraytracing_amd.tracer import TRAVERSE_EXACT, TRAVERSE_ZCULL, PathTracer  # noqa: E402


def cases():
    from test_gpu_limits import FAN_ROT, chain_config, empty_leaf_c1, root_leaf_scene
    yield scene("c3", 67, 45)
    yield root_leaf_scene("coincident130", 9, 8, False)
    yield empty_leaf_c1()[0]
    yield chain_config("leafleft", 0, FAN_ROT)          # the spill area


def main():
    with PathTracer(0) as pt:
        print(pt.version())
        for cfg in cases():
            rays = np.concatenate([camera_rays(cfg)] + [isect_rays.make_rays(cfg.packed, cfg.camera, fam, 333, 13)
                                                        for fam in isect_rays.FAMILIES])
            rays[5, 0], rays[70, 3:6] = np.nan, 0.0     # two invalid rays among them
            ok = np.ones(len(rays), bool)
            ok[[5, 70]] = False
            pt.upload_scene(cfg.packed)
            for mode in (TRAVERSE_ZCULL, TRAVERSE_EXACT):
                pt.set_options(mode)
                for any_hit in (False, True):
                    rec = pt.query_rays(rays, any_hit)            # (raises on PNRT_E_TRACE)
                    ref = pyoracle.Oracle(cfg).intersect(rays[ok], 1 if any_hit else 0, 0)
                    if not np.array_equal(rec[ok, :13], ref) or rec[ok, 14:].any() or not (rec[~ok, 14] == 1).all():
                        print(f"case {cfg.name} mode {mode} any_hit {any_hit}: records differ")
                        return 1
            print(f"case {cfg.name}: ok")
    print("QUERY-WORKER-DONE")
    return 0


if __name__ == "__main__":
    sys.exit(main())
