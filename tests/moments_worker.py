"""Child process of tests/test_gpu_moments.py: a context created under the
PNRT_BATCH_BYTES of this process's environment (the cap is read by pnrt_create)
renders frames 0 .. n - 1 of a guides_common scene in one call with the sample
moments enabled, and writes the moments image, then the accumulation image
(float32) to <out>.  Prints "plan <frames_per_batch> <n_batches>".

usage: moments_worker.py <scene> <width> <height> <n_frames> <out>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), HERE]

from guides_common import scene  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402


def main():
    name, w, h, n, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    with PathTracer(0) as pt:
        pt.load(scene(name, w, h))
        pt.enable_moments()
        p = pt.batch_plan(n)
        pt.render(0, n)
        mom, acc = pt.read_moments(), pt.read_accum()
    with open(out, "wb") as f:
        f.write(mom.tobytes())
        f.write(acc.tobytes())
    print(f"plan {p['frames_per_batch']} {p['n_batches']}")


if __name__ == "__main__":
    main()
