"""Child process of tests/test_gpu_adaptive.py: a context created under the
PNRT_BATCH_BYTES of this process's environment (the cap is read by pnrt_create)
renders frames 0, 1 of a guides_common scene with pnrt_render, then frames
2 .. 2 + n - 1 with one pnrt_render_adaptive call, and writes the moments image, then
the accumulation image (float32) to <out>.  Prints
"plan <frames_per_batch> <n_batches> <n_active_tiles>".

usage: adaptive_worker.py <scene> <width> <height> <n_frames> <threshold> <out>"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), HERE]

from guides_common import scene  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402


def main():
    name, w, h, n, thr, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]), sys.argv[6]
    with PathTracer(0) as pt:
        pt.load(scene(name, w, h))
        pt.enable_moments()
        pt.render(0, 2)
        st = pt.render_adaptive(2, n, thr, 2)
        mom, acc = pt.read_moments(), pt.read_accum()
    with open(out, "wb") as f:
        f.write(mom.tobytes())
        f.write(acc.tobytes())
    print(f"plan {st['frames_per_batch']} {st['n_batches']} {st['n_active_tiles']}")


if __name__ == "__main__":
    main()
