"""Child process of tests/test_gpu_rays_adaptive.py: pnrt_render_rays_adaptive on the library
PNRT_DEVICE_LIB names -- the `bounds` diagnostic library, which checks every fetch and store
index of the integrator kernels against its array and reports a violation as PNRT_E_TRACE (the
reads below raise it: no fault word is set when they return).  The ray buffer comes from the HIP
runtime (no torch in this process).  The pnrt_set_frame camera's rays against
pnrt_render_adaptive; no-ray records in active pixels; a capped context's three batches; a
shard.  Prints one "case <name>: ok" line per case and exits non-zero on the first difference
or error."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), HERE]

import numpy as np  # noqa: E402

import adaptive_ref as A  # noqa: E402
import test_gpu_cameras as T  # noqa: E402  (its scenes and helpers; nothing runs on import)
from rays_worker import device_buffer, poke  # noqa: E402
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

F = np.float32


def blank_tile(buf, cfg, stride):
    """No-ray records (zeros) over tile 1 -- rows 0..7, columns 8..15 -- of sets 0..3 (the one set when stride is 0):
    colour 0 in every frame, so the tile has converged whatever the threshold."""
    from pnraytracing_amd import build
    hip = ctypes.CDLL(os.path.join(build.ROCM, "lib", "libamdhip64.so"))
    for k in range(1 if stride == 0 else 4):
        for y in range(8):
            at = buf + 32 * (k * stride + y * cfg.width + 8)
            assert hip.hipMemset(ctypes.c_void_p(at), 0, ctypes.c_size_t(8 * 32)) == 0


def start(pt, cfg, rays, stride):
    """Frames 0..3 of `rays` (blank_tile applied) with the moments on -> (the median threshold, accumulation,
    moments, active mask)."""
    T.load(pt, cfg)
    pt.enable_moments(True)
    pt.render_rays(0, 4, rays, stride)
    thr = float(F(np.median(pt.read_error())))
    acc, mom = pt.read_accum(), pt.read_moments()
    mask = A.active(mom, thr, 2)
    assert 0 < mask.sum() < mask.size
    return thr, acc, mom, mask


def main():
    with PathTracer(0) as pt:
        print(pt.version())
        buf = device_buffer(10 * (67 * 45 + 11))             # the largest buffer below; the process's end frees it
        # the pnrt_set_frame camera's rays: pnrt_render_adaptive's images and statistics
        cfg = T.scene("c1", 67, 45)
        T.load(pt, cfg)
        rays = pt.make_rays("pinhole", cfg.camera, out=buf)
        pt.synchronize()
        blank_tile(buf, cfg, 0)                              # (the adaptive calls never render that tile)
        thr, _, _, _ = start(pt, cfg, rays, 0)
        st = pt.render_rays_adaptive(4, 6, rays, 0, thr, 2)
        acc, mom = pt.read_accum(), pt.read_moments()
        start(pt, cfg, rays, 0)
        assert pt.render_adaptive(4, 6, thr, 2) == st and 0 < st["n_active_tiles"] < st["n_tiles"]
        T.same(pt.read_accum(), acc, "pinhole rays vs pnrt_render_adaptive: accumulation")
        T.same(pt.read_moments(), mom, "pinhole rays vs pnrt_render_adaptive: moments")
        print("case pinhole rays are pnrt_render_adaptive: ok")
        # no-ray records in active pixels of the call's set (set 1; the state's frames read set 0)
        cfg = T.scene("c1", 37, 19)
        pix = 37 * 19
        T.load(pt, cfg)
        rays = pt.make_rays("pinhole", cfg.camera, 0, 2, pix, out=buf)
        pt.synchronize()
        blank_tile(buf, cfg, 0)
        thr, acc0, mom0, mask = start(pt, cfg, rays, 0)
        st = pt.render_rays_adaptive(4, 3, rays + 32 * pix, 0, thr, 2)
        acc, mom = pt.read_accum(), pt.read_moments()
        where = np.argwhere(mask)
        spots = [tuple(int(v) for v in where[i]) for i in (0, len(where) // 2, len(where) - 1)]
        for (y, x), (word, value) in zip(spots, ((1, np.nan), (6, np.inf), (0, -np.inf))):
            poke(buf, pix + y * 37 + x, word, value)
        start(pt, cfg, rays, 0)
        assert pt.render_rays_adaptive(4, 3, rays + 32 * pix, 0, thr, 2) == st
        acc2, mom2 = pt.read_accum(), pt.read_moments()
        black = np.zeros((19, 37), bool)
        for y, x in spots:
            black[y, x] = True
        zacc, zmom, _ = A.render(acc0, mom0, [np.zeros((19, 37, 3), F)] * 3, [4, 5, 6], thr, 2)
        assert np.array_equal(T.bits(acc2[black]), T.bits(zacc[black])) and np.array_equal(T.bits(mom2[black]), T.bits(zmom[black]))
        assert np.array_equal(T.bits(acc2[~black]), T.bits(acc[~black])) and np.array_equal(T.bits(mom2[~black]), T.bits(mom[~black]))
        print("case no-ray records in active pixels: ok")
        # a six-frame call with a set per frame, then the same call in three batches under a cap
        cfg = T.scene("c1", 24, 16)
        pix, stride = 24 * 16, 24 * 16 + 11
        T.load(pt, cfg)
        sets = pt.make_rays("pinhole", cfg.camera, 0, 10, stride, out=buf, aa_width=1.0, lens_radius=0.15, focus_distance=7.0,
                            per_pixel=1)
        pt.synchronize()
        blank_tile(buf, cfg, stride)
        thr, _, _, _ = start(pt, cfg, sets, stride)
        st = pt.render_rays_adaptive(4, 6, sets + 32 * 4 * stride, stride, thr, 2)
        acc, mom = pt.read_accum(), pt.read_moments()
        # (a frame of 8 * tiles x 8 pixels has the call's path slots, colour and record bytes per frame)
        pt.set_frame(8 * st["n_active_tiles"], 8, cfg.camera, cfg.max_depth)
        by2, by3 = (pt.cameras_batch_plan(k)["batch_bytes"] for k in (2, 3))
        with T.capped_tracer((by2 + by3) // 2) as t:
            start(t, cfg, sets, stride)
            st2 = t.render_rays_adaptive(4, 6, sets + 32 * 4 * stride, stride, thr, 2)
            assert (st2["frames_per_batch"], st2["n_batches"]) == (2, 3) and dict(st2, frames_per_batch=6, n_batches=1) == st
            T.same(t.read_accum(), acc, "three batches under a cap: accumulation")
            T.same(t.read_moments(), mom, "three batches under a cap: moments")
        print("case six frames in three batches: ok")
        # a shard's rows (local-row tiles) of the same call
        start(pt, cfg, sets, stride)
        before = pt.read_accum()
        part = pt.render_rays_adaptive(4, 6, sets + 32 * 4 * stride, stride, thr, 2, 3, 2, 1)
        got = pt.read_accum()
        rows = (np.arange(16) // 3) % 2 == 1
        assert 0 < part["n_active_pixels"] <= st["n_active_pixels"] and part["n_tiles"] == 3 * 1
        assert np.array_equal(T.bits(got[rows]), T.bits(acc[rows])) and np.array_equal(T.bits(got[~rows]), T.bits(before[~rows]))
        print("case a shard's rows: ok")
    print("RAYS-ADAPTIVE-WORKER-DONE")


if __name__ == "__main__":
    main()
