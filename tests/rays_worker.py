"""Child process of tests/test_gpu_rays.py: caller ray buffers on the library
PNRT_DEVICE_LIB names -- the `bounds` diagnostic library, which checks every fetch and
store index of the integrator kernels against its array and reports a violation as
PNRT_E_TRACE.  Pinhole rays against the oracle, bit for bit; a fisheye set per frame (no-ray
records, a gap between the sets) and its guide images for the error alone; hand-made NaN and
infinite records; a capped context's three batches.  Prints one
"case <name> mode <m>: ok" line per case and exits non-zero on the first difference or error."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"), HERE]

import numpy as np  # noqa: E402

import test_gpu_cameras as T  # noqa: E402  (its scenes and helpers; nothing runs on import)
from pnraytracing_amd.tracer import PathTracer  # noqa: E402

F = np.float32


def device_buffer(records):
    """Device memory for `records` ray records from the HIP runtime itself (no torch in this process)."""
    from pnraytracing_amd import build
    hip = ctypes.CDLL(os.path.join(build.ROCM, "lib", "libamdhip64.so"))
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(32 * records)) == 0 and p.value
    return p.value


def poke(buf, record, word, value):
    """Overwrite float `word` of ray record `record` in the device buffer (hipMemcpy, host to device)."""
    from pnraytracing_amd import build
    hip = ctypes.CDLL(os.path.join(build.ROCM, "lib", "libamdhip64.so"))
    v = ctypes.c_float(value)
    assert hip.hipMemcpy(ctypes.c_void_p(buf + 32 * record + 4 * word), ctypes.byref(v), ctypes.c_size_t(4), 1) == 0


def main():
    with PathTracer(0) as pt:
        print(pt.version())
        buf = device_buffer(4 * (48 * 32 + 9))               # the largest buffer below; the process's end frees it
        pt.upload_scene(T.scene("c1", 16, 8).packed)
        D = pt.device_info()["stack_limit"] - 2
        cases = [(T.scene("c1", 37, 19), 5), (T.scene("c2wide", 48, 32), 3), (T.root_leaf_scene(16, 8), 3),
                 (T.leaf200_scene(16, 8), 3), (T.fan_chain_scene(16, 8, D), 3)]
        for cfg, n in cases:
            ref = T.oracle_cameras(cfg, 0, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (n, 1)))
            for mode in T.MODES:
                T.load(pt, cfg, mode)
                rays = pt.make_rays("pinhole", cfg.camera, out=buf)
                pt.render_rays(0, n, rays)
                T.same(pt.read_accum(), ref, f"{cfg.name} x {n} mode {mode}")
                print(f"case {cfg.name} x {n} mode {mode}: ok")
        # hand-made no-ray records among pinhole rays: black there, the oracle's pixels everywhere else
        cfg = T.scene("c1", 37, 19)
        ref = T.oracle_cameras(cfg, 0, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (5, 1)))
        spots = {(2, 5): (1, np.nan), (18, 33): (6, np.inf), (9, 8): (0, -np.inf), (0, 4): (4, np.nan)}   # (y, x): (float, value)
        for mode in T.MODES:
            T.load(pt, cfg, mode)
            rays = pt.make_rays("pinhole", cfg.camera, out=buf)
            pt.synchronize()
            for (y, x), (word, value) in spots.items():
                poke(buf, y * 37 + x, word, value)
            pt.render_rays(0, 5, rays)
            got = pt.read_accum()
            black = np.zeros((19, 37), bool)
            for y, x in spots:
                black[y, x] = True
            assert ref[black][:, :3].any(axis=1).all() and not got[black][:, :3].any()
            T.same(got[~black][None], ref[~black][None], f"{cfg.name} with no-ray records mode {mode}")
            print(f"case {cfg.name} with no-ray records mode {mode}: ok")
        # three batches of a five-frame call with a set per frame (a cap between two and three frames' bytes)
        cfg = T.scene("c1", 16, 8)
        T.load(pt, cfg)
        by2, by3 = (pt.cameras_batch_plan(k)["batch_bytes"] for k in (2, 3))
        ref = T.oracle_cameras(cfg, 0, np.tile(np.asarray(cfg.camera, F).reshape(1, 12), (5, 1)))
        with T.capped_tracer((by2 + by3) // 2) as t:
            for mode in T.MODES:
                T.load(t, cfg, mode)
                assert t.cameras_batch_plan(5)["n_batches"] == 3
                sets = t.make_rays("pinhole", cfg.camera, 0, 5, 16 * 8 + 3, out=buf)
                t.render_rays(0, 5, sets, 16 * 8 + 3)
                t.synchronize()
                T.same(t.read_accum(), ref, f"{cfg.name} x 5 in three batches mode {mode}")
                print(f"case {cfg.name} x 5 in three batches mode {mode}: ok")
        cfg = T.scene("c2wide", 48, 32)
        for mode in T.MODES:
            T.load(pt, cfg, mode)
            pix = 48 * 32
            sets = pt.make_rays("fisheye", cfg.camera, 0, 4, pix + 9, out=buf, fov_deg=220.0, aa_width=1.0, per_pixel=1)
            pt.render_rays(0, 4, sets, pix + 9, 4, 3, 1)          # a shard's rows
            pt.render_rays(0, 4, sets, pix + 9)
            img = pt.read_accum()                                 # (a bounds violation raises here: PNRT_E_TRACE)
            assert np.isfinite(img).all() and img[..., :3].any()
            pt.render_guides_rays(sets)
            assert pt.read_aov("position")[..., 3].any()
            print(f"case fisheye sets mode {mode}: ok")
    print("RAYS-WORKER-DONE")


if __name__ == "__main__":
    main()
