"""tests/abi/c_abi_rays_adaptive -- a C11 caller of pnrt_make_rays, pnrt_render_rays(0, 4) and
pnrt_render_rays_adaptive -- against the Python path: the same statistics, accumulation and
moments, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_cameras as T          # its scenes and helpers; nothing runs on import
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_rays_adaptive")
F = np.float32


def test_compiled_c_caller_renders_like_python(tmp_path):
    assert os.path.exists(EXE), "tests/abi/c_abi_rays_adaptive not built (python -c 'import __graft_entry__ as g; g.build()')"
    src = open(os.path.join(HERE, "abi", "c_abi_rays_adaptive.c")).read()
    assert "_Static_assert(sizeof(pnrt_adaptive_stats) == 40" in src
    W, Hh = 40, 24
    cfg = T.scene("c2", W, Hh)
    pix = W * Hh
    path, out = str(tmp_path / "s.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    with PathTracer(0) as pt:
        T.load(pt, cfg)
        pt.enable_moments(True)
        sets = pt.make_rays("fisheye", cfg.camera, 0, 9, pix + 3, fov_deg=200.0, aa_width=1.0, per_pixel=1)
        pt.render_rays(0, 4, sets, pix + 3)
        thr = float(F(np.median(pt.read_error())))
        st = pt.render_rays_adaptive(4, 5, int(sets.data_ptr()) + 32 * 4 * (pix + 3), pix + 3, thr, 2)
        acc, mom = pt.read_accum(), pt.read_moments()
    assert 0 < st["n_active_pixels"] < pix and st["n_batches"] == 1
    r = subprocess.run([EXE, path, "5", "3", "200.0", "1.0", repr(thr), out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("expected error:") == 5 and "aligned" in r.stdout and "threshold" in r.stdout and "moments" in r.stdout
    got_stats = [int(v) for v in r.stdout.split("stats")[1].split()[:6]]
    assert got_stats == [st[k] for k in ("n_pixels", "n_active_pixels", "n_tiles", "n_active_tiles", "frames_per_batch", "n_batches")]
    got = np.fromfile(out, F)
    assert got.size == pix * 8
    T.same(got[:pix * 4].reshape(Hh, W, 4), acc, "the C caller's accumulation")
    T.same(got[pix * 4:].reshape(Hh, W, 4), mom, "the C caller's moments")
    assert acc[..., :3].any()
