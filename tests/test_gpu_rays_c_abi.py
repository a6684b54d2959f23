"""tests/abi/c_abi_rays -- a C11 caller of pnrt_make_rays, pnrt_render_rays and
pnrt_render_guides_rays -- against the Python path: the same accumulation, rays and guide
image, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import test_gpu_cameras as T          # its scenes and helpers; nothing runs on import
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_rays")
F = np.float32


def test_compiled_c_caller_renders_like_python(tmp_path):
    assert os.path.exists(EXE), "tests/abi/c_abi_rays not built (python -c 'import __graft_entry__ as g; g.build()')"
    src = open(os.path.join(HERE, "abi", "c_abi_rays.c")).read()
    assert "_Static_assert(sizeof(pnrt_ray) == 32" in src and "_Static_assert(sizeof(pnrt_ray_camera) == 76" in src
    W, Hh = 40, 24
    cfg = T.scene("c2", W, Hh)
    path, out = str(tmp_path / "s.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    r = subprocess.run([EXE, path, "3", "5", "3", "200.0", "1.0", "1", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("expected error:") == 5 and "reserved" in r.stdout and "aligned" in r.stdout
    got = np.fromfile(out, F)
    pix = W * Hh
    assert got.size == pix * 16
    acc, set0, nrm = got[:pix * 4].reshape(Hh, W, 4), got[pix * 4:pix * 12].reshape(pix, 8), got[pix * 12:].reshape(Hh, W, 4)
    with PathTracer(0) as pt:
        T.load(pt, cfg)
        sets = pt.make_rays("fisheye", cfg.camera, 3, 5, pix + 3, fov_deg=200.0, aa_width=1.0, per_pixel=1)
        pt.render_rays(3, 5, sets, pix + 3)
        T.same(acc, pt.read_accum(), "the C caller's image")
        assert np.array_equal(T.bits(set0), T.bits(sets.cpu().numpy()[:pix]))
        pt.render_guides_rays(sets)
        T.same(nrm, pt.read_aov("normal"), "the C caller's normal image")
    assert acc[..., :3].any() and not set0[:, 3].any()
