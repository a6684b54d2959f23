"""Reprojection under the camera models from a COMPILED C caller (no Python, no ctypes, no C++):
tests/abi/c_abi_reproject_view.c includes include/pnrt.h as C -- with _Static_asserts on the
struct sizes --, links libpnrt.so and runs the anchor sequence and one pnrt_reproject_view on
a "PND1" scene file.  Its statistics and images must equal the Python path's (which
tests/test_gpu_reproject_view.py pins to the restatement)."""
import os
import subprocess

import numpy as np
import pytest

import reproject_common as C
import reproject_view_common as VC
from guides_common import bits, scene
from pnraytracing_amd import _native as N
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_reproject_view")
W, H = VC.W, VC.Hh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["fisheye-c1-rotate", "pinhole-to-equirect"])
def test_compiled_c_caller_reprojects_like_python(tmp_path, case):
    assert os.path.exists(EXE), "tests/abi/c_abi_reproject_view not built (python -c 'import __graft_entry__ as g; g.build()')"
    src = open(os.path.join(HERE, "abi", "c_abi_reproject_view.c")).read()
    assert src.count("_Static_assert(sizeof(pnrt_") == 3
    name, move = "c1", "rotate"
    # the file's camera is the scene's: both views start there; "pinhole-to-equirect": pinhole into equirect, coarse tolerance
    models, fov, tol = (("fisheye", "fisheye"), VC.FISHEYE_FOV, 0.02) if case == "fisheye-c1-rotate" else (("pinhole", "equirect"), 180.0, 0.13)
    cfg = scene(name, W, H)
    cam_a, cam_b = C.camera_a(name, W, H), C.camera_b(name, move, W, H)
    path, out = str(tmp_path / "s.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    r = subprocess.run([EXE, path, repr(C.THRESHOLD), *(str(N.CAM_MODELS.index(m)) for m in models), repr(fov), repr(tol), out,
                        *(repr(float(v)) for v in cam_b.reshape(-1))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("expected error:") == 2 and "not enabled" in r.stdout and "reproject_view: to:" in r.stdout
    got_stats = tuple(int(v) for v in r.stdout.split("stats")[1].split()[:6])
    got = np.fromfile(out, np.float32).reshape(2, H, W, 4)
    with PathTracer(0) as pt:
        C.run_state(pt, name, W, H)
        st = pt.reproject_view((models[0], cam_a, fov), (models[1], cam_b, fov), position_tolerance=tol)
        acc, mom = pt.read_accum(), pt.read_moments()
    assert got_stats == (st["n_pixels"], *C.stats_tuple(st)) and st["n_reprojected"] >= 30
    if case in VC.TABLE:
        assert got_stats[1:] == VC.TABLE[case]
    assert np.array_equal(bits(got[0]), bits(acc)) and np.array_equal(bits(got[1]), bits(mom))
