"""Temporal reprojection from a COMPILED C caller (no Python, no ctypes, no C++):
tests/abi/c_abi_reproject.c includes include/pnrt.h as C -- with _Static_asserts on both
struct sizes --, links libpnrt.so and runs the anchor sequence, a camera move and one
pnrt_reproject on a "PND1" scene file.  Its statistics and images must equal the Python
path's (which tests/test_gpu_reproject.py pins to the restatement)."""
import os
import subprocess

import numpy as np
import pytest

import reproject_common as C
from guides_common import bits, scene
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_reproject")
W, H = C.W, C.H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("max_history", [0, 3], ids=["defaults", "cap3"])
def test_compiled_c_caller_reprojects_like_python(tmp_path, max_history):
    assert os.path.exists(EXE), "tests/abi/c_abi_reproject not built (python -c 'import __graft_entry__ as g; g.build()')"
    src = open(os.path.join(HERE, "abi", "c_abi_reproject.c")).read()
    assert src.count("_Static_assert(sizeof(pnrt_reproject_") == 2
    name, move = "c3", "translate"
    cfg = scene(name, W, H)
    cam_b = C.camera_b(name, move, W, H)
    path, out = str(tmp_path / "s.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    r = subprocess.run([EXE, path, repr(C.THRESHOLD), str(max_history), out, *(repr(float(v)) for v in cam_b.reshape(-1))],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "expected error:" in r.stdout and "not enabled" in r.stdout               # a code and a message, no exit()
    got_stats = tuple(int(v) for v in r.stdout.split("stats")[1].split()[:6])
    got = np.fromfile(out, np.float32).reshape(2, H, W, 4)
    with PathTracer(0) as pt:
        C.run_state(pt, name, W, H)
        pt.set_frame(W, H, cam_b, cfg.max_depth)
        st = pt.reproject(C.camera_a(name, W, H), max_history=max_history or None)
        acc, mom = pt.read_accum(), pt.read_moments()
    assert got_stats == (st["n_pixels"], *C.stats_tuple(st))
    if not max_history:
        assert got_stats[1:] == C.REPLAY[(name, move)]
    assert np.array_equal(bits(got[0]), bits(acc)) and np.array_equal(bits(got[1]), bits(mom))
