"""An in-place geometry edit from a COMPILED C caller (no Python, no ctypes, no C++):
tests/abi/c_abi_refit.c includes include/pnrt.h as C, links libpnrt.so, uploads a "PND1"
scene file, calls pnrt_update_vertices with new light areas, reads the boxes back and
renders two frames.  Its bytes must equal the Python path's (which tests/test_gpu_refit.py
pins to the oracle and to the refit rule)."""
import os
import subprocess

import numpy as np
import pytest

import refit_common as C
from pnraytracing_amd import build
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_refit")

pytestmark = pytest.mark.gpu


def test_compiled_c_caller_edits_like_python(tmp_path):
    build.build_refit_abi_caller()
    assert os.path.exists(EXE), "tests/abi/c_abi_refit not built (python -c 'import __graft_entry__ as g; g.build()')"
    cfg = C.scene("C1")
    first, rec = C.edit("C1")
    new = H.refit_packed(cfg.packed, first, rec)
    path, epath, out = str(tmp_path / "s.bin"), str(tmp_path / "edit.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    with open(epath, "wb") as f:
        f.write(np.array([first, len(rec), 1], np.int32).tobytes())
        f.write(np.array([new.lights_sum_area], np.float32).tobytes())
        f.write(np.ascontiguousarray(rec, np.float32).tobytes())
        f.write(np.ascontiguousarray(new.lights, np.float32).tobytes())
    r = subprocess.run([EXE, path, epath, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "expected error:" in r.stdout and "upload_scene first" in r.stdout      # a code and a message, no exit()
    nn = len(cfg.packed.nodes)
    got = np.fromfile(out, np.uint32)
    assert len(got) == nn * 12 + C.W * C.Hh * 4
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.update_vertices(first, rec, lights=new.lights, lights_sum_area=new.lights_sum_area)
        boxes = pt.read_bvh_boxes(cfg.packed.nodes)
        pt.reset_accum()
        pt.render(0, 2)
        img = pt.read_accum()
    assert np.array_equal(got[:nn * 12], boxes.view(np.uint32).reshape(-1))
    assert np.array_equal(boxes.view(np.uint32), new.nodes.view(np.uint32))
    assert np.array_equal(got[nn * 12:], img.view(np.uint32).reshape(-1)) and img[..., :3].any()
    assert f"{len(rec)} vertices from {first} edited" in r.stdout
