"""A model defined and moved by a matrix from a COMPILED C caller (no Python, no ctypes, no
C++): tests/abi/c_abi_place.c includes include/pnrt.h as C, links libpnrt.so, uploads a
"PND1" scene file, calls pnrt_define_model, pnrt_place_models and pnrt_read_vertices and
prints the hash of the records.  It must equal the hash of the Python path's records
(which tests/test_gpu_place.py pins to the host library and to tests/place_ref.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import place_ref as P
import refit_common as C
from pnraytracing_amd import build
from pnraytracing_amd import host as H
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_place")

pytestmark = pytest.mark.gpu


def fnv1a64(data: bytes) -> int:
    """64-bit FNV-1a, as the caller computes it."""
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_compiled_c_caller_places_like_python(tmp_path):
    build.build_place_abi_caller()
    assert os.path.exists(EXE), "tests/abi/c_abi_place not built (python -c 'import __graft_entry__ as g; g.build()')"
    cfg = C.scene("C1")
    first, rec = C.edit("C1")
    mesh = H.mesh_quad(27.5)
    m = H.model_matrix([H.translate(0, 5.0, 0), H.rotate(180.0, 0, 0, 1), H.scale(0.035)])
    path, ppath = str(tmp_path / "s.bin"), str(tmp_path / "place.bin")
    S.export_pnd1(cfg, path)
    with open(ppath, "wb") as f:
        f.write(np.array([first, len(rec), 1], np.int32).tobytes())
        f.write(np.ascontiguousarray(m, np.float32).tobytes())
        f.write(H.model_records(mesh).tobytes())
    r = subprocess.run([EXE, path, ppath], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "expected error:" in r.stdout and "upload_scene first" in r.stdout and "unknown model 0" in r.stdout
    got = re.search(r"model 0: (\d+) vertices from (\d+) placed, sizeof\(pnrt_placement\) 72, hash ([0-9a-f]{16})", r.stdout)
    assert got, r.stdout
    assert (int(got.group(1)), int(got.group(2))) == (len(rec), first)
    with PathTracer(0) as pt:
        pt.load(cfg)
        mid = pt.define_model(first, H.model_records(mesh))
        pt.place_models([(mid, m)], relight=True)
        verts = pt.read_vertices(first, len(rec))
    assert np.array_equal(P.bits(verts), P.bits(P.words8(rec)))
    assert int(got.group(3), 16) == fnv1a64(verts.tobytes())
