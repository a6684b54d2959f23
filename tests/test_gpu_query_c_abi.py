"""Ray queries from a COMPILED C caller (no Python, no ctypes, no C++):
tests/abi/c_abi_query.c includes include/pnrt.h as C, links libpnrt.so, uploads a
"PND1" scene file and calls pnrt_query_rays once per kind on a ray file.  Its records
must equal the Python path's (which tests/test_gpu_query.py pins to the oracle)."""
import os
import subprocess

import numpy as np
import pytest

import isect_rays
from guides_common import scene
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_query")

pytestmark = pytest.mark.gpu


def test_compiled_c_caller_queries_like_python(tmp_path):
    assert os.path.exists(EXE), "tests/abi/c_abi_query not built (python -c 'import __graft_entry__ as g; g.build()')"
    cfg = scene("c3", 67, 45)
    rays = np.concatenate([isect_rays.make_rays(cfg.packed, cfg.camera, fam, 300, 9) for fam in isect_rays.FAMILIES])
    path, rpath, out = str(tmp_path / "s.bin"), str(tmp_path / "rays.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    rays.tofile(rpath)
    r = subprocess.run([EXE, path, rpath, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "expected error:" in r.stdout and "upload_scene first" in r.stdout      # a code and a message, no exit()
    got = np.fromfile(out, np.uint32).reshape(2, len(rays), 16)
    with PathTracer(0) as pt:
        pt.upload_scene(cfg.packed)
        want = np.stack([pt.query_rays(rays), pt.query_rays(rays, any_hit=True)])
    assert np.array_equal(got, want)
    assert 0 < (got[0, :, 0] != 0).sum() < len(rays)
    assert f"{len(rays)} rays: {int(got[0, :, 0].sum())} closest hits, {int(got[1, :, 0].sum())} occluded" in r.stdout
