"""The sample moments and the convergence statistics from a COMPILED C caller (no
Python, no ctypes, no C++): tests/abi/c_abi_convergence.c includes include/pnrt.h
as C, links libpnrt.so and runs pnrt_enable_moments -> render -> pnrt_convergence
-> pnrt_read_moments on a "PND1" scene file.  Its moments image and its 48-byte
statistics record must equal the Python path's (which tests/test_gpu_moments.py
pins to the restatement)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from guides_common import bits, scene
from pnraytracing_amd import _native as N
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import CONVERGENCE_FIELDS, PathTracer

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_convergence")

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("selector", [(1, 1, 0), (8, 2, 1)], ids=["full", "shard1of2"])
def test_compiled_c_caller_measures_like_python(tmp_path, selector):
    assert os.path.exists(EXE), "tests/abi/c_abi_convergence not built (python -c 'import __graft_entry__ as g; g.build()')"
    cfg = scene("c3", 67, 45)
    path, out = str(tmp_path / "s.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    r = subprocess.run([EXE, path, "6", "0.25", *map(str, selector), out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "expected error:" in r.stdout and "enable_moments first" in r.stdout      # a code and a message, no exit()
    raw = open(out, "rb").read()
    n = cfg.height * cfg.width * 16
    assert len(raw) == n + 48
    got = np.frombuffer(raw[:n], np.float32).reshape(cfg.height, cfg.width, 4)
    st = N.ConvergenceStats.from_buffer_copy(raw[n:])
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        for k in range(6):
            pt.render(k, 1)
        want, stats = pt.read_moments(), pt.convergence(0.25, *selector)
    assert np.array_equal(bits(got), bits(want))
    assert {f: getattr(st, f) for f in CONVERGENCE_FIELDS} == {f: stats[f] for f in CONVERGENCE_FIELDS}
    assert st.reserved == 0 and 0 < st.n_above < st.n_measured == st.n_pixels
    assert ctypes.sizeof(st) == 48
