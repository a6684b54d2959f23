"""The variance-guided preview from a COMPILED C caller (no Python, no ctypes, no
C++): tests/abi/c_abi_denoise_variance.c includes include/pnrt.h as C, links
libpnrt.so and runs pnrt_enable_moments -> render -> pnrt_denoise_variance ->
pnrt_read_denoised on a "PND1" scene file.  Its images must equal the Python
path's, bit for bit (which tests/test_gpu_denoise_variance.py pins to the
restatement)."""
import os
import subprocess

import numpy as np
import pytest

from guides_common import bits, scene
from pnraytracing_amd import scenes as S
from pnraytracing_amd.tracer import PathTracer

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "abi", "c_abi_denoise_variance")

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("levels,sigmas", [(0, (4.0, 0.25, 0.5)), (3, (1.5, 0.5, 1.5))], ids=["defaults", "levels3"])
def test_compiled_c_caller_denoises_like_python(tmp_path, levels, sigmas):
    assert os.path.exists(EXE), "tests/abi/c_abi_denoise_variance not built (python -c 'import __graft_entry__ as g; g.build()')"
    cfg = scene("c3", 67, 45)
    path, out = str(tmp_path / "s.bin"), str(tmp_path / "out.bin")
    S.export_pnd1(cfg, path)
    r = subprocess.run([EXE, path, "4", str(levels), *(repr(float(v)) for v in sigmas), out], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "expected error:" in r.stdout and "never enabled" in r.stdout             # a code and a message, no exit()
    got = np.fromfile(out, np.float32).reshape(2, cfg.height, cfg.width, 4)
    with PathTracer(0) as pt:
        pt.load(cfg)
        pt.enable_moments()
        for k in range(4):
            pt.render(k, 1)
        pt.render_guides()
        if levels:
            pt.denoise_variance(levels, *sigmas)
        else:
            pt.denoise_variance()
        want, mom = pt.read_denoised(), pt.read_moments()
    bad = int(np.count_nonzero(np.any(bits(got[0]) != bits(want), axis=-1)))
    assert bad == 0, f"{bad} pixels of the denoised image differ"
    assert np.array_equal(bits(got[1]), bits(mom))
