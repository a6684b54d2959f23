"""Every compile-time switch that survives in the device sources still compiles
for gfx950 (VERDICT r3 "Next" 6: switches only tools/ use must not rot
unseen).  Device-only compiles (hipcc --cuda-device-only -c), in parallel; the
product library itself is built by the session fixture.

  stats / timing   the trace census and drain-timing builds (tools/census.py,
                   tools/trace_stats.py, tools/ws_probe.py)
  guard1 / bounds  build.py DIAG_VARIANTS (tests/test_gpu_fault.py)
  pipes1           one call in flight (the census build's -DWF_PIPES=1)
  tunables         trace block 128 / 512, LDS stack depth 12, refill threshold,
                   grid caps, frames per batch, call staggering off / other points
  dn_cached        both denoisers with every level's taps through the caches
"""
import concurrent.futures
import os
import subprocess

import pytest

from pnraytracing_amd import build

VARIANTS = {
    "stats": ["-DPNRT_DIAG_BUILD", "-DWF_PIPES=1", "-DWF_STATS=1"],
    "timing": ["-DPNRT_DIAG_BUILD", "-DWF_TIMING=1"],
    "coopstat": ["-DPNRT_DIAG_BUILD", "-DWF_DIAG_COOPSTAT=1"],
    "guard1": build.DIAG_VARIANTS["guard1"],
    "bounds": build.DIAG_VARIANTS["bounds"],
    "pipes1": ["-DWF_PIPES=1"],
    "block128": ["-DWF_TRACE_BLOCK=128"],
    "block512": ["-DWF_TRACE_BLOCK=512", "-DWF_TRACE_WAVES=4"],
    "stack12": ["-DWF_STACK=12"],
    "tunables": ["-DWF_REFILL_PCT=50", "-DWF_TRACE_GRID_PCT=40", "-DWF_TRACE_GRID_PCT_LARGE=90",
                 "-DWF_MAX_CHUNK_FRAMES=8", "-DWF_QSHARDS=8", "-DWF_KIND_ORDER=0x012"],
    "nostagger": ["-DWF_STAGGER=0"],
    "stagger": ["-DWF_STAGGER=5", "-DWF_STAGGER_PATHS=4000000", "-DWF_TRACE_GRID_PCT_ONE=90"],
    "dn_cached": ["-DDN_LDS_MAX_STEP=0"],
}


def _compile(name, flags, out_dir):
    # build.py's device recipe (its -fPIC -shared are unused here), device code only
    cmd = build.device_cmd(os.path.join(out_dir, f"{name}.o"), ["--cuda-device-only", "-c", *flags], src_hash="switch")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return name, r.returncode, r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(build.HIPCC), reason="hipcc not installed")
def test_every_switch_compiles(tmp_path):
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        res = list(ex.map(lambda kv: _compile(kv[0], kv[1], str(tmp_path)), VARIANTS.items()))
    bad = [(n, err) for n, rc, err in res if rc != 0]
    assert not bad, "\n".join(f"{n}: {e}" for n, e in bad)


def test_result_changing_switches_need_the_diag_flag(tmp_path):
    """A fault-injection switch without -DPNRT_DIAG_BUILD is a compile error, so
    it can never end up in libpnrt.so."""
    if not os.path.exists(build.HIPCC):
        pytest.skip("hipcc not installed")
    name, rc, err = _compile("guard_nodiag", ["-DWF_DIAG_GUARD=1"], str(tmp_path))
    assert rc != 0 and "PNRT_DIAG_BUILD" in err
