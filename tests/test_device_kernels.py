"""The kernels the product build of the device library holds are exactly the listed ones.

The host code decides which instantiations of the kernel templates exist (pnrt_device.hip:
PathSource::with_pack, with_bool), so a dispatch that instantiates a pack nobody launches
costs build time and code size and fails no other test.  A device-only compile with the
product flags; only the names on the `.amdhsa_kernel` lines are read, demangled and sorted.

A kernel added or removed on purpose: update tests/golden/device_kernels.txt with it.
"""
import os
import shutil
import subprocess

import pytest

from pnraytracing_amd import build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_kernels.txt")
CXXFILT = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")


def kernel_names(listing):
    """Sorted demangled names of the kernels in a device assembly listing."""
    with open(listing) as f:
        mangled = [ln.split()[1] for ln in f if ln.strip().startswith(".amdhsa_kernel ")]
    out = subprocess.run([CXXFILT], input="\n".join(mangled) + "\n", capture_output=True, text=True, check=True).stdout
    return sorted(out.splitlines())


@pytest.mark.skipif(not os.path.exists(build.HIPCC), reason="hipcc not installed")
@pytest.mark.skipif(CXXFILT is None, reason="no C++ demangler (c++filt, llvm-cxxfilt) installed")
def test_product_kernel_set(tmp_path):
    listing = str(tmp_path / "product.s")
    cmd = build.device_cmd(listing, ["--cuda-device-only", "-S"], src_hash="same")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(GOLDEN) as f:
        want = [ln.rstrip("\n") for ln in f if ln.strip()]
    have = kernel_names(listing)
    assert len(have) == len(set(have)), "a kernel is emitted twice"
    # (demanglers differ in spacing only)
    squeeze = lambda names: sorted(n.replace(" ", "") for n in names)  # noqa: E731
    assert squeeze(have) == squeeze(want), (
        "kernels not in the list: %s; listed kernels missing: %s" % (sorted(set(have) - set(want)), sorted(set(want) - set(have))))
