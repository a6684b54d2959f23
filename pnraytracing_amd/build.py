"""In-tree build of the native libraries (no JIT cache, nothing installed).

    libpnrt_host.so  g++   csrc/host/pnrt_host.cpp, csrc/pn_glm.h   (host scene library)
    libpnrt.so       hipcc csrc/pnrt_device.hip, gfx950     (device library)
    oracle/liboracle.so    gcc (TEST-ONLY parity oracle; see oracle/)
    oracle/_ref/ref_driver g++ on /root/reference headers (only where present)
    oracle/_ref/shader_driver g++ on the reference's compute shader, translated (only where present)

Floating point: every library is built with -ffp-contract=off and without
fast-math so the HIP kernel, the host library and the oracle evaluate the
same IEEE binary32 operation sequences (bit-exact parity).
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
INC = os.path.join(REPO, "include")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("PNRT_OFFLOAD_ARCH", "gfx950")
ROCM = "/opt/rocm"             # headers and libraries of the HIP runtime and RCCL, for the callers that use them

DEVICE_SRCS = ["pnrt_device.hip"]
DEVICE_DEPS = ["pnrt_device.hip", "pt_diag.h", "pt_common.h", "pt_kernel.h", "pt_shade.h", "pt_path.h", "pt_passes.h", "pt_wf.h",
               "pt_env.h", "pt_bvh.h", "pt_guides.h", "pt_denoise.h", "pt_moments.h", "pt_adaptive.h", "pt_query.h", "pn_math.h",
               "sobol_v.inc", "pt_denoise_var.h", "pt_reproject.h", "pt_display.h", "pt_refit.h", "pt_cameras.h", "pt_rays.h",
               "pt_reproject_view.h", "pt_place.h", "pn_glm.h"]


def _run(cmd, cwd=None):
    print("+", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True, cwd=cwd)


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_host(force=False):
    out = os.path.join(PKG, "libpnrt_host.so")
    src = os.path.join(CSRC, "host", "pnrt_host.cpp")
    if force or _stale(out, [src, os.path.join(CSRC, "pn_glm.h"), os.path.join(INC, "pnrt_host.h")]):
        _run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
              "-Wall", "-I", INC, src, "-o", out])
    return out


def device_source_hash() -> str:
    """sha256 (16 hex) of the device library's sources, stamped into
    pnrt_version() so a stale prebuilt libpnrt.so is detectable."""
    h = hashlib.sha256()
    for d in [os.path.join(CSRC, d) for d in DEVICE_DEPS] + [os.path.join(INC, "pnrt.h")]:
        h.update(os.path.basename(d).encode())
        h.update(open(d, "rb").read())
    return h.hexdigest()[:16]


# Every device compile -- the product, the diagnostic variants, the tools' listings and the
# tests' switch builds -- takes these flags, so that all of them vouch for the product's code.
# No SLP packing into v_pk_*_f32: the register pairs it needs cost the trace kernel a wave
# per SIMD and the setup kernels one.
DEVICE_FLAGS = ["-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-fno-gpu-rdc", "-fno-slp-vectorize"]


def _device_deps():
    return [os.path.join(CSRC, d) for d in DEVICE_DEPS] + [os.path.join(INC, "pnrt.h")]


def device_cmd(out, extra=(), opt="-O3", src_hash=None):
    """The command line that compiles the device sources into `out`."""
    return [HIPCC, f"--offload-arch={ARCH}", opt, *DEVICE_FLAGS, f'-DPNRT_SRC_HASH="{src_hash or device_source_hash()}"',
            "-I", INC, *extra, *[os.path.join(CSRC, s) for s in DEVICE_SRCS], "-o", out]


def build_device(force=False, extra=()):
    out = os.path.join(PKG, "libpnrt.so")
    if force or extra or _stale(out, _device_deps()):
        _run(device_cmd(out, extra, os.environ.get("PNRT_OPT", "-O3")))
    return out


# Diagnostic device libraries the GPU tests load in a child process (PNRT_DEVICE_LIB):
# never the product library (pnrt_version() says DIAGNOSTIC BUILD).
#   guard1  the trace kernel's block-queue claim gives up after one attempt, so
#           queued rays go untraced: pnrt_* must report PNRT_E_TRACE
#   bounds  every fetch / store index of the integrator kernels checked against its
#           array (pt_diag.h WF_DIAG_BOUNDS): a violation is reported as PNRT_E_TRACE
#   coop    every ray handed to the cooperative finish after a hash-chosen 0..24 lane
#           steps (pt_diag.h WF_DIAG_COOP), with the bounds checks: same images
#   coopsmall  the same with the finishes' limits shrunk (WF_DIAG_COOP_SMALL), so the
#           closest-hit restart (-2) and the one-entry depth-first regime run routinely
DIAG_VARIANTS = {"guard1": ["-DPNRT_DIAG_BUILD", "-DWF_DIAG_GUARD=1"],
                 "bounds": ["-DPNRT_DIAG_BUILD", "-DWF_DIAG_BOUNDS=1"],
                 "coop": ["-DPNRT_DIAG_BUILD", "-DWF_DIAG_COOP=24", "-DWF_DIAG_BOUNDS=1"],
                 "coopsmall": ["-DPNRT_DIAG_BUILD", "-DWF_DIAG_COOP=24", "-DWF_DIAG_COOP_SMALL=1", "-DWF_DIAG_BOUNDS=1"],
                 # the trace census (tools/census.py; moot-ray counts, tests/test_gpu_moot.py)
                 "stats": ["-DPNRT_DIAG_BUILD", "-DWF_PIPES=1", "-DWF_STATS=1"]}


def variant_path(name: str) -> str:
    return os.path.join(PKG, "variants", f"libpnrt_{name}.so")


def build_diag_variants(force=False):
    os.makedirs(os.path.join(PKG, "variants"), exist_ok=True)
    for name, flags in DIAG_VARIANTS.items():
        out = variant_path(name)
        if force or _stale(out, _device_deps()):
            _run(device_cmd(out, flags))


# TEST-ONLY compiled callers of include/pnrt.h (and include/pnrt_host.h), which exercise the
# drop-in boundary without Python: tests/abi/<source> -> tests/abi/<name>, .cpp with g++, .c as
# C11 with gcc.  Each is linked against libpnrt.so and the libraries listed here; one that lists
# -lpnrt_host depends on the host library and its header too.
ABI_CALLERS = {
    "c_abi_render.cpp": ["-lpnrt_host"],     # a render through both libraries (tests/test_gpu_c_abi.py)
    "c_abi_dloop.cpp": [],                   # the reference's render loop (one pnrt_render per frame), for parity and timing
    "c_abi_denoise.c": [],                   # the guide images and the denoised preview (tests/test_gpu_denoise_c_abi.py)
    "c_abi_convergence.c": [],               # the sample moments and the convergence statistics (tests/test_gpu_moments_c_abi.py)
    "c_abi_query.c": [],                     # ray queries, both kinds (tests/test_gpu_query_c_abi.py)
    "c_abi_denoise_variance.c": [],          # the variance-guided preview (tests/test_gpu_denoise_variance_c_abi.py)
    "c_abi_reproject.c": [],                 # temporal reprojection (tests/test_gpu_reproject_c_abi.py)
    "c_abi_reproject_view.c": [],            # reprojection between camera models (tests/test_gpu_reproject_view_c_abi.py)
    "c_abi_display.c": [],                   # the display transform and auto exposure (tests/test_gpu_display_c_abi.py)
    # the multi-GPU caller: one process, one RCCL communicator per device (ncclCommInitAll + ncclGather)
    "c_abi_multigpu.cpp": ["-lpnrt_host", "-lamdhip64", "-lrccl"],
    # an in-place geometry edit: pnrt_update_vertices, pnrt_read_bvh_boxes (tests/test_gpu_refit_c_abi.py)
    "c_abi_refit.c": [],
    # a camera sequence (pnrt_camera_sequence) rendered with pnrt_render_cameras (tests/test_gpu_cameras.py)
    "c_abi_cameras.c": ["-lpnrt_host", "-lm"],
    # a fisheye ray set (pnrt_make_rays) rendered with pnrt_render_rays and pnrt_render_guides_rays (tests/test_gpu_rays_c_abi.py)
    "c_abi_rays.c": ["-lamdhip64"],
    # pnrt_render_rays(0, 4), then pnrt_render_rays_adaptive over fisheye sets (tests/test_gpu_rays_adaptive_c_abi.py)
    "c_abi_rays_adaptive.c": ["-lamdhip64"],
    # a model defined and placed by a matrix: pnrt_define_model, pnrt_place_models, pnrt_read_vertices (tests/test_gpu_place_c_abi.py)
    "c_abi_place.c": [],
}


def _abi_caller(source, force):
    """Compile one caller where it is stale; None when its source, a header or a library is missing."""
    libs = ABI_CALLERS[source]
    src = os.path.join(REPO, "tests", "abi", source)
    out = os.path.splitext(src)[0]
    deps = [src, os.path.join(INC, "pnrt.h"), os.path.join(PKG, "libpnrt.so")]
    if "-lpnrt_host" in libs:
        deps += [os.path.join(INC, "pnrt_host.h"), os.path.join(PKG, "libpnrt_host.so")]
    if not all(os.path.exists(d) for d in deps):
        return None
    if force or _stale(out, deps):
        cc = ["g++", "-std=c++17"] if source.endswith(".cpp") else ["gcc", "-std=c11"]
        hip = "-lamdhip64" in libs           # the caller uses the HIP runtime itself: ROCm's headers and libraries

        def rocm(*args):
            return list(args) if hip else []
        _run([*cc, "-O2", "-Wall", *rocm("-D__HIP_PLATFORM_AMD__"), "-I", INC, *rocm("-I", f"{ROCM}/include"), src, "-o", out,
              "-L", PKG, *rocm("-L", f"{ROCM}/lib"), "-lpnrt", *libs, "-Wl,-rpath,$ORIGIN/../../pnraytracing_amd",
              *rocm(f"-Wl,-rpath,{ROCM}/lib"), f"-Wl,-rpath-link,{ROCM}/lib"])
    return out


def build_abi_caller(force=False):
    """tests/abi/c_abi_render and the callers that came with it (every ABI_CALLERS entry but those below);
    None, and nothing built, without c_abi_render's source, both headers and both libraries."""
    need = [os.path.join(REPO, "tests", "abi", "c_abi_render.cpp"), os.path.join(INC, "pnrt.h"), os.path.join(INC, "pnrt_host.h"),
            os.path.join(PKG, "libpnrt.so"), os.path.join(PKG, "libpnrt_host.so")]
    if not all(os.path.exists(d) for d in need):
        return None
    outs = [_abi_caller(source, force) for source in ABI_CALLERS if source not in ("c_abi_refit.c", "c_abi_cameras.c", "c_abi_rays.c", "c_abi_rays_adaptive.c", "c_abi_place.c")]
    return outs[0]


def build_refit_abi_caller(force=False):
    return _abi_caller("c_abi_refit.c", force)


def build_cameras_abi_caller(force=False):
    return _abi_caller("c_abi_cameras.c", force)


def build_rays_abi_caller(force=False):
    return _abi_caller("c_abi_rays.c", force)


def build_rays_adaptive_abi_caller(force=False):
    return _abi_caller("c_abi_rays_adaptive.c", force)


def build_place_abi_caller(force=False):
    return _abi_caller("c_abi_place.c", force)


def build_oracle(force=False):
    odir = os.path.join(REPO, "oracle")
    _run(["make", "-s", "-C", odir] + (["-B"] if force else []))
    ref = os.environ.get("PNRT_REFERENCE", "/root/reference")
    if os.path.isdir(os.path.join(ref, "include")):
        _run(["make", "-s", "-C", os.path.join(odir, "ref"), f"REF={ref}"] + (["-B"] if force else []))
    # the reference's compute shader, translated to C++ where it lies: oracle/_ref/shader_driver
    if os.path.isfile(os.path.join(ref, "shaders", "ray_tracing.comp")):
        _run(["make", "-s", "-C", os.path.join(odir, "shader"), f"REF={ref}", f"PYTHON={sys.executable}"] + (["-B"] if force else []))


def build_all(force=False):
    build_host(force)
    build_device(force)
    build_diag_variants(force)
    build_abi_caller(force)
    build_refit_abi_caller(force)
    build_cameras_abi_caller(force)
    build_rays_abi_caller(force)
    build_rays_adaptive_abi_caller(force)
    build_place_abi_caller(force)
    build_oracle(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
