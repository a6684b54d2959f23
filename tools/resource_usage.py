#!/usr/bin/env python3
"""Resource usage of every kernel of the device library, one line each, from the
compiler's -Rpass-analysis=kernel-resource-usage remarks (no GPU needed):

    <kernel> | SGPRs VGPRs AGPRs scratch[B/lane] occupancy[waves/SIMD] SGPR-spills VGPR-spills LDS[B/block]

Kernels are named as the source names them (demangled, arguments dropped; an empty
template argument list is dropped too, so pt_wf_gen_setup<> reads pt_wf_gen_setup),
sorted, so the listings of two trees compare line by line.

usage: tools/resource_usage.py [<repository root>] > listing.txt"""
import os
import re
import subprocess
import sys
import tempfile

KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
        "LDS Size [bytes/block]"]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def short(name):
    name = re.sub(r"^void ", "", name)
    depth, end = 0, len(name)
    for i, ch in enumerate(name):                    # cut at the argument list's parenthesis (outside <...>)
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            end = i
            break
    return name[:end].replace("<>", "")


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from pnraytracing_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = build.device_cmd(os.path.join(tmp, "libpnrt.so"), ["-Rpass-analysis=kernel-resource-usage"], src_hash="listing")
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in err.split("\n"):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            cur = kernels.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    names = demangle(list(kernels))
    print("# kernel | " + " ".join(k.split(" [")[0].replace(" ", "") for k in KEYS))
    for line in sorted(f"{short(names[k])} | " + " ".join(kernels[k][key] for key in KEYS) for k in kernels):
        print(line)


if __name__ == "__main__":
    main()
