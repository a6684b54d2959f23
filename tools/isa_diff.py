#!/usr/bin/env python3
"""Compare the per-kernel instruction streams of two device-assembly files
(hipcc --cuda-device-only -S), e.g. before and after a source refactor that
must not change the product kernels:

    tools/isa_diff.py old.s new.s [name-map old=new ...]

Comments, directives and basic-block label numbers are normalised away; a
kernel whose instruction stream is identical prints "same".  One that differs
prints "REORDERED" when the two streams are the same multiset of instructions
(the same work in another order), "DIFFERENT" otherwise, and then the unified
diff of the two normalised streams, at most DIFF_LINES lines of it.  Kernels
present on one side only are listed.  Exit status 1 when any common kernel
is not "same"."""
import collections
import difflib
import re
import sys

DIFF_LINES = 40


def kernels(lines):
    out, cur, body = {}, None, []
    for line in lines:
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            cur, body = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = body
            cur = None
            continue
        t = line.split(";")[0].strip()
        if not t or t.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", t):
                body.append("LBB:")
            continue
        body.append(re.sub(r"\.LBB\d+_\d+", "LBB", t))
    return out


def compare(a, b, rename=None):
    """The report's lines and the number of common kernels that are not the same."""
    rename = rename or {}
    rep, bad = [], 0
    for k in sorted(a):
        kb = rename.get(k, k)
        if kb not in b:
            rep.append(f"only in old: {k}")
            continue
        if a[k] == b[kb]:
            rep.append(f"same      {len(a[k]):6d} lines  {k[:90]}")
            continue
        bad += 1
        va = sum(1 for x in a[k] if x.startswith("v_"))
        vb = sum(1 for x in b[kb] if x.startswith("v_"))
        word = "REORDERED" if collections.Counter(a[k]) == collections.Counter(b[kb]) else "DIFFERENT"
        rep.append(f"{word} {len(a[k]):6d} -> {len(b[kb]):6d} lines, VALU {va} -> {vb}  {k[:90]}")
        diff = list(difflib.unified_diff(a[k], b[kb], "old", "new", n=1, lineterm=""))
        rep += ["    " + x for x in diff[:DIFF_LINES]]
        if len(diff) > DIFF_LINES:
            rep.append(f"    ... {len(diff) - DIFF_LINES} more diff lines")
    for k in sorted(set(b) - {rename.get(x, x) for x in a}):
        rep.append(f"only in new: {k}")
    return rep, bad


def main():
    a, b = kernels(open(sys.argv[1])), kernels(open(sys.argv[2]))
    rep, bad = compare(a, b, dict(x.split("=", 1) for x in sys.argv[3:]))
    print("\n".join(rep))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
