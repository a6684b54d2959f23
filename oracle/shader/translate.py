"""oracle/shader/translate.py -- TEST INFRASTRUCTURE: turn the reference's
shaders/ray_tracing.comp, where it lies, into C++ that compiles against
glsl_shim.hpp.  Text surgery only; this script holds patterns, never shader
lines, and its output goes to oracle/_ref/ (git-ignored, never committed).

    python translate.py <ray_tracing.comp> <out.inc>

What it does:
  * comments removed (they are not ASCII),
  * `#version`, `layout(...)` qualifiers and `uniform` stripped; the `layout(...) in;`
    work-group declaration dropped,
  * the `buffer NAME { T x[]; };` block becomes a plain array `T x[N];`,
  * parameter qualifiers: `in T x` -> `T x`, `out|inout T x` -> `T& x`,
  * unsuffixed floating literals get an `f` (GLSL literals are 32-bit), in the
    `#define`s too; the build compiles the result with -Werror=double-promotion,
  * the swizzles `.rgb`, `.rg`, `.xy` become member calls,
  * `main` is renamed `shader_main`,
  * GLSL evaluates call and constructor arguments left to right, C++ does not
    promise that: a vector constructor with more than one side-effecting argument
    is emitted with braces (a braced list IS evaluated left to right); any other
    call or operator expression with more than one such argument stops the
    translation with an error.
"""
from __future__ import annotations

import re
import sys

DEBUG_WORDS = 64
VECTOR_CTORS = ("vec2", "vec3", "vec4", "ivec2", "ivec3")
KEYWORDS = {"if", "for", "while", "return", "switch", "else", "do"}


class TranslateError(Exception):
    pass


def strip_comments(s: str) -> str:
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"//[^\n]*", "", s)


def suffix_literals(s: str) -> tuple[str, int]:
    pat = re.compile(r"(?<![\w.])((?:\d+\.\d*|\.\d+)(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+)(?![\w.])")
    return pat.subn(r"\1f", s)


def match_paren(s: str, i: int) -> int:
    """Index of the parenthesis closing the one at s[i]."""
    depth = 0
    for j in range(i, len(s)):
        if s[j] in "([{":
            depth += 1
        elif s[j] in ")]}":
            depth -= 1
            if depth == 0:
                return j
    raise TranslateError("unbalanced parenthesis")


def split_top(s: str, sep: str = ",") -> list[str]:
    out, depth, cur = [], 0, []
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == sep and depth == 0:
            out.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    out.append("".join(cur))
    return out


def functions(s: str) -> dict[str, tuple[str, str]]:
    """name -> (parameter list, body) of every function definition."""
    out = {}
    for m in re.finditer(r"\b(\w+)\s+(\w+)\s*\(([^()]*)\)\s*\{", s):
        if m.group(1) in KEYWORDS or m.group(2) in KEYWORDS:
            continue
        end = match_paren(s, m.end() - 1)
        out[m.group(2)] = (m.group(3), s[m.end():end])
    return out


def impure_functions(s: str) -> set[str]:
    """Functions with a side effect a caller can observe: an `out`/`inout`
    parameter, a write to a global that is not a uniform, or a call to one."""
    fns = functions(s)
    top = s
    for _, body in fns.values():
        top = top.replace(body, "")
    top = re.sub(r"\bstruct\s+\w+\s*\{[^{}]*\}\s*;", "", top)
    mutable = {m.group(1) for m in re.finditer(r"^\s*(?:uint|int|float|ivec2|ivec3|vec2|vec3)\s+(\w+)\s*;", top, flags=re.M)
               if not re.search(r"\buniform\b[^;\n]*\b" + m.group(1) + r"\s*;", top)}
    impure = set()
    for name, (params, body) in fns.items():
        if re.search(r"\b(out|inout)\b", params):
            impure.add(name)
        for g in mutable:
            if re.search(r"\b" + g + r"\b\s*(=(?!=)|[-+*/^|&]=|\+\+|--)", body) or re.search(r"(\+\+|--)\s*" + g + r"\b", body):
                impure.add(name)
    changed = True
    while changed:
        changed = False
        for name, (_, body) in fns.items():
            if name not in impure and any(re.search(r"\b" + f + r"\s*\(", body) for f in impure):
                impure.add(name)
                changed = True
    return impure


def count_impure(expr: str, impure: set[str]) -> int:
    return sum(len(re.findall(r"\b" + f + r"\s*\(", expr)) for f in impure)


def order_arguments(s: str, impure: set[str]) -> tuple[str, int]:
    """Brace the vector constructors with several side-effecting arguments; fail on
    anything else whose operands C++ may evaluate in another order than GLSL."""
    fixed = 0
    i = 0
    out = []
    call = re.compile(r"\b(\w+)\s*\(")
    while True:
        m = call.search(s, i)
        if not m:
            out.append(s[i:])
            break
        name = m.group(1)
        open_ = m.end() - 1
        close = match_paren(s, open_)
        args = split_top(s[open_ + 1:close])
        n_side = sum(1 for a in args if count_impure(a, impure) > 0)
        is_def = re.match(r"\s*\{", s[close + 1:]) is not None
        if n_side > 1 and name not in KEYWORDS and not is_def:
            if name not in VECTOR_CTORS:
                raise TranslateError(f"call of {name} has {n_side} side-effecting arguments; C++ leaves their order open")
            out.append(s[i:m.start()] + name + "{" + s[open_ + 1:close] + "}")
            fixed += 1
            i = close + 1
            continue
        out.append(s[i:m.end()])
        i = m.end()
    s = "".join(out)
    # operators: a statement (or one declarator of a declaration) may hold two side-effecting
    # calls only when one encloses the other, or when a sequencing operator stands between them
    braced = re.compile(r"\b(?:" + "|".join(VECTOR_CTORS) + r")\s*\{[^{}]*\}")
    for _, body in functions(s).values():
        for stmt in re.split(r"[;{}]", braced.sub("0", body)):          # braced constructors: ordered
            for part in split_top(stmt):
                calls = [m for f in impure for m in re.finditer(r"\b" + f + r"\s*\(", part)]
                spans = sorted((m.start(), match_paren(part, m.end() - 1)) for m in calls)
                for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                    if b0 < a1:
                        continue                                          # nested: inner runs first
                    if not re.search(r"&&|\|\||\?", part[a1:b0]):
                        raise TranslateError(f"two side-effecting calls in one expression: {part.strip()[:60]}")
    return s, fixed


def translate(src: str) -> tuple[str, dict]:
    info = {}
    s = strip_comments(src)
    impure = impure_functions(s)
    info["impure"] = sorted(impure)
    s = re.sub(r"^\s*#version[^\n]*\n", "\n", s, flags=re.M)
    s = re.sub(r"^\s*layout\s*\([^)]*\)\s*in\s*;[^\n]*\n", "\n", s, flags=re.M)
    s, n = re.subn(r"layout\s*\([^)]*\)\s*buffer\s+\w+\s*\{\s*(\w+)\s+(\w+)\s*\[\s*\]\s*;\s*\}\s*;",
                   rf"\1 \2[{DEBUG_WORDS}];", s)
    info["buffer_blocks"] = n
    s = re.sub(r"layout\s*\([^)]*\)\s*", "", s)
    s, info["uniforms"] = re.subn(r"\buniform\s+", "", s)
    s, info["out_params"] = re.subn(r"\b(?:out|inout)\s+(\w+)\s+(\w+)", r"\1& \2", s)
    s, info["in_params"] = re.subn(r"\bin\s+(\w+)\s+(\w+)", r"\1 \2", s)
    s, info["literals"] = suffix_literals(s)
    s, info["swizzles"] = re.subn(r"\.(rgb|rg|xy)\b(?!\s*\()", r".\1()", s)
    s, n = re.subn(r"\bvoid\s+main\s*\(\s*\)", "void shader_main()", s)
    if n != 1:
        raise TranslateError("expected exactly one main()")
    s, info["braced"] = order_arguments(s, impure)
    if re.search(r"[^\x00-\x7f]", s):
        raise TranslateError("non-ASCII text outside comments")
    return s, info


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    src = open(argv[1], encoding="latin-1").read()
    out, info = translate(src)
    with open(argv[2], "w") as f:
        f.write("// generated from the reference's compute shader by oracle/shader/translate.py -- never commit\n")
        f.write(out)
    print("translate:", " ".join(f"{k}={v if not isinstance(v, list) else ','.join(v)}" for k, v in info.items()))
    return 0


if __name__ == "__main__":
    try:
        sys.exit(main(sys.argv))
    except TranslateError as e:
        print("translate.py:", e, file=sys.stderr)
        sys.exit(1)
