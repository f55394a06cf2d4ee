#!/usr/bin/env python3
"""Which functions differ between two assembly files (make -C quic-test_amd/csrc asm, on two trees).
Usage: asm_diff.py <a.s> <b.s>

The files are split per function symbol (with the function's .amdhsa_kernel block, its register
and LDS budget), comments are dropped and local labels renumbered in order of appearance, and
the texts are compared.  Prints every function that differs with both line counts and the
demangled name, and how many functions are on one side only.  Exit status 1 if anything differs.
Text only: it knows nothing about particular instructions."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

_FUNC = re.compile(r"^\t\.type\t(\S+),@function\n", re.M)
_FUNC_END = re.compile(r"^\.Lfunc_end\d+:.*\n", re.M)
_LABEL = re.compile(r"\.L[A-Za-z_$]*\d+(?:_\d+)?")


def _normalise(text):
    """Comment-free lines with the local labels numbered in order of first appearance."""
    labels = {}
    lines = []
    for line in text.splitlines():
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        lines.append(_LABEL.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), line))
    return lines


def functions(text):
    """{symbol: normalised lines} of every function of an assembly file."""
    out = {}
    for m in _FUNC.finditer(text):
        name = m.group(1)
        end = _FUNC_END.search(text, m.end())
        body = text[m.end():end.start() if end else len(text)]
        k = re.search(r"^\t\.amdhsa_kernel %s\n.*?^\t\.end_amdhsa_kernel\n" % re.escape(name), text[m.end():], re.M | re.S)
        out[name] = _normalise(body + (k.group(0) if k else ""))
    return out


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return {n: n for n in names}
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True)
    plain = res.stdout.splitlines()
    return dict(zip(names, plain)) if res.returncode == 0 and len(plain) == len(names) else {n: n for n in names}


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    a, b = (functions(Path(p).read_text()) for p in argv[1:])
    both = [n for n in a if n in b]
    differ = [n for n in both if a[n] != b[n]]
    only_a = [n for n in a if n not in b]
    only_b = [n for n in b if n not in a]
    plain = demangle(differ + only_a + only_b)
    for n in differ:
        print(f"differs  {len(a[n]):6d} {len(b[n]):6d}  {plain[n]}")
    for n in only_a:
        print(f"only in {argv[1]}: {plain[n]}")
    for n in only_b:
        print(f"only in {argv[2]}: {plain[n]}")
    print(f"{len(both)} functions on both sides, {len(differ)} differ; {len(only_a)} only in {argv[1]}, "
          f"{len(only_b)} only in {argv[2]}")
    return 1 if differ or only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
