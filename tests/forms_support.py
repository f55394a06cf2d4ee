"""What the four address-table forms tests (test_gather_forms.py, test_gather_var_forms.py,
test_scatter_forms.py, test_scatter_encode_forms.py) share: the paths, the constants of DESIGN.md
§5b "Address-table calls" that their tables are written from, and the build and run of a stand-alone
host program (tests/csrc/table_forms_dump.cpp and the *_test.cpp programs).  A plain module: no
fixtures, no tests.
"""
import os
import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "quic-test_amd" / "csrc"
TESTS_CSRC = Path(__file__).parent / "csrc"
DUMP_SRC = TESTS_CSRC / "table_forms_dump.cpp"
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]

POL_NT_LOAD, POL_NT_STORE, POL_NO_COEF_BRANCH, POL_COMPACT_OUT = 1, 2, 4, 1024
GATHER_POL = POL_NT_LOAD | POL_NT_STORE | POL_COMPACT_OUT    # every table recover
ENCODE_POL = POL_NT_STORE                                    # every table encode
COMPILED_SHAPES = {(10, 3), (10, 2), (10, 1), (4, 2), (20, 5)}
RUNTIME_ROWS = 8                                    # rows per pass: the runtime-k recovers' and the encodes'
SHAPES = [(10, 3), (10, 1), (10, 2), (4, 2), (20, 5), (6, 3), (7, 4), (12, 6), (12, 9), (16, 4)]   # forms_dump's ten
SIZES = list(range(1, 2101)) + [4096, 8192, 9000]
MIN_P = 16


def _build(d, name, src, flags, extra=()):
    exe = d / name
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", str(CSRC), str(src), *map(str, extra),
                    "-o", str(exe)], check=True)
    return exe


def _run(exe, *args):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("QUICFEC_")}
    out = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120, env=clean)
    assert out.returncode == 0, (out.stdout[-500:], out.stderr[-2000:])
    return out.stdout.splitlines(), out.stderr
