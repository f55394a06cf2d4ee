"""The scatter encode (fec_encode_scatter_rs_dev) without a GPU:
  * which bytes a lane stores (csrc/fec_scatter_encode_cut.hpp) into a heap block of exactly the
    symbol length, as a stand-alone program run plain and under AddressSanitizer + UBSan -- the
    sanitized run is the check that no byte before a destination or at or past destination + L is
    written and that a NULL destination is never dereferenced (tests/csrc/scatter_encode_cut_test.cpp);
  * which forms csrc/fec_forms.hpp decides at every packet size (tests/csrc/table_forms_dump.cpp scatter_encode)
    against a table written from DESIGN.md §5b;
  * the call's place in the header, the binding and both libraries, and the trace name.
"""
import re
import subprocess
from pathlib import Path

import pytest

from forms_support import CSRC, DUMP_SRC, ENCODE_POL, MIN_P, REPO, RUNTIME_ROWS, SANITIZE, SHAPES, SIZES, TESTS_CSRC, _build, _run

CUT_SIZES = [16, 17, 260, 1025, 1200, 2100]


# DESIGN.md §5b, "Scatter encode"
def expected_launches(k, r, P, var):
    """The launches of one scatter encode by the table, or None where it is refused: every shape at
    runtime k, passes of up to eight rows, the first owning the XOR row; `direct` is 1 for the
    length-table form."""
    if P < MIN_P:
        return None
    return [f"encode_scatter k=0 r={min(RUNTIME_ROWS, r - row0)} first={int(row0 == 0)} pol={ENCODE_POL} "
            f"direct={int(bool(var))} aux={row0}" for row0 in range(0, r, RUNTIME_ROWS)]


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("scatter_encode_forms")


# ------------------------------------------------------------------------------------------
# The store cut
# ------------------------------------------------------------------------------------------
def _store_cases():
    """How many fall to each case by the rule as the issue and the header state it.  L >= 16: column
    c < ceil(L/16) stores the 16 bytes at min(16c, L - 16) whole, columns with 16c >= L nothing;
    4 <= L < 16: column 0 stores ceil(L/4) dwords at 0, 4, ..., the last shifted back to L - 4;
    1 <= L < 4: column 0 stores L bytes; L = 0 nothing.  Every (P, L) once with a destination and once
    with NULL.  column / columnback / none / null count (P, L, column); dword / dwordback / byte count
    stores."""
    n = dict(column=0, columnback=0, dword=0, dwordback=0, byte=0, none=0, null=0)
    for P in CUT_SIZES:
        cpp = -(-P // 16)
        for L in range(P + 1):
            for c in range(cpp):
                if 16 * c >= L:
                    n["none"] += 2                                           # both runs
                    continue
                n["null"] += 1
                if L >= 16:
                    n["column" if 16 * c + 16 <= L else "columnback"] += 1
                elif L >= 4:
                    back = L % 4 != 0
                    n["dword"] += -(-L // 4) - back
                    n["dwordback"] += back
                else:
                    n["byte"] += L
    return n


def test_store_cut_plain_and_under_sanitizers(work_dir):
    """Every P of the GPU test's sizes, every L in 0..P and every column on a heap block of exactly L
    bytes: after all columns stored their pieces every byte holds its value.  Once plain, once with
    AddressSanitizer and UBSan linked in statically: no report, the same output -- nothing outside
    [destination, destination + L) is written, and the NULL destination is never dereferenced."""
    src = TESTS_CSRC / "scatter_encode_cut_test.cpp"
    plain, err = _run(_build(work_dir, "cut_plain", src, []))
    assert plain[-1] == "ok", (plain, err)
    counts = {ln.split()[0]: int(ln.split()[1]) for ln in plain[:-1]}
    want = _store_cases()
    assert all(v > 0 for v in want.values())                                 # the sweep meets every case
    assert counts == want
    sanitized, err = _run(_build(work_dir, "cut_sanitized", src, SANITIZE))
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


# ------------------------------------------------------------------------------------------
# Which form runs
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump_exe(work_dir):
    return _build(work_dir, "dump_plain", DUMP_SRC, [], [CSRC / "fec_knobs.cpp"])


@pytest.fixture(scope="module")
def dump_lines(dump_exe):
    return _run(dump_exe, "scatter_encode")[0]


def _line(k, r, P, var):
    launches = expected_launches(k, r, P, var)
    return f"encode_scatter var={var} k={k} r={r} P={P} | " + ("refused" if launches is None else " ; ".join(launches))


def test_decided_scatter_encode_forms_equal_the_table(dump_lines):
    """table_encode_form (csrc/fec_forms.hpp) at every size of the ten shapes, without and with a
    length table, against the table above: refused below 16, one launch per 8 rows."""
    want = [_line(k, r, P, var) for k, r in SHAPES for P in SIZES for var in (0, 1)]
    assert len(dump_lines) == 2 * len(SHAPES) * len(SIZES)
    assert dump_lines == want
    assert sum(ln.endswith("refused") for ln in dump_lines) == 2 * len(SHAPES) * (MIN_P - 1)
    two = [ln for ln in dump_lines if ln.count("encode_scatter k=0") == 2]
    assert two and all(" k=12 r=9 " in ln and "r=8 first=1" in ln and "r=1 first=0" in ln and "aux=8" in ln for ln in two)
    assert all(ln.count("encode_scatter k=0") == 1 for ln in dump_lines if " r=9 " not in ln and not ln.endswith("refused"))


def test_compiled_scatter_encode_forms_are_the_tables(dump_exe, dump_lines):
    """The list the launcher's dispatch is expanded from holds exactly the forms the table can ask
    for over every r in 1..63 (k + r <= 64): 1..8 rows as the first pass and as a later one, without
    and with the length table."""
    compiled, _ = _run(dump_exe, "scatter_encode", "--compiled")
    rows, _ = _run(dump_exe, "scatter_encode", "--rows")
    assert rows == [_line(1, r, 1200, var) for r in range(1, 64) for var in (0, 1)]
    asked = {re.sub(r"aux=\d+", "aux=0", launch) for ln in rows + dump_lines if not ln.endswith("refused")
             for launch in ln.split(" | ")[1].split(" ; ")}
    want = {f"encode_scatter k=0 r={n} first={f} pol={ENCODE_POL} direct={v} aux=0"
            for n in range(1, RUNTIME_ROWS + 1) for f in (0, 1) for v in (0, 1)}
    assert len(compiled) == len(want) == 32 and set(compiled) == want
    assert asked == want


def test_scatter_encode_forms_dump_under_sanitizers(work_dir, dump_exe, dump_lines):
    exe = _build(work_dir, "dump_sanitized", DUMP_SRC, SANITIZE, [CSRC / "fec_knobs.cpp"])
    lines, err = _run(exe, "scatter_encode")
    assert lines == dump_lines
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    assert _run(exe, "scatter_encode", "--compiled")[0] == _run(dump_exe, "scatter_encode", "--compiled")[0]
    assert _run(exe, "scatter_encode", "--rows")[0] == _run(dump_exe, "scatter_encode", "--rows")[0]


def test_scatter_encode_launch_ids_equal_the_binding(dump_exe, quicfec_mod):
    """ScatterEncodeLaunchForm (csrc/fec_knobs.hpp) one for one against
    quicfec.SCATTER_ENCODE_LAUNCH_FORMS: by the compiled numbers and by the enum's text; numbered on
    from 25, apart from the four other lists."""
    ids = {int(ln.split()[1]): ln.split()[0] for ln in _run(dump_exe, "scatter_encode", "--ids")[0]}
    assert ids == quicfec_mod.SCATTER_ENCODE_LAUNCH_FORMS == {25: "encode_scatter"}
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class ScatterEncodeLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == quicfec_mod.SCATTER_ENCODE_LAUNCH_FORMS
    others = (set(quicfec_mod.LAUNCH_FORMS) | set(quicfec_mod.GATHER_LAUNCH_FORMS) | set(quicfec_mod.GATHER_VAR_LAUNCH_FORMS) |
              set(quicfec_mod.SCATTER_LAUNCH_FORMS))
    assert not set(quicfec_mod.SCATTER_ENCODE_LAUNCH_FORMS) & others
    assert min(quicfec_mod.SCATTER_ENCODE_LAUNCH_FORMS) == max(others) + 1


# ------------------------------------------------------------------------------------------
# Declarations and exports
# ------------------------------------------------------------------------------------------
def test_header_declares_the_scatter_encode_call():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fec_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fec_encode_scatter_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_packet_addrs,"
                     r"\s*const uint32_t\*\s*d_packet_lens,\s*const uint64_t\*\s*d_dest_addrs,\s*uint64_t num_groups,"
                     r"\s*uint32_t k,\s*uint32_t r,\s*uint32_t packet_size,\s*uint32_t\*\s*d_symbol_len_out,"
                     r"\s*void\*\s*stream\)\s*;", text)


def test_binding_and_both_libraries_have_the_scatter_encode_call(quicfec_mod):
    assert "fec_encode_scatter_rs_dev" in quicfec_mod.HIP_SYMBOLS
    assert callable(quicfec_mod.Context.encode_scatter_dev)
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert "fec_encode_scatter_rs_dev" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = Path(lib).read_bytes()
        for name in quicfec_mod.SCATTER_ENCODE_LAUNCH_FORMS.values():        # the name lives with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    """A NULL context is answered with FEC_ERR_NULL and a message before any device is touched."""
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    table, lens, dests = 0x1000, 0x3000, 0x2000       # never dereferenced: the context is checked first
    assert lib.fec_encode_scatter_rs_dev(None, table, lens, dests, 1, 10, 3, 1200, None, None) == quicfec_mod.FEC_ERR_NULL
    assert "context" in quicfec_mod.last_error(lib)
