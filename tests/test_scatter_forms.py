"""The scatter recover (fec_recover_scatter_rs_dev) without a GPU:
  * which bytes a lane stores (csrc/fec_scatter_cut.hpp) into a heap block of exactly the symbol
    length, as a stand-alone program run plain and under AddressSanitizer + UBSan -- the sanitized
    run is the check that no byte before a destination or at or past destination + L is written and
    that a NULL destination is never dereferenced (tests/csrc/scatter_cut_test.cpp);
  * which forms csrc/fec_forms.hpp decides at every packet size (tests/csrc/table_forms_dump.cpp scatter)
    against a table written from DESIGN.md §5b;
  * the call's place in the header, the binding and both libraries, and the trace names.
"""
import re
import subprocess
from pathlib import Path

import pytest

from forms_support import (COMPILED_SHAPES, CSRC, DUMP_SRC, GATHER_POL, MIN_P, POL_NO_COEF_BRANCH, REPO, RUNTIME_ROWS,
                           SANITIZE, SHAPES, SIZES, TESTS_CSRC, _build, _run)

CUT_SIZES = [16, 17, 260, 1025, 1200, 2100]
LANES = 64


# DESIGN.md §5b, "Scatter recover"
def expected_launches(k, r, P, var):
    """The launches of one scatter recover by the table, or None where it is refused.  `first` is 1
    for the length-table form."""
    if P < MIN_P:
        return None
    first = int(bool(var))
    if (k, r) in COMPILED_SHAPES:
        return ["classify_scatter", f"recover_scatter k={k} r={r} first={first} pol={GATHER_POL} aux=0"]
    pol = GATHER_POL | POL_NO_COEF_BRANCH
    return ["classify_scatter"] + [f"recover_scatter k=0 r={RUNTIME_ROWS} first={first} pol={pol} aux={m0}"
                                   for m0 in range(0, r, RUNTIME_ROWS)]


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("scatter_forms")


# ------------------------------------------------------------------------------------------
# The store cut
# ------------------------------------------------------------------------------------------
def _store_cases():
    """How many (P, L, pass, lane) fall to each store case by the header's own statement of the
    walk: L >= 4 whole 1-KiB passes of 16-B pieces, then 256-B passes of 4-B pieces with the tail
    shifted back to end at L; L = 1..3 one byte per lane below L; L = 0 nothing.  Every (P, L) once
    with a destination and once with NULL."""
    n = dict(piece16=0, piece4=0, piece4back=0, byte=0, none=0, null=0)
    for P in CUT_SIZES:
        for L in range(P + 1):
            if L == 0:
                n["none"] += 2 * LANES                                       # both runs: no pass at all
            elif L < 4:
                n["byte"] += L
                n["none"] += LANES - L
                n["null"] += LANES
            else:
                main_end = L & ~1023
                tail = range(main_end, L, 256)
                n["piece16"] += LANES * (main_end // 1024)
                for base in tail:
                    whole = sum(base + 4 * lane + 4 <= L for lane in range(LANES))
                    n["piece4"] += whole
                    n["piece4back"] += LANES - whole
                n["null"] += LANES * (main_end // 1024 + len(tail))
    return n


def test_store_cut_plain_and_under_sanitizers(work_dir):
    """Every P of the GPU test's sizes and every L in 0..P on a heap block of exactly L bytes: after
    all 64 lanes stored their pieces every byte holds its value.  Once plain, once with
    AddressSanitizer and UBSan linked in statically: no report, the same output -- nothing outside
    [destination, destination + L) is written, and the NULL destination is never dereferenced."""
    src = TESTS_CSRC / "scatter_cut_test.cpp"
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
    return _run(dump_exe, "scatter")[0]


def test_decided_scatter_forms_equal_the_table(dump_lines):
    """table_recover_form (csrc/fec_forms.hpp) at every size of the ten shapes, without and with a length
    table, against the table above."""
    want = []
    for k, r in SHAPES:
        for P in SIZES:
            for var in (0, 1):
                launches = expected_launches(k, r, P, var)
                want.append(f"scatter var={var} k={k} r={r} P={P} | " + ("refused" if launches is None else " ; ".join(launches)))
    assert len(dump_lines) == 2 * len(SHAPES) * len(SIZES)
    assert dump_lines == want
    assert sum(ln.endswith("refused") for ln in dump_lines) == 2 * len(SHAPES) * (MIN_P - 1)
    assert any(ln.count("recover_scatter") == 2 for ln in dump_lines)        # k=12 r=9: rows 0..7, then 8


def test_compiled_scatter_forms_are_the_tables(dump_exe, dump_lines):
    """The list the launcher's dispatch is expanded from holds exactly the forms the table can ask
    for: per compiled shape and for runtime k one without and one with the length table."""
    compiled, _ = _run(dump_exe, "scatter", "--compiled")
    want = {f"recover_scatter k={k} r={r} first={v} pol={GATHER_POL} aux=0" for k, r in COMPILED_SHAPES for v in (0, 1)}
    want |= {f"recover_scatter k=0 r={RUNTIME_ROWS} first={v} pol={GATHER_POL | POL_NO_COEF_BRANCH} aux=0" for v in (0, 1)}
    assert len(compiled) == len(want) == 12 and set(compiled) == want
    asked = {re.sub(r"aux=\d+", "aux=0", launch) for ln in dump_lines if not ln.endswith("refused")
             for launch in ln.split(" | ")[1].split(" ; ")[1:]}
    assert asked == want


def test_scatter_forms_dump_under_sanitizers(work_dir, dump_exe, dump_lines):
    exe = _build(work_dir, "dump_sanitized", DUMP_SRC, SANITIZE, [CSRC / "fec_knobs.cpp"])
    lines, err = _run(exe, "scatter")
    assert lines == dump_lines
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


def test_scatter_launch_ids_equal_the_binding(dump_exe, quicfec_mod):
    """ScatterLaunchForm (csrc/fec_knobs.hpp) one for one against quicfec.SCATTER_LAUNCH_FORMS: by
    the compiled numbers and by the enum's text; numbered on from 23, apart from the other lists."""
    ids = {int(ln.split()[1]): ln.split()[0] for ln in _run(dump_exe, "scatter", "--ids")[0]}
    assert ids == quicfec_mod.SCATTER_LAUNCH_FORMS == {23: "classify_scatter", 24: "recover_scatter"}
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class ScatterLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == quicfec_mod.SCATTER_LAUNCH_FORMS
    others = set(quicfec_mod.LAUNCH_FORMS) | set(quicfec_mod.GATHER_LAUNCH_FORMS) | set(quicfec_mod.GATHER_VAR_LAUNCH_FORMS)
    assert not set(quicfec_mod.SCATTER_LAUNCH_FORMS) & others and min(quicfec_mod.SCATTER_LAUNCH_FORMS) == max(others) + 1


# ------------------------------------------------------------------------------------------
# Declarations and exports
# ------------------------------------------------------------------------------------------
def test_header_declares_the_scatter_call():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fec_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fec_recover_scatter_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_shard_addrs,"
                     r"\s*const uint32_t\*\s*d_shard_lens,\s*const uint64_t\*\s*d_dest_addrs,\s*uint64_t num_groups,"
                     r"\s*uint32_t k,\s*uint32_t r,\s*uint32_t packet_size,\s*uint8_t\*\s*d_status,"
                     r"\s*uint64_t\*\s*d_masks_out,\s*uint32_t\*\s*d_symbol_len_out,\s*void\*\s*stream\)\s*;", text)


def test_binding_and_both_libraries_have_the_scatter_call(quicfec_mod):
    assert "fec_recover_scatter_rs_dev" in quicfec_mod.HIP_SYMBOLS
    assert callable(quicfec_mod.Context.recover_scatter_dev)
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert "fec_recover_scatter_rs_dev" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = Path(lib).read_bytes()
        for name in quicfec_mod.SCATTER_LAUNCH_FORMS.values():               # names live with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    """A NULL context is answered with FEC_ERR_NULL and a message before any device is touched."""
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    table, lens, dests = 0x1000, 0x3000, 0x2000       # never dereferenced: the context is checked first
    assert lib.fec_recover_scatter_rs_dev(None, table, lens, dests, 1, 10, 3, 1200, None, None, None,
                                          None) == quicfec_mod.FEC_ERR_NULL
    assert "context" in quicfec_mod.last_error(lib)
