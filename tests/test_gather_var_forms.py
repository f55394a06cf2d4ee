"""The variable-length address-table calls (fec_recover_gather_var_rs_dev,
fec_encode_gather_var_rs_dev) without a GPU:
  * the length-masked piece load (csrc/fec_varlen.hpp) against its byte-wise definition, as a
    stand-alone program run plain and under AddressSanitizer + UBSan -- the sanitized run is the
    check of the no-over-read rule (tests/csrc/varlen_window_test.cpp);
  * which forms csrc/fec_forms.hpp decides at every packet size (tests/csrc/table_forms_dump.cpp gather_var)
    against a table written from DESIGN.md §5b;
  * the two calls' place in the header, the binding and both libraries.
"""
import re
import subprocess

import pytest

from forms_support import (COMPILED_SHAPES, CSRC, DUMP_SRC, ENCODE_POL, GATHER_POL, MIN_P, POL_NO_COEF_BRANCH, REPO,
                           RUNTIME_ROWS, SANITIZE, SHAPES, SIZES, TESTS_CSRC, _build, _run)


# DESIGN.md §5b, "Variable-length address tables"
def expected_recover_launches(k, r, P):
    """The launches of one variable-length gather recover by the table, or None where it is refused."""
    if P < MIN_P:
        return None
    if (k, r) in COMPILED_SHAPES:
        return ["classify_gather_var", f"recover_gather_var k={k} r={r} pol={GATHER_POL} aux=0"]
    pol = GATHER_POL | POL_NO_COEF_BRANCH
    return ["classify_gather_var"] + [f"recover_gather_var k=0 r={RUNTIME_ROWS} pol={pol} aux={m0}"
                                      for m0 in range(0, r, RUNTIME_ROWS)]


def expected_encode_launches(k, r, P):
    """Every shape at runtime k, passes of up to eight rows, the first one owning the XOR row."""
    if P < MIN_P:
        return None
    return [f"encode_gather_var k=0 r={min(RUNTIME_ROWS, r - row0)} first={int(row0 == 0)} pol={ENCODE_POL} aux={row0}"
            for row0 in range(0, r, RUNTIME_ROWS)]


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("gather_var_forms")


# ------------------------------------------------------------------------------------------
# The length-masked piece load
# ------------------------------------------------------------------------------------------
def _window_kinds(nb, lens=range(97), offs=range(97)):
    """How many (len, off) fall to each kind by the header's own statement of the four cases."""
    n = {"none": 0, "full": 0, "back": 0, "bytes": 0}
    for ln in lens:
        for off in offs:
            kind = "none" if off >= ln else "full" if off + nb <= ln else "back" if ln >= nb else "bytes"
            n[kind] += 1
    return n


def test_varlen_window_plain_and_under_sanitizers(work_dir):
    """Every NB in {4, 16}, len in 0..96 and off in 0..96 on a heap block of exactly len bytes: the
    assembled piece equals the byte-wise definition.  Once plain, once with AddressSanitizer and
    UBSan linked in statically: no report, the same output -- nothing at or past p + len is read."""
    src = TESTS_CSRC / "varlen_window_test.cpp"
    plain, err = _run(_build(work_dir, "varlen_plain", src, []))
    assert plain[-1] == "ok", (plain, err)
    counts = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in plain if ln.startswith("NB=")}
    for nb in (4, 16):
        want = _window_kinds(nb)
        assert all(v > 0 for v in want.values())                             # the sweep meets all four cases
        assert {kind: counts[(f"NB={nb}", kind)] for kind in want} == want
    sanitized, err = _run(_build(work_dir, "varlen_sanitized", src, SANITIZE))
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
    return _run(dump_exe, "gather_var")[0]


def test_decided_gather_var_forms_equal_the_table(dump_lines):
    """table_recover_form and table_encode_form's pass structure (csrc/fec_forms.hpp) at every size
    of the ten shapes against the table above."""
    want = []
    for k, r in SHAPES:
        for P in SIZES:
            for name, launches in (("gather_var", expected_recover_launches(k, r, P)),
                                   ("encode_var", expected_encode_launches(k, r, P))):
                want.append(f"{name} k={k} r={r} P={P} | " + ("refused" if launches is None else " ; ".join(launches)))
    assert len(dump_lines) == 2 * len(SHAPES) * len(SIZES)
    assert dump_lines == want
    # the table names every route at least once: refused, each compiled shape, one and two passes
    assert sum(ln.endswith("refused") for ln in dump_lines) == 2 * len(SHAPES) * (MIN_P - 1)
    assert any(ln.count("recover_gather_var") == 2 for ln in dump_lines)     # k=12 r=9: rows 0..7, then 8
    assert any(ln.count("encode_gather_var") == 2 and "first=0" in ln for ln in dump_lines)


def test_compiled_gather_var_forms_are_the_tables(dump_exe, dump_lines):
    """The list the launcher's dispatch is expanded from holds exactly the forms the table can ask
    for: one per compiled shape and the runtime-k one."""
    compiled, _ = _run(dump_exe, "gather_var", "--compiled")
    want = {f"recover_gather_var k={k} r={r} pol={GATHER_POL} aux=0" for k, r in COMPILED_SHAPES}
    want.add(f"recover_gather_var k=0 r={RUNTIME_ROWS} pol={GATHER_POL | POL_NO_COEF_BRANCH} aux=0")
    assert len(compiled) == len(want) == 6 and set(compiled) == want
    asked = {re.sub(r"aux=\d+", "aux=0", launch) for ln in dump_lines
             if ln.startswith("gather_var") and not ln.endswith("refused")
             for launch in ln.split(" | ")[1].split(" ; ")[1:]}
    assert asked == want


def test_gather_var_encode_passes_at_every_row_count(dump_exe):
    """The encode's pass structure at k = 1, P = 1200 and every r in 1..63 (k + r <= 64) against the
    table: ceil(r / 8) launches, the first with first=1 from row 0, full passes of 8 rows and a last
    one of the rest -- every row count 1..8 both as the first pass and as a later one."""
    rows, _ = _run(dump_exe, "gather_var", "--rows")
    assert rows == [f"encode_var k=1 r={r} P=1200 | " + " ; ".join(expected_encode_launches(1, r, 1200))
                    for r in range(1, 64)]
    assert [ln.count("encode_gather_var") for ln in rows] == [-(-r // RUNTIME_ROWS) for r in range(1, 64)]
    asked = {re.sub(r"aux=\d+", "aux=0", launch) for ln in rows for launch in ln.split(" | ")[1].split(" ; ")}
    assert asked == {f"encode_gather_var k=0 r={n} first={f} pol={ENCODE_POL} aux=0"
                     for n in range(1, RUNTIME_ROWS + 1) for f in (0, 1)}


def test_gather_var_forms_dump_under_sanitizers(work_dir, dump_exe, dump_lines):
    exe = _build(work_dir, "dump_sanitized", DUMP_SRC, SANITIZE, [CSRC / "fec_knobs.cpp"])
    lines, err = _run(exe, "gather_var")
    assert lines == dump_lines
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    assert _run(exe, "gather_var", "--compiled")[0] == _run(dump_exe, "gather_var", "--compiled")[0]


# ------------------------------------------------------------------------------------------
# Declarations and exports
# ------------------------------------------------------------------------------------------
GATHER_VAR_CALLS = ("fec_recover_gather_var_rs_dev", "fec_encode_gather_var_rs_dev")


def test_header_declares_the_gather_var_calls():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fec_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fec_recover_gather_var_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_shard_addrs,"
                     r"\s*const uint32_t\*\s*d_shard_lens,\s*uint64_t num_groups,\s*uint32_t k,\s*uint32_t r,"
                     r"\s*uint32_t packet_size,\s*uint8_t\*\s*d_rebuilt,\s*uint8_t\*\s*d_status,"
                     r"\s*uint64_t\*\s*d_masks_out,\s*uint32_t\*\s*d_symbol_len_out,\s*void\*\s*stream\)\s*;", text)
    assert re.search(r"\bint\s+fec_encode_gather_var_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_packet_addrs,"
                     r"\s*const uint32_t\*\s*d_packet_lens,\s*uint64_t num_groups,\s*uint32_t k,\s*uint32_t r,"
                     r"\s*uint32_t packet_size,\s*uint8_t\*\s*d_parity,\s*uint32_t\*\s*d_symbol_len_out,"
                     r"\s*void\*\s*stream\)\s*;", text)


def test_binding_and_both_libraries_have_the_gather_var_calls(quicfec_mod):
    assert set(GATHER_VAR_CALLS) <= set(quicfec_mod.HIP_SYMBOLS)
    assert callable(quicfec_mod.Context.recover_gather_var_dev) and callable(quicfec_mod.Context.encode_gather_var_dev)
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True,
                             check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(GATHER_VAR_CALLS) <= exported, lib
    # the new kernels' trace names are a list of their own; the two existing lists are as they were
    assert quicfec_mod.GATHER_VAR_LAUNCH_FORMS == {20: "classify_gather_var", 21: "recover_gather_var",
                                                   22: "encode_gather_var"}
    assert not set(quicfec_mod.GATHER_VAR_LAUNCH_FORMS) & (set(quicfec_mod.LAUNCH_FORMS) | set(quicfec_mod.GATHER_LAUNCH_FORMS))


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    """Both calls answer a NULL context with FEC_ERR_NULL and a message before touching any device."""
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    table, lens, out = 0x1000, 0x3000, 0x2000         # never dereferenced: the context is checked first
    assert lib.fec_recover_gather_var_rs_dev(None, table, lens, 1, 10, 3, 1200, out, None, None, None,
                                             None) == quicfec_mod.FEC_ERR_NULL
    assert "context" in quicfec_mod.last_error(lib)
    assert lib.fec_encode_gather_var_rs_dev(None, table, lens, 1, 10, 3, 1200, out, None, None) == quicfec_mod.FEC_ERR_NULL
    assert "context" in quicfec_mod.last_error(lib)
