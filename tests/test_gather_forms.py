"""The address-table calls (fec_recover_gather_rs_dev, fec_encode_gather_rs_dev) without a GPU:
which recover_gather form csrc/fec_forms.hpp decides at every packet size (through
tests/csrc/table_forms_dump.cpp gather, against a table written from DESIGN.md §5b), and the two
calls' place in the header, the binding and both libraries.
"""
import re
import subprocess

import pytest

from forms_support import (COMPILED_SHAPES, CSRC, DUMP_SRC, GATHER_POL, MIN_P, POL_NO_COEF_BRANCH, REPO, RUNTIME_ROWS,
                           SANITIZE, SHAPES, SIZES, _build, _run)


# DESIGN.md §5b, "Recover from an address table"
def expected_launches(k, r, P):
    """The launches of one gather recover by the table, or None where the call is refused."""
    if P < MIN_P:
        return None
    if (k, r) in COMPILED_SHAPES:
        return ["classify_gather", f"recover_gather k={k} r={r} pol={GATHER_POL} aux=0"]
    pol = GATHER_POL | POL_NO_COEF_BRANCH
    return ["classify_gather"] + [f"recover_gather k=0 r={RUNTIME_ROWS} pol={pol} aux={m0}"
                                  for m0 in range(0, r, RUNTIME_ROWS)]


@pytest.fixture(scope="module")
def dump_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("gather_forms_dump")


@pytest.fixture(scope="module")
def dump_lines(dump_dir):
    return _run(_build(dump_dir, "plain", DUMP_SRC, [], [CSRC / "fec_knobs.cpp"]), "gather")[0]


def test_decided_gather_forms_equal_the_table(dump_lines):
    """table_recover_form (csrc/fec_forms.hpp) at every size of the ten shapes against the table above."""
    want = []
    for k, r in SHAPES:
        for P in SIZES:
            launches = expected_launches(k, r, P)
            want.append(f"gather k={k} r={r} P={P} | " + ("refused" if launches is None else " ; ".join(launches)))
    assert len(dump_lines) == len(SHAPES) * len(SIZES)
    assert dump_lines == want
    # the table names every route at least once: refused, each compiled shape, one and two passes
    assert sum(ln.endswith("refused") for ln in dump_lines) == len(SHAPES) * (MIN_P - 1)
    assert any(ln.count("recover_gather") == 2 for ln in dump_lines)       # k=12 r=9: rows 0..7, then 8


def test_compiled_gather_forms_are_the_tables(dump_dir, dump_lines):
    """The list the launcher's dispatch is expanded from holds exactly the forms the table can ask
    for: one per compiled shape and the runtime-k one."""
    compiled, _ = _run(dump_dir / "plain", "gather", "--compiled")
    want = {f"recover_gather k={k} r={r} pol={GATHER_POL} aux=0" for k, r in COMPILED_SHAPES}
    want.add(f"recover_gather k=0 r={RUNTIME_ROWS} pol={GATHER_POL | POL_NO_COEF_BRANCH} aux=0")
    assert len(compiled) == len(want) == 6 and set(compiled) == want
    asked = {re.sub(r"aux=\d+", "aux=0", launch) for ln in dump_lines if not ln.endswith("refused")
             for launch in ln.split(" | ")[1].split(" ; ")[1:]}
    assert asked == want


def test_gather_forms_dump_under_sanitizers(dump_dir, dump_lines):
    """The deciding code as a stand-alone host program under AddressSanitizer and UBSan: one run,
    no report, the same lines.  The runtimes are linked into the program itself, so whatever else
    the environment loads into it, their place in the library list is not in question."""
    exe = _build(dump_dir, "sanitized", DUMP_SRC, SANITIZE, [CSRC / "fec_knobs.cpp"])
    lines, err = _run(exe, "gather")
    assert lines == dump_lines
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    assert _run(exe, "gather", "--compiled")[0] == _run(dump_dir / "plain", "gather", "--compiled")[0]


GATHER_CALLS = ("fec_recover_gather_rs_dev", "fec_encode_gather_rs_dev")


def test_header_declares_the_gather_calls():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "fec_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+fec_recover_gather_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_shard_addrs,"
                     r"\s*uint64_t num_groups,\s*uint32_t k,\s*uint32_t r,\s*uint32_t packet_size,\s*uint8_t\*\s*d_rebuilt,"
                     r"\s*uint8_t\*\s*d_status,\s*uint64_t\*\s*d_masks_out,\s*void\*\s*stream\)\s*;", text)
    assert re.search(r"\bint\s+fec_encode_gather_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_packet_addrs,"
                     r"\s*uint64_t num_groups,\s*uint32_t k,\s*uint32_t r,\s*uint32_t packet_size,\s*uint8_t\*\s*d_parity,"
                     r"\s*void\*\s*stream\)\s*;", text)


def test_binding_and_both_libraries_have_the_gather_calls(quicfec_mod):
    assert set(GATHER_CALLS) <= set(quicfec_mod.HIP_SYMBOLS)
    assert callable(quicfec_mod.Context.recover_gather_dev) and callable(quicfec_mod.Context.encode_gather_dev)
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True,
                             check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(GATHER_CALLS) <= exported, lib
    # the gather kernels' trace names are a list of their own; the decode list is as it was
    assert quicfec_mod.GATHER_LAUNCH_FORMS == {18: "classify_gather", 19: "recover_gather"}
    assert not set(quicfec_mod.GATHER_LAUNCH_FORMS) & set(quicfec_mod.LAUNCH_FORMS)


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    """Both calls answer a NULL context with FEC_ERR_NULL and a message before touching any device."""
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    table, out = 0x1000, 0x2000                       # never dereferenced: the context is checked first
    assert lib.fec_recover_gather_rs_dev(None, table, 1, 10, 3, 1200, out, None, None, None) == quicfec_mod.FEC_ERR_NULL
    assert "context" in quicfec_mod.last_error(lib)
    assert lib.fec_encode_gather_rs_dev(None, table, 1, 10, 3, 1200, out, None) == quicfec_mod.FEC_ERR_NULL
    assert "context" in quicfec_mod.last_error(lib)
