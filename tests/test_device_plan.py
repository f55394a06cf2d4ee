"""Device-built recovery records (FEC_PLAN_DEVICE) for the shapes past the codebook cap, no GPU needed:
  * the record builder (csrc/fec_plan_build.hpp) against the host's build_record, byte for byte, as
    a stand-alone program run plain and under AddressSanitizer + UBSan with every record in a heap
    block of exactly its size (tests/csrc/plan_build_test.cpp);
  * the arena, chunk and workspace arithmetic of csrc/fec_forms.hpp (tests/csrc/plan_chunks_test.cpp);
  * fec_decode_plan_mode's place in the header, the binding and both libraries, the new test
    switch and the trace name.
"""
import re
import subprocess
from pathlib import Path

import pytest

from forms_support import CSRC, REPO, SANITIZE, TESTS_CSRC, _build, _run

# past the 2 GiB cap by gf256.hpp's codebook_layout (the issue's table) / within it
SPARSE_SHAPES = [(20, 7), (20, 8), (24, 6), (12, 12), (16, 16), (32, 8), (60, 4), (30, 20), (32, 32)]
DENSE_SHAPES = [(16, 8), (32, 5), (20, 6), (10, 10), (50, 4), (10, 3), (20, 5)]
CHUNK_SHAPES = [(4, 2), (5, 5), (10, 3), (12, 12), (20, 7), (24, 6), (16, 16), (32, 8), (60, 4), (30, 20), (32, 32)]
ARENA = 64 << 20
MASK_KINDS = ("none", "bad", "xor", "single", "full", "skip_rows", "first_last", "built")


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("device_plan")


# ------------------------------------------------------------------------------------------
# 1. Record bytes
# ------------------------------------------------------------------------------------------
def test_records_equal_build_record_plain_and_under_sanitizers(work_dir):
    """Every pattern of (4,2), (5,5), (10,3) and 2,000 drawn masks of each of eight large shapes:
    mask_losses equals a bit-by-bit count, and the record the 64 lanes write into a heap block of exactly
    record_bytes(k, e) bytes equals build_record's.  Once plain, once with AddressSanitizer and
    UBSan linked in statically: no report and the same counts -- no byte outside a record is
    touched.  Every kind of mask the builder has a case for was met."""
    src = TESTS_CSRC / "plan_build_test.cpp"
    plain, err = _run(_build(work_dir, "build_plain", src, []))
    assert plain[-1] == "ok", (plain, err)
    counts = {ln.split()[0]: int(ln.split()[1]) for ln in plain[:-1]}
    print(counts)
    assert set(counts) == set(MASK_KINDS)
    for kind in MASK_KINDS:
        assert counts[kind] > 0, kind
    # the exhaustive shapes alone: every mask with 1 <= e <= alive rows builds a record
    exhaustive = 0
    for k, r in [(4, 2), (5, 5), (10, 3)]:
        for m in range(1 << (k + r)):
            e, lost_rows = bin(m & ((1 << k) - 1)).count("1"), bin(m >> k).count("1")
            exhaustive += 1 <= e <= r - lost_rows
    assert counts["built"] >= exhaustive + 8 * 2000 * 7 // 8   # 7 of the 8 kinds drawn are always recoverable
    sanitized, err = _run(_build(work_dir, "build_sanitized", src, SANITIZE))
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]


# ------------------------------------------------------------------------------------------
# 2. Chunk arithmetic
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chunk_lines(work_dir):
    exe = _build(work_dir, "chunks_sanitized", TESTS_CSRC / "plan_chunks_test.cpp", SANITIZE, [CSRC / "fec_knobs.cpp"])
    lines, err = _run(exe)
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    assert lines[-1] == "ok", (lines[-3:], err)
    return lines[:-1]


def _stride(k, r):
    return 128 + min(k, r) * k * 32            # gf256.hpp record_bytes(k, min(k, r))


def test_chunks_tile_the_groups_inside_the_arena(chunk_lines):
    """The program checks the tiling, the slots and the workspace itself (it exits non-zero
    otherwise); here its lines are compared with the same sizes worked out from the issue's rules:
    stride = record_bytes(k, min(k, r)), per_chunk = min(G, max(1, budget // stride))."""
    want = []
    for k, r in CHUNK_SHAPES:
        s = _stride(k, r)
        for budget in (ARENA, s, s + 1, 5 * s):
            for G in (1, 4, 5, 67, 2**32 - 1):
                per = min(G, max(1, budget // s))
                chunks = -(-G // per)
                masks = (4 * G + 7) & ~7
                symlen = masks + 8 * G
                arena = (symlen + 4 * G + 255) & ~255
                want.append(f"k={k} r={r} budget={budget} G={G} | stride={s} per_chunk={per} arena={per * s} "
                            f"chunks={chunks} last={G - (chunks - 1) * per} "
                            f"ws=rec_off:0,masks:{masks},symlen:{symlen},arena:{arena},bytes:{arena + per * s}")
    assert chunk_lines == want
    # the GPU test's case: five slots, 67 groups -> 14 chunks of 5, ..., 5, 2
    assert any(ln.startswith(f"k=16 r=16 budget={5 * _stride(16, 16)} G=67 |") and " per_chunk=5 " in ln
               and " chunks=14 last=2 " in ln for ln in chunk_lines)


def test_every_record_offset_is_below_the_markers():
    """The largest rec_off a 64 MiB arena can hold is far below kRecBad, whatever the shape."""
    hpp = (CSRC / "fec_forms.hpp").read_text()
    assert re.search(r"constexpr uint32_t kPlanRecLimit = 0xFFFFFFFEu;", hpp)
    assert re.search(r"constexpr uint32_t kRecBad = 0xFFFFFFFEu;", (CSRC / "fec_kernels.hpp").read_text())
    assert re.search(r"constexpr uint64_t kPlanArenaBytes = 64ull << 20;", hpp)
    assert ARENA // 32 < 0xFFFFFFFE


def test_sparse_and_dense_shapes_are_the_issues(work_dir):
    """Which shapes a device plan serves: exactly those codebook_layout refuses under the 2 GiB cap."""
    src = work_dir / "layout.cpp"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "gf256.hpp"\nint main(int c, char** v) {\n'
                   "  for (int i = 1; i + 1 < c; i += 2) {\n    qfec::CodebookLayout L;\n"
                   '    std::printf("%d\\n", qfec::codebook_layout(std::atoi(v[i]), std::atoi(v[i + 1]), 2ull << 30, L) ? 1 : 0);\n'
                   "  }\n  return 0;\n}\n")
    exe = _build(work_dir, "layout", src, [])
    shapes = SPARSE_SHAPES + DENSE_SHAPES
    lines, _ = _run(exe, *[str(x) for kr in shapes for x in kr])
    assert [int(x) for x in lines] == [0] * len(SPARSE_SHAPES) + [1] * len(DENSE_SHAPES)


# ------------------------------------------------------------------------------------------
# 3. Surface
# ------------------------------------------------------------------------------------------
def test_header_declares_the_mode_call():
    raw = (REPO / "include" / "fec_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+fec_decode_plan_mode\s*\(\s*FECEncoderCtx\*\s*ctx,\s*int\s+mode\s*\)\s*;", text)
    assert re.search(r"^#define FEC_PLAN_CODEBOOK 0\s*$", text, re.M)
    assert re.search(r"^#define FEC_PLAN_DEVICE 1\s*$", text, re.M)
    # the address-table block's refusal is now conditional on the mode
    block = raw[raw.index("Refused with nothing launched or written"):]
    block = block[:block.index("*/")]
    assert "unless the context is" in block and "FEC_PLAN_DEVICE" in block


def test_binding_and_both_libraries_have_the_mode_call(quicfec_mod):
    assert "fec_decode_plan_mode" in quicfec_mod.HIP_SYMBOLS
    assert callable(quicfec_mod.Context.decode_plan_mode)
    assert (quicfec_mod.FEC_PLAN_CODEBOOK, quicfec_mod.FEC_PLAN_DEVICE) == (0, 1)
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert "fec_decode_plan_mode" in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = Path(lib).read_bytes()
        for name in quicfec_mod.PLAN_LAUNCH_FORMS.values():      # names live with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


def test_arena_switch_is_in_the_test_library_only(quicfec_mod):
    assert b"QUICFEC_PLAN_ARENA_BYTES" not in Path(quicfec_mod.LIB_PATH).read_bytes()
    assert b"QUICFEC_PLAN_ARENA_BYTES" in Path(quicfec_mod.TEST_LIB_PATH).read_bytes()


def test_plan_launch_id_equals_the_binding(quicfec_mod):
    """PlanLaunchForm (csrc/fec_knobs.hpp) against quicfec.PLAN_LAUNCH_FORMS: numbered on from the
    scatter encode's 25, in a list of its own."""
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class PlanLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == quicfec_mod.PLAN_LAUNCH_FORMS == {26: "build_records"}
    others = (set(quicfec_mod.LAUNCH_FORMS) | set(quicfec_mod.GATHER_LAUNCH_FORMS) | set(quicfec_mod.GATHER_VAR_LAUNCH_FORMS)
              | set(quicfec_mod.SCATTER_LAUNCH_FORMS) | set(quicfec_mod.SCATTER_ENCODE_LAUNCH_FORMS))
    assert min(quicfec_mod.PLAN_LAUNCH_FORMS) == max(others) + 1


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    lib.fec_decode_plan_mode.restype, lib.fec_decode_plan_mode.argtypes = quicfec_mod._int, [quicfec_mod._vp, quicfec_mod._int]
    assert lib.fec_decode_plan_mode(None, quicfec_mod.FEC_PLAN_DEVICE) == quicfec_mod.FEC_ERR_NULL
    assert lib.fec_decode_plan_mode(None, 7) == quicfec_mod.FEC_ERR_NULL


def test_new_kernel_is_built_and_hashed():
    """fec_plan.hip is an object of both libraries and among the hashed sources."""
    mk = (CSRC / "Makefile").read_text()
    assert "fec_plan.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    # the objects both libraries share are derived from SRCS: make's own link lines name the object
    dry = subprocess.run(["make", "-C", str(CSRC), "-n", "-B", "../lib/libfec_hip.so", "../lib/libfec_hip_test.so"],
                         capture_output=True, text=True, check=True).stdout
    links = [ln for ln in dry.splitlines() if " -shared " in ln]
    assert len(links) == 2 and all("../lib/fec_plan.o" in ln.split() for ln in links), links
    import sys
    sys.path.insert(0, str(CSRC))
    import src_hash
    names = {p.name for p in src_hash.source_files()}
    assert {"fec_plan.hip", "fec_plan_build.hpp"} <= names
