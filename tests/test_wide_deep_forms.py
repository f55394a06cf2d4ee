"""The wide calls past min(k, r) <= 32 (fec_wide_rows_mode, FEC_WIDE_ROWS_ALL), no GPU needed:
  * csrc/fec_plan_build_deep.hpp against the definition of a recovery record, against the wide
    builder where both serve, and its header byte for byte, as a stand-alone program run plain and
    under AddressSanitizer + UBSan (tests/csrc/plan_build_deep_test.cpp);
  * the served rule, the path and the arena of csrc/fec_forms.hpp in both modes
    (tests/csrc/wide_deep_forms_test.cpp), with wide_served unchanged;
  * the call's place in the header, the binding, both libraries, the Makefile, the source hash and
    the launch trace's names.
"""
import re
import subprocess
import sys

import pytest

from forms_support import CSRC, REPO, SANITIZE, TESTS_CSRC, _build, _run

DEEP_SHAPES = [(33, 33), (65, 65), (100, 100), (128, 128), (40, 216), (216, 40), (96, 160)]
CAPPED_SHAPES = [(60, 5), (224, 32), (32, 224), (32, 32), (255, 1), (1, 255), (10, 3)]
PLANTED_E = (1, 2, 32, 33, 64, 65)
ARENA = 64 << 20
SERVED, SHAPE, ROWS, PACKET, NO_GROUPS, GROUPS = range(6)            # fec_forms.hpp WideRefusal
REFUSED, WIDE, DEEP = range(3)                                       # fec_forms.hpp WidePath
CAPPED, ALL = 0, 1                                                   # fec_hip.h FEC_WIDE_ROWS_*


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wide_deep")


def _stride(k, r):
    return 512 + min(k, r) * k * 32


# ------------------------------------------------------------------------------------------
# 1. The record builder
# ------------------------------------------------------------------------------------------
def test_deep_records_plain_and_under_sanitizers(work_dir):
    """Every record built with one lane and with 256, in heap blocks of exactly its size: the
    coefficients rebuild the erased shards by the definition, the header is the stated one byte for
    byte, and for e <= 32 the tables are the wide builder's."""
    src = TESTS_CSRC / "plan_build_deep_test.cpp"
    plain, err = _run(_build(work_dir, "plan_build_deep_plain", src, []))
    assert plain[-1] == "ok", (plain, err)
    sanitized, err = _run(_build(work_dir, "plan_build_deep_sanitized", src, SANITIZE))
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    counts = {ln.split()[0]: int(ln.split()[1]) for ln in plain[:-1]}
    assert set(counts) == {f"{k}+{r}" for k, r in DEEP_SHAPES + [(32, 32), (224, 32)]}
    for k, r in DEEP_SHAPES + [(32, 32), (224, 32)]:
        emax = min(k, r)
        planted = {e for e in PLANTED_E + (emax,) if e <= emax}
        assert counts[f"{k}+{r}"] == 3 * len(planted) + 200, (k, r)


# ------------------------------------------------------------------------------------------
# 2. Served shapes, the path, the arena
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forms_exe(work_dir):
    return _build(work_dir, "wide_deep_forms", TESTS_CSRC / "wide_deep_forms_test.cpp", SANITIZE, [CSRC / "fec_knobs.cpp"])


def _routes(forms_exe, cases):
    lines, err = _run(forms_exe, *[str(x) for c in cases for x in c])
    assert lines[-1] == "ok" and "runtime error" not in err, (lines, err)
    assert len(lines) == len(cases) + 1
    return [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in ln.split()} for ln in lines[:-1]]


def test_route_of_every_shape_in_both_modes(forms_exe):
    """A shape wide_served serves takes the wide path in either mode; a shape past the cap is refused
    for its rows in the capped mode and takes the deep path in FEC_WIDE_ROWS_ALL; ceil(min(k, r) / 8)
    consumer launches per chunk on either path."""
    cases = [(mode, 67, k, r, 16) for mode in (CAPPED, ALL) for k, r in DEEP_SHAPES + CAPPED_SHAPES]
    for (mode, G, k, r, P), row in zip(cases, _routes(forms_exe, cases)):
        passes = -(-min(k, r) // 8)
        if (k, r) in CAPPED_SHAPES:
            assert row == {"path": WIDE, "why": SERVED, "passes": passes, "capped": SERVED, "all": SERVED}, (mode, k, r)
        elif mode == CAPPED:
            assert row == {"path": REFUSED, "why": ROWS, "passes": 0, "capped": ROWS, "all": SERVED}, (k, r)
        else:
            assert row == {"path": DEEP, "why": SERVED, "passes": passes, "capped": ROWS, "all": SERVED}, (k, r)
    assert -(-128 // 8) == 16


def test_wide_served_still_answers_rows(forms_exe):
    """wide_served is the capped mode's rule, unchanged: (33, 33) and (128, 128) are refused for their rows."""
    got = _routes(forms_exe, [(ALL, 67, 33, 33, 16), (ALL, 67, 128, 128, 16), (CAPPED, 67, 100, 100, 1200)])
    assert [row["capped"] for row in got] == [ROWS, ROWS, ROWS]


def test_refusals_in_both_modes(forms_exe):
    """What neither mode serves, with the reason each gives: the capped mode names the rows before the
    packet size, as wide_served does; FEC_WIDE_ROWS_ALL has no rows to name.  An unknown mode is the
    capped one to wide_route (the shim refuses to set it)."""
    bad = [((CAPPED, 67, 200, 57, 16), SHAPE), ((ALL, 67, 200, 57, 16), SHAPE), ((ALL, 67, 0, 5, 16), SHAPE), ((ALL, 67, 5, 0, 16), SHAPE),
           ((ALL, 67, 256, 1, 16), SHAPE), ((ALL, 67, 129, 128, 16), SHAPE), ((CAPPED, 67, 33, 33, 15), ROWS), ((ALL, 67, 33, 33, 15), PACKET),
           ((ALL, 67, 60, 5, 15), PACKET), ((CAPPED, 0, 128, 128, 16), ROWS), ((ALL, 0, 128, 128, 16), NO_GROUPS),
           ((ALL, 2**32, 128, 128, 16), GROUPS), ((ALL, 2**32, 60, 5, 16), GROUPS), ((2, 67, 33, 33, 16), ROWS), ((-1, 67, 128, 128, 16), ROWS)]
    for (case, why), row in zip(bad, _routes(forms_exe, [c for c, _ in bad])):
        assert row["path"] == REFUSED and row["why"] == why and row["passes"] == 0, case
    ok = _routes(forms_exe, [(ALL, 2**32 - 1, 128, 128, 16), (ALL, 1, 33, 33, 9000), (2, 67, 60, 5, 16)])
    assert [row["path"] for row in ok] == [DEEP, DEEP, WIDE]


def test_deep_arena_sizes(forms_exe):
    """wide_deep_slot_stride(k, r) = 512 + min(k, r) * k * 32, the wide formula past its cap: 524,800 B at
    128 + 128, 127 slots under the 64 MiB budget; one slot when the budget is below a stride; the
    workspace is G record offsets, then the arena, 256-B aligned."""
    cases = []
    for k, r in DEEP_SHAPES:
        s = _stride(k, r)
        for budget in (0, s - 1, s, 5 * s, 5 * s + 1):
            for G in (1, 5, 67, 2**32 - 1):
                cases.append((budget, G, k, r))
    lines, err = _run(forms_exe, "--arena", *[str(x) for c in cases for x in c])
    assert lines[-1] == "ok" and "runtime error" not in err, (lines[-3:], err)
    for (budget, G, k, r), ln in zip(cases, lines[:-1]):
        s = _stride(k, r)
        per = min(G, max(1, (budget or ARENA) // s))
        at = (4 * G + 7 & ~7) + 255 & ~255
        assert ln == f"per_chunk={per} stride={s} arena={per * s} chunks={-(-G // per)} arena_at={at} bytes={at + per * s}", (budget, G, k, r)
    s = _stride(128, 128)
    assert s == 524800 and ARENA // s == 127
    assert lines[cases.index((0, 2**32 - 1, 128, 128))].startswith(f"per_chunk=127 stride={s} ")
    assert lines[cases.index((s - 1, 67, 128, 128))].startswith(f"per_chunk=1 stride={s} ")
    assert ARENA // 32 < 0xFFFFFFFE and s // 32 < 0xFFFFFFFE     # every record offset is below the markers
    # the scratch arithmetic of the builder against a CU's 160 KiB: three workgroups
    hpp = (CSRC / "fec_plan_build_deep.hpp").read_text()
    assert "static_assert(sizeof(DeepPlanScratch) == 49664" in hpp
    assert 128 + 128 + 256 + 3 * 128 * 128 == 49664 and 3 * 49664 <= 160 * 1024 < 4 * 49664


# ------------------------------------------------------------------------------------------
# 3. Surface
# ------------------------------------------------------------------------------------------
CALL = "fec_wide_rows_mode"


def test_header_declares_the_mode():
    raw = (REPO / "include" / "fec_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"^#define FEC_WIDE_ROWS_CAPPED 0\s*$", text, re.M) and re.search(r"^#define FEC_WIDE_ROWS_ALL 1\s*$", text, re.M)
    assert re.search(r"\bint\s+fec_wide_rows_mode\s*\(\s*FECEncoderCtx\*\s*ctx,\s*int\s+mode\s*\)\s*;", text)
    # the pinned sentences stay; the one that said nothing recovers these shapes names the mode
    assert "min(k, r) <= 32" in raw and "160 KiB" in raw
    assert re.search(r"that no wide call recovers\s*\*\s*unless the context is in FEC_WIDE_ROWS_ALL", raw)
    section = raw[raw.index("FEC_WIDE_ROWS_CAPPED (default)"):raw.index("#define FEC_WIDE_ROWS_CAPPED")]
    for words in ("524,800 B", "127 groups", "ceil(min(k, r) / 8)", "up to 16", "512 + min(k, r) * k * 32", "FEC_ERR_NULL",
                  "FEC_ERR_RANGE", "unchanged", "the same launches, the same bytes", "fec_encoder_free"):
        assert words in section, words


def test_binding_and_both_libraries_have_the_mode(quicfec_mod):
    q = quicfec_mod
    assert CALL in q.HIP_SYMBOLS and callable(q.Context.wide_rows_mode)
    assert (q.FEC_WIDE_ROWS_CAPPED, q.FEC_WIDE_ROWS_ALL) == (0, 1)
    for lib in (q.LIB_PATH, q.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert CALL in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = open(lib, "rb").read()
        for name in q.WIDE_DEEP_LAUNCH_FORMS.values():               # names live with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


def test_launch_ids_equal_the_binding(quicfec_mod, forms_exe):
    q = quicfec_mod
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class WideDeepLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == q.WIDE_DEEP_LAUNCH_FORMS == {33: "build_records_deep", 34: "decode_wide_deep", 35: "recover_scatter_wide_deep"}
    assert min(q.WIDE_DEEP_LAUNCH_FORMS) == 33 == max(q.WIDE_ENCODE_LAUNCH_FORMS) + 1
    lines, _ = _run(forms_exe, "--ids")
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in lines[:-1])
    assert {v: k for k, v in q.WIDE_DEEP_LAUNCH_FORMS.items()}.items() <= got.items()
    # the consumers over a deep record are the wide kernels with one more form bit; the slots passes are the wide path's own
    assert got["deep_record_bit"] == 16384 and got["deep_record_bit"] & (got["pol_slots"] | 8191 | 8192) == 0
    assert got["pol_in_place"] == (q.POL_NT_STORE | q.POL_NO_COEF_BRANCH | 16384)
    assert got["pol_slots"] == (q.POL_NT_STORE | q.POL_NO_COEF_BRANCH | q.POL_COMPACT_OUT)
    assert got["pol_table"] == (q.POL_NT_LOAD | q.POL_NT_STORE | q.POL_NO_COEF_BRANCH | q.POL_COMPACT_OUT | 16384)
    # the existing lists are as they were
    assert q.WIDE_LAUNCH_FORMS == {27: "classify_wide", 28: "build_records_wide", 29: "decode_wide"}
    assert q.WIDE_TABLE_LAUNCH_FORMS == {30: "classify_table_wide", 31: "recover_scatter_wide"}
    assert q.WIDE_ENCODE_LAUNCH_FORMS == {32: "encode_scatter_wide"}
    others = [q.LAUNCH_FORMS, q.GATHER_LAUNCH_FORMS, q.GATHER_VAR_LAUNCH_FORMS, q.SCATTER_LAUNCH_FORMS, q.SCATTER_ENCODE_LAUNCH_FORMS,
              q.PLAN_LAUNCH_FORMS, q.WIDE_LAUNCH_FORMS, q.WIDE_TABLE_LAUNCH_FORMS, q.WIDE_ENCODE_LAUNCH_FORMS]
    for d in others:
        assert not set(d) & set(q.WIDE_DEEP_LAUNCH_FORMS)
        assert not set(d.values()) & set(q.WIDE_DEEP_LAUNCH_FORMS.values())


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    for mode in (0, 1, 2):
        assert lib.fec_wide_rows_mode(None, mode) == quicfec_mod.FEC_ERR_NULL


def test_new_unit_is_built_and_hashed():
    mk = (CSRC / "Makefile").read_text()
    assert "fec_wide_deep.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    dry = subprocess.run(["make", "-C", str(CSRC), "-n", "-B", "../lib/libfec_hip.so", "../lib/libfec_hip_test.so"],
                         capture_output=True, text=True, check=True).stdout
    links = [ln for ln in dry.splitlines() if " -shared " in ln]
    assert len(links) == 2 and all("../lib/fec_wide_deep.o" in ln.split() for ln in links), links
    # the builder's header is a prerequisite of the new unit and of the two units whose kernels read its layout
    for unit in ("fec_wide_deep", "fec_wide", "fec_wide_table"):
        deps = re.search(rf"^\$\(OUT_DIR\)/{unit}\.o [^:]*: (.*)$", mk, re.M).group(1).split()
        assert {"fec_plan_build_deep.hpp", "fec_wide_head.hpp", "fec_mask_wide.hpp"} <= set(deps), unit
    sys.path.insert(0, str(CSRC))
    import src_hash
    assert {"fec_wide_deep.hip", "fec_plan_build_deep.hpp"} <= {p.name for p in src_hash.source_files()}


def test_the_shim_asks_the_forms_and_nothing_else():
    """The three calls route through wide_route; no shape arithmetic of their own."""
    shim = (CSRC / "fec_shim.cpp").read_text()
    assert shim.count("qfec::wide_route(") == 1 and shim.count("qfec::wide_served(") == 1
    assert shim.count("wide_deep_admitted(what, ctx, G, k, r, P, &rc)") == 2       # wide_call and the table call
    assert shim.count("qfec::wide_deep_arena(") == 2 and shim.count("qfec::wide_rows_mode_known(") == 1
    body = shim[shim.index("QFEC_EXPORT int fec_wide_rows_mode"):]
    body = body[:body.index("\n}\n")]
    assert "std::lock_guard<std::mutex> lk(ctx->mu)" in body and "FEC_ERR_RANGE" in body and "FEC_ERR_NULL" in body
    assert not re.search(r"kWideMaxRows\s*[<>]|> 32|<= 32\b", shim[shim.index("bool wide_deep_admitted"):shim.index("QFEC_EXPORT int fec_decode_wide_rs_dev")])
