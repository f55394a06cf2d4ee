"""The wide scatter encode (fec_encode_scatter_wide_rs_dev; k + r <= 256 from scattered packets), no
GPU needed:
  * the call's place in the header, the binding, both libraries, the Makefile, the source hash and
    the launch trace's names;
  * wide_encode_served as the one statement of what is refused and wide_encode_form as the one place
    that decides the passes, as a stand-alone program run plain and under AddressSanitizer + UBSan
    (tests/csrc/wide_encode_forms_test.cpp).
"""
import re
import subprocess
import sys

import numpy as np
import pytest

from forms_support import CSRC, GATHER_POL, POL_NO_COEF_BRANCH, REPO, SANITIZE, TESTS_CSRC, _build, _run

CALL = "fec_encode_scatter_wide_rs_dev"
# the shapes of tests/test_gpu_wide_encode.py
SHAPES = [(65, 3), (64, 9), (129, 17), (224, 32), (32, 224), (128, 128), (33, 33), (255, 1), (1, 255), (100, 20),
          (10, 3), (12, 9), (32, 32)]
SERVED, SHAPE, PACKET, NO_GROUPS, TOO_MANY = range(5)                        # fec_forms.hpp WideEncodeRefusal
WIDE_SERVED, WIDE_ROWS = 0, 2                                                # fec_forms.hpp WideRefusal
POL = GATHER_POL | POL_NO_COEF_BRANCH                                        # kWideEncodePol = kWideTablePol


# ------------------------------------------------------------------------------------------
# 1. Surface
# ------------------------------------------------------------------------------------------
def test_header_declares_the_call():
    raw = (REPO / "include" / "fec_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+fec_encode_scatter_wide_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_packet_addrs,"
                     r"\s*const uint32_t\*\s*d_packet_lens,\s*const uint64_t\*\s*d_dest_addrs,\s*uint64_t\s+num_groups,"
                     r"\s*uint32_t\s+k,\s*uint32_t\s+r,\s*uint32_t\s+packet_size,\s*uint32_t\*\s*d_symbol_len_out,"
                     r"\s*void\*\s*stream\s*\)\s*;", text)
    assert "no wide address-table encode" not in raw
    # the full contract, not "as above": what the section itself states
    flat = lambda t: re.sub(r"\s*\n \*\s*", " ", t)
    section = flat(raw[raw.index("wide scatter encode"):raw.index("int fec_encode_scatter_wide_rs_dev")])
    for words in ("k + r <= 256", "There is no min(k, r) cap", "builds no record", "33 + 33, 128 + 128 and 1 + 255", "byte for byte",
                  "Address 0 means absent", "never dereferenced", "clamped to P", "followed by zeros",
                  "No byte at or past address + len is read", "length entry is ignored", "NULL: every present packet",
                  "written for every group", "0 when none is present", "not wanted", "exactly L_g bytes",
                  "L_g == 0 writes nothing and dereferences nothing", "must not overlap", "drained by fec_encoder_free",
                  "no workspace", "FEC_ERR_NULL", "FEC_ERR_RANGE", "packet_size < 16", "num_groups == 0 or >= 2^32"):
        assert words in section, words
    # and next to the recover's cap, so that nobody reads one rule into the other
    recover = flat(raw[raw.index("wide scatter recover"):raw.index("int fec_recover_scatter_wide_rs_dev")])
    assert "min(k, r) <= 32" in recover and CALL in recover and "builds no record" in recover


def test_binding_and_both_libraries_have_the_call(quicfec_mod):
    assert CALL in quicfec_mod.HIP_SYMBOLS
    assert callable(quicfec_mod.Context.encode_scatter_wide_dev)
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert CALL in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = open(lib, "rb").read()
        for name in quicfec_mod.WIDE_ENCODE_LAUNCH_FORMS.values():           # names live with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


def test_launch_ids_continue_and_collide_with_none(quicfec_mod):
    q = quicfec_mod
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class WideEncodeLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == q.WIDE_ENCODE_LAUNCH_FORMS == {32: "encode_scatter_wide"}
    assert min(q.WIDE_ENCODE_LAUNCH_FORMS) == max(q.WIDE_TABLE_LAUNCH_FORMS) + 1
    others = [q.LAUNCH_FORMS, q.GATHER_LAUNCH_FORMS, q.GATHER_VAR_LAUNCH_FORMS, q.SCATTER_LAUNCH_FORMS,
              q.SCATTER_ENCODE_LAUNCH_FORMS, q.PLAN_LAUNCH_FORMS, q.WIDE_LAUNCH_FORMS, q.WIDE_TABLE_LAUNCH_FORMS]
    for d in others:
        assert not set(d) & set(q.WIDE_ENCODE_LAUNCH_FORMS)
        assert not set(d.values()) & set(q.WIDE_ENCODE_LAUNCH_FORMS.values())
    # every id in the header's enums is named by exactly one dictionary of the reader
    ids = [int(x) for x in re.findall(r"^\s*k\w+ = (\d+),", hpp[hpp.index("enum class LaunchForm"):hpp.index("struct LaunchRecord")], re.M)]
    named = [i for d in others + [q.WIDE_ENCODE_LAUNCH_FORMS] for i in d]
    assert sorted(ids) == sorted(named) == list(range(1, 33))
    import inspect
    assert "WIDE_ENCODE_LAUNCH_FORMS" in inspect.getsource(q.launch_trace)


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.fec_encode_scatter_wide_rs_dev(None, p, None, p, 1, 65, 3, 16, None, None) == quicfec_mod.FEC_ERR_NULL
    assert b"context" in lib.fec_hip_last_error() and CALL.encode() in lib.fec_hip_last_error()
    assert not buf.any()


def test_new_unit_is_built_and_hashed():
    mk = (CSRC / "Makefile").read_text()
    assert "fec_wide_encode.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    dry = subprocess.run(["make", "-C", str(CSRC), "-n", "-B", "../lib/libfec_hip.so", "../lib/libfec_hip_test.so"],
                         capture_output=True, text=True, check=True).stdout
    links = [ln for ln in dry.splitlines() if " -shared " in ln]
    assert len(links) == 2 and all("../lib/fec_wide_encode.o" in ln.split() for ln in links), links
    # the headers only this unit and its neighbours include are its prerequisites
    deps = re.search(r"^\$\(OUT_DIR\)/fec_wide_encode\.o [^:]*: (.*)$", mk, re.M).group(1).split()
    assert {"fec_scatter_decode.hpp", "fec_scatter_cut.hpp", "fec_varlen.hpp"} <= set(deps)
    unit = (CSRC / "fec_wide_encode.hip").read_text()
    for inc in re.findall(r'#include "(\w+\.hpp)"', unit):
        assert inc in deps or inc in re.search(r"^KERNEL_HDRS := (.*)$", mk, re.M).group(1).split(), inc
    sys.path.insert(0, str(CSRC))
    import src_hash
    assert "fec_wide_encode.hip" in {p.name for p in src_hash.source_files()}


def test_the_unit_reuses_the_recovers_pieces():
    """The walk, the store cut and the masked load are the shared ones; the bound of encode_scatter is
    where it was."""
    unit = (CSRC / "fec_wide_encode.hip").read_text()
    for words in ("scatter_decode<0, MAXE, POL, true>", "load_masked<NW, POL>", "VarSurvivorsLds{slice, len_slice}",
                  "for_wave_passes(", "wide_encode_form(", "WideEncodeLaunchForm::kEncodeScatterWide", "t.aux = m0", "t.first = VAR"):
        assert words in unit, words
    for words in ("scatter_walk(", "var_window<", "var_load<", "scatter_store<"):   # not restated here
        assert words not in unit, words
    shim = (CSRC / "fec_shim.cpp").read_text()
    assert "k + r exceeds %u shards per group\", what, k, r, qfec::kMaxDecodeShards" in shim


# ------------------------------------------------------------------------------------------
# 2. The served rule and the form
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wide_encode")


@pytest.fixture(scope="module")
def programs(work_dir):
    src = TESTS_CSRC / "wide_encode_forms_test.cpp"
    extra = [CSRC / "fec_knobs.cpp"]
    return _build(work_dir, "wide_encode_plain", src, [], extra), _build(work_dir, "wide_encode_sanitized", src, SANITIZE, extra)


def _both(programs, *args):
    plain, err = _run(programs[0], *args)
    assert plain[-1] == "ok", (plain[-3:], err)
    sanitized, err = _run(programs[1], *args)
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    return plain[:-1]


def test_wide_encode_served_is_the_rule_of_the_call(programs):
    """What the call refuses is what wide_encode_served refuses: the shim asks it and nothing else, and
    there is no rows cap in it."""
    cases = [((67, k, r, 16), SERVED) for k, r in SHAPES]
    cases += [((2**32 - 1, 224, 32, 1200), SERVED), ((1, 128, 128, 2100), SERVED), ((67, 1, 1, 16), SERVED),
              ((67, 0, 5, 16), SHAPE), ((67, 5, 0, 16), SHAPE), ((67, 200, 57, 16), SHAPE), ((67, 256, 1, 16), SHAPE),
              ((67, 255, 255, 16), SHAPE), ((67, 65, 3, 15), PACKET), ((67, 65, 3, 0), PACKET),
              ((0, 65, 3, 16), NO_GROUPS), ((2**32, 65, 3, 16), TOO_MANY)]
    lines = _both(programs, *[str(x) for c, _ in cases for x in c])
    got = [tuple(int(f.split("=")[1]) for f in ln.split()) for ln in lines]
    assert [g[0] for g in got] == [why for _, why in cases]
    # the wide recover's rule refuses exactly the shapes past its rows cap among the served ones
    for (args, why), (_, wide) in zip(cases, got):
        if why == SERVED:
            assert wide == (WIDE_ROWS if min(args[1], args[2]) > 32 else WIDE_SERVED), args
    assert {(33, 33), (128, 128)} <= {a[1:3] for (a, _), g in zip(cases, got) if g == (SERVED, WIDE_ROWS)}
    shim = (CSRC / "fec_shim.cpp").read_text()
    body = shim[shim.index("QFEC_EXPORT int fec_encode_scatter_wide_rs_dev"):]
    body = body[:body.index("\n}\n")]
    assert "wide_encode_refused(what, G, k, r, P)" in body
    for other in ("wide_refused(", "check_gather_shape", "wide_served(", "get_encode_plan"):
        assert other not in body, other
    assert shim.count("qfec::wide_encode_served(") == 1
    assert shim.count("qfec::wide_served(") == 1
    hpp = (CSRC / "fec_forms.hpp").read_text()
    rule = hpp[hpp.index("constexpr WideEncodeRefusal wide_encode_served"):]
    rule = rule[:rule.index("\n}\n")]
    assert "kWideMaxRows" not in rule and "wide_served(" not in rule


def test_the_form_function_decides_the_passes(programs):
    """ceil(r / 8) passes of 8 rows at every shape, with and without the length table, r = 1 on the XOR
    path; the packet size chooses nothing; a refused shape has no form."""
    cases = [(k, r, P, var) for k, r in SHAPES for P in (16, 1200) for var in (0, 1)]
    cases += [(k, r, 272, 1) for k, r in ((200, 1), (100, 8), (100, 9), (32, 32), (33, 33), (128, 128), (1, 255))]
    refused = [(0, 5, 16, 0), (5, 0, 16, 1), (200, 57, 16, 0), (65, 3, 15, 1)]
    lines = _both(programs, "--form", *[str(x) for c in cases + refused for x in c])
    assert len(lines) == len(cases) + len(refused)
    for (k, r, P, var), ln in zip(cases, lines):
        assert ln == f"supported=1 passes={-(-r // 8)} pass_rows=8 var={var} xor_only={int(r == 1)} pol={POL}", (k, r, P, var)
    for ln in lines[len(cases):]:
        assert ln == "supported=0 passes=0 pass_rows=0 var=0 xor_only=0 pol=0"
    passes = {r: -(-r // 8) for r in (1, 8, 9, 32, 33, 128, 255)}
    assert passes == {1: 1, 8: 1, 9: 2, 32: 4, 33: 5, 128: 16, 255: 32}
    assert {r for _, r, _, _ in cases} >= set(passes)
