"""The wide address-table recover (fec_recover_scatter_wide_rs_dev; k + r <= 256 from scattered
shards), no GPU needed:
  * the call's place in the header, the binding, both libraries, the Makefile, the source hash and
    the launch trace's names;
  * the workspace and the chunk walk of csrc/fec_forms.hpp (wide_table_workspace over wide_arena,
    plan_chunks) and wide_served as the one statement of what is refused, as a stand-alone program
    run plain and under AddressSanitizer + UBSan (tests/csrc/wide_table_forms_test.cpp).
"""
import re
import subprocess
import sys

import numpy as np
import pytest

from forms_support import CSRC, REPO, SANITIZE, TESTS_CSRC, _build, _run

CALL = "fec_recover_scatter_wide_rs_dev"
SHAPES = [(60, 5), (224, 32), (32, 224), (255, 1), (1, 255)]
GROUPS = (1, 5, 67, 2**32 - 1)
ARENA = 64 << 20
SERVED, SHAPE, ROWS, PACKET, NO_GROUPS, TOO_MANY = range(6)          # fec_forms.hpp WideRefusal


# ------------------------------------------------------------------------------------------
# 1. Surface
# ------------------------------------------------------------------------------------------
def test_header_declares_the_call():
    raw = (REPO / "include" / "fec_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+fec_recover_scatter_wide_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint64_t\*\s*d_shard_addrs,"
                     r"\s*const uint32_t\*\s*d_shard_lens,\s*const uint64_t\*\s*d_dest_addrs,\s*uint64_t\s+num_groups,"
                     r"\s*uint32_t\s+k,\s*uint32_t\s+r,\s*uint32_t\s+packet_size,\s*uint8_t\*\s*d_status,"
                     r"\s*uint64_t\*\s*d_masks_out,\s*uint32_t\*\s*d_symbol_len_out,\s*void\*\s*stream\s*\)\s*;", text)
    assert "address-table forms of the wide calls" not in raw
    # the full contract, not "as above": what the section itself states
    section = raw[raw.index("wide scatter recover"):raw.index("int fec_recover_scatter_wide_rs_dev")]
    for words in ("min(k, r) <= 32", "Address 0 is", "clamped", "never", "not wanted", "exactly L_g bytes", "FEC_WIDE_MASK_WORDS",
                  "at and above k + r is zero", "fec_decode_plan_mode", "FEC_ERR_NULL", "FEC_ERR_RANGE", "byte for byte"):
        assert words in section, words


def test_binding_and_both_libraries_have_the_call(quicfec_mod):
    assert CALL in quicfec_mod.HIP_SYMBOLS
    assert callable(quicfec_mod.Context.recover_scatter_wide_dev)
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert CALL in {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = open(lib, "rb").read()
        for name in quicfec_mod.WIDE_TABLE_LAUNCH_FORMS.values():    # names live with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


def test_launch_ids_equal_the_binding(quicfec_mod):
    q = quicfec_mod
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class WideTableLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == q.WIDE_TABLE_LAUNCH_FORMS == {30: "classify_table_wide", 31: "recover_scatter_wide"}
    assert min(q.WIDE_TABLE_LAUNCH_FORMS) == max(q.WIDE_LAUNCH_FORMS) + 1
    assert q.WIDE_LAUNCH_FORMS == {27: "classify_wide", 28: "build_records_wide", 29: "decode_wide"}
    others = [q.LAUNCH_FORMS, q.GATHER_LAUNCH_FORMS, q.GATHER_VAR_LAUNCH_FORMS, q.SCATTER_LAUNCH_FORMS,
              q.SCATTER_ENCODE_LAUNCH_FORMS, q.PLAN_LAUNCH_FORMS, q.WIDE_LAUNCH_FORMS]
    for d in others:
        assert not set(d) & set(q.WIDE_TABLE_LAUNCH_FORMS)
        assert not set(d.values()) & set(q.WIDE_TABLE_LAUNCH_FORMS.values())


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.fec_recover_scatter_wide_rs_dev(None, p, None, p, 1, 60, 5, 16, None, None, None, None) == quicfec_mod.FEC_ERR_NULL
    assert b"context" in lib.fec_hip_last_error()
    assert not buf.any()


def test_new_unit_is_built_and_hashed():
    mk = (CSRC / "Makefile").read_text()
    assert "fec_wide_table.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    dry = subprocess.run(["make", "-C", str(CSRC), "-n", "-B", "../lib/libfec_hip.so", "../lib/libfec_hip_test.so"],
                         capture_output=True, text=True, check=True).stdout
    links = [ln for ln in dry.splitlines() if " -shared " in ln]
    assert len(links) == 2 and all("../lib/fec_wide_table.o" in ln.split() for ln in links), links
    # the headers only this unit and its two neighbours include are its prerequisites
    deps = re.search(r"^\$\(OUT_DIR\)/fec_wide_table\.o [^:]*: (.*)$", mk, re.M).group(1).split()
    assert {"fec_mask_wide.hpp", "fec_wide_head.hpp", "fec_scatter_decode.hpp", "fec_scatter_cut.hpp", "fec_varlen.hpp"} <= set(deps)
    sys.path.insert(0, str(CSRC))
    import src_hash
    assert {"fec_wide_table.hip", "fec_wide_head.hpp", "fec_scatter_decode.hpp"} <= {p.name for p in src_hash.source_files()}


# ------------------------------------------------------------------------------------------
# 2. Workspace and chunking
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wide_table")


def _stride(k, r):
    return 512 + min(k, r) * k * 32


def _cases():
    out = []
    for k, r in SHAPES:
        s = _stride(k, r)
        for budget in (0, s, s - 1):
            for G in GROUPS:
                for own_masks in (0, 1):
                    for own_symlen in (0, 1):
                        out.append((budget, G, k, r, own_masks, own_symlen))
    return out


def _expected(budget, G, k, r, own_masks, own_symlen):
    s = _stride(k, r)
    per = min(G, max(1, (budget or ARENA) // s))
    masks = 4 * G + 7 & ~7
    symlen = masks + (32 * G if own_masks else 0)
    arena = symlen + (4 * G if own_symlen else 0) + 255 & ~255
    return (f"per_chunk={per} stride={s} rec_off=0 masks={masks} symlen={symlen} arena={arena} bytes={arena + per * s} "
            f"chunks={-(-G // per)} passes={-(-min(k, r) // 8)}")


def test_workspace_and_chunks_plain_and_under_sanitizers(work_dir):
    """G record offsets, G x 32 B of masks when the caller gives none, G u32 when lengths are given but
    no output for L_g, then the arena, 256-B aligned: the four combinations, G in {1, 5, 67, 2^32 - 1},
    five shapes, the default budget, one stride and one stride minus one (one group per chunk)."""
    src = TESTS_CSRC / "wide_table_forms_test.cpp"
    cases = _cases()
    args = ["--workspace", *[str(x) for c in cases for x in c]]
    extra = [CSRC / "fec_knobs.cpp"]
    plain, err = _run(_build(work_dir, "wide_table_plain", src, [], extra), *args)
    assert plain[-1] == "ok", (plain[-3:], err)
    sanitized, err = _run(_build(work_dir, "wide_table_sanitized", src, SANITIZE, extra), *args)
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    assert len(plain) == len(cases) + 1
    for c, ln in zip(cases, plain):
        assert ln == _expected(*c), c
    # one stride holds one group per chunk, and so does one stride minus one; the default holds 291 of 224+32
    s = _stride(224, 32)
    assert plain[cases.index((s, 67, 224, 32, 1, 1))].startswith(f"per_chunk=1 stride={s} ")
    assert plain[cases.index((s - 1, 67, 224, 32, 1, 1))].startswith(f"per_chunk=1 stride={s} ")
    assert plain[cases.index((0, 2**32 - 1, 224, 32, 1, 1))].startswith(f"per_chunk={ARENA // s} stride={s} ")
    assert ARENA // s == 291


def test_wide_served_is_the_rule_of_the_call(work_dir):
    """What the call refuses is what wide_served refuses: the shim asks it and nothing else."""
    exe = _build(work_dir, "wide_table_served", TESTS_CSRC / "wide_table_forms_test.cpp", SANITIZE, [CSRC / "fec_knobs.cpp"])
    cases = [((67, k, r, 16), SERVED) for k, r in SHAPES + [(10, 3), (20, 5), (32, 32), (100, 20), (64, 2), (127, 3), (190, 5)]]
    cases += [((2**32 - 1, 224, 32, 1200), SERVED), ((67, 0, 5, 16), SHAPE), ((67, 5, 0, 16), SHAPE), ((67, 200, 57, 16), SHAPE),
              ((67, 33, 33, 16), ROWS), ((67, 60, 5, 15), PACKET), ((0, 60, 5, 16), NO_GROUPS), ((2**32, 60, 5, 16), TOO_MANY)]
    lines, err = _run(exe, *[str(x) for c, _ in cases for x in c])
    assert lines[-1] == "ok" and "runtime error" not in err, (lines, err)
    assert [int(ln.split("=")[1]) for ln in lines[:-1]] == [why for _, why in cases]
    shim = (CSRC / "fec_shim.cpp").read_text()
    body = shim[shim.index("QFEC_EXPORT int fec_recover_scatter_wide_rs_dev"):]
    body = body[:body.index("\n}\n")]
    assert "wide_refused(what, G, k, r, P)" in body and "check_gather_shape" not in body
    assert shim.count("qfec::wide_served(") == 1
