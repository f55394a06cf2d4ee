"""The packed recovers for every shape (fec_recover_packed_rs_dev, fec_recover_packed_wide_rs_dev), no
GPU needed:
  * the calls' place in the header, the binding, both libraries, the Makefile, the source hash and
    the launch trace's names;
  * the route (csrc/fec_forms.hpp packed_route, packed_wide_route) and the workspace layout
    (packed_workspace over packed_arena) as a stand-alone program run plain and under
    AddressSanitizer + UBSan (tests/csrc/packed_any_forms_test.cpp).
"""
import re
import subprocess
import sys

import numpy as np
import pytest

from forms_support import CSRC, REPO, SANITIZE, TESTS_CSRC, _build, _run

CALLS = ("fec_recover_packed_rs_dev", "fec_recover_packed_wide_rs_dev")
# fec_forms.hpp PackedPath, PackedRefusal and the mode bits
REFUSED, EMPTY, DELEGATE, CODEBOOK, DEVICE_PLAN, WIDE, DEEP = range(7)
SERVED, SHAPE, ROWS, PACKET, NO_GROUPS, TOO_MANY, ROW_INDEX, NO_CODEBOOK = range(8)
PLAN_DEVICE, ROWS_ALL = 1, 4
ARENA = 64 << 20


# ------------------------------------------------------------------------------------------
# 1. Surface
# ------------------------------------------------------------------------------------------
def test_header_declares_both_calls_with_their_contracts():
    raw = (REPO / "include" / "fec_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    tail = (r"\s*uint64_t\s+num_groups,\s*uint32_t\s+k,\s*uint32_t\s+r,\s*uint32_t\s+packet_size,\s*uint8_t\*\s*d_rebuilt,"
            r"\s*uint32_t\*\s*d_row_start,\s*uint64_t\*\s*d_total,\s*uint8_t\*\s*d_status,\s*void\*\s*stream\s*\)\s*;")
    head = r"\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint8_t\*\s*d_data,\s*const uint8_t\*\s*d_parity,\s*const uint64_t\*\s*"
    assert re.search(r"\bint\s+fec_recover_packed_rs_dev" + head + r"d_masks," + tail, text)
    assert re.search(r"\bint\s+fec_recover_packed_wide_rs_dev" + head + r"d_erasure_masks\s*," + tail, text)
    # each section states the contract itself, not "as above"
    one = raw[raw.index("packed recover for every shape, one-word masks"):raw.index("int fec_recover_packed_rs_dev")]
    wide = raw[raw.index("packed recover for every shape, four-word masks"):raw.index("int fec_recover_packed_wide_rs_dev")]
    common = ("only read", "bits at and above", "rows_g", "sum of rows_h for h < g", "every group", "d_row_start[g] + m",
              "at\n *     or past total * packet_size", "d_total (nullable", "every byte written", "must not overlap",
              "NULL = the context's own stream", "fec_encoder_free", "no host synchronise and no readback", "ONE workspace",
              "block sums", "record offsets", "record arena", "stale", "launch nothing and write nothing", "FEC_ERR_NULL",
              "FEC_ERR_RANGE", "min(k, r) >= 2^32", "Zero pivot", "status 1", "unwritten")
    for section in (one, wide):
        assert "as above" not in section
        for words in common:
            assert words in section, words
    for words in ("fec_recover_batch_rs_dev", "k + r <= 64", "packet_size >= 16", "num_groups == 0 is served", "FEC_PLAN_DEVICE",
                  "FEC_PLAN_CODEBOOK", "never reads masks\n *     back", "fec_recover_gather_rs_dev", "byte for byte",
                  "fec_recover_batch_rs_dev_packed"):
        assert words in one, words
    for words in ("fec_recover_wide_rs_dev", "FEC_WIDE_MASK_WORDS", "k + r <= 256", "min(k, r) <= 32", "FEC_WIDE_ROWS_ALL",
                  "0 < num_groups < 2^32", "always built on the device", "k + r <= 64", "byte for byte", "whatever words 1..3 hold"):
        assert words in wide, words


def test_binding_and_both_libraries_have_the_calls(quicfec_mod):
    q = quicfec_mod
    assert set(CALLS) <= set(q.HIP_SYMBOLS)
    assert callable(q.Context.recover_packed_any_dev) and callable(q.Context.recover_packed_wide_dev)
    for lib in (q.LIB_PATH, q.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert set(CALLS) <= {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = open(lib, "rb").read()
        for name in q.PACKED_LAUNCH_FORMS.values():              # names live with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


def test_launch_ids_equal_the_binding(quicfec_mod):
    q = quicfec_mod
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class PackedLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == q.PACKED_LAUNCH_FORMS == {36: "rows_block_sums_wide", 37: "rows_write_wide", 38: "recover_packed",
                                                 39: "recover_packed_wide"}
    assert min(q.PACKED_LAUNCH_FORMS) == 36 == max(q.WIDE_DEEP_LAUNCH_FORMS) + 1
    others = [q.LAUNCH_FORMS, q.GATHER_LAUNCH_FORMS, q.GATHER_VAR_LAUNCH_FORMS, q.SCATTER_LAUNCH_FORMS,
              q.SCATTER_ENCODE_LAUNCH_FORMS, q.PLAN_LAUNCH_FORMS, q.WIDE_LAUNCH_FORMS, q.WIDE_TABLE_LAUNCH_FORMS,
              q.WIDE_ENCODE_LAUNCH_FORMS, q.WIDE_DEEP_LAUNCH_FORMS]
    for d in others:
        assert not set(d) & set(q.PACKED_LAUNCH_FORMS)
        assert not set(d.values()) & set(q.PACKED_LAUNCH_FORMS.values())


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_arguments_are_refused_without_a_gpu(quicfec_mod, which):
    """NULL checks come before any device call: each one names its argument and writes nothing."""
    q = quicfec_mod
    lib = q.load_library() if which == "product" else q.load_test_library()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    for call, masks in ((lib.fec_recover_packed_rs_dev, "d_masks"), (lib.fec_recover_packed_wide_rs_dev, "d_erasure_masks")):
        assert call(None, p, p, p, 1, 20, 5, 16, p, p, None, None, None) == q.FEC_ERR_NULL
        assert b"context" in lib.fec_hip_last_error()
    assert not buf.any()


def test_new_unit_is_built_and_hashed():
    mk = (CSRC / "Makefile").read_text()
    assert "fec_packed.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    dry = subprocess.run(["make", "-C", str(CSRC), "-n", "-B", "../lib/libfec_hip.so", "../lib/libfec_hip_test.so"],
                         capture_output=True, text=True, check=True).stdout
    links = [ln for ln in dry.splitlines() if " -shared " in ln]
    assert len(links) == 2 and all("../lib/fec_packed.o" in ln.split() for ln in links), links
    deps = re.search(r"^\$\(OUT_DIR\)/fec_packed\.o [^:]*: (.*)$", mk, re.M).group(1).split()
    assert {"fec_scan.hpp", "fec_mask_wide.hpp", "fec_wide_head.hpp"} <= set(deps)
    assert "fec_scan.hpp" in re.search(r"^\$\(OUT_DIR\)/fec_runs\.o [^:]*: (.*)$", mk, re.M).group(1).split()
    assert "fec_scan.hpp" in re.search(r"^PROBE_HDRS := (.*)$", mk, re.M).group(1).split()
    sys.path.insert(0, str(CSRC))
    import src_hash
    assert {"fec_packed.hip", "fec_scan.hpp"} <= {p.name for p in src_hash.source_files()}
    # loaded at its first call, like the other non-contiguous units
    kernels = (CSRC / "fec_kernels.hpp").read_text()
    assert "load_packed_unit" not in kernels


def test_the_shim_only_launches():
    """The path is packed_route's / packed_wide_route's; the shim asks them and nothing else."""
    shim = (CSRC / "fec_shim.cpp").read_text()
    for call, route in (("fec_recover_packed_rs_dev", "qfec::packed_route("), ("fec_recover_packed_wide_rs_dev", "qfec::packed_wide_route(")):
        body = shim[shim.index("QFEC_EXPORT int " + call):]
        body = body[:body.index("\n}\n")]
        assert route in body and "wide_served" not in body and "decode_form" not in body
    assert shim.count("qfec::packed_route(") == 1 and shim.count("qfec::packed_wide_route(") == 1
    # one workspace request for everything the new consumers keep there
    locked = shim[shim.index("int packed_call_locked("):]
    locked = locked[:locked.index("\n}\n")]
    assert locked.count("stream_workspace(") == 1 and "packed_workspace(" in locked


# ------------------------------------------------------------------------------------------
# 2. The stand-alone program
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("packed_any")
    src = TESTS_CSRC / "packed_any_forms_test.cpp"
    extra = [CSRC / "fec_knobs.cpp"]
    return _build(d, "packed_any_plain", src, [], extra), _build(d, "packed_any_sanitized", src, SANITIZE, extra)


def _both(programs, args):
    plain, err = _run(programs[0], *args)
    assert plain[-1] == "ok", (plain[-3:], err)
    sanitized, err = _run(programs[1], *args)
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    return plain[:-1]


def _routes(programs, cases):
    """cases: (wide, bits, G, k, r, P) -> [(path, why, passes, dense)]"""
    args = [str(x) for c in cases for x in ("route", *c)]
    lines = _both(programs, args)
    assert len(lines) == len(cases)
    return [tuple(int(f.split("=")[1]) for f in ln.split()) for ln in lines]


def test_what_the_old_call_serves_is_delegated(programs):
    """k=10 with r = 1, 2, 3 and k=4 r=2 at 256 < P <= 2047, k=10 r=2 also at 16..256: exactly these."""
    shapes = [(10, 3), (10, 1), (10, 2), (4, 2), (20, 5), (6, 3), (16, 16)]
    lines = _both(programs, [str(x) for k, r in shapes for x in ("delegates", k, r, 4200)])
    want = {(10, 3): "257-2047", (10, 1): "257-2047", (4, 2): "257-2047", (10, 2): "16-2047", (20, 5): "", (6, 3): "", (16, 16): ""}
    assert lines == ["delegates=" + want[s] for s in shapes]
    # and whatever the modes say
    got = _routes(programs, [(0, bits, 1031, k, r, P) for bits in (0, PLAN_DEVICE, ROWS_ALL, PLAN_DEVICE | ROWS_ALL)
                             for k, r, P in ((10, 3, 1200), (10, 2, 700), (4, 2, 513), (10, 2, 16), (10, 1, 2047))])
    assert all(g == (DELEGATE, SERVED, 0, 1) for g in got), got


def test_one_word_routes(programs):
    cases = [((0, 0, 1031, k, r, P), (CODEBOOK, SERVED, -(-min(k, r) // 8), 1))
             for k, r, P in ((20, 5, 1200), (10, 3, 200), (10, 3, 3000), (6, 3, 1200), (4, 2, 16), (10, 3, 1037), (10, 3, 2048),
                             (10, 3, 256), (7, 4, 16))]
    cases[5] = ((0, 0, 1031, 10, 3, 1037), (DELEGATE, SERVED, 0, 1))           # an odd size the old call serves
    for k, r, P in ((16, 16, 272), (60, 4, 48), (32, 8, 16)):
        cases.append(((0, 0, 1031, k, r, P), (REFUSED, NO_CODEBOOK, 0, 0)))
        cases.append(((0, ROWS_ALL, 1031, k, r, P), (REFUSED, NO_CODEBOOK, 0, 0)))
        cases.append(((0, PLAN_DEVICE, 1031, k, r, P), (DEVICE_PLAN, SERVED, -(-min(k, r) // 8), 0)))
    cases += [((0, PLAN_DEVICE, 1031, 20, 5, 1200), (CODEBOOK, SERVED, 1, 1)),     # a dense shape keeps its codebook
              ((0, 0, 0, 20, 5, 1200), (EMPTY, SERVED, 0, 1)), ((0, 0, 0, 16, 16, 16), (EMPTY, SERVED, 0, 0)),
              ((0, 0, 2**32 - 1, 20, 1, 16), (CODEBOOK, SERVED, 1, 1)),
              # refusals, in the order they are looked at
              ((0, 0, 1031, 20, 5, 15), (REFUSED, PACKET, 0, 1)), ((0, PLAN_DEVICE, 1031, 60, 5, 16), (REFUSED, SHAPE, 0, 0)),
              ((0, 0, 1031, 0, 5, 16), (REFUSED, SHAPE, 0, 0)), ((0, 0, 1031, 5, 0, 16), (REFUSED, SHAPE, 0, 0)),
              ((0, 0, 2**32, 20, 1, 16), (REFUSED, TOO_MANY, 0, 1)), ((0, 0, 2**30, 10, 4, 16), (REFUSED, ROW_INDEX, 0, 1)),
              ((0, 0, 2**30 - 1, 10, 4, 16), (CODEBOOK, SERVED, 1, 1)), ((0, 0, 2**31, 20, 2, 16), (REFUSED, ROW_INDEX, 0, 1)),
              ((0, 0, 0, 20, 5, 15), (REFUSED, PACKET, 0, 1))]
    got = _routes(programs, [c for c, _ in cases])
    assert got == [w for _, w in cases], [(c, g, w) for (c, w), g in zip(cases, got) if g != w]


def test_wide_routes(programs):
    cases = [((1, bits, 67, k, r, 16), (WIDE, SERVED, -(-min(k, r) // 8), 0))
             for bits in (0, ROWS_ALL, PLAN_DEVICE) for k, r in ((60, 5), (224, 32), (32, 224), (255, 1), (1, 255), (100, 20), (20, 5), (10, 3), (16, 16))]
    for k, r in ((40, 40), (33, 33), (128, 128)):
        cases.append(((1, 0, 13, k, r, 48), (REFUSED, ROWS, 0, 0)))
        cases.append(((1, PLAN_DEVICE, 13, k, r, 48), (REFUSED, ROWS, 0, 0)))
        cases.append(((1, ROWS_ALL, 13, k, r, 48), (DEEP, SERVED, -(-min(k, r) // 8), 0)))
    cases += [((1, ROWS_ALL, 67, 60, 5, 16), (WIDE, SERVED, 1, 0)),
              ((1, 0, 67, 60, 5, 15), (REFUSED, PACKET, 0, 0)), ((1, ROWS_ALL, 67, 40, 40, 15), (REFUSED, PACKET, 0, 0)),
              ((1, 0, 67, 200, 57, 16), (REFUSED, SHAPE, 0, 0)), ((1, ROWS_ALL, 67, 129, 128, 16), (REFUSED, SHAPE, 0, 0)),
              ((1, 0, 67, 0, 5, 16), (REFUSED, SHAPE, 0, 0)), ((1, 0, 0, 60, 5, 16), (REFUSED, NO_GROUPS, 0, 0)),
              ((1, 0, 2**32, 60, 5, 16), (REFUSED, TOO_MANY, 0, 0)), ((1, 0, 2**31, 60, 2, 16), (REFUSED, ROW_INDEX, 0, 0)),
              ((1, 0, 2**31 - 1, 60, 2, 16), (WIDE, SERVED, 1, 0)), ((1, ROWS_ALL, 2**26, 64, 64, 16), (REFUSED, ROW_INDEX, 0, 0)),
              ((1, 0, 2**32 - 1, 255, 1, 16), (WIDE, SERVED, 1, 0))]
    got = _routes(programs, [c for c, _ in cases])
    assert got == [w for _, w in cases], [(c, g, w) for (c, w), g in zip(cases, got) if g != w]


def _stride(path, k, r):
    return (128 if path == DEVICE_PLAN else 512) + min(k, r) * k * 32


def test_workspace_layout(programs):
    """Block sums (one u32 per 1024 groups), G record offsets, the arena: disjoint, the u32 arrays 8-B
    and the arena 256-B aligned, the total the sum; G in {1, 1025, 2^32 - 1}, with and without an arena."""
    cases = [(path, G, k, r, budget) for path, k, r in ((CODEBOOK, 20, 5), (DEVICE_PLAN, 16, 16), (DEVICE_PLAN, 60, 4), (WIDE, 224, 32),
                                                        (WIDE, 20, 5), (DEEP, 40, 40), (DEEP, 128, 128))
             for G in (1, 1025, 2**32 - 1) for budget in (0, 1)]
    lines = _both(programs, [str(x) for c in cases for x in ("workspace", *c)])
    assert len(lines) == len(cases)
    for (path, G, k, r, budget), ln in zip(cases, lines):
        got = {f.split("=")[0]: int(f.split("=")[1]) for f in ln.split()}
        blocks = -(-G // 1024)
        rec_off = 4 * blocks + 7 & ~7
        arena = rec_off + 4 * G + 255 & ~255
        if path == CODEBOOK:
            per, stride = 0, 0
        else:
            stride = _stride(path, k, r)
            per = min(G, max(1, (budget if budget else ARENA) // stride))
        assert got == dict(block_sums=0, rec_off=rec_off, arena=arena, bytes=arena + per * stride, per_chunk=per, stride=stride), (path, G, k, r)
    # G = 1025 takes two block sums, so the record offsets start at byte 8; one block leaves 4 B of padding
    assert "rec_off=8 " in lines[cases.index((CODEBOOK, 1025, 20, 5, 0))] and "rec_off=8 " in lines[cases.index((CODEBOOK, 1, 20, 5, 0))]
