"""The wide calls (k + r <= 256, four mask words per group), no GPU needed:
  * the numpy restatement of the wide rule (tests/wide_masks.py) against a plain per-bit loop, and
    against unread_shards.roles on word 0 for k + r <= 64;
  * csrc/fec_mask_wide.hpp against a per-bit loop and csrc/fec_plan_build_wide.hpp against
    build_record and against the definition of a recovery record, as stand-alone programs run plain
    and under AddressSanitizer + UBSan (tests/csrc/mask_wide_test.cpp, plan_build_wide_test.cpp);
  * the served-shape rule and the arena sizes of csrc/fec_forms.hpp (tests/csrc/wide_forms_test.cpp);
  * the calls' place in the header, the binding, both libraries and the launch trace's names.
"""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import unread_shards as us
import wide_masks as wm
from forms_support import CSRC, REPO, SANITIZE, TESTS_CSRC, _build, _run

WIDE_SHAPES = [(60, 5), (64, 2), (65, 3), (127, 3), (190, 5), (224, 32), (32, 224), (255, 1), (1, 255), (100, 20)]
NARROW_SHAPES = [(10, 3), (16, 16), (32, 32), (60, 4)]
ARENA = 64 << 20
SERVED, SHAPE, ROWS, PACKET, NO_GROUPS, GROUPS = range(6)          # fec_forms.hpp WideRefusal


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wide")


def _drawn(G, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, np.iinfo(np.uint64).max, size=(G, 4), dtype=np.uint64, endpoint=True)
    m[::3] &= rng.integers(0, np.iinfo(np.uint64).max, size=m[::3].shape, dtype=np.uint64, endpoint=True)
    m[::3] &= rng.integers(0, np.iinfo(np.uint64).max, size=m[::3].shape, dtype=np.uint64, endpoint=True)
    m[0], m[1] = 0, np.iinfo(np.uint64).max
    return m


# ------------------------------------------------------------------------------------------
# 1. The numpy rule
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", WIDE_SHAPES + NARROW_SHAPES)
def test_numpy_rule_equals_a_per_bit_loop(k, r):
    masks = _drawn(60, [k, r])
    ro = wm.roles(masks, k, r)
    for g, words in enumerate(masks):
        bit = lambda s: (int(words[s // 64]) >> (s % 64)) & 1
        lost_d = [bit(j) == 1 for j in range(k)]
        lost_p = [bit(k + i) == 1 for i in range(r)]
        e, alive = sum(lost_d), [i for i in range(r) if not lost_p[i]]
        ok = e <= len(alive)
        chosen = set(alive[:e]) if ok else set()
        assert ro.lost_d[g].tolist() == lost_d and ro.lost_p[g].tolist() == lost_p and bool(ro.ok[g]) == ok
        assert set(np.flatnonzero(ro.chosen[g]).tolist()) == chosen
        assert np.array_equal(ro.unread_p[g], ~ro.chosen[g])
    assert np.array_equal(wm.from_bits(wm.to_bits(masks)), masks)
    junked = wm.with_high_junk(masks, k, r, 7)
    top = -(-(k + r) // 64) * 64
    assert wm.to_bits(junked)[:, top:].all() and np.array_equal(wm.to_bits(junked)[:, :k + r], wm.to_bits(masks)[:, :k + r])
    if top > k + r:
        assert wm.to_bits(junked)[:, k + r:top].any() and not wm.to_bits(junked)[:, k + r:top].all()


@pytest.mark.parametrize("k,r", NARROW_SHAPES)
def test_numpy_rule_equals_the_one_word_rule_on_word_0(k, r):
    """k + r <= 64: unread_shards.roles of word 0, whatever words 1..3 hold."""
    masks = _drawn(200, [k, r, 1])
    a, b = wm.roles(masks, k, r), us.roles(masks[:, 0], k, r)
    for f in ("lost_d", "lost_p", "chosen", "unread_p", "ok"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (masks[:, 1:] != 0).any()


# ------------------------------------------------------------------------------------------
# 2. The C++ rule and the record builder
# ------------------------------------------------------------------------------------------
def _plain_and_sanitized(work_dir, name):
    src = TESTS_CSRC / f"{name}.cpp"
    plain, err = _run(_build(work_dir, f"{name}_plain", src, []))
    assert plain[-1] == "ok", (plain, err)
    sanitized, err = _run(_build(work_dir, f"{name}_sanitized", src, SANITIZE))
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    return {ln.split()[0]: int(ln.split()[1]) for ln in plain[:-1]}


def test_mask_rule_plain_and_under_sanitizers(work_dir):
    """Every function of fec_mask_wide.hpp against a per-bit loop, every shift 0..255, and fec_mask.hpp
    for 10+3 and 32+32; no report under AddressSanitizer and UBSan (a shift by 64 would be one)."""
    counts = _plain_and_sanitized(work_dir, "mask_wide_test")
    shapes = [(60, 5), (64, 2), (65, 3), (127, 3), (190, 5), (224, 32), (32, 224), (255, 1), (1, 255), (10, 3), (32, 32)]
    assert set(counts) == {f"{k}+{r}" for k, r in shapes}
    assert all(n >= 300 for n in counts.values())


def test_records_plain_and_under_sanitizers(work_dir):
    """The wide builder's records in heap blocks of exactly their size: equal to build_record's ids and
    tables for k + r <= 64, and rebuilding the erased shards by the definition for every wide shape."""
    counts = _plain_and_sanitized(work_dir, "plan_build_wide_test")
    every = 0
    for k, r in [(4, 2), (10, 3)]:
        n = 0
        for m in range(1 << (k + r)):
            e, lost_rows = bin(m & ((1 << k) - 1)).count("1"), bin(m >> k).count("1")
            n += 1 <= e <= r - lost_rows
        assert counts[f"{k}+{r}"] == n
        every += n
    assert every > 0 and counts["16+16"] >= 1500 and counts["32+32"] >= 1500
    for k, r in WIDE_SHAPES:
        assert counts[f"{k}+{r}"] >= 502, (k, r)


# ------------------------------------------------------------------------------------------
# 3. Served shapes and sizes
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forms_exe(work_dir):
    return _build(work_dir, "wide_forms", TESTS_CSRC / "wide_forms_test.cpp", SANITIZE, [CSRC / "fec_knobs.cpp"])


def _served(forms_exe, cases):
    lines, err = _run(forms_exe, *[str(x) for c in cases for x in c])
    assert lines[-1] == "ok" and "runtime error" not in err, (lines, err)
    return [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in ln.split()} for ln in lines[:-1]]


def test_served_shape_rule(forms_exe):
    """k >= 1, r >= 1, k + r <= 256, min(k, r) <= 32, P >= 16, 0 < G < 2^32; the header is 512 B."""
    ok = [(67, k, r, 16) for k, r in WIDE_SHAPES + NARROW_SHAPES] + [(2**32 - 1, 223, 32, 1200), (1, 1, 1, 16), (1, 32, 32, 9000)]
    got = _served(forms_exe, ok)
    for (G, k, r, P), row in zip(ok, got):
        assert row == {"served": SERVED, "stride": 512 + min(k, r) * k * 32, "passes": -(-min(k, r) // 8)}, (G, k, r, P)
    bad = [((67, 200, 57, 16), SHAPE), ((67, 33, 33, 16), ROWS), ((67, 100, 100, 16), ROWS), ((67, 60, 5, 15), PACKET),
           ((0, 60, 5, 16), NO_GROUPS), ((2**32, 60, 5, 16), GROUPS), ((67, 0, 5, 16), SHAPE), ((67, 5, 0, 16), SHAPE),
           ((67, 256, 1, 16), SHAPE), ((67, 128, 128, 16), ROWS)]
    got = _served(forms_exe, [c for c, _ in bad])
    assert [row["served"] for row in got] == [why for _, why in bad]


def test_arena_sizes(forms_exe):
    """wide_slot_stride(k, r) = 512 + min(k, r) * k * 32; per_chunk = min(G, max(1, budget // stride)):
    291 slots at 224 + 32 under the 64 MiB budget, one slot when the budget is below a stride; the
    workspace is G record offsets, then the arena, 256-B aligned."""
    cases = []
    for k, r in WIDE_SHAPES + NARROW_SHAPES:
        s = 512 + min(k, r) * k * 32
        for budget in (0, s - 1, s, 5 * s, 5 * s + 1):
            for G in (1, 5, 67, 2**32 - 1):
                cases.append((budget, G, k, r))
    lines, err = _run(forms_exe, "--arena", *[str(x) for c in cases for x in c])
    assert lines[-1] == "ok" and "runtime error" not in err, (lines[-3:], err)
    for (budget, G, k, r), ln in zip(cases, lines[:-1]):
        s = 512 + min(k, r) * k * 32
        per = min(G, max(1, (budget or ARENA) // s))
        at = (4 * G + 7 & ~7) + 255 & ~255
        assert ln == f"per_chunk={per} arena={per * s} rec_off=0 arena_at={at} bytes={at + per * s}", (budget, G, k, r)
    s = 512 + 32 * 224 * 32
    assert s == 229888 and ARENA // s == 291
    assert f"per_chunk=291 arena={291 * s} " in lines[cases.index((0, 2**32 - 1, 224, 32))]
    assert lines[cases.index((s - 1, 67, 224, 32))].startswith(f"per_chunk=1 arena={s} ")
    assert re.search(r"constexpr uint64_t kPlanArenaBytes = 64ull << 20;", (CSRC / "fec_forms.hpp").read_text())
    assert ARENA // 32 < 0xFFFFFFFE and s // 32 < 0xFFFFFFFE     # every record offset is below the markers


# ------------------------------------------------------------------------------------------
# 4. Surface
# ------------------------------------------------------------------------------------------
WIDE_CALLS = ("fec_decode_wide_rs_dev", "fec_recover_wide_rs_dev")


def test_header_declares_the_wide_calls():
    raw = (REPO / "include" / "fec_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"^#define FEC_WIDE_MASK_WORDS 4\s*$", text, re.M)
    assert re.search(r"\bint\s+fec_decode_wide_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*uint8_t\*\s*d_data,\s*const uint8_t\*\s*d_parity,"
                     r"\s*const uint64_t\*\s*d_erasure_masks,\s*uint64_t\s+num_groups,\s*uint32_t\s+k,\s*uint32_t\s+r,"
                     r"\s*uint32_t\s+packet_size,\s*uint8_t\*\s*d_status,\s*void\*\s*stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+fec_recover_wide_rs_dev\s*\(\s*FECEncoderCtx\*\s*ctx,\s*const uint8_t\*\s*d_data,\s*const uint8_t\*\s*d_parity,"
                     r"\s*const uint64_t\*\s*d_erasure_masks,\s*uint64_t\s+num_groups,\s*uint32_t\s+k,\s*uint32_t\s+r,"
                     r"\s*uint32_t\s+packet_size,\s*uint8_t\*\s*d_rebuilt,\s*uint8_t\*\s*d_status,\s*void\*\s*stream\s*\)\s*;", text)
    assert "Decode requires k + r <= 64" not in raw
    assert "min(k, r) <= 32" in raw and "160 KiB" in raw


def test_binding_and_both_libraries_have_the_wide_calls(quicfec_mod):
    assert set(WIDE_CALLS) <= set(quicfec_mod.HIP_SYMBOLS)
    assert callable(quicfec_mod.Context.decode_wide_dev) and callable(quicfec_mod.Context.recover_wide_dev)
    assert quicfec_mod.WIDE_MASK_WORDS == 4
    for lib in (quicfec_mod.LIB_PATH, quicfec_mod.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
        assert set(WIDE_CALLS) <= {ln.split()[-1] for ln in out.splitlines() if " T " in ln}, lib
        blob = Path(lib).read_bytes()
        for name in quicfec_mod.WIDE_LAUNCH_FORMS.values():          # names live with the reader, in neither library
            assert (name + "\0").encode() not in blob, (lib, name)


def test_wide_launch_ids_equal_the_binding(quicfec_mod):
    hpp = (CSRC / "fec_knobs.hpp").read_text()
    enum = re.search(r"enum class WideLaunchForm : int64_t \{(.*?)\};", hpp, re.S).group(1)
    text_ids = {int(m.group(2)): re.sub(r"(?<!^)(?=[A-Z])", "_", m.group(1)).lower()
                for m in re.finditer(r"^\s*k(\w+) = (\d+),", enum, re.M)}
    assert text_ids == quicfec_mod.WIDE_LAUNCH_FORMS == {27: "classify_wide", 28: "build_records_wide", 29: "decode_wide"}
    assert min(quicfec_mod.WIDE_LAUNCH_FORMS) == max(quicfec_mod.PLAN_LAUNCH_FORMS) + 1


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_null_context_is_refused_without_a_gpu(quicfec_mod, which):
    lib = quicfec_mod.load_library() if which == "product" else quicfec_mod.load_test_library()
    buf = np.zeros(64, dtype=np.uint8)
    p = buf.ctypes.data
    assert lib.fec_decode_wide_rs_dev(None, p, p, p, 1, 60, 5, 16, None, None) == quicfec_mod.FEC_ERR_NULL
    assert lib.fec_recover_wide_rs_dev(None, p, p, p, 1, 60, 5, 16, p, None, None) == quicfec_mod.FEC_ERR_NULL
    assert b"context" in lib.fec_hip_last_error()


def test_new_unit_is_built_and_hashed():
    mk = (CSRC / "Makefile").read_text()
    assert "fec_wide.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    dry = subprocess.run(["make", "-C", str(CSRC), "-n", "-B", "../lib/libfec_hip.so", "../lib/libfec_hip_test.so"],
                         capture_output=True, text=True, check=True).stdout
    links = [ln for ln in dry.splitlines() if " -shared " in ln]
    assert len(links) == 2 and all("../lib/fec_wide.o" in ln.split() for ln in links), links
    import sys
    sys.path.insert(0, str(CSRC))
    import src_hash
    assert {"fec_wide.hip", "fec_mask_wide.hpp", "fec_plan_build_wide.hpp"} <= {p.name for p in src_hash.source_files()}
