"""The rule of an erasure mask (csrc/fec_mask.hpp), the one statement the kernels and the host both
call, against gf256.hpp's build_record / codebook_layout and the oracle's shard walk, no GPU needed:
a stand-alone program (tests/csrc/mask_rule_test.cpp) run plain and under AddressSanitizer + UBSan."""
import pytest

from forms_support import SANITIZE, TESTS_CSRC, _build, _run

MASK_KINDS = ("empty", "all_data", "no_parity", "xor", "single", "exact_rows", "skip_rows", "first_last", "bad",
              "picked", "placed")
EXHAUSTIVE = [(4, 2), (10, 1), (10, 2), (10, 3), (5, 5)]
DRAWN = [(20, 5), (60, 4), (32, 32), (63, 1)]


@pytest.fixture(scope="module")
def work_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("mask_rule")


def test_mask_rule_equals_build_record_plain_and_under_sanitizers(work_dir):
    """Every mask of the four mask-addressed shapes and of (5,5), 2,000 drawn masks (junk above k + r)
    of four large shapes, and the planted masks in all nine: losses, rows per group, the pick, the
    ranks and the record's place are the independent statements'.  Once plain, once with
    AddressSanitizer and UBSan linked in statically: the same lines and no report -- no path shifts
    by 64, (63,1) and (32,32) included.  Every kind of mask the rule has a case for was met."""
    src = TESTS_CSRC / "mask_rule_test.cpp"
    plain, err = _run(_build(work_dir, "rule_plain", src, []))
    assert plain[-1] == "ok", (plain, err)
    counts = {ln.split()[0]: int(ln.split()[1]) for ln in plain[:-1]}
    print(counts)
    assert set(counts) == set(MASK_KINDS)
    for kind in MASK_KINDS:
        assert counts[kind] > 0, kind
    # the exhaustive shapes alone: every mask with 1 <= e <= alive rows is picked and placed
    exhaustive = 0
    for k, r in EXHAUSTIVE:
        for m in range(1 << (k + r)):
            e, lost_rows = bin(m & ((1 << k) - 1)).count("1"), bin(m >> k).count("1")
            exhaustive += 1 <= e <= r - lost_rows
    assert counts["placed"] >= exhaustive
    assert counts["picked"] >= exhaustive + len(DRAWN) * 2000 // 4   # a quarter of the draws is always recoverable
    sanitized, err = _run(_build(work_dir, "rule_sanitized", src, SANITIZE))
    assert sanitized == plain
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
