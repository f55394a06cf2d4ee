"""The layouts tests/test_gpu_cross_family.py relies on, checked with no GPU: its table of
representatives through tests/csrc/workspace_dump.cpp (fec_forms.hpp's workspace arithmetic, built
with AddressSanitizer and UBSan as a stand-alone program), and its seeded draw.

A caller stream has one workspace buffer that every call carves in its own way and nobody clears
(csrc/fec_shim.cpp stream_workspace).  The GPU tests queue A, then B, then A at its other G on one
stream, for every ordered pair of the table; here the table is shown to really put one family's
regions over another's.  If someone changes a shape and a property is lost, this fails on the CPU.
"""
import re

import pytest

import cross_family as xf
import test_gpu_cross_family as xg
from forms_support import CSRC, SANITIZE

REPS = xg.REPRESENTATIVES


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return xf.build_dump(tmp_path_factory.mktemp("cross_family"), SANITIZE)


@pytest.fixture(scope="module")
def layouts(dump):
    """{(id, case index): layout} at the product library's arena budget."""
    queries = [(f"{rep.id}@{i}", rep, G, 0) for rep in REPS for i, G in enumerate(rep.groups)]
    got = xf.dump_layouts(dump, queries)
    return {(rep.id, i): got[f"{rep.id}@{i}"] for rep in REPS for i in range(len(rep.groups))}


def sequences(layouts):
    """(A, B, the layouts of A, B, A at its other G) for every ordered pair, A itself included."""
    for A in REPS:
        for B in REPS:
            yield A, B, [layouts[A.id, 0], layouts[B.id, 0], layouts[A.id, 1]]


def transitions(layouts):
    """(the representative and layout of a call, those of the call queued right behind it) over every
    sequence: A then B, and B then A at its other G."""
    for A, B, (a, b, a2) in sequences(layouts):
        yield A, a, B, b
        yield B, b, A, a2


def test_the_table_is_the_issues(layouts):
    """Twelve rows, two different G each, and the strides and sizes the table names."""
    assert [rep.id for rep in REPS] == ["prefix", "tiled", "book_slots", "plan_dev", "plan_host", "gather", "scatter_own",
                                        "scatter_plan", "wide", "wide_table", "deep", "deep_table"]
    for rep in REPS:
        assert len(rep.groups) == 2 and rep.groups[0] != rep.groups[1] and min(rep.groups) >= 3
        assert rep.groups[1] in (131, 67) or 3 <= rep.groups[1] <= 9
    assert [xg.BY_ID[i].groups[0] for i in ("prefix", "tiled", "book_slots", "deep_table")] == [3000, 1031, 261, 9]
    assert all(rep.groups[0] == 67 for rep in REPS if rep.id not in ("prefix", "tiled", "book_slots", "deep_table"))
    assert layouts["plan_dev", 0].stride == 8320 and layouts["wide", 0].stride == 229888
    assert layouts["deep_table", 0].stride == 524800
    assert layouts["prefix", 0].bytes == 12 and layouts["tiled", 0].bytes == 4 * 1031
    assert layouts["scatter_own", 0].bytes == 2 * 4 * 67 and xf.regions(layouts["scatter_own", 0])["symlen"] == (268, 536)
    # at the product budget no representative is chunked: one arena slot per group
    for (name, i), L in layouts.items():
        assert L.per_chunk in (0, L.G), (name, i)
    # the largest upload of the address-table and wide rows: wide_table's shards, 67 x 120 x 1037 B
    assert max(max(rep.groups) * (rep.k + rep.r) * rep.P for rep in REPS if rep.groups[0] in (9, 67)) == 67 * 120 * 1037


def test_restated_sizes_are_still_the_sources():
    """workspace_dump.cpp restates three sizes that are not in a host-only header: the lines it names
    are still in fec_runs.hip and fec_shim.cpp."""
    runs = (CSRC / "fec_runs.hip").read_text()
    assert re.search(r"constexpr uint32_t kRowsPerThread = 4;", runs)
    assert re.search(r"constexpr uint32_t kRowsPerBlock = 256 \* kRowsPerThread;", runs)
    assert re.search(r"rows_prefix_workspace_bytes\(uint64_t groups\) \{\s*return \(\(groups \+ kRowsPerBlock - 1\) / "
                     r"kRowsPerBlock\) \* sizeof\(uint32_t\);", runs)
    shim = (CSRC / "fec_shim.cpp").read_text()
    assert "QFEC_HIP(stream_workspace(ctx, s, G * sizeof(uint32_t), &ws));" in shim
    assert "stream_workspace(ctx, s, ws_words * G * sizeof(uint32_t), &ws)" in shim
    assert "if (ws_words == 2) a.symlen = a.rec_off + G;" in shim
    assert "stream_workspace(ctx, s, qfec::rows_prefix_workspace_bytes(G), &ws)" in shim


def test_arenas_of_different_families_start_inside_each_other(layouts):
    """(i) For every ordered pair of distinct arena families among plan, wide and deep there are
    representatives A, B, B queued right behind A, with B's arena starting inside A's and another
    stride: B's records are built over A's, at other offsets."""
    found = set()
    for A, a, B, b in transitions(layouts):
        fa, fb = xf.ARENA_FAMILIES.get(A.layout), xf.ARENA_FAMILIES.get(B.layout)
        if fa and fb and fa != fb and a.arena <= b.arena < a.bytes and a.stride != b.stride:
            found.add((fa, fb))
    assert found == {(x, y) for x in ("plan", "wide", "deep") for y in ("plan", "wide", "deep") if x != y}


def test_masks_and_symbol_lengths_meet_arenas(layouts):
    """(ii) Calls B queued right behind A where B's masks, and where B's symbol lengths, lie wholly inside
    A's arena; and where B's arena lies over A's masks, for the 8-B masks of the plan layout and the 32-B
    masks of the wide table."""
    inside, over = set(), set()
    for A, a, B, b in transitions(layouts):
        ra, rb = xf.regions(a), xf.regions(b)
        for name in ("masks", "symlen"):
            if name in rb and "arena" in ra and ra["arena"][0] <= rb[name][0] and rb[name][1] <= ra["arena"][1]:
                inside.add((name, B.layout))
        if xf.overlap(rb.get("arena"), ra.get("masks")):
            over.add(A.layout)
    assert {("symlen", "plan"), ("symlen", "wide_table")} <= inside, inside
    assert any(name == "masks" for name, _ in inside), inside
    assert {"plan", "wide_table", "deep_table"} <= over, over


def test_record_offsets_meet_block_sums(layouts):
    """(iii) B's record offsets lie over A's block sums, and the reverse."""
    ab = ba = False
    for A, a, B, b in transitions(layouts):
        ra, rb = xf.regions(a), xf.regions(b)
        ab |= xf.overlap(rb.get("rec_off"), ra.get("block_sums"))
        ba |= xf.overlap(rb.get("block_sums"), ra.get("rec_off"))
    assert ab and ba


def test_every_sequence_grows_or_reuses(layouts):
    """(iv) In every A, B, A' a call needs more bytes than any before it on the sequence (the buffer
    grows: a stream synchronise and a new allocation under queued work) or fewer (a larger buffer,
    last laid out by another call, is reused); over the table both happen to every representative, and
    to every one but the smallest both happen behind another call."""
    grows, reuses, grows_later = set(), set(), set()
    for A, B, seq in sequences(layouts):
        events = 0
        for pos, (rep, L) in enumerate(zip((A, B, A), seq)):
            before = max([x.bytes for x in seq[:pos]], default=0)
            if L.bytes > before:
                grows.add(rep.id)
                if pos:
                    grows_later.add(rep.id)
            elif L.bytes < before:
                reuses.add(rep.id)
            events += L.bytes != before
        assert events >= 2, (A.id, B.id)                                       # the first call and one more
    ids = {rep.id for rep in REPS}
    assert grows == ids
    assert reuses == ids
    assert grows_later == ids - {"prefix"}                                    # nothing is smaller than the block sums


def test_small_arena_budgets_chunk_every_walk(dump):
    """(v) The budgets of test_small_arena_walks_across_families give 2 <= per_chunk < G for its six calls,
    at six different strides."""
    queries = [(family, xg.BY_ID[family], xg.BY_ID[family].groups[0], xg.arena_budget(xg.BY_ID[family], slots))
               for family, slots in xg.ARENA_WALK]
    got = xf.dump_layouts(dump, queries)
    assert [family for family, _ in xg.ARENA_WALK] == ["plan_dev", "scatter_plan", "wide", "wide_table", "deep", "deep_table"]
    for family, slots in xg.ARENA_WALK:
        L = got[family]
        assert L.per_chunk == slots and 2 <= L.per_chunk < L.G, family
        assert L.bytes - L.arena == slots * L.stride and xg.arena_budget(xg.BY_ID[family], slots) == slots * L.stride
        assert xg.BUILD_FORM[xg.BY_ID[family].layout].startswith("build_records")
    assert len({got[family].stride for family, _ in xg.ARENA_WALK}) == 6


def test_modes_refuse_what_the_shim_refuses():
    """cross_family.refusal against the rules it restates: the deep path needs FEC_WIDE_ROWS_ALL
    (fec_forms.hpp wide_route), a table recover of a shape past the codebook cap FEC_PLAN_DEVICE."""
    for rep in REPS:
        deep = min(rep.k, rep.r) > 32 and rep.k + rep.r > 64
        table_past_cap = rep.id == "scatter_plan"
        for plan in (xf.PLAN_CODEBOOK, xf.PLAN_DEVICE):
            for rows in (xf.ROWS_CAPPED, xf.ROWS_ALL):
                want = "min(k, r)" if deep and rows == xf.ROWS_CAPPED else \
                    "sparse-plan" if table_past_cap and plan == xf.PLAN_CODEBOOK else None
                assert xf.refusal(rep, plan, rows) == want, (rep.id, plan, rows)
        assert deep == (rep.rows == xf.ROWS_ALL), rep.id
    shim = (CSRC / "fec_shim.cpp").read_text()
    assert "sparse-plan shape" in shim and "min(k, r) exceeds" in shim


def test_random_blocks_hold_before_anything_is_launched():
    """The committed blocks of test_random_sequences: each holds at least ten distinct families, both
    directions of each mode switch, an expected refusal and three calls per stream; the draw is a
    function of its seed alone."""
    seeds = []
    for block in range(6):
        seed = xf.block_seed(xg.SEED, block, REPS, xg.ENCODES, xg.cases_of)
        seq = xf.draw_block(seed, REPS, xg.ENCODES, xg.cases_of)
        again = xf.draw_block(seed, REPS, xg.ENCODES, xg.cases_of)
        assert [vars(c) for c in seq] == [vars(c) for c in again]
        assert len(seq) == 24 and xf.block_problems(seq) == []
        assert len({c.family for c in seq}) >= 10
        assert sum(bool(c.refused) for c in seq) >= 1 and min(sum(c.stream == s for c in seq) for s in range(3)) >= 3
        for c in seq:                                                          # a refusal is what the modes of its moment say
            rep = xg.BY_ID.get(c.family)
            assert c.refused == (xf.refusal(rep, c.plan, c.rows) if rep else None)
        seeds.append(tuple(seed))
    assert len(set(seeds)) == 6
    # a block without a switch is told apart
    quiet = xf.draw_block([1, 2, 3], REPS[:3], (), xg.cases_of)
    assert xf.block_problems(quiet)
