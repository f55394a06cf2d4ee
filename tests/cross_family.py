"""What tests/test_gpu_cross_family.py and tests/test_cross_family_layout.py share, with no GPU and no
fixtures: the row type of the representative table, the build and parse of
tests/csrc/workspace_dump.cpp (how a call carves the caller stream's workspace, fec_shim.cpp
stream_workspace), the byte regions of a layout, which call the context's modes refuse, and the
seeded draw of test_random_sequences with the properties a block must hold.  A plain module, like
forms_support.py.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from forms_support import CSRC, TESTS_CSRC, _build, _run

PLAN_CODEBOOK, PLAN_DEVICE = 0, 1                    # include/fec_hip.h FEC_PLAN_*
ROWS_CAPPED, ROWS_ALL = 0, 1                         # include/fec_hip.h FEC_WIDE_ROWS_*
HINTS = (-1.0, 0.001, 0.5)                           # fec_decode_loss_hint: unknown, the scan form's share, above it

# One workspace-using call.  groups: its two cases' G, the table's first.  layout, own_masks,
# own_symlen: workspace_dump's query.  plan, rows: the mode the call needs to be served as the table
# says (None: either).
Rep = namedtuple("Rep", "id call k r P groups layout own_masks own_symlen plan rows")

ARENA_FAMILIES = {"plan": "plan", "wide": "wide", "wide_table": "wide", "deep": "deep", "deep_table": "deep"}


# ------------------------------------------------------------------------------------------
# Layouts
# ------------------------------------------------------------------------------------------
def build_dump(work_dir, flags=()):
    return _build(work_dir, "workspace_dump", TESTS_CSRC / "workspace_dump.cpp", list(flags), [CSRC / "fec_knobs.cpp"])


def dump_layouts(exe, queries):
    """queries: (name, rep, G, budget).  {name: layout} with the dump's columns as attributes."""
    args = []
    for name, rep, G, budget in queries:
        args += [name, rep.layout, rep.k, rep.r, G, int(rep.own_masks), int(rep.own_symlen), budget]
    lines, _ = _run(exe, *map(str, args))
    assert len(lines) == len(queries)
    out = {}
    for (name, rep, G, _), line in zip(queries, lines):
        head, *fields = line.split()
        assert head == name
        L = SimpleNamespace(rep=rep, **{f.split("=")[0]: int(f.split("=")[1]) for f in fields})
        assert L.G == G
        out[name] = L
    return out


def regions(L):
    """{region: (first byte, one past the last)} of a layout; a region the layout lacks is absent."""
    G, kind = L.G, L.rep.layout
    first = "block_sums" if kind == "prefix" else "rec_off"
    out = {first: (0, L.masks if kind == "prefix" else 4 * G)}
    if L.symlen > L.masks:
        out["masks"] = (L.masks, L.symlen)
    if kind == "offsets2" or (L.rep.own_symlen and kind in ("plan", "wide_table", "deep_table")):
        out["symlen"] = (L.symlen, L.symlen + 4 * G)                         # the arena behind it is 256-B aligned
    if L.bytes > L.arena:
        out["arena"] = (L.arena, L.bytes)
    for lo, hi in out.values():
        assert 0 <= lo < hi <= L.bytes
    return out


def overlap(a, b):
    return a is not None and b is not None and max(a[0], b[0]) < min(a[1], b[1])


# ------------------------------------------------------------------------------------------
# Modes
# ------------------------------------------------------------------------------------------
def refusal(rep, plan, rows):
    """The words of the refusal when a context in (plan, rows) is given rep's call, None when served."""
    if rep.layout in ("deep", "deep_table") and rows != ROWS_ALL:
        return "min(k, r)"
    if rep.id == "scatter_plan" and plan != PLAN_DEVICE:
        return "sparse-plan"
    return None


# ------------------------------------------------------------------------------------------
# The draw of test_random_sequences
# ------------------------------------------------------------------------------------------
CALLS_PER_BLOCK = 24
STREAMS = 3                                          # the context's own (NULL), side stream 1, side stream 2


def draw_block(seed, reps, encodes, cases_of):
    """24 calls: (switch or None, family, case, stream, the modes the call meets, refusal words or
    None).  A context starts in FEC_PLAN_CODEBOOK, FEC_WIDE_ROWS_CAPPED with no loss hint; a switch of a
    mode goes to the other mode, a switch of the hint to another of HINTS."""
    rng = np.random.default_rng(seed)
    by_id = {rep.id: rep for rep in reps}
    families = [rep.id for rep in reps] + list(encodes)
    plan, rows, hint = PLAN_CODEBOOK, ROWS_CAPPED, HINTS[0]
    seq = []
    for _ in range(CALLS_PER_BLOCK):
        switch = None
        if rng.integers(6) == 0:
            what = ("plan", "rows", "hint")[rng.integers(3)]
            if what == "plan":
                plan = PLAN_DEVICE if plan == PLAN_CODEBOOK else PLAN_CODEBOOK
                switch = ("plan", plan)
            elif what == "rows":
                rows = ROWS_ALL if rows == ROWS_CAPPED else ROWS_CAPPED
                switch = ("rows", rows)
            else:
                hint = [h for h in HINTS if h != hint][rng.integers(len(HINTS) - 1)]
                switch = ("hint", hint)
        family = families[rng.integers(len(families))]
        case = int(rng.integers(cases_of(family)))
        stream = int(rng.integers(STREAMS))
        refused = refusal(by_id[family], plan, rows) if family in by_id else None
        seq.append(SimpleNamespace(switch=switch, family=family, case=case, stream=stream, plan=plan, rows=rows,
                                   refused=refused))
    return seq


def block_problems(seq):
    """What a block lacks of: ten distinct families, both directions of each mode switch, an expected
    refusal, three calls on each stream.  Empty: the block holds."""
    problems = []
    if len({c.family for c in seq}) < 10:
        problems.append("fewer than ten families")
    switches = {c.switch for c in seq if c.switch and c.switch[0] != "hint"}
    for want in (("plan", PLAN_DEVICE), ("plan", PLAN_CODEBOOK), ("rows", ROWS_ALL), ("rows", ROWS_CAPPED)):
        if want not in switches:
            problems.append(f"no switch to {want}")
    if not any(c.refused for c in seq):
        problems.append("no refusal")
    for s in range(STREAMS):
        if sum(c.stream == s for c in seq) < 3:
            problems.append(f"fewer than three calls on stream {s}")
    return problems


def block_seed(base, block, reps, encodes, cases_of, tries=4096):
    """The first seed [base, block, n] whose draw holds: a property of the draw, found on the CPU."""
    for n in range(tries):
        seed = [base, block, n]
        if not block_problems(draw_block(seed, reps, encodes, cases_of)):
            return seed
    raise AssertionError(f"no block of {CALLS_PER_BLOCK} calls holds within {tries} seeds")
