"""Which way a host-memory call goes (csrc/fec_routes.hpp), without a GPU: the stand-alone program
tests/csrc/routes_dump.cpp prints what the header decides over a grid of pointer classes, sizes and
limit overrides, and every line is compared with the rule as DESIGN.md §8 states it, written out
here a second time.  The host's classify rule of an erasure mask against a numpy statement of it,
the pipeline's chunk size and the window of a call's packet offsets likewise.  The program runs
plain and with AddressSanitizer + UBSan linked in statically; both must print the same.
"""
import itertools

import numpy as np
import pytest

from forms_support import SANITIZE, TESTS_CSRC, _build, _run

SRC = TESTS_CSRC / "routes_dump.cpp"
CLASSES = "HPD"                                     # pageable host, page-locked host, device
MIB = 1 << 20
UNLIMITED = (1 << 64) - 1
STAGED_LIMIT = 2 * MIB                              # "up to 2 MiB staged"
HUGE = 10 ** 12
OVERRIDES = [-1, 0, HUGE]                           # QUICFEC_SMALL_CALL_BYTES: unset, 0, huge
SIZES = [0, 1, STAGED_LIMIT - 1, STAGED_LIMIT, STAGED_LIMIT + 1, HUGE - 1, HUGE, HUGE + 1, UNLIMITED - 1, UNLIMITED]
G = 100
NEEDS = [0, G // 2, G // 2 + 1]
MASK_SHAPES = [(10, 3), (20, 5), (4, 2), (1, 1), (1, 63), (63, 1), (32, 32)]


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("host_routes")
    return d, _build(d, "routes_plain", SRC, []), _build(d, "routes_sanitized", SRC, SANITIZE)


def _both(exes, *args):
    """The program's lines, the same from the plain and the sanitized build, no sanitizer report."""
    _, plain, sanitized = exes
    lines, _ = _run(plain, *args)
    again, err = _run(sanitized, *args)
    assert again == lines
    assert "runtime error" not in err and "AddressSanitizer" not in err, err[-2000:]
    return lines


# ------------------------------------------------------------------------------------------
# The rule of DESIGN.md §8, stated here on its own
# ------------------------------------------------------------------------------------------
def _limit(override, all_pinned):
    """Zero-copy up to: the override when set; else no limit for page-locked buffers, 2 MiB staged."""
    return override if override >= 0 else UNLIMITED if all_pinned else STAGED_LIMIT


def encode_expected(data, out, off, override, nbytes):
    if off or "D" in (data, out):
        return "staged"
    return "zero_copy" if nbytes <= _limit(override, data == out == "P") else "pipelined"


def decode_expected(data, parity, masks, status, override, nbytes, need):
    if "D" in (data, parity, masks, status):
        return "staged"
    small = nbytes <= _limit(override, data == parity == "P")
    few = 2 * need <= G                             # at most half the groups need a rebuild
    if not (small or few):
        return "pipelined"
    return "nothing" if need == 0 else "zero_copy" if small else "compacted"


def legacy_expected(slab, out, override, nbytes, span):
    """(route, window rebased)."""
    if slab == "D":
        return "staged", 0
    lim = _limit(override, slab == out == "P")
    if out != "D" and nbytes <= lim and (slab == "P" or span <= lim):
        return "zero_copy", int(slab != "P")
    return "staged", 1


def test_limits_are_the_documented_ones(exes):
    consts = dict(ln.split() for ln in _both(exes, "consts"))
    assert {k: int(v) for k, v in consts.items()} == {
        "zero_copy_pinned_bytes": UNLIMITED, "zero_copy_staged_bytes": STAGED_LIMIT, "compact_max_share": 2,
        "pipe_chunk_bytes": 64 * MIB, "pipe_slots": 3}


def test_encode_routes_equal_the_table(exes):
    lines = _both(exes, "encode")
    want = [f"encode data={d} out={o} off={off} limit={ov} bytes={b} | {encode_expected(d, o, off, ov, b)}"
            for d in CLASSES for o in CLASSES for off in (0, 1) for ov in OVERRIDES for b in SIZES]
    assert lines == want
    assert {ln.split(" | ")[1] for ln in lines} == {"zero_copy", "pipelined", "staged"}
    # the edges: a staged call flips just over 2 MiB, a page-locked one never, override 0 at the first byte
    assert "encode data=H out=P off=0 limit=-1 bytes=2097152 | zero_copy" in lines
    assert "encode data=H out=P off=0 limit=-1 bytes=2097153 | pipelined" in lines
    assert f"encode data=P out=P off=0 limit=-1 bytes={UNLIMITED} | zero_copy" in lines
    assert "encode data=P out=P off=0 limit=0 bytes=0 | zero_copy" in lines
    assert "encode data=P out=P off=0 limit=0 bytes=1 | pipelined" in lines


def test_decode_routes_equal_the_table(exes):
    lines = _both(exes, "decode")
    want = [f"decode data={d} parity={p} masks={m} status={s} limit={ov} bytes={b} need={n} | "
            f"{decode_expected(d, p, m, s, ov, b, n)}"
            for d in CLASSES for p in CLASSES for m in CLASSES for s in CLASSES for ov in OVERRIDES for b in SIZES
            for n in NEEDS]
    assert lines == want
    assert {ln.split(" | ")[1] for ln in lines} == {"nothing", "zero_copy", "compacted", "pipelined", "staged"}
    big = "decode data=H parity=H masks=H status=H limit=0 bytes=2097153"
    assert [ln.split(" | ")[1] for ln in lines if ln.startswith(big)] == ["nothing", "compacted", "pipelined"]


def test_legacy_routes_equal_the_table(exes):
    lines = _both(exes, "legacy")
    want = []
    for sl, o, ov, b, span in itertools.product(CLASSES, CLASSES, OVERRIDES, SIZES, SIZES):
        route, rebase = legacy_expected(sl, o, ov, b, span)
        want.append(f"legacy slab={sl} out={o} limit={ov} bytes={b} span={span} | {route} rebase={rebase}")
    assert lines == want
    assert {ln.split(" | ")[1] for ln in lines} == {"zero_copy rebase=0", "zero_copy rebase=1", "staged rebase=0",
                                                     "staged rebase=1"}


# ------------------------------------------------------------------------------------------
# The host's classify rule
# ------------------------------------------------------------------------------------------
def _rule(masks, k, r):
    """e lost data shards, unrecoverable iff e > 0 and e > r - (lost parity rows); bits above k + r ignored."""
    bits = ((masks[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)
    e = bits[:, :k].sum(axis=1)
    alive = r - bits[:, k:k + r].sum(axis=1)
    return e, (e > 0) & (e > alive), bits[:, :k]


def _mask_of(positions):
    return np.uint64(sum(1 << int(p) for p in positions))


def _mask_cases():
    """(kind, k, r, mask): random masks of 0..r+1 lost shards; e == alive and e == alive + 1 for every e
    the shape allows; and, where k + r < 64, the same with bits set above k + r."""
    rng = np.random.default_rng(0x5EED0808)
    cases = []
    for k, r in MASK_SHAPES:
        for _ in range(300):
            t = int(rng.integers(0, r + 2))
            cases.append(("random", k, r, _mask_of(rng.choice(k + r, size=t, replace=False))))
        for e in range(1, min(k, r + 1) + 1):
            for dead, kind in ((r - e, "equal"), (r - e + 1, "over")):     # alive = r - dead
                if 0 <= dead <= r:
                    data = rng.choice(k, size=e, replace=False)
                    par = k + rng.choice(r, size=dead, replace=False)
                    cases.append((kind, k, r, _mask_of(np.concatenate([data, par]))))
        if k + r < 64:
            mine = [c for c in cases if c[1:3] == (k, r)]
            for kind, _, _, m in mine[:300:7] + mine[300:]:             # some random ones, every edge one
                junk = (int(rng.integers(0, 1 << 62)) << (k + r)) % (1 << 64) | (1 << 63)
                cases.append(("above_" + kind, k, r, np.uint64(int(m) | junk)))
    return cases


def test_mask_losses_equal_the_numpy_rule(exes):
    cases = _mask_cases()
    path = exes[0] / "masks.txt"
    path.write_text("".join(f"{k} {r} {int(m):x}\n" for _, k, r, m in cases))
    lines = _both(exes, "masks", str(path))
    assert len(lines) == len(cases)
    seen = {}
    for (kind, k, r, m), ln in zip(cases, lines):
        e, unrec, data_bits = _rule(np.array([m], dtype=np.uint64), k, r)
        shards = ",".join(str(j) for j in np.flatnonzero(data_bits[0]))
        assert ln == f"{k} {r} {int(m):x} | lost={e[0]} unrecoverable={int(unrec[0])} shards={shards}", (kind, ln)
        seen.setdefault(kind, []).append(bool(unrec[0]))
    # both branches: some random masks are unrecoverable, fewer than half
    assert 0 < sum(seen["random"]) < len(seen["random"]) / 2
    assert seen["equal"] and not any(seen["equal"])             # e == alive: recoverable
    assert seen["over"] and all(seen["over"])                   # e == alive + 1: not
    assert any(seen["above_random"]) and not all(seen["above_random"])
    assert seen["above_equal"] and not any(seen["above_equal"]) and all(seen["above_over"])


# ------------------------------------------------------------------------------------------
# Chunks and windows
# ------------------------------------------------------------------------------------------
def test_pipe_chunk_groups(exes):
    lines = _both(exes, "chunks")
    kinds = set()
    for ln in lines:
        query, got = ln.split(" | ")
        chunk, in_g, n = (int(f.split("=")[1]) for f in query.split())
        assert int(got) == min(max(chunk // in_g, 1), n), ln
        kinds.add("under_one_group" if chunk < in_g else "equal_n" if chunk // in_g == n else
                  "over_n" if chunk // in_g > n else "inside")
    assert kinds == {"under_one_group", "equal_n", "over_n", "inside"}
    assert "chunk=67 in_g=68 n=7 | 1" in lines and "chunk=476 in_g=68 n=7 | 7" in lines
    assert "chunk=67108864 in_g=12000 n=1000 | 1000" in lines and "chunk=24000 in_g=12000 n=1000 | 2" in lines


def test_offset_window(exes):
    cases = []
    for bits in (32, 64):
        top = 1 << bits
        cases += [(bits, 1200, [4800]),                                       # a single packet
                  (bits, 100, [900, 700, 500, 300, 107]),                     # descending
                  (bits, 17, [3, 3 + 17 * 5, 3 + 17 * 2]),
                  (bits, 1200, [top - 1200, 64, top - 2400]),                 # hi + P at the type's top
                  (bits, 16, [top - 16])]
    path = exes[0] / "windows.txt"
    path.write_text("".join(f"{bits} {P} {' '.join(map(str, offs))}\n" for bits, P, offs in cases))
    lines = _both(exes, "windows", str(path))
    want = []
    for bits, P, offs in cases:
        lo, hi = min(offs), max(offs)
        want.append(f"lo={lo} hi={hi} span={(hi + P - lo) % (1 << 64)} | " + " ".join(str(o - lo) for o in offs))
    assert lines == want
