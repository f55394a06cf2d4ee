"""fec_recover_packed_rs_dev and fec_recover_packed_wide_rs_dev on the GPU: the packed layout (the
rebuilt packets of all groups back to back, group g's rows from row_start[g]) for every shape a slot
recover serves.

Outputs are pre-filled with 0x5A, row starts and the total with junk, statuses with 7.  One-word
cases come from test_gpu_packed._case (the oracle's decode; junk in every shard the rule does not
read and in the mask bits at and above k + r), wide cases from test_gpu_wide.Case (the truth is the
original data; junk in the partial word above k + r, all ones in the whole words above).  Every case
runs once on the context's stream and once on a side stream and checks: the rows, the row starts
against a host prefix sum, the total, every status byte, data / parity / masks unchanged, and every
byte of d_rebuilt at and past total * P still 0x5A.
"""
import os
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import unread_shards as us
from test_gpu_gather import hooks_ctx, product_ctx
from test_gpu_packed import _case
from test_gpu_wide import SHAPES as WIDE_SHAPES
from test_gpu_wide import Case, main_case, planted_groups
from test_gpu_wide_deep import wide_case as deep_case

pytestmark = pytest.mark.gpu

SEED = 0x9AC4ED00
POL = 2 | 4 | 1024                                                             # fec_forms.hpp kPackedPol
G_WORD = 1031
G_EDGE = 2051                                                                  # three 1024-group blocks, G mod 4 = 3


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases: what a call is given and what it must leave
# ------------------------------------------------------------------------------------------
def _expect(k, r, P, d_in, p_in, masks, status, rows_per_group, rows, wide):
    G = len(status)
    start = np.concatenate([[0], np.cumsum(rows_per_group)[:-1]]).astype(np.uint32)
    assert len(rows) == int(np.sum(rows_per_group)) and G * min(k, r) < 2**32
    return SimpleNamespace(k=k, r=r, P=P, G=G, d_in=d_in, p_in=p_in, masks=masks, status=np.asarray(status, dtype=np.uint8),
                           start=start, per_group=np.asarray(rows_per_group, dtype=np.int64),
                           rows=np.ascontiguousarray(rows).reshape(-1, P), wide=wide)


def _from_word(oracle, k, r, P, masks, **need):
    broken, par_in, st_exp, start, exp, masks_in = _case(oracle, k, r, P, len(masks), masks, **need)
    lost = us.roles(masks, k, r).lost_d.sum(axis=1)
    x = _expect(k, r, P, broken, par_in, masks_in, st_exp, np.where(st_exp == 0, lost, 0), exp, False)
    assert np.array_equal(x.start, start)
    return x


def _from_wide(c):
    rows = [c.slots[g, :c.e[g]] for g in np.flatnonzero(c.rebuilds)]
    rows = np.concatenate(rows) if rows else np.zeros((0, c.P), dtype=np.uint8)
    return _expect(c.k, c.r, c.P, c.d_in, c.p_in, c.masks, c.status, np.where(c.rebuilds, c.e, 0), rows, True)


def drawn_masks(k, r, P, G=G_WORD):
    """As test_gpu_packed.test_packed_rows_match_oracle draws them: 0 .. r + 1 lost shards per group."""
    rng = np.random.default_rng(k * 1000 + r * 100 + P)
    masks = np.zeros(G, dtype=np.uint64)
    for g in range(G):
        for s in rng.permutation(k + r)[: rng.integers(0, r + 2)]:
            masks[g] |= np.uint64(1) << np.uint64(int(s))
    return masks


@lru_cache(maxsize=None)
def word_case(oracle, k, r, P):
    return _from_word(oracle, k, r, P, drawn_masks(k, r, P))


@lru_cache(maxsize=None)
def wide_main(oracle, k, r, P):
    return _from_wide(main_case(oracle, k, r, P))


def iid_bits(k, r, G, loss, seed):
    bits = np.zeros((G, 256), dtype=bool)
    bits[:, :k + r] = np.random.default_rng([SEED, seed]).random((G, k + r)) < loss
    return bits


def _first_block_holds_every_kind(x):
    """On the CPU, before any launch: the first 1024-group block holds an unrecoverable group, an
    untouched one and a group of each e in 1..3."""
    first = slice(0, 1024)
    assert (x.status[first] == 1).any()
    low = x.masks.reshape(x.G, -1).copy()
    if x.wide:
        untouched = ~np.unpackbits(low.view(np.uint8), axis=1, bitorder="little")[:, :x.k + x.r].astype(bool).any(axis=1)
    else:
        untouched = (low[:, 0] & np.uint64((1 << (x.k + x.r)) - 1)) == 0
    assert untouched[first].any()
    for e in (1, 2, 3):
        assert (x.per_group[first] == e).any(), e


@lru_cache(maxsize=None)
def edge_case(oracle, wide):
    """About 10 % iid loss over G = 2051 groups: (20, 5, 16) one-word, (60, 5, 16) four-word."""
    if wide:
        x = _from_wide(Case(oracle, 60, 5, 16, iid_bits(60, 5, G_EDGE, 0.10, 1), SEED + 1))
    else:
        bits = iid_bits(20, 5, G_EDGE, 0.10, 2)[:, :25]
        masks = (bits * np.left_shift(np.uint64(1), np.arange(25, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
        x = _from_word(oracle, 20, 5, 16, masks)
    assert x.G == G_EDGE and x.G % 4 == 3 and -(-x.G // 1024) == 3
    _first_block_holds_every_kind(x)
    return x


@lru_cache(maxsize=None)
def zero_rows_case(oracle, wide):
    """Every group untouched or unrecoverable (six data shards lost against five rows): no row at all."""
    k, r, P, G = (60, 5, 16, 67) if wide else (20, 5, 272, 515)
    rng = np.random.default_rng([SEED, 3, int(wide)])
    bits = np.zeros((G, 256), dtype=bool)
    for g in range(1, G, 2):
        bits[g, rng.choice(k, size=6, replace=False)] = True
    if wide:
        x = _from_wide(Case(oracle, k, r, P, bits, SEED + 3))
    else:
        masks = (bits[:, :k + r] * np.left_shift(np.uint64(1), np.arange(k + r, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)
        data = oracle.splitmix_bytes(G * k * P, SEED + 4)
        par = oracle.rs_encode(data, G, k, r, P)
        d_in, p_in = us.inputs(data, par, masks, k, r, P, SEED + 5, need_lost_below=False)
        masks_in = us.high_bits(masks, k, r, SEED + 6, need_full=False)
        ref = d_in.copy()
        _, st = oracle.rs_decode(ref, p_in, masks_in, G, k, r, P)
        assert np.array_equal(ref, d_in)
        x = _expect(k, r, P, d_in, p_in, masks_in, st, np.zeros(G, dtype=np.int64), np.zeros((0, P), dtype=np.uint8), False)
    assert len(x.rows) == 0 and (x.status[1::2] == 1).all() and (x.status[0::2] == 0).all()
    return x


# ------------------------------------------------------------------------------------------
# Calls
# ------------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make(torch, x, mask_pad=0):
    """Device buffers of one call; mask_pad: the masks start that many u64 into their allocation."""
    b = SimpleNamespace(x=x, mask_pad=mask_pad)
    b.dd, b.dp = _dev(torch, x.d_in), _dev(torch, x.p_in)
    flat = np.ascontiguousarray(x.masks).reshape(-1).view(np.int64)
    b.dm_whole = _dev(torch, np.concatenate([np.full(mask_pad, 0x0123456789ABCDEF, dtype=np.int64), flat]))
    b.dm = b.dm_whole[mask_pad:]
    b.out = torch.full((max(1, x.G * min(x.k, x.r)) * x.P,), 0x5A, dtype=torch.uint8, device="cuda")
    b.rs = torch.full((x.G,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    b.tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    b.st = torch.full((x.G,), 7, dtype=torch.uint8, device="cuda")
    return b


def call(ctx, b, stream=None, total=True, status=True):
    x = b.x
    fn = ctx.recover_packed_wide_dev if x.wide else ctx.recover_packed_any_dev
    fn(b.dd, b.dp, b.dm, x.G, x.k, x.r, x.P, b.out, b.rs, b.tot if total else None, b.st if status else None,
       stream=stream.cuda_stream if stream is not None else None)


def check(b, what="", total=True, status=True):
    x = b.x
    what = (what, "wide" if x.wide else "word", x.k, x.r, x.P)
    n = len(x.rows)
    assert int(b.tot.item()) == (n if total else -1), (what, "total")
    rs = b.rs.cpu().numpy().view(np.uint32)
    assert np.array_equal(rs, x.start), (what, "row starts", int(np.flatnonzero(rs != x.start)[0]))
    st = b.st.cpu().numpy()
    if status:
        assert np.array_equal(st, x.status), (what, "status", int(np.flatnonzero(st != x.status)[0]))
    else:
        assert (st == 7).all(), what
    o = b.out.cpu().numpy()
    got = o[:n * x.P].reshape(n, x.P)
    if not np.array_equal(got, x.rows):
        row = int(np.flatnonzero((got != x.rows).any(axis=1))[0])
        g = int(np.searchsorted(x.start, row, side="right") - 1)
        raise AssertionError((what, "rows", f"row {row} of group {g}, its row {row - int(x.start[g])} of {int(x.per_group[g])}"))
    assert (o[n * x.P:] == 0x5A).all(), (what, "a byte at or past total * P was written")
    assert np.array_equal(b.dd.cpu().numpy(), x.d_in), (what, "data changed")
    assert np.array_equal(b.dp.cpu().numpy(), x.p_in), (what, "parity changed")
    m = b.dm_whole.cpu().numpy().view(np.uint64)
    assert np.array_equal(m[b.mask_pad:], np.ascontiguousarray(x.masks).reshape(-1)), (what, "masks changed")
    assert (m[:b.mask_pad] == np.uint64(0x0123456789ABCDEF)).all(), what


def run_twice(torch, ctx, x, what="", mask_pad=0):
    """Once on the context's stream, once on a side stream."""
    calls = [make(torch, x, mask_pad), make(torch, x, mask_pad)]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    call(ctx, calls[0])
    call(ctx, calls[1], side)
    ctx.synchronize()
    torch.cuda.synchronize()
    for i, b in enumerate(calls):
        check(b, (what, ("context stream", "side stream")[i]))
    return calls


def plan_device_ctx(q, hooks=False):
    ctx = hooks_ctx(q) if hooks else product_ctx(q)
    ctx.decode_plan_mode(q.FEC_PLAN_DEVICE)
    return ctx


def rows_all_ctx(q):
    ctx = product_ctx(q)
    ctx.wide_rows_mode(q.FEC_WIDE_ROWS_ALL)
    return ctx


# ------------------------------------------------------------------------------------------
# 1. One-word, shapes the old call refuses
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(20, 5, 1200), (10, 3, 200), (10, 3, 3000), (6, 3, 1200), (4, 2, 16), (10, 3, 1037), (6, 3, 1037)])
def test_codebook_shapes(gpu_ctx, oracle_mod, torch_cuda, k, r, P):
    """(10, 3, 1037) is an odd size, its 4-B tail shifted back: the old call serves it, so this is its output."""
    run_twice(torch_cuda, gpu_ctx, word_case(oracle_mod, k, r, P))


@pytest.mark.parametrize("k,r,P", [(16, 16, 272), (60, 4, 48)])
def test_shapes_past_the_codebook_cap(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    x = word_case(oracle_mod, k, r, P)
    if (k, r) == (16, 16):
        assert ((x.per_group >= 9) & (x.per_group <= 16)).any(), "no group takes two row passes"
    with plan_device_ctx(quicfec_mod) as ctx:
        run_twice(torch_cuda, ctx, x)


# ------------------------------------------------------------------------------------------
# 2. One-word, shapes the old call serves: byte for byte its output
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(10, 3, 1200), (10, 2, 700), (4, 2, 513)])
def test_served_by_the_old_call_is_the_old_call(gpu_ctx, oracle_mod, torch_cuda, k, r, P):
    torch = torch_cuda
    x = word_case(oracle_mod, k, r, P)
    new = run_twice(torch, gpu_ctx, x)
    old = make(torch, x)
    torch.cuda.synchronize()
    gpu_ctx.recover_packed_dev(old.dd, old.dp, old.dm, x.G, k, r, P, old.out, old.rs, old.tot, old.st)
    gpu_ctx.synchronize()
    for b in new:
        for name in ("out", "rs", "tot", "st"):
            assert torch.equal(getattr(b, name), getattr(old, name)), name


# ------------------------------------------------------------------------------------------
# 3. Chunks and the launch trace
# ------------------------------------------------------------------------------------------
def expected_trace(G, wide, per_chunk, passes, wave_groups, build, direct=True):
    """DESIGN §5b "Packed recover for every shape": the row prefix, the classify over [0, G); per plan
    chunk the record build (none on the codebook path, one launch per chunk on the deep path), then
    ceil(min(k, r) / 8) passes of the consumer; each wave-per-group launch at most wave_groups groups.
    (form, first group, groups, aux, pol)."""
    w = "_wide" if wide else ""
    out = [("rows_block_sums" + w, 0, G, -1, -1)]
    out += [] if direct else [("rows_scan_blocks", 0, G, -1, -1)]
    out += [("rows_write" + w, 0, G, -1, -1), ("classify" + w, 0, G, -1, -1)]
    for c0 in range(0, G, per_chunk):
        cn = min(per_chunk, G - c0)
        pieces = [(g0, min(wave_groups, cn - g0)) for g0 in range(0, cn, wave_groups)]
        if build == "build_records_deep":
            out.append((build, c0, cn, 0, -1))
        elif build:
            out += [(build, c0 + g0, gn, g0, -1) for g0, gn in pieces]
        for p in range(passes):
            out += [("recover_packed" + w, c0 + g0, gn, 8 * p, POL) for g0, gn in pieces]
    return out


def _trace(q, lib):
    return [(t["form"], t["first_item"], t["items"], t["aux"], t["pol"]) for t in q.launch_trace(lib)]


@pytest.mark.parametrize("which", ["codebook", "device_plan", "wide"])
def test_chunked_walk(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, which):
    """The test library with 7 (wide: 3) workgroups per wave-per-group launch and, where records are built,
    an arena of a third of the groups: results as ever -- row starts stay global in every chunk -- and
    the launches the design's table names with the chunk bounds."""
    torch, q = torch_cuda, quicfec_mod
    lib = q.load_test_library()
    if which == "codebook":
        x, env, per_chunk, wave, build = word_case(oracle_mod, 20, 5, 1200), {"QUICFEC_MAX_WAVE_BLOCKS": "7"}, G_WORD, 28, None
    elif which == "device_plan":
        x = word_case(oracle_mod, 16, 16, 272)
        stride = 128 + 16 * 16 * 32                                            # fec_forms.hpp plan_slot_stride
        env = {"QUICFEC_MAX_WAVE_BLOCKS": "7", "QUICFEC_PLAN_ARENA_BYTES": str(400 * stride)}
        per_chunk, wave, build = 400, 28, "build_records"
    else:
        x = wide_main(oracle_mod, 100, 20, 48)
        stride = 512 + 20 * 100 * 32                                           # fec_forms.hpp wide_slot_stride
        env = {"QUICFEC_MAX_WAVE_BLOCKS": "3", "QUICFEC_PLAN_ARENA_BYTES": str(25 * stride)}
        per_chunk, wave, build = 25, 12, "build_records_wide"
    assert which == "codebook" or -(-x.G // per_chunk) >= 3
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    with (plan_device_ctx(q, hooks=True) if which == "device_plan" else hooks_ctx(q)) as ctx:
        b = make(torch, x)
        torch.cuda.synchronize()
        q.launch_trace(lib)
        call(ctx, b, torch.cuda.current_stream())
        ctx.synchronize()
        torch.cuda.synchronize()
        trace = _trace(q, lib)
    check(b, which)
    assert trace == expected_trace(x.G, x.wide, per_chunk, -(-min(x.k, x.r) // 8), wave, build)


# ------------------------------------------------------------------------------------------
# 4. Prefix edges, both mask widths
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct_blocks", [None, "1"])
@pytest.mark.parametrize("wide", [False, True])
def test_prefix_edges(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, wide, direct_blocks):
    """G = 2051: three 1024-group blocks, the last partial, G mod 4 = 3; the masks one u64 into their
    allocation (8-B aligned only); the two-launch prefix and (QUICFEC_ROWS_DIRECT_BLOCKS=1 below the
    three blocks) the one with the separate scan of the block sums."""
    torch, q = torch_cuda, quicfec_mod
    lib = q.load_test_library()
    x = edge_case(oracle_mod, wide)
    if direct_blocks:
        monkeypatch.setenv("QUICFEC_ROWS_DIRECT_BLOCKS", direct_blocks)
    with hooks_ctx(q) as ctx:
        q.launch_trace(lib)
        calls = run_twice(torch, ctx, x, direct_blocks, mask_pad=1)
        forms = [t["form"] for t in q.launch_trace(lib)]
    assert calls[0].dm.data_ptr() % 16 == 8
    w = "_wide" if wide else ""
    prefix = ["rows_block_sums" + w] + (["rows_scan_blocks"] if direct_blocks else []) + ["rows_write" + w]
    assert forms[:len(prefix) + 1] == prefix + ["classify" + w]
    assert forms.count("rows_scan_blocks") == (2 if direct_blocks else 0)


# ------------------------------------------------------------------------------------------
# 5. No rows at all; nullable outputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_all_groups_with_zero_rows(gpu_ctx, oracle_mod, torch_cuda, wide):
    calls = run_twice(torch_cuda, gpu_ctx, zero_rows_case(oracle_mod, wide))
    for b in calls:
        assert int(b.tot.item()) == 0 and bool((b.out == 0x5A).all()) and bool((b.rs == 0).all())


@pytest.mark.parametrize("wide", [False, True])
def test_total_and_status_are_nullable(gpu_ctx, oracle_mod, torch_cuda, wide):
    torch = torch_cuda
    x = wide_main(oracle_mod, 60, 5, 16) if wide else word_case(oracle_mod, 6, 3, 1200)
    b = make(torch, x)
    torch.cuda.synchronize()
    call(gpu_ctx, b, torch.cuda.Stream(), total=False, status=False)
    gpu_ctx.synchronize()
    torch.cuda.synchronize()
    check(b, "no total, no status", total=False, status=False)


# ------------------------------------------------------------------------------------------
# 6. Wide
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(k, r, min(sizes)) for k, r, sizes in WIDE_SHAPES] + [(224, 32, 1200)])
def test_wide_shapes(gpu_ctx, oracle_mod, torch_cuda, k, r, P):
    """test_gpu_wide.SHAPES, each at its smallest size (100 + 20: 1037, an odd size), and 224 + 32 at
    1200 B; G = 67 with the planted kinds.  Expected: Case.slots compacted in group order; and the
    same rows as fec_recover_wide_rs_dev's slots compacted by the row starts this call returned."""
    torch = torch_cuda
    assert set(planted_groups(k, r)) >= {"untouched", "parity_only", "short_by_one", "xor", "full_lowest_rows"}
    x = wide_main(oracle_mod, k, r, P)
    calls = run_twice(torch, gpu_ctx, x)
    slots = torch.full((x.G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.recover_wide_dev(calls[0].dd, calls[0].dp, calls[0].dm, x.G, k, r, P, slots)
    gpu_ctx.synchronize()
    s = slots.cpu().numpy().reshape(x.G, r, P)
    for b in calls:
        rs, total = b.rs.cpu().numpy().view(np.uint32).astype(np.int64), int(b.tot.item())
        per = np.diff(np.append(rs, total))
        compact = [s[g, :per[g]] for g in np.flatnonzero(per)]
        compact = np.concatenate(compact) if compact else np.zeros((0, P), dtype=np.uint8)
        assert np.array_equal(b.out.cpu().numpy()[:total * P].reshape(total, P), compact)


# ------------------------------------------------------------------------------------------
# 7. Wide at k + r <= 64
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(20, 5, 272), (10, 3, 1200)])
def test_one_word_shapes_through_the_wide_call(gpu_ctx, oracle_mod, torch_cuda, k, r, P):
    """Words 1..3 all ones: byte for byte what fec_recover_packed_rs_dev gives for word 0."""
    torch = torch_cuda
    x = wide_main(oracle_mod, k, r, P)
    assert (x.masks[:, 1:] == np.iinfo(np.uint64).max).all()
    wide = run_twice(torch, gpu_ctx, x)
    word = SimpleNamespace(**{**vars(x), "masks": x.masks[:, 0].copy(), "wide": False})
    narrow = run_twice(torch, gpu_ctx, word)
    for name in ("out", "rs", "tot", "st"):
        assert torch.equal(getattr(wide[0], name), getattr(narrow[0], name)), name
        assert torch.equal(getattr(wide[1], name), getattr(narrow[1], name)), name


# ------------------------------------------------------------------------------------------
# 8. Deep: min(k, r) > 32
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(40, 40, 48), (33, 33, 16)])
def test_deep_shapes(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """Refused in the default mode with nothing written; served and exact in FEC_WIDE_ROWS_ALL, where a
    capped shape on the same context gives the capped mode's bytes."""
    torch, q = torch_cuda, quicfec_mod
    x = _from_wide(deep_case(oracle_mod, k, r, P, 13))
    capped = wide_main(oracle_mod, 60, 5, 16)
    with product_ctx(q) as ctx:
        b = make(torch, x)
        torch.cuda.synchronize()
        with pytest.raises(q.FecError) as ei:
            call(ctx, b)
        assert ei.value.code == q.FEC_ERR_RANGE and "min(k, r)" in ctx.last_error()
        ctx.synchronize()
        torch.cuda.synchronize()
        assert bool((b.out == 0x5A).all()) and bool((b.rs == 0x7FFFFFFF).all()) and int(b.tot.item()) == -1 and bool((b.st == 7).all())
        before = run_twice(torch, ctx, capped)
    with rows_all_ctx(q) as ctx:
        run_twice(torch, ctx, x)
        after = run_twice(torch, ctx, capped)
    for name in ("out", "rs", "tot", "st"):
        assert torch.equal(getattr(before[1], name), getattr(after[1], name)), name


# ------------------------------------------------------------------------------------------
# 9. Refusals
# ------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(quicfec_mod, oracle_mod, torch_cuda):
    torch, q = torch_cuda, quicfec_mod
    lib = q.load_test_library()
    xw, xd = word_case(oracle_mod, 4, 2, 16), wide_main(oracle_mod, 60, 5, 16)
    with hooks_ctx(q) as ctx:
        bw, bd = make(torch, xw), make(torch, xd)
        torch.cuda.synchronize()
        q.launch_trace(lib)
        word = lambda G, k, r, P: ctx.recover_packed_any_dev(bw.dd, bw.dp, bw.dm, G, k, r, P, bw.out, bw.rs, bw.tot, bw.st)
        wide = lambda G, k, r, P: ctx.recover_packed_wide_dev(bd.dd, bd.dp, bd.dm, G, k, r, P, bd.out, bd.rs, bd.tot, bd.st)
        for fn, (G, k, r, P), text in (
                (word, (xw.G, 4, 2, 15), "below 16"), (word, (xw.G, 60, 5, 16), "k+r<=64"), (word, (xw.G, 0, 2, 16), "k+r<=64"),
                (word, (2**30, 10, 4, 16), "32-bit row indices"), (word, (2**32, 4, 2, 16), "32-bit group indices"),
                (word, (xw.G, 16, 16, 16), "exceeds the"), (word, (xw.G, 60, 4, 16), "FEC_PLAN_DEVICE"),
                (wide, (xd.G, 60, 5, 15), "below 16"), (wide, (xd.G, 200, 57, 16), "k+r<=256"), (wide, (xd.G, 40, 40, 16), "min(k, r)"),
                (wide, (0, 60, 5, 16), "num_groups is 0"), (wide, (2**32, 60, 5, 16), "32-bit group indices"),
                (wide, (2**31, 60, 2, 16), "32-bit row indices")):
            with pytest.raises(q.FecError) as ei:
                fn(G, k, r, P)
            assert ei.value.code == q.FEC_ERR_RANGE and text in ctx.last_error(), (G, k, r, P, ctx.last_error())
        p = lambda t: t.data_ptr()
        for b, x, fn, masks in ((bw, xw, lib.fec_recover_packed_rs_dev, "d_masks"), (bd, xd, lib.fec_recover_packed_wide_rs_dev, "d_erasure_masks")):
            args = [ctx.handle, p(b.dd), p(b.dp), p(b.dm), x.G, x.k, x.r, x.P, p(b.out), p(b.rs), p(b.tot), p(b.st), None]
            for i, name in ((0, "context"), (1, "d_data"), (2, "d_parity"), (3, masks), (8, "d_rebuilt"), (9, "d_row_start")):
                bad = list(args)
                bad[i] = None
                assert fn(*bad) == q.FEC_ERR_NULL and name in q.last_error(lib), (name, q.last_error(lib))
        ctx.synchronize()
        torch.cuda.synchronize()
        assert q.launch_trace(lib) == []
        for b, x in ((bw, xw), (bd, xd)):
            assert bool((b.out == 0x5A).all()) and bool((b.rs == 0x7FFFFFFF).all()) and int(b.tot.item()) == -1
            assert bool((b.st == 7).all())
            assert np.array_equal(b.dd.cpu().numpy(), x.d_in) and np.array_equal(b.dp.cpu().numpy(), x.p_in)
        # no groups: served, nothing launched, the total is 0
        ctx.recover_packed_any_dev(bw.dd, bw.dp, bw.dm, 0, 4, 2, 16, bw.out, bw.rs, bw.tot, bw.st)
        ctx.synchronize()
        assert int(bw.tot.item()) == 0 and q.launch_trace(lib) == [] and bool((bw.rs == 0x7FFFFFFF).all())
        bw.tot.fill_(-1)
        torch.cuda.synchronize()
        for b in (bw, bd):                                                     # and the same buffers are served
            call(ctx, b)
        ctx.synchronize()
    check(bw)
    check(bd)


# ------------------------------------------------------------------------------------------
# 10. The workspace across calls on one stream
# ------------------------------------------------------------------------------------------
def test_three_families_queued_on_one_stream(quicfec_mod, oracle_mod, torch_cuda):
    """A slot recover (20 + 5), the packed call for 16 + 16 on the device plan and the wide packed call
    queued on one side stream with no host synchronise between them: the record offsets of the first,
    then block sums, record offsets and an arena of two different strides, all in one buffer."""
    torch, q = torch_cuda, quicfec_mod
    xs, xp, xw = word_case(oracle_mod, 20, 5, 1200), word_case(oracle_mod, 16, 16, 272), wide_main(oracle_mod, 100, 20, 1037)
    stream = torch.cuda.Stream()
    with plan_device_ctx(q) as ctx:
        bs, bp, bw = make(torch, xs), make(torch, xp), make(torch, xw)
        slots = torch.full((xs.G * xs.r * xs.P,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.recover_dev(bs.dd, bs.dp, bs.dm, xs.G, xs.k, xs.r, xs.P, slots, bs.st, stream=stream.cuda_stream)
        call(ctx, bp, stream)
        call(ctx, bw, stream)
        torch.cuda.synchronize()
    check(bp, "device plan")
    check(bw, "wide")
    assert np.array_equal(bs.st.cpu().numpy(), xs.status)
    want = np.full((xs.G, xs.r, xs.P), 0x5A, dtype=np.uint8)
    for g in np.flatnonzero(xs.per_group):
        want[g, :xs.per_group[g]] = xs.rows[xs.start[g]:xs.start[g] + xs.per_group[g]]
    assert np.array_equal(slots.cpu().numpy().reshape(xs.G, xs.r, xs.P), want)
