"""The wide calls past min(k, r) <= 32 on the GPU: fec_decode_wide_rs_dev (in place),
fec_recover_wide_rs_dev (slots) and fec_recover_scatter_wide_rs_dev (tables) on a context in
FEC_WIDE_ROWS_ALL, for k + r <= 256 with min(k, r) up to 128.

The truth is the original data, as in test_gpu_wide.py and test_gpu_wide_table.py, whose cases, device
buffers and checks these tests use: parity is oracle.rs_encode's (which serves k + r <= 256), junk
fills every lost shard, every parity row the rule does not read and every mask bit at and above
k + r; outputs are pre-filled 0x5A between guard bytes, statuses 0xAA; the calls run on a side stream.
Every case goes through both contiguous calls and through the table call without and with a length
table.  The shapes are the smallest at which the deep path can still go wrong:

    33 + 33    P = 16, 1025   one row past the cap; the last of 5 passes has one row
    65 + 65    P = 48         e and the ids cross 64
    128 + 128  P = 16, 48     the whole scratch; 128 erased ids; 16 passes; shard 255
    216 + 40   P = 48         survivor ids and chosen rows up to 255
    40 + 216   P = 48         chosen rows in words 2-3
    100 + 100  P = 1037, 4096, G = 9   tail pieces; whole 1-KiB passes

G = 67 but for 100 + 100, whose 9 groups are all planted: XOR, a single loss with row 0 lost, the
three full kinds, e = 32, e = 33, untouched and short by one (the other kinds ride in the G = 67 cases).
"""
import os
import threading
from functools import lru_cache

import numpy as np
import pytest

import test_gpu_wide as tw
import test_gpu_wide_table as tt
import wide_masks as wm
from test_gpu_gather import hooks_ctx, product_ctx
from test_gpu_wide import drawn_group, planted_groups

pytestmark = pytest.mark.gpu

SEED = 0xDEE90000
GUARD = 256
CASES = [(33, 33, 16, 67), (33, 33, 1025, 67), (65, 65, 48, 67), (128, 128, 16, 67), (128, 128, 48, 67), (216, 40, 48, 67),
         (40, 216, 48, 67), (100, 100, 1037, 9), (100, 100, 4096, 9)]
SMALL_KINDS = ("xor", "single_row_0_lost", "full_lowest_rows", "full_highest_rows", "full_spread", "e32", "e33", "untouched",
               "short_by_one")
POL_DEEP = 16384                                                              # fec_forms.hpp kDeepRecord
POL_IN_PLACE, POL_SLOTS, POL_TABLE = 2 | 4 | POL_DEEP, 2 | 4 | 1024, 1 | 2 | 4 | 1024 | POL_DEEP


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


def deep_ctx(q, hooks=False):
    ctx = hooks_ctx(q) if hooks else product_ctx(q)
    ctx.wide_rows_mode(q.FEC_WIDE_ROWS_ALL)
    return ctx


def _stride(k, r):
    return 512 + min(k, r) * k * 32                                            # fec_forms.hpp wide_deep_slot_stride


# ------------------------------------------------------------------------------------------
# Cases
# ------------------------------------------------------------------------------------------
def _group(k, lost_data, lost_rows=()):
    b = np.zeros(256, dtype=bool)
    b[list(lost_data)] = True
    b[[k + i for i in lost_rows]] = True
    return b


def _bits(k, r, G, salt):
    """The planted kinds of test_gpu_wide.planted_groups, e = 32 and e = 33 where the shape holds them
    (lost shards spread, the lowest rows lost so that the chosen ones lie higher), then drawn groups."""
    kinds = planted_groups(k, r)
    emax = min(k, r)
    for e in (32, 33):
        if e <= emax:
            kinds[f"e{e}"] = [_group(k, np.linspace(0, k - 1, e).round().astype(int), range(min(3, r - e)))]
    if G < 3 * sum(len(v) for v in kinds.values()):
        kinds = {kind: kinds[kind] for kind in SMALL_KINDS}
    bits, planted = [], {}
    for kind, groups in kinds.items():
        planted[kind] = [(len(bits) + i, b) for i, b in enumerate(groups)]
        bits += groups
    assert len(bits) <= G
    rng = np.random.default_rng([SEED, salt])
    bits += [drawn_group(k, r, rng) for _ in range(G - len(bits))]
    return np.array(bits), planted


def _check_planted(c, planted, k, r):
    emax = min(k, r)
    first = {kind: groups[0][0] for kind, groups in planted.items()}
    for kind in ("full_lowest_rows", "full_highest_rows", "full_spread"):
        assert c.rebuilds[first[kind]] and c.e[first[kind]] == emax, kind
    assert c.rebuilds[first["xor"]] and c.e[first["xor"]] == 1 and c.ro.chosen[first["xor"], 0]
    assert c.rebuilds[first["single_row_0_lost"]] and c.ro.lost_p[first["single_row_0_lost"], 0]
    assert not c.rebuilds[first["untouched"]] and c.status[first["untouched"]] == 0
    assert c.status[first["short_by_one"]] == 1
    for e in (32, 33):
        if e <= emax:
            assert c.rebuilds[first[f"e{e}"]] and c.e[first[f"e{e}"]] == e
    # the precondition of every test here, on the CPU before any launch
    assert c.rebuilds.sum() * 4 >= 3 * c.G, "fewer than three quarters of the groups are rebuilt"


@lru_cache(maxsize=None)
def wide_case(oracle, k, r, P, G=67):
    salt = k * 1000000 + r * 10000 + P
    bits, planted = _bits(k, r, G, salt)
    c = tw.Case(oracle, k, r, P, bits, SEED + salt, planted)
    if G >= 67:
        tw.check_kinds(c, {kind: v for kind, v in planted.items() if not kind.startswith("e3")})
    _check_planted(c, planted, k, r)
    return c


@lru_cache(maxsize=None)
def table_case(oracle, k, r, P, G=67):
    salt = k * 1000000 + r * 10000 + P + 7
    bits, planted = _bits(k, r, G, salt)
    c = tt.Case(oracle, k, r, P, bits, SEED + salt, planted)
    _check_planted(c, planted, k, r)
    return c


def run_all(torch, ctx, oracle, k, r, P, G, what=""):
    """Both contiguous calls and the table call, without and with the length table."""
    calls = tw.run_both(torch, ctx, wide_case(oracle, k, r, P, G), what)
    tc = table_case(oracle, k, r, P, G)
    calls.append(tt.run(torch, ctx, tc, False, "slots", what))
    calls.append(tt.run(torch, ctx, tc, True, "odd", what))
    return calls


# ------------------------------------------------------------------------------------------
# 1. Shapes and sizes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P,G", CASES)
def test_shapes_and_sizes(quicfec_mod, oracle_mod, torch_cuda, k, r, P, G):
    """Rebuilt rows equal the original data in place, in slots and at the table's destinations (exactly
    L_g bytes each); every status byte, untouched slots and destinations, guards, and every input the
    calls only read."""
    with deep_ctx(quicfec_mod) as ctx:
        run_all(torch_cuda, ctx, oracle_mod, k, r, P, G)


# ------------------------------------------------------------------------------------------
# 2. The mode
# ------------------------------------------------------------------------------------------
def _refused(q, ctx, lib, calls, tb, k, r):
    c = calls[0].c
    for b in calls:
        with pytest.raises(q.FecError) as ei:
            tw.launch(ctx, b)
        assert ei.value.code == q.FEC_ERR_RANGE and "min(k, r) exceeds 32 rows" in ctx.last_error(), ctx.last_error()
    with pytest.raises(q.FecError) as ei:
        tt.launch(ctx, tb)
    assert ei.value.code == q.FEC_ERR_RANGE and "min(k, r) exceeds 32 rows" in ctx.last_error()
    assert f"fec_recover_scatter_wide_rs_dev: k={k} r={r}: min(k, r) exceeds 32 rows per group" == ctx.last_error()
    ctx.synchronize()
    assert q.launch_trace(lib) == []
    for b in calls:
        assert (b.swhole == 0xAA).all().item() and np.array_equal(b.dd.cpu().numpy(), c.d_in)
    assert (calls[1].owhole == 0x5A).all().item()
    assert np.array_equal(tb.owhole.cpu().numpy(), tb.expect_before) and (tb.swhole.cpu().numpy()[GUARD:-GUARD] == 0xAA).all()


def test_default_mode_refuses_and_the_switch_serves(quicfec_mod, oracle_mod, torch_cuda):
    """A default context refuses 33 + 33 with FEC_ERR_RANGE and today's text, launches nothing and writes
    nothing; the same context serves the same buffers after fec_wide_rows_mode(ALL); back in the capped
    mode it refuses again; an unknown mode is refused and leaves the mode as it was."""
    torch, q = torch_cuda, quicfec_mod
    lib = q.load_test_library()
    k, r, P = 33, 33, 16
    c, tc = wide_case(oracle_mod, k, r, P), table_case(oracle_mod, k, r, P)
    with hooks_ctx(q) as ctx:
        calls = [tw.make_call(torch, c, "in_place"), tw.make_call(torch, c, "slots")]
        tb = tt.make_call(torch, tc, True, "packed")
        tb.expect_before = tb.owhole.cpu().numpy().copy()
        torch.cuda.synchronize()
        q.launch_trace(lib)
        _refused(q, ctx, lib, calls, tb, k, r)
        for bad in (2, -1, 7):
            with pytest.raises(q.FecError) as ei:
                ctx.wide_rows_mode(bad)
            assert ei.value.code == q.FEC_ERR_RANGE and "unknown mode" in ctx.last_error()
        _refused(q, ctx, lib, calls, tb, k, r)                                 # still the default
        ctx.wide_rows_mode(q.FEC_WIDE_ROWS_ALL)
        with pytest.raises(q.FecError):
            ctx.wide_rows_mode(2)                                              # and still ALL after a refused switch
        for b in calls:
            tw.launch(ctx, b)
        tt.launch(ctx, tb)
        ctx.synchronize()
        torch.cuda.synchronize()
        for b in calls:
            tw.check(b, "after the switch")
        tt.check(tb, "after the switch")
        assert {t["form"] for t in q.launch_trace(lib)} == {"classify_wide", "classify_table_wide", "build_records_deep",
                                                             "decode_wide_deep", "decode_wide", "recover_scatter_wide_deep"}
        ctx.wide_rows_mode(q.FEC_WIDE_ROWS_CAPPED)
        again = [tw.make_call(torch, c, "in_place"), tw.make_call(torch, c, "slots")]
        tb2 = tt.make_call(torch, tc, True, "packed")
        tb2.expect_before = tb2.owhole.cpu().numpy().copy()
        torch.cuda.synchronize()
        _refused(q, ctx, lib, again, tb2, k, r)


def _full_trace(q, lib):
    return [tuple(t[f] for f in q.LAUNCH_FIELDS) for t in q.launch_trace(lib)]


@pytest.mark.parametrize("k,r,P", [(224, 32, 16), (60, 5, 272)])
def test_capped_shapes_are_untouched_by_the_mode(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """min(k, r) <= 32: the same launches, field by field, and the same bytes in either mode."""
    torch, q = torch_cuda, quicfec_mod
    lib = q.load_test_library()
    c, tc = tw.main_case(oracle_mod, k, r, P), tt.main_case(oracle_mod, k, r, P)
    seen = []
    with hooks_ctx(q) as ctx:
        for mode in (q.FEC_WIDE_ROWS_CAPPED, q.FEC_WIDE_ROWS_ALL, q.FEC_WIDE_ROWS_CAPPED):
            ctx.wide_rows_mode(mode)
            calls = [tw.make_call(torch, c, "in_place"), tw.make_call(torch, c, "slots")]
            tbs = [tt.make_call(torch, tc, False, "slots"), tt.make_call(torch, tc, True, "odd")]
            torch.cuda.synchronize()
            q.launch_trace(lib)
            for b in calls:
                tw.launch(ctx, b)
            for b in tbs:
                tt.launch(ctx, b)
            ctx.synchronize()
            torch.cuda.synchronize()
            trace = _full_trace(q, lib)
            for b in calls:
                tw.check(b, mode)
            for b in tbs:
                tt.check(b, mode)
            outs = [calls[0].dwhole, calls[0].swhole, calls[1].owhole, calls[1].swhole] + [x for b in tbs for x in (b.owhole, b.swhole, b.mwhole, b.lwhole)]
            seen.append((trace, [o.cpu().numpy().copy() for o in outs]))
    forms = {t[0] for t in seen[0][0]}
    assert forms == {"classify_wide", "build_records_wide", "decode_wide", "classify_table_wide", "recover_scatter_wide"}
    for trace, outs in seen[1:]:
        assert trace == seen[0][0]
        assert all(np.array_equal(a, b) for a, b in zip(outs, seen[0][1]))


# ------------------------------------------------------------------------------------------
# 3. Round trips of what the encodes produce
# ------------------------------------------------------------------------------------------
def test_encode_batch_then_decode_wide_at_128_plus_128(quicfec_mod, oracle_mod, torch_cuda):
    """fec_encode_batch_rs_dev's parity, 128 + 128, then losses of up to 128 shards per group rebuilt in place."""
    torch, q = torch_cuda, quicfec_mod
    k, r, P, G = 128, 128, 48, 67
    c = wide_case(oracle_mod, k, r, P, G)
    with deep_ctx(q) as ctx:
        data = tw._dev(torch, c.data)
        parity = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.encode_dev(data, G, k, r, P, parity, stream=stream.cuda_stream)
        torch.cuda.synchronize()
        par = parity.cpu().numpy()
        assert np.array_equal(par, c.par), "the encode's parity is not the oracle's"
        # the case's junk over what is lost or not read, around the device's own parity
        _, p_in = wm.inputs(c.data, par, c.ro, P, c.seed + 1)
        b = tw.make_call(torch, c, "in_place")
        b.dp = tw._dev(torch, p_in)
        torch.cuda.synchronize()
        tw.launch(ctx, b, stream)
        torch.cuda.synchronize()
    tw.check(b, "round trip")
    assert c.e.max() == 128 and np.array_equal(b.dd.cpu().numpy()[np.repeat(c.ro.ok, k * P)], c.data[np.repeat(c.ro.ok, k * P)])


def test_encode_scatter_wide_then_recover_scatter_wide_at_33_plus_33(quicfec_mod, oracle_mod, torch_cuda):
    """fec_encode_scatter_wide_rs_dev's parity from packets of their own lengths at odd addresses, then
    fec_recover_scatter_wide_rs_dev with the same length table: every rebuilt packet is its original
    bytes, zeros up to L_g, exactly L_g bytes written between guards; one destination not wanted; one
    group whose packets are all empty (L_g = 0) writes nothing."""
    torch, q = torch_cuda, quicfec_mod
    k, r, P, G, n = 33, 33, 1025, 12, 66
    rng = np.random.default_rng([SEED, 3333])
    S = P + 22                                                                 # odd stride: every residue
    tl = rng.integers(0, P + 1, size=(G, k))
    tl[:, 0] = rng.choice([P, 1024, 1023, 257, 5, 1], size=G)                  # L_g from a data packet
    tl = np.minimum(tl, tl[:, :1])
    tl[5] = 0                                                                  # L_g = 0
    L = tl.max(axis=1)
    raw = oracle_mod.splitmix_bytes(G * k * P, SEED + 3333).reshape(G, k, P)
    orig = np.where(np.arange(P)[None, None, :] < tl[:, :, None], raw, 0).astype(np.uint8)
    junk = rng.integers(1, 256, size=(G, k, S), dtype=np.uint8)                # past each packet's length: junk
    pk = junk.copy()
    pk[:, :, :P] = np.where(np.arange(P)[None, None, :] < tl[:, :, None], orig, junk[:, :, :P])
    arena = torch.cat([torch.full((1,), 0x5A, dtype=torch.uint8), torch.from_numpy(pk.reshape(-1))]).cuda()
    pk_at = arena.data_ptr() + 1 + np.arange(G * k, dtype=np.uint64).reshape(G, k) * S
    parity = torch.full((1 + G * r * S + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    par_at = parity.data_ptr() + 1 + np.arange(G * r, dtype=np.uint64).reshape(G, r) * S
    dev64 = lambda a: tw._dev(torch, np.ascontiguousarray(a).astype(np.uint64).view(np.int64).reshape(-1))
    dev32 = lambda a: tw._dev(torch, np.ascontiguousarray(a).astype(np.uint32).view(np.int32).reshape(-1))
    sym_enc = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    # losses: e = 33, e = 32 from the top rows, singles, a pair; group 5 (empty) loses three
    bits = np.zeros((G, 256), dtype=bool)
    bits[0, :k] = True
    bits[1, :32] = True
    bits[1, k:k + 1] = True
    for g in range(2, G):
        e = int(rng.integers(1, 34))
        bits[g, rng.choice(k, size=e, replace=False)] = True
        bits[g, k + rng.choice(r, size=int(rng.integers(0, r - e + 1)), replace=False)] = True
    ro = wm.roles(wm.from_bits(bits), k, r)
    assert ro.ok.all() and ro.lost_d[5].any()
    lost = np.concatenate([ro.lost_d, ro.lost_p], axis=1)
    lens = np.concatenate([tl, np.repeat(L[:, None], r, axis=1)], axis=1)
    lens = np.where(lost, 0xDEADBEEF, lens)                                    # a lost entry's length is junk
    out = torch.full((GUARD + G * k * S + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    out_off = GUARD + 3 + np.arange(G * k, dtype=np.int64).reshape(G, k) * S   # odd, guards of S - L_g >= 22 between
    trap = torch.full((4096 + P,), 0x5A, dtype=torch.uint8, device="cuda")
    dests = np.full((G, k), trap.data_ptr() + 1027, dtype=np.uint64)
    expect = np.full(out.numel(), 0x5A, dtype=np.uint8)
    unwanted = (0, int(np.flatnonzero(ro.lost_d[0])[7]))
    for g in range(G):
        for j in np.flatnonzero(ro.lost_d[g]):
            if (g, int(j)) == unwanted:
                dests[g, j] = 0
                continue
            dests[g, j] = out.data_ptr() + out_off[g, j]
            expect[out_off[g, j]:out_off[g, j] + L[g]] = orig[g, j, :L[g]]
    st = torch.full((G,), 0xAA, dtype=torch.uint8, device="cuda")
    sym_rec = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    masks_out = torch.full((G * 4,), -1, dtype=torch.int64, device="cuda")
    with deep_ctx(q) as ctx:
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        ctx.encode_scatter_wide_dev(dev64(pk_at), dev32(tl), dev64(par_at), G, k, r, P, sym_enc, stream=stream.cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(sym_enc.cpu().numpy(), L.astype(np.int32))
        rows = parity.cpu().numpy()[1:1 + G * r * S].reshape(G, r, S)
        want = oracle_mod.rs_encode(np.ascontiguousarray(orig).reshape(-1), G, k, r, P, 8).reshape(G, r, P)
        for g in range(G):
            assert np.array_equal(rows[g, :, :L[g]], want[g, :, :L[g]]) and (rows[g, :, L[g]:] == 0x5A).all(), g
        addrs = np.where(lost, 0, np.concatenate([pk_at, par_at], axis=1))
        # a parity row the rule does not read is overwritten with junk on the device
        for g, i in zip(*np.nonzero(ro.unread_p & ~ro.lost_p)):
            at = 1 + (g * r + i) * S
            parity[at:at + P] = 0xC3
        torch.cuda.synchronize()
        ctx.recover_scatter_wide_dev(dev64(addrs), dev32(lens), dev64(dests), G, k, r, P, st, masks_out, sym_rec, stream=stream.cuda_stream)
        torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), expect)
    assert (st.cpu().numpy() == 0).all() and (trap == 0x5A).all().item()
    assert np.array_equal(sym_rec.cpu().numpy(), L.astype(np.int32)) and L[5] == 0
    assert np.array_equal(masks_out.cpu().numpy().view(np.uint64).reshape(G, 4), wm.from_bits(bits))
    assert np.array_equal(arena.cpu().numpy()[1:], pk.reshape(-1))


# ------------------------------------------------------------------------------------------
# 4. Chunks and the launch trace
# ------------------------------------------------------------------------------------------
def expected_trace(G, per_chunk, passes, wave_groups, api, var=False):
    """DESIGN §5b "Wide shapes past the rows cap": the wide path's classify over [0, G); per plan chunk one
    build_records_deep over the chunk's groups (a workgroup each, slot 0 first), then
    ceil(min(k, r) / 8) passes of the consumer, each launch at most wave_groups groups.
    (form, first group, groups, aux, pol, first)."""
    classify = "classify_table_wide" if api == "table" else "classify_wide"
    consumer = {"in_place": ("decode_wide_deep", POL_IN_PLACE, -1), "slots": ("decode_wide", POL_SLOTS, -1),
                "table": ("recover_scatter_wide_deep", POL_TABLE, int(var))}[api]
    out = [(classify, 0, G, -1, -1, -1)]
    for c0 in range(0, G, per_chunk):
        cn = min(per_chunk, G - c0)
        out.append(("build_records_deep", c0, cn, 0, -1, -1))
        pieces = [(g0, min(wave_groups, cn - g0)) for g0 in range(0, cn, wave_groups)]
        for p in range(passes):
            out += [(consumer[0], c0 + g0, gn, 8 * p, consumer[1], consumer[2]) for g0, gn in pieces]
    return out


@pytest.mark.parametrize("k,r,P", [(33, 33, 16), (128, 128, 16)])
def test_chunked_walk(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P):
    """The test library at its defaults, with 12 groups per consumer launch, with the arena lowered to
    five strides and to one stride minus one (one group per chunk): the launches of the design's
    table, one build and ceil(min(k, r) / 8) consumer passes per chunk, and outputs identical to the
    unchunked run's."""
    torch, q = torch_cuda, quicfec_mod
    lib = q.load_test_library()
    c, tc = wide_case(oracle_mod, k, r, P), table_case(oracle_mod, k, r, P)
    G, passes = c.G, -(-min(k, r) // 8)
    s = _stride(k, r)
    settings = [({}, G, 1 << 40), ({"QUICFEC_MAX_WAVE_BLOCKS": "3"}, G, 12),
                ({"QUICFEC_MAX_WAVE_BLOCKS": "3", "QUICFEC_PLAN_ARENA_BYTES": str(5 * s)}, 5, 12),
                ({"QUICFEC_MAX_WAVE_BLOCKS": "3", "QUICFEC_PLAN_ARENA_BYTES": str(s - 1)}, 1, 12)]
    first = None
    with deep_ctx(q, hooks=True) as ctx:
        for i, (env, per_chunk, wave_groups) in enumerate(settings):
            for name in ("QUICFEC_MAX_WAVE_BLOCKS", "QUICFEC_PLAN_ARENA_BYTES"):
                monkeypatch.delenv(name, raising=False)
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            var = i % 2 == 1
            calls = [tw.make_call(torch, c, "in_place"), tw.make_call(torch, c, "slots")]
            tb = tt.make_call(torch, tc, var, "slots")
            torch.cuda.synchronize()
            q.launch_trace(lib)
            for b in calls:
                tw.launch(ctx, b, torch.cuda.current_stream())
            tt.launch(ctx, tb, torch.cuda.current_stream())
            ctx.synchronize()
            torch.cuda.synchronize()
            trace = [(t["form"], t["first_item"], t["items"], t["aux"], t["pol"], t["first"]) for t in q.launch_trace(lib)]
            for b in calls:
                tw.check(b, env)
            tt.check(tb, env)
            want = (expected_trace(G, per_chunk, passes, wave_groups, "in_place") + expected_trace(G, per_chunk, passes, wave_groups, "slots")
                    + expected_trace(G, per_chunk, passes, wave_groups, "table", var))
            assert trace == want, env
            builds = [t for t in trace if t[0] == "build_records_deep"]
            assert len(builds) == 3 * -(-G // per_chunk)
            outs = [calls[0].dwhole.cpu().numpy(), calls[1].owhole.cpu().numpy(), calls[0].swhole.cpu().numpy()]
            if first is None:
                first = outs
            assert all(np.array_equal(a, b) for a, b in zip(outs, first)), env


# ------------------------------------------------------------------------------------------
# 5. State across calls
# ------------------------------------------------------------------------------------------
def test_a_capped_and_two_deep_shapes_queued_on_one_stream(quicfec_mod, oracle_mod, torch_cuda):
    """60 + 5 on the wide path, then 33 + 33 and 65 + 65 on the deep path, then 60 + 5 again, on one side
    stream with no host synchronise between them, each workspace larger than the one before."""
    torch = torch_cuda
    cases = [tw.main_case(oracle_mod, 60, 5, 16), wide_case(oracle_mod, 33, 33, 16), wide_case(oracle_mod, 65, 65, 48)]
    assert _stride(60, 5) < _stride(33, 33) < _stride(65, 65)
    stream = torch.cuda.Stream()
    with deep_ctx(quicfec_mod) as ctx:
        calls = [tw.make_call(torch, c, api) for c, api in zip(cases, ("slots", "in_place", "slots"))]
        calls.append(tw.make_call(torch, cases[0], "in_place"))
        tbs = [tt.make_call(torch, table_case(oracle_mod, 65, 65, 48), True, "odd"), tt.make_call(torch, tt.main_case(oracle_mod, 60, 5, 16), True, "odd")]
        torch.cuda.synchronize()
        for b in calls:
            tw.launch(ctx, b, stream)
        for b in tbs:
            tt.launch(ctx, b, stream, masks=False, symlen=False)                # the workspace holds them
        torch.cuda.synchronize()
    for i, b in enumerate(calls):
        tw.check(b, i)
    for b in tbs:
        tt.check(b, masks=False, symlen=False)


def test_two_threads_on_two_streams(quicfec_mod, oracle_mod, torch_cuda):
    """Two host threads, each with its own side stream and its own deep shape, six calls each on one
    context from a barrier: each stream's records are its own workspace's."""
    torch = torch_cuda
    cases = [wide_case(oracle_mod, 33, 33, 16), wide_case(oracle_mod, 65, 65, 48)]
    work = [[tw.make_call(torch, cases[t], ("in_place", "slots")[j % 2]) for j in range(6)] for t in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2)
    errors = []

    def run(t, ctx):
        try:
            barrier.wait(timeout=60)
            for b in work[t]:
                tw.launch(ctx, b, streams[t])
        except BaseException as e:                                             # re-raised in the test
            errors.append((t, e))

    with deep_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        threads = [threading.Thread(target=run, args=(t, ctx)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
    if errors:
        raise errors[0][1]
    for t in range(2):
        for j, b in enumerate(work[t]):
            tw.check(b, (t, j))


def test_free_with_deep_calls_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """Three deep calls queued on a side stream and the context freed at once: fec_encoder_free drains them
    (they read the context's parity matrix and the stream's workspace), so every output is complete."""
    torch = torch_cuda
    c, tc = wide_case(oracle_mod, 100, 100, 4096, 9), table_case(oracle_mod, 100, 100, 4096, 9)
    calls = [tw.make_call(torch, c, "slots"), tw.make_call(torch, c, "in_place")]
    tb = tt.make_call(torch, tc, True, "slots")
    stream = torch.cuda.Stream()
    ctx = deep_ctx(quicfec_mod)
    torch.cuda.synchronize()
    for b in calls:
        tw.launch(ctx, b, stream)
    tt.launch(ctx, tb, stream, masks=False, symlen=False)
    ctx.close()
    assert stream.query()                                                      # the free drained the stream
    torch.cuda.synchronize()
    for b in calls:
        tw.check(b)
    tt.check(tb, masks=False, symlen=False)


# ------------------------------------------------------------------------------------------
# 6. Nullable arguments
# ------------------------------------------------------------------------------------------
def test_nullable_arguments(quicfec_mod, oracle_mod, torch_cuda):
    """d_status of the contiguous calls; d_status, d_masks_out and d_symbol_len_out of the table call in
    turn and all at once, without (d_shard_lens NULL) and with a length table: what is given as ever,
    what is not given untouched."""
    torch = torch_cuda
    c, tc = wide_case(oracle_mod, 65, 65, 48), table_case(oracle_mod, 65, 65, 48)
    given = [dict(), dict(st=False), dict(masks=False), dict(symlen=False), dict(st=False, masks=False, symlen=False)]
    with deep_ctx(quicfec_mod) as ctx:
        plain = [tw.make_call(torch, c, "in_place"), tw.make_call(torch, c, "slots")]
        tbs = [(tt.make_call(torch, tc, var, "packed", seed=i), kw) for var in (False, True) for i, kw in enumerate(given)]
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        for b in plain:
            tw.launch(ctx, b, stream, st=False)
        for b, kw in tbs:
            tt.launch(ctx, b, stream, **kw)
        torch.cuda.synchronize()
    for b in plain:
        tw.check(b, "no status", status=False)
    for b, kw in tbs:
        tt.check(b, kw, **kw)
