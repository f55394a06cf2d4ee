"""Every contiguous call family with its buffers across byte offset 2^32.

Every kernel finds its bytes as base + (g * rows + row) * P + column.  The products are written in
64 bits by hand, and a rewrite that lets a uint32_t into one of them passes every other GPU test:
none of them puts a byte of the kernel form it reaches at or past offset 2^32.  These cases do, for
each buffer the table below names, and each asserts on the host that the buffer exceeds
2^32 + 2^20 bytes before anything is launched.

Truth.  Data is fec_fill_random_dev's stream over the whole buffer (non-periodic), every output is
prefilled with 0xA5.  The CPU oracle runs on host windows only: the groups big_buffers.boundary_groups
names for every buffer of the call (the two ends and the groups around every multiple of 2^32) are
copied to the host as the call was given them and as it left them, and compared with
oracle.splitmix_bytes, oracle.rs_encode and oracle.rs_decode on that group alone.  The oracle's decode
stops at 64 shards.  So the wide and deep decoders (k + r > 64: the 40 + 32 and 66 + 66 cases) are never
compared with an independent decoder in this file: their rebuilt rows, in the host windows too, are
compared only with the original data, the stream, to which the encode windows pin the parity they
read.  tests/test_gpu_wide.py and test_gpu_wide_deep.py do the same for the same reason.  The whole buffers are checked on the device, in slabs of at most half a
GiB of the widest buffer:
  - encode: the same call again over each range of big_buffers.pieces, every base pointer advanced
    to the piece's first group, into a scratch tensor that must equal the piece of the parity.
    Inside a piece no offset reaches 2^31, where the rest of the suite pins the kernels to the oracle.
    The parity lies at an odd address between guard bytes that must stay 0xA5.
  - recover, slots: slot (g, m) equals data shard lost[g][m] of the stream, every other slot is 0xA5,
    statuses are the host's, the masks are unwritten.
  - recover, packed: the same rows at row_start[g] + m, row_start the host's exclusive sum, *d_total,
    0xA5 after the last row.
  - decode in place: the buffer is the generator's stream again (big_buffers.same_as_stream), once
    the unrecoverable groups, which must have been left as they came, are refilled.
The rebuilt rows are compared with the stream itself as soon as a call has run, so that one output
is live at a time (the largest case then holds 24.1 GiB).

Masks.  Every ordinary group loses min(k, r) data shards, drawn per group, so that the packed output
passes the line too.  Every S-th group, S = big_buffers.special_every, is special instead: nothing
lost, only parity lost, one short of full (all rows alive, and row 0 lost), unrecoverable by one row.
Lost data shards and the parity rows the rule does not read hold another stream's bytes before every
decode; the bits at and above k + r hold junk (test_gpu_parity._high, wide_masks.with_high_junk).

A case skips only when torch.cuda.mem_get_info() reports less free memory than it needs, before it
allocates anything.
"""
import gc
import os
import traceback

import numpy as np
import pytest

import big_buffers as bb
import unread_shards as us
import wide_masks as wm
from test_gpu_parity import _high, _masks_unwritten

pytestmark = [pytest.mark.gpu, pytest.mark.slow]

SEED = 0x46B0000
JUNK_SEED = SEED ^ 0x7A11
FILL = 0xA5
FRONT, BACK = 67, 64                 # guard bytes: the parity starts at an odd address
SLAB_BYTES = 1 << 29                 # of the widest buffer, per slab of groups
STAGE = 8192                         # POL_STAGE_ROWS of a launch record


# The switches of the test library (csrc/fec_knobs.cpp) that choose a kernel form or cut a launch into
# chunks.  The product library ignores them; the two traced calls of the test library must not see them.
ROUTING_SWITCHES = ("QUICFEC_MAX_WAVE_BLOCKS", "QUICFEC_MAX_LAUNCH_THREADS", "QUICFEC_ENCODE_TILE", "QUICFEC_ENCODE_BLOCKS",
                    "QUICFEC_ENCODE_WAVES", "QUICFEC_ENCODE_BITS", "QUICFEC_ENCODE_STAGE", "QUICFEC_DECODE_WAVES",
                    "QUICFEC_ROWS_DIRECT_BLOCKS", "QUICFEC_RUNS_STAGE", "QUICFEC_DECODE_SCAN", "QUICFEC_PACKED_RUNS",
                    "QUICFEC_PLAN_ARENA_BYTES")


@pytest.fixture(autouse=True)
def _no_routing_switches(monkeypatch):
    """Every case starts from the library's own choice of form: none of the routing switches set.
    Every other variable, a library path among them, stays as the session has it."""
    for name in ROUTING_SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _need(torch, nbytes, what):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB are free")


def _run(torch, ctx, call, *args, **kw):
    """One library call on the context's own stream, between torch's work and torch's reads."""
    torch.cuda.synchronize()
    call(*args, **kw)
    ctx.synchronize()


def _run_and_free(torch, body, *contexts):
    """Run a case's device part.  Every tensor of the case is a local of `body` (or of what it calls), so
    all of them are dropped when it returns; when it raises, the frames the traceback keeps are cleared
    first.  Then the contexts are closed and the cache is emptied, failure included."""
    try:
        body()
    except BaseException as exc:
        traceback.clear_frames(exc.__traceback__)
        raise
    finally:
        for c in contexts:
            if c is not None:
                c.close()
        gc.collect()
        torch.cuda.empty_cache()


def _full(torch, n, value=FILL):
    return torch.full((int(n),), value, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------
# Losses, on the host
# ------------------------------------------------------------------------------------------
def _lose(rng, n, count):
    """(len(count), n) bool with exactly count[g] of n set per row, drawn."""
    keys = rng.random((len(count), n))
    kth = np.sort(keys, axis=1)[np.arange(len(count)), np.maximum(count, 1) - 1]
    return (keys <= kth[:, None]) & (count > 0)[:, None]


def draw_losses(G, k, r, S, salt, ordinary=None, special_all_data=False):
    """(G, k + r) bool, shard s lost in column s.  ordinary: (lo, hi) lost data shards of an ordinary
    group, default min(k, r) each.  Specials (big_buffers.special_groups) cycle through five kinds,
    or lose every data shard (special_all_data)."""
    rng = np.random.default_rng([SEED, salt])
    emax = min(k, r)
    e = np.full(G, emax) if ordinary is None else rng.integers(ordinary[0], ordinary[1] + 1, size=G)
    bits = np.zeros((G, k + r), dtype=bool)
    bits[:, :k] = _lose(rng, k, e)
    sp = bb.special_groups(G, S)
    kinds = {}
    if special_all_data:
        bits[sp] = False
        bits[sp, :k] = True
        return bits, {"all_data": sp}
    kind = np.arange(len(sp)) % 5
    bits[sp] = False
    for i, name in enumerate(("untouched", "parity_only", "short_of_full", "short_of_full_row_0_lost", "unrecoverable")):
        g = sp[kind == i]
        kinds[name] = g
        if name == "parity_only":
            bits[g, k:] = _lose(rng, r, rng.integers(1, r + 1, size=len(g)))
        elif name.startswith("short_of_full"):
            bits[g, :k] = _lose(rng, k, np.full(len(g), emax - 1))
            if name.endswith("row_0_lost") and r >= 2:
                bits[g, k] = True
        elif name == "unrecoverable":                       # emax lost, emax - 1 rows alive
            bits[g, :k] = _lose(rng, k, np.full(len(g), emax))
            bits[g, k:] = _lose(rng, r, np.full(len(g), r - emax + 1))
    return bits, kinds


class Losses:
    """The host's expectation for one set of masks: roles, statuses, slot sources, row starts."""

    def __init__(self, bits, k, r, wide):
        G = len(bits)
        self.k, self.r, self.G, self.wide = k, r, G, wide
        if wide:
            b256 = np.zeros((G, 256), dtype=bool)
            b256[:, :k + r] = bits
            self.masks = wm.from_bits(b256)
            self.ro = wm.roles(self.masks, k, r)
        else:
            assert k + r <= 64
            self.masks = (bits.astype(np.uint64) << np.arange(k + r, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
            self.ro = us.roles(self.masks, k, r)
        ro = self.ro
        assert np.array_equal(ro.lost_d, bits[:, :k]) and np.array_equal(ro.lost_p, bits[:, k:])
        self.e = ro.lost_d.sum(axis=1)
        self.status = (~ro.ok).astype(np.uint8)
        self.rebuilds = ro.ok & (self.e >= 1)
        self.rows = np.where(self.rebuilds, self.e, 0).astype(np.int64)
        ends = np.cumsum(self.rows)
        self.total = int(ends[-1])
        self.row_start = (ends - self.rows).astype(np.int64)             # exclusive sum
        # slot m of group g holds data shard src[g, m]; -1: the slot stays unwritten
        n = min(k, r)
        first_lost = np.argsort(~ro.lost_d, axis=1, kind="stable")[:, :n]   # lost shards first, ascending
        src = np.full((G, r), -1, dtype=np.int64)
        src[:, :n] = np.where((np.arange(n)[None, :] < self.e[:, None]) & self.rebuilds[:, None], first_lost, -1)
        self.src = src
        assert ((src >= 0).sum(axis=1) == self.rows).all()


def masks_in_of(lo, P):
    """What the calls are given as masks: junk in every bit the rule ignores."""
    if lo.wide:
        return wm.with_high_junk(lo.masks, lo.k, lo.r, SEED + P)
    return _high(lo.masks, lo.k, lo.r, P)


# ------------------------------------------------------------------------------------------
# Device work, in slabs
# ------------------------------------------------------------------------------------------
def _slabs(G, bytes_per_group):
    step = max(1, SLAB_BYTES // bytes_per_group)
    return [(a, min(G, a + step)) for a in range(0, G, step)]


def put_junk(torch, ctx, buf, G, n, P, where, scratch):
    """buf as (G, n, P): shard (g, j) with where[g, j] gets the bytes of the junk stream at its own
    offset; every other byte stays."""
    for a, b in _slabs(G, n * P):
        w = where[a:b]
        if not bool(w.any()):
            continue
        size = (b - a) * n * P
        _run(torch, ctx, ctx.fill_random_dev, scratch, size, JUNK_SEED + n, a * n * P)
        buf[a * n * P:b * n * P].view(b - a, n, P)[w] = scratch[:size].view(b - a, n, P)[w]
    torch.cuda.synchronize()


def _truth_rows(torch, ctx, scratch, src, a, b, k, P, seed):
    """(written (n, r) bool, rows (nnz, P)): the stream's shards src[a:b] names, in (g, m) order."""
    n = b - a
    _run(torch, ctx, ctx.fill_random_dev, scratch, n * k * P, seed, a * k * P)
    truth = scratch[:n * k * P].view(n, k, P)
    s = src[a:b]
    written = s >= 0
    gi = torch.nonzero(written)[:, 0]
    return written, truth[gi, s[written]]


def check_slots(torch, ctx, out, lo, P, src, scratch, seed, what):
    G, k, r = lo.G, lo.k, lo.r
    for a, b in _slabs(G, k * P):
        n = b - a
        written, rows = _truth_rows(torch, ctx, scratch, src, a, b, k, P, seed)
        exp = torch.full((n, r, P), FILL, dtype=torch.uint8, device="cuda")
        exp[written] = rows
        got = out[a * r * P:b * r * P].view(n, r, P)
        if not torch.equal(got, exp):
            g = a + bb.first_true(torch, (got != exp).view(n, -1).any(dim=1))
            pytest.fail(f"{what}: the slots of group {g} (bytes {g * r * P}..{(g + 1) * r * P} of the output) are not "
                        f"its lost shards {np.flatnonzero(lo.ro.lost_d[g]).tolist()} followed by 0xA5; status {lo.status[g]}")
        del exp, rows, written


def check_packed(torch, ctx, out, rs, tot, lo, P, src, scratch, seed, what):
    G, k = lo.G, lo.k
    got_rs = rs.cpu().numpy().view(np.uint32).astype(np.int64)
    wrong = np.flatnonzero(got_rs != lo.row_start)
    assert len(wrong) == 0, f"{what}: row_start[{wrong[0]}] = {got_rs[wrong[0]]}, the host's sum is {lo.row_start[wrong[0]]}"
    assert int(tot.item()) == lo.total, f"{what}: *d_total"
    ends = lo.row_start + lo.rows
    for a, b in _slabs(G, k * P):
        _, rows = _truth_rows(torch, ctx, scratch, src, a, b, k, P, seed)
        t0, t1 = int(lo.row_start[a]), int(ends[b - 1])
        assert rows.shape[0] == t1 - t0
        got = out[t0 * P:t1 * P].view(t1 - t0, P)
        if not torch.equal(got, rows):
            t = t0 + bb.first_true(torch, (got != rows).any(dim=1))
            g = int(np.searchsorted(ends, t, side="right"))
            pytest.fail(f"{what}: packed row {t} (byte {t * P} of the output), row {t - lo.row_start[g]} of group {g}, "
                        f"is not its lost shard {np.flatnonzero(lo.ro.lost_d[g]).tolist()}")
        del rows
    tail = out[lo.total * P:]
    for s in range(0, int(tail.numel()), bb.SLAB):
        assert bool((tail[s:s + bb.SLAB] == FILL).all()), f"{what}: bytes after the last row were written"


def _group_rows(t, idx, G, per):
    """Groups idx of a flat device buffer of G groups of `per` bytes, on the host: (len(idx), per)."""
    return t.view(G, per)[idx].cpu().numpy()


# ------------------------------------------------------------------------------------------
# The case
# ------------------------------------------------------------------------------------------
class Names:
    """The calls of one row of the table, by family."""

    def __init__(self, slots=None, packed=(), decode=None):
        self.slots, self.packed, self.decode = slots, tuple(packed), decode


def _encode_checks(torch, ctx, oracle, data, whole, par, G, k, r, P, seed, crossing):
    # guard bytes around the parity
    assert bool((whole[:FRONT] == FILL).all()) and bool((whole[FRONT + G * r * P:] == FILL).all()), "guard bytes written"
    # host windows: the stream, and the oracle's parity of the group alone
    win = sorted(set(g for rows in crossing for g in bb.boundary_groups(G, rows, P)))
    idx = torch.tensor(win, device="cuda")
    d_win, p_win = _group_rows(data, idx, G, k * P), _group_rows(par, idx, G, r * P)
    for i, g in enumerate(win):
        assert np.array_equal(d_win[i], oracle.splitmix_bytes(k * P, seed, g * k * P)), f"data of group {g} is not the stream"
        assert np.array_equal(p_win[i], oracle.rs_encode(np.ascontiguousarray(d_win[i]), 1, k, r, P)), \
            f"encode: the parity of boundary group {g} (bytes {g * r * P}..{(g + 1) * r * P}) is not the oracle's"
    # the whole buffer: the same call over pieces whose offsets stay below 2^31
    ranges = bb.pieces(G, max(k, r) * P)
    scratch = _full(torch, max(g1 - g0 for g0, g1 in ranges) * r * P)
    for g0, g1 in ranges:
        n = (g1 - g0) * r * P
        scratch.fill_(FILL)
        _run(torch, ctx, ctx.encode_dev, data[g0 * k * P:g1 * k * P], g1 - g0, k, r, P, scratch[:n])
        piece = par[g0 * r * P:g1 * r * P]
        if not torch.equal(scratch[:n], piece):
            at = bb.first_true(torch, scratch[:n] != piece)
            pytest.fail(f"encode: group {g0 + at // (r * P)} (byte {g0 * r * P + at} of the parity) differs from the "
                        f"same call over groups {g0}..{g1} alone")
    del scratch
    return win


def run_case(torch, quicfec, oracle, hooks_lib, k, r, P, G, names, crosses, wide=False, ordinary=None,
             special_all_data=False, rounds=(None,), wide_rows_all=False, trace=None, refused=()):
    """One row of the table.  crosses: the buffers the row claims to cross, of data, parity, slots,
    packed.  rounds: decode_plan_mode of each pass over the recovers and the decode (None: as the
    context comes).  refused: (round, call) pairs include/fec_hip.h says are refused with
    FEC_ERR_RANGE.  trace: {"encode": (form, k, r, pol bit), "decode": form} to assert of one extra
    call through the test library."""
    emax = min(k, r)
    decodes = names.decode is not None
    seed = SEED + k * 1000 + r
    lo = S = None
    # ---- on the host, before anything is allocated or launched ----
    sizes = {"data": G * k * P, "parity": G * r * P, "slots": G * r * P}
    if decodes:
        # the rows that must still cross with the specials rebuilding nothing: the packed rows where
        # the row claims them, else its slots, else the data itself
        S = bb.special_every(G, emax if "packed" in crosses else r if "slots" in crosses else k, P)
        bits, kinds = draw_losses(G, k, r, S, k * 100 + r, ordinary, special_all_data)
        lo = Losses(bits, k, r, wide)
        sizes["packed"] = lo.total * P
        assert G * emax < 2**32
    for name in crosses:
        assert bb.crosses(sizes[name]), f"{name}: {sizes[name]} bytes do not cross 2^32 + 2^20"
    out_bytes = max([G * r * P if names.slots else 0] + [G * emax * P + BACK for _ in names.packed])
    _need(torch, sizes["data"] + sizes["parity"] + out_bytes + 4 * SLAB_BYTES + 2 * bb.SLAB + (1 << 30),
          f"k={k} r={r} P={P} G={G}")
    ctx = quicfec.Context(device=0)
    hooks = quicfec.Context(device=0, lib=hooks_lib) if trace else None
    def body():
        if wide_rows_all:
            ctx.wide_rows_mode(quicfec.FEC_WIDE_ROWS_ALL)
        data = torch.empty(G * k * P, dtype=torch.uint8, device="cuda")
        whole = _full(torch, FRONT + G * r * P + BACK)
        par = whole[FRONT:FRONT + G * r * P]
        _run(torch, ctx, ctx.fill_random_dev, data, G * k * P, seed)
        if trace and "encode" in trace:
            form, fk, fr, bit = trace["encode"]
            hooks.synchronize()
            quicfec.launch_trace(hooks.lib)
            _run(torch, hooks, hooks.encode_dev, data, G, k, r, P, par)
            recs = quicfec.launch_trace(hooks.lib)
            assert recs and all((t["form"], t["k"], t["r"]) == (form, fk, fr) and t["pol"] & bit == bit for t in recs), recs[:3]
            assert sum(t["items"] for t in recs) == G
            whole.fill_(FILL)
        # ---- encode ----
        _run(torch, ctx, ctx.encode_dev, data, G, k, r, P, par)
        win = _encode_checks(torch, ctx, oracle, data, whole, par, G, k, r, P, seed, [k, r])
        if not decodes:
            return
        # ---- what the decodes are given ----
        masks_in = masks_in_of(lo, P)
        dm = torch.from_numpy(masks_in.view(np.int64)).cuda()
        scratch = torch.empty(SLAB_BYTES, dtype=torch.uint8, device="cuda")      # every slab fits
        lost_d, unread_p = torch.from_numpy(lo.ro.lost_d).cuda(), torch.from_numpy(lo.ro.unread_p).cuda()
        src = torch.from_numpy(lo.src).cuda()
        put_junk(torch, ctx, par, G, r, P, unread_p, scratch)
        put_junk(torch, ctx, data, G, k, P, lost_d, scratch)
        # the windows of every buffer of the calls: data, parity, slots, and the groups of the packed rows
        ends = lo.row_start + lo.rows
        packed_groups = [int(np.searchsorted(ends, t, side="right")) for t in bb.boundary_groups(max(lo.total, 1), 1, P)
                         if t < lo.total]
        win = sorted(set(win) | set(packed_groups))
        idx = torch.tensor(win, device="cuda")
        d_in, p_in = _group_rows(data, idx, G, k * P), _group_rows(par, idx, G, r * P)
        ref, ref_status = d_in.copy(), np.zeros(len(win), dtype=np.uint8)
        for i, g in enumerate(win):
            stream = oracle.splitmix_bytes(k * P, seed, g * k * P)
            if k + r <= 64:
                row = np.ascontiguousarray(ref[i])
                m1 = np.ascontiguousarray(masks_in.reshape(G, -1)[g, :1])
                _, st = oracle.rs_decode(row, np.ascontiguousarray(p_in[i]), m1, 1, k, r, P)
                ref[i], ref_status[i] = row, st[0]
                assert st[0] == lo.status[g] and (st[0] == 1 or np.array_equal(row, stream)), g
            else:
                ref_status[i] = lo.status[g]
                if lo.status[g] == 0:
                    ref[i] = stream
        bad = torch.from_numpy(np.flatnonzero(lo.status == 1)).cuda()
        bad_in = data.view(G, k * P)[bad].clone()

        def window_slots(o, what):
            o_win = _group_rows(o, idx, G, r * P).reshape(len(win), r, P)
            for i, g in enumerate(win):
                exp = np.full((r, P), FILL, dtype=np.uint8)
                if ref_status[i] == 0:
                    lost = np.flatnonzero(lo.ro.lost_d[g])
                    exp[:len(lost)] = ref[i].reshape(k, P)[lost]
                assert np.array_equal(o_win[i], exp), f"{what}: the slots of boundary group {g} are not the oracle's"

        def window_packed(o, what):
            for i, g in enumerate(win):
                t, n = int(lo.row_start[g]), int(lo.rows[g])
                got = o[t * P:(t + n) * P].cpu().numpy().reshape(n, P)
                lost = np.flatnonzero(lo.ro.lost_d[g])[:n]
                assert np.array_equal(got, ref[i].reshape(k, P)[lost]), \
                    f"{what}: rows {t}..{t + n} of boundary group {g} are not the oracle's"

        def statuses(st, what):
            got = st.cpu().numpy()
            wrong = np.flatnonzero(got != lo.status)
            assert len(wrong) == 0, f"{what}: status of group {wrong[0]} is {got[wrong[0]]}"
            assert _masks_unwritten(dm, masks_in), f"{what}: the masks were written"

        if trace and "decode" in trace:
            hooks.synchronize()
            quicfec.launch_trace(hooks.lib)
            _run(torch, hooks, hooks.decode_dev, data, par, dm, G, k, r, P, None)
            recs = [t for t in quicfec.launch_trace(hooks.lib) if t["form"] != "classify"]
            assert recs and all((t["form"], t["k"], t["r"]) == (trace["decode"], k, r) for t in recs), recs[:3]
            assert sum(t["items"] for t in recs) == G
            put_junk(torch, ctx, data, G, k, P, lost_d, scratch)

        for rnd, mode in enumerate(rounds):
            if mode is not None:
                ctx.decode_plan_mode(mode)
            tag = f"round {rnd}: "
            if rnd > 0:
                put_junk(torch, ctx, data, G, k, P, lost_d, scratch)
            # ---- recover, slots ----
            if names.slots:
                out, st = _full(torch, G * r * P), _full(torch, G, 7)
                _run(torch, ctx, getattr(ctx, names.slots), data, par, dm, G, k, r, P, out, st)
                statuses(st, tag + names.slots)
                window_slots(out, tag + names.slots)
                check_slots(torch, ctx, out, lo, P, src, scratch, seed, tag + names.slots)
                out = None
            # ---- recover, packed ----
            for name in names.packed:
                out, st = _full(torch, G * emax * P + BACK), _full(torch, G, 7)
                rs = torch.full((G,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")
                tot = torch.full((1,), -5, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                if (rnd, name) in refused:
                    with pytest.raises(quicfec.FecError) as ei:
                        getattr(ctx, name)(data, par, dm, G, k, r, P, out, rs, tot, st)
                    ctx.synchronize()
                    assert ei.value.code == quicfec.FEC_ERR_RANGE
                    assert bool((out == FILL).all()) and bool((rs == 0x3C3C3C3C).all()) and int(tot.item()) == -5
                    assert bool((st == 7).all())
                else:
                    _run(torch, ctx, getattr(ctx, name), data, par, dm, G, k, r, P, out, rs, tot, st)
                    statuses(st, tag + name)
                    window_packed(out, tag + name)
                    check_packed(torch, ctx, out, rs, tot, lo, P, src, scratch, seed, tag + name)
                out = rs = None
            # ---- decode in place ----
            st = _full(torch, G, 7)
            _run(torch, ctx, getattr(ctx, names.decode), data, par, dm, G, k, r, P, st)
            statuses(st, tag + names.decode)
            d_out = _group_rows(data, idx, G, k * P)
            for i, g in enumerate(win):
                assert np.array_equal(d_out[i], ref[i]), f"{tag}{names.decode}: boundary group {g} is not the oracle's"
            # unrecoverable groups are left as they came; refilled, the buffer is the stream again
            assert torch.equal(data.view(G, k * P)[bad], bad_in), f"{tag}{names.decode}: an unrecoverable group was written"
            torch.cuda.synchronize()
            for g in np.flatnonzero(lo.status == 1):
                ctx.fill_random_dev(data[g * k * P:(g + 1) * k * P], k * P, seed, int(g) * k * P)
            ctx.synchronize()
            at = bb.same_as_stream(ctx, torch, data, seed)
            assert at is None, (f"{tag}{names.decode}: byte {at} of the data (group {at // (k * P)}, shard {at // P % k}) "
                                f"is not the stream's")
            if rnd + 1 < len(rounds):                             # the next round's unrecoverable groups come as before
                data.view(G, k * P)[bad] = bad_in
    _run_and_free(torch, body, ctx, hooks)


# ------------------------------------------------------------------------------------------
# The table
# ------------------------------------------------------------------------------------------
@pytest.fixture
def env(torch_cuda, quicfec_mod, oracle_mod, quicfec_hooks):
    return torch_cuda, quicfec_mod, oracle_mod, quicfec_hooks


def test_k10_r3_product_forms(env):
    """The headline shape past the headline size: encode_v16<10,3> staged, the mask-addressed slot
    recover, both packed recovers, decode_fused.  Data crosses three lines, parity, slots and packed
    rows one."""
    run_case(*env, 10, 3, 1200, 1_200_000, Names("recover_dev", ("recover_packed_dev", "recover_packed_any_dev"), "decode_dev"),
             crosses=("data", "parity", "slots", "packed"),
             trace={"encode": ("encode_v16", 10, 3, STAGE), "decode": "decode_fused"})


def test_k20_r5_bit_sliced_and_record_addressed(env):
    """encode_bits<20,5>, the record-addressed recovers and decode_fused.  Data crosses four lines."""
    run_case(*env, 20, 5, 1200, 720_000, Names("recover_dev", ("recover_packed_any_dev",), "decode_dev"),
             crosses=("data", "parity", "slots", "packed"),
             trace={"encode": ("encode_bits", 20, 5, 0), "decode": "decode_fused"})


def test_k16_r16_runtime_k_both_plans(env):
    """Runtime k at an odd packet size, two row passes of the encode; the recovers and the decode once
    with the host-built sparse plan and once with records built on the device.  The packed recover
    never reads masks back: on a context in FEC_PLAN_CODEBOOK it refuses this shape with nothing
    written (include/fec_hip.h), which the first round asserts."""
    quicfec = env[1]
    run_case(*env, 16, 16, 1201, 224_000, Names("recover_dev", ("recover_packed_any_dev",), "decode_dev"),
             crosses=("data", "parity", "slots", "packed"), rounds=(quicfec.FEC_PLAN_CODEBOOK, quicfec.FEC_PLAN_DEVICE),
             refused=((0, "recover_packed_any_dev"),))


def test_k8_r8_byte_per_lane_encode(env):
    """P < 16: the byte-per-lane encode, 44.8 million groups.  Encode only."""
    run_case(*env, 8, 8, 12, 44_800_000, Names(), crosses=("data", "parity"))


def test_k10_r1_xor_only(env):
    """The XOR-only encode and its decode.  Only the data crosses: parity past the line would take
    43 GB of data at r = 1."""
    run_case(*env, 10, 1, 1200, 360_000, Names(decode="decode_dev"), crosses=("data",))


def test_k40_r32_wide_four_word_masks(env):
    """The wide decoders at min(k, r) = 32: slots, packed rows and in place, masks of four words."""
    run_case(*env, 40, 32, 1200, 112_000, Names("recover_wide_dev", ("recover_packed_wide_dev",), "decode_wide_dev"),
             crosses=("data", "parity", "slots", "packed"), wide=True)


def test_k66_r66_deep_rows(env):
    """Past the cap on min(k, r), FEC_WIDE_ROWS_ALL: the deep path.  Ordinary groups lose 1 to 4 data
    shards and each special group all 66: slot offsets do not depend on e, and the packed crossing is
    the 40 + 32 case's."""
    run_case(*env, 66, 66, 1200, 54_400, Names("recover_wide_dev", (), "decode_wide_dev"),
             crosses=("data", "parity", "slots"), wide=True, ordinary=(1, 4), special_all_data=True, wide_rows_all=True)


# ------------------------------------------------------------------------------------------
# Address-table calls: the contiguous outputs of the gather calls past 4 GiB
# ------------------------------------------------------------------------------------------
# Sources may alias, so the cost is tables, not packets.  An arena of M = 1021 groups is built, run
# and checked against the oracle byte for byte by the helpers of test_gpu_gather.py and
# test_gpu_gather_var.py (arena parity from encode_dev, checked against the oracle for all M groups).
# Group g of the big call points at arena group g % M, with its lost entries and its lengths, so its
# output must be the M-group call's output for g % M: compared on the device, in slabs.
# M * rows * P has an odd factor, so a write displaced by 2^32 bytes lands on other content.
M = 1021


def _rep(torch, a, b):
    return torch.arange(a, b, device="cuda") % M


def big_table(torch, small, G, n):
    """(G * n,) of small's dtype: row g is row g % M of small (M, n), built in slabs."""
    small = small.view(M, n)
    out = torch.empty(G * n, dtype=small.dtype, device="cuda")
    for a, b in _slabs(G, n * small.element_size()):
        out[a * n:b * n].view(b - a, n).copy_(small[_rep(torch, a, b)])
    return out


def check_against_small(torch, out, G, small, what):
    """out as (G, per): row g equals row g % M of small (M, per); the first group that differs is named."""
    small = small.reshape(M, -1)
    per = small.shape[1]
    out = out.view(G, per)
    for a, b in _slabs(G, per * small.element_size()):
        exp = small[_rep(torch, a, b)]
        if not torch.equal(out[a:b], exp):
            g = a + bb.first_true(torch, (out[a:b] != exp).any(dim=1))
            pytest.fail(f"{what}: group {g} (bytes {g * per}..{(g + 1) * per} of the output) is not the {M}-group call's "
                        f"group {g % M}")
        del exp


def _a5(torch, small_out, written):
    """The M-group call's slots with 0xA5 where it wrote nothing (its helpers prefill 0x5A)."""
    exp = small_out.clone().view(M, written.shape[1], -1)
    exp[torch.from_numpy(~written).cuda()] = FILL
    return exp


def _written(c):
    lost_d = c.lost[:, :c.k]
    w = np.zeros((c.G, c.r), dtype=bool)
    gi, ji = np.nonzero(lost_d & (c.status == 0)[:, None])
    w[gi, (np.cumsum(lost_d, axis=1) - 1)[gi, ji]] = True
    return w


def _windows(torch, out, G, r, P, want, what):
    """Boundary groups of the output on the host against the oracle's rows of the arena group."""
    win = bb.boundary_groups(G, r, P)
    got = _group_rows(out, torch.tensor(win, device="cuda"), G, r * P)
    for i, g in enumerate(win):
        assert np.array_equal(got[i], want[g % M].reshape(-1)), f"{what}: boundary group {g} is not the oracle's"


def test_gather_calls_contiguous_outputs(env):
    """fec_recover_gather_rs_dev, fec_encode_gather_rs_dev and the two calls with a length per entry
    (lengths drawn from 16..P) at k=10 r=3 P=1200, 1.2 million groups: the output is 4.32 GB, the
    table 125 MB."""
    torch, quicfec, oracle, _ = env
    import test_gpu_gather as gg
    import test_gpu_gather_var as gv
    k, r, P, G = 10, 3, 1200, 1_200_000
    assert bb.crosses(G * r * P) and 2**32 % (M * r * P) != 0 and G % M != 0
    _need(torch, G * r * P + G * (k + r) * 12 + 6 * SLAB_BYTES + (1 << 30), f"gather calls k={k} r={r} P={P} G={G}")
    rng = np.random.default_rng([SEED, 0x7AB1E])
    masks = gg.perm_masks(k, r, M, SEED + 1)
    c = gg.make_case(oracle, k, r, P, masks, SEED + 2)
    dl, pl = rng.integers(16, P + 1, size=(M, k)), rng.integers(16, P + 1, size=(M, r))
    cv = gv.make_case(oracle, k, r, P, masks, dl, pl, SEED + 3)
    present = rng.random((M, k)) < 0.85
    present[:3] = [[True] * k, [False] * k, [False] * (k - 1) + [True]]
    ce = gv.make_case(oracle, k, r, P, [0] * M, dl, np.zeros((M, r), dtype=np.int64), SEED + 4, present=present)
    ctx = quicfec.Context(device=0)
    def body():
        # the arena's parity: encode_dev's, checked against the oracle for all M groups
        dd, dp = torch.from_numpy(np.array(c.data)).cuda(), _full(torch, M * r * P)
        _run(torch, ctx, ctx.encode_dev, dd, M, k, r, P, dp)
        assert np.array_equal(dp.cpu().numpy(), c.par)

        def outputs():
            whole = _full(torch, G * r * P + BACK)
            return whole, whole[:G * r * P]

        def per_group(got, small, what):
            assert torch.equal(got, small[_rep(torch, 0, G)]), f"{what} differs from the {M}-group call's"

        # ---- recover_gather_dev ----
        b = gg.run_recover(torch, ctx, c, SEED + 5)                      # every byte against the oracle
        table = big_table(torch, b.table, G, k + r)
        whole, out = outputs()
        st, mo = _full(torch, G, 7), torch.full((G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
        _run(torch, ctx, ctx.recover_gather_dev, table, G, k, r, P, out, st, mo)
        small = _a5(torch, b.out, _written(c))
        check_against_small(torch, out, G, small, "recover_gather_dev")
        _windows(torch, out, G, r, P, small.cpu().numpy(), "recover_gather_dev")
        per_group(st, b.st, "recover_gather_dev: status")
        per_group(mo, b.mo, "recover_gather_dev: masks")
        assert bool((whole[G * r * P:] == FILL).all())
        # ---- recover_gather_var_dev ----
        b = gv.run_recover(torch, ctx, cv, SEED + 6)
        table, lens = big_table(torch, b.table, G, k + r), big_table(torch, b.lens, G, k + r)
        whole.fill_(FILL)
        st.fill_(7)
        sym = torch.full((G,), 0x77777777, dtype=torch.int32, device="cuda")
        _run(torch, ctx, ctx.recover_gather_var_dev, table, lens, G, k, r, P, out, st, mo, sym)
        small = _a5(torch, b.out, _written(cv))
        check_against_small(torch, out, G, small, "recover_gather_var_dev")
        _windows(torch, out, G, r, P, small.cpu().numpy(), "recover_gather_var_dev")
        per_group(st, b.st, "recover_gather_var_dev: status")
        per_group(mo, b.mo, "recover_gather_var_dev: masks")
        per_group(sym, b.sym, "recover_gather_var_dev: symbol lengths")
        assert bool((whole[G * r * P:] == FILL).all())
        # ---- encode_gather_dev ----
        e = gg.make_encode(torch, c, SEED + 7)
        _run(torch, ctx, gg.launch_encode, ctx, e)
        gg.check_encode(e)
        table = big_table(torch, e.table, G, k)
        whole.fill_(FILL)
        _run(torch, ctx, ctx.encode_gather_dev, table, G, k, r, P, out)
        check_against_small(torch, out, G, e.par, "encode_gather_dev")
        _windows(torch, out, G, r, P, np.asarray(c.par).reshape(M, r * P), "encode_gather_dev")
        assert bool((whole[G * r * P:] == FILL).all())
        # ---- encode_gather_var_dev ----
        e = gv.make_encode(torch, ce, SEED + 8)
        _run(torch, ctx, gv.launch_encode, ctx, e)
        gv.check_encode(e)
        table, lens = big_table(torch, e.table, G, k), big_table(torch, e.lens, G, k)
        whole.fill_(FILL)
        sym.fill_(0x77777777)
        _run(torch, ctx, ctx.encode_gather_var_dev, table, lens, G, k, r, P, out, sym)
        check_against_small(torch, out, G, e.par, "encode_gather_var_dev")
        _windows(torch, out, G, r, P, np.asarray(ce.par).reshape(M, r * P), "encode_gather_var_dev")
        per_group(sym, e.sym, "encode_gather_var_dev: symbol lengths")
        assert bool((whole[G * r * P:] == FILL).all())
    _run_and_free(torch, body, ctx)


# ------------------------------------------------------------------------------------------
# Address tables whose own bytes pass 4 GiB (addrs + g0 * n, entries = gn * n)
# ------------------------------------------------------------------------------------------
TRAP = 0x7FFFFFFF                    # the length of a lost entry: ignored


def table_case(oracle, k, r, P, with_lens, salt):
    """M groups for the scatter calls at r = 1, on the host: packets (zero past their length), the
    parity the oracle gives, one lost data shard per group, and what the two calls must leave at a
    16-byte destination row prefilled with 0xA5."""
    assert r == 1 and P == 16
    rng = np.random.default_rng([SEED, salt])
    raw = oracle.splitmix_bytes(M * k * P, SEED + salt).reshape(M, k, P)
    if with_lens:
        sym = rng.integers(1, P + 1, size=M)                                  # the group's symbol length
        sym[:4] = [P, 1, P - 1, 5]
        dlens = rng.integers(0, P + 1, size=(M, k)) % (sym[:, None] + 1)
        dlens[np.arange(M), rng.integers(0, k, size=M)] = sym               # one packet has it
        plens = rng.integers(sym, P + 1)                                    # a repair packet carries at least that
    else:
        sym, dlens, plens = np.full(M, P), np.full((M, k), P), np.full(M, P)
    data = np.where(np.arange(P)[None, None, :] < dlens[:, :, None], raw, 0).astype(np.uint8)
    par = oracle.rs_encode(np.ascontiguousarray(data).reshape(-1), M, k, r, P).reshape(M, P)
    assert np.array_equal(par, np.bitwise_xor.reduce(data, axis=1))          # row 0 is the XOR repair packet
    assert not (par * (np.arange(P)[None, :] >= sym[:, None])).any()
    lost = rng.integers(0, k, size=M)
    lost[:2] = [0, k - 1]
    # encode: exactly sym bytes of the row
    enc = np.full((M, P), FILL, dtype=np.uint8)
    cut = np.arange(P)[None, :] < sym[:, None]
    enc[cut] = par[cut]
    # recover: the symbol length over the present entries, that many bytes of the lost packet
    present = np.ones((M, k), dtype=bool)
    present[np.arange(M), lost] = False
    sym_rec = np.maximum(np.where(present, dlens, 0).max(axis=1), plens)
    want = data[np.arange(M), lost]
    others = np.where(present[:, :, None], data, 0)
    assert np.array_equal(np.bitwise_xor.reduce(others, axis=1) ^ par, want)   # what the one row rebuilds
    if k + r <= 64:
        broken = np.where(present[:, :, None], data, 0xEE).astype(np.uint8).reshape(-1)
        masks = np.left_shift(np.uint64(1), lost.astype(np.uint64))
        bad, _ = oracle.rs_decode(broken, np.ascontiguousarray(par).reshape(-1), masks, M, k, r, P)
        assert bad == 0 and np.array_equal(broken.reshape(M, k, P), data)
    rec = np.full((M, P), FILL, dtype=np.uint8)
    cut = np.arange(P)[None, :] < sym_rec[:, None]
    rec[cut] = want[cut]
    # what the arena holds: the raw packets, and each parity row cut at its length with 0xEE after it
    praw = np.where(np.arange(P)[None, :] < plens[:, None], par, 0xEE).astype(np.uint8)
    return dict(raw=raw, praw=praw, dlens=dlens, plens=plens, sym=sym, sym_rec=sym_rec, lost=lost, enc=enc, rec=rec)


@pytest.mark.parametrize("k,G,wide,with_lens", [(63, 8_600_000, False, False), (255, 2_200_000, True, True),
                                                (255, 2_200_000, True, False)],
                         ids=["one_word_k63", "wide_k255_lens", "wide_k255_no_lens"])
def test_scatter_tables_past_4gib(env, k, G, wide, with_lens):
    """The scatter encode and the scatter recover (one lost data shard per group) at r = 1, P = 16,
    with so many groups that the address table's own bytes pass 4 GiB: 4.33 and 4.40 GB at k = 63
    (one-word calls), 4.49 and 4.51 GB at k = 255 (wide calls, with a length table and without).
    Sources are an arena of M groups; destinations are distinct 16-byte rows of an arena prefilled
    with 0xA5, and the recover's ignored destination entries point at trap rows that must stay 0xA5."""
    torch, quicfec, oracle, _ = env
    r, P = 1, 16
    n = k + r
    assert bb.crosses(G * k * 8) and bb.crosses(G * n * 8) and G % M != 0
    assert 2**32 % (M * k * 8) != 0 and 2**32 % (M * n * 8) != 0
    _need(torch, 2 * G * n * 8 + G * n * 4 + G * 64 + 4 * SLAB_BYTES + (1 << 30), f"scatter tables k={k} G={G}")
    c = table_case(oracle, k, r, P, with_lens, k + int(with_lens))
    ctx = quicfec.Context(device=0)
    encode = ctx.encode_scatter_wide_dev if wide else ctx.encode_scatter_dev
    recover = ctx.recover_scatter_wide_dev if wide else ctx.recover_scatter_dev
    words = 4 if wide else 1
    def body():
        table = lens = dest = arena = None
        # the source arena at an odd address, and the M-group tables
        src = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), c["raw"].reshape(-1), c["praw"].reshape(-1)])).cuda()
        d0 = src.data_ptr() + 3
        p0 = d0 + M * k * P
        addr_d = d0 + (np.arange(M * k, dtype=np.int64) * P).reshape(M, k)
        addr_p = p0 + (np.arange(M, dtype=np.int64) * P).reshape(M, 1)
        rec_addr = np.concatenate([addr_d, addr_p], axis=1)
        rec_addr[np.arange(M), c["lost"]] = 0
        rec_lens = np.concatenate([c["dlens"], c["plens"][:, None]], axis=1)
        rec_lens[np.arange(M), c["lost"]] = TRAP
        trap = _full(torch, k * P)
        trap_m = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(trap.data_ptr() + np.arange(k, dtype=np.int64) * P, (M, k)))).cuda()
        lost_m = torch.from_numpy(c["lost"]).cuda()
        masks_m = np.zeros((M, words), dtype=np.uint64)
        masks_m[np.arange(M), c["lost"] >> 6] = np.left_shift(np.uint64(1), (c["lost"] & 63).astype(np.uint64))
        small = {"enc_addr": addr_d, "enc_lens": c["dlens"].astype(np.int32), "rec_addr": rec_addr,
                 "rec_lens": rec_lens.astype(np.int32)}
        small = {name: torch.from_numpy(np.ascontiguousarray(a)).cuda() for name, a in small.items()}

        def dests(groups, arena, recovering):
            """The destination table of `groups` groups: row g of the arena for the row the call writes."""
            rows = arena.data_ptr() + torch.arange(groups, device="cuda") * P
            if not recovering:
                return rows
            out = torch.empty(groups * k, dtype=torch.int64, device="cuda")
            for a, b in _slabs(groups, k * 8):
                t = trap_m[_rep(torch, a, b)]
                t[torch.arange(b - a, device="cuda"), lost_m[_rep(torch, a, b)]] = rows[a:b]
                out[a * k:b * k].view(b - a, k).copy_(t)
            return out

        def call(groups, recovering):
            """One call over `groups` groups, group g standing for arena group g % M.  Returns the
            destination arena and the per-group outputs; the tables stay in the enclosing scope."""
            nonlocal table, lens, dest, arena
            table = lens = dest = arena = None
            width = n if recovering else k
            which = "rec" if recovering else "enc"
            table = big_table(torch, small[which + "_addr"], groups, width)
            lens = big_table(torch, small[which + "_lens"], groups, width) if with_lens else None
            arena = _full(torch, groups * P + BACK)
            dest = dests(groups, arena, recovering)
            sym = torch.full((groups,), 0x77777777, dtype=torch.int32, device="cuda")
            if recovering:
                st = _full(torch, groups, 7)
                mo = torch.full((groups * words,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
                _run(torch, ctx, recover, table, lens, dest, groups, k, r, P, st, mo, sym)
                return arena, {"status": st, "masks": mo.view(groups, words), "symbol lengths": sym}
            _run(torch, ctx, encode, table, lens, dest, groups, k, r, P, sym)
            return arena, {"symbol lengths": sym}

        for recovering, what in ((False, encode.__name__), (True, recover.__name__)):
            # the M-group call, every byte against the host
            got_m, outs_m = call(M, recovering)
            got_m = got_m.clone()
            want = c["rec"] if recovering else c["enc"]
            assert np.array_equal(got_m[:M * P].cpu().numpy().reshape(M, P), want), f"{what} at G = {M}"
            assert bool((got_m[M * P:] == FILL).all()) and bool((trap == FILL).all())
            assert np.array_equal(outs_m["symbol lengths"].cpu().numpy(), c["sym_rec"] if recovering else c["sym"])
            if recovering:
                assert not outs_m["status"].any()
                assert np.array_equal(outs_m["masks"].cpu().numpy().view(np.uint64), masks_m)
            # the big call
            assert bb.crosses(G * (n if recovering else k) * 8)
            got, outs = call(G, recovering)
            check_against_small(torch, got[:G * P], G, got_m[:M * P], what)
            for name, t in outs.items():
                assert torch.equal(t, outs_m[name][_rep(torch, 0, G)]), f"{what}: {name} differ from the {M}-group call's"
            assert bool((got[G * P:] == FILL).all()) and bool((trap == FILL).all()), f"{what}: guard or trap rows written"
            # host windows: the boundary groups of every table that crosses
            width = n if recovering else k
            crossing = [(table, width)] + ([(dest, k)] if recovering else [])
            win = sorted(set(g for _, w in crossing for g in bb.boundary_groups(G, w, 8)))
            idx = torch.tensor(win, device="cuda")
            rows = got[:G * P].view(G, P)[idx].cpu().numpy()
            tab = table.view(G, width)[idx].cpu().numpy()
            small_tab = small[("rec" if recovering else "enc") + "_addr"].cpu().numpy()
            for i, g in enumerate(win):
                assert np.array_equal(tab[i], small_tab[g % M]), f"{what}: the table's row {g}"
                assert np.array_equal(rows[i], want[g % M]), f"{what}: the row of boundary group {g} is not the host's"
            if recovering:
                dwin = dest.view(G, k)[idx].cpu().numpy()
                for i, g in enumerate(win):
                    assert dwin[i, c["lost"][g % M]] == arena.data_ptr() + g * P
    _run_and_free(torch, body, ctx)
