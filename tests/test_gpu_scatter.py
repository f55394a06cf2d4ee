"""fec_recover_scatter_rs_dev on the GPU: the address-table recover that writes every rebuilt packet
to a table of destinations, exactly the group's symbol length L_g of it.  Expected bytes come from
the oracle on zero-padded inputs (test_gpu_gather_var.make_case).  Bit-exact, no tolerance.

Source arenas are test_gpu_gather_var.build_arena's.  Destinations live in an allocation pre-filled
0x5A (a guard of 256 bytes at each end); by default each destination has exactly L_g bytes and is
followed by a pad of 1..37 bytes, so destination addresses take every residue mod 16 and a byte
written before a destination or at or past destination + L_g changes a byte that must stay 0x5A.
The entries the call must ignore (present shards, untouched groups, unrecoverable groups) point
into a canary buffer of P bytes between guards, filled 0xC3: a valid address, so a wrong kernel
fails a comparison instead of faulting.

After every call: the source arenas are byte-identical to before; the whole destination allocation
equals the expected image (rows in place, 0x5A everywhere else); the canary is intact; status
(pre-filled 7), the derived masks and the symbol lengths equal the expected ones.
"""
import os
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_gather import GUARD, _planted, guarded, hooks_ctx, iid_masks, perm_masks, product_ctx
from test_gpu_gather_var import (G_MAIN, JUNK_LEN, build_arena, dealt_lengths, edge_lengths, main_case, make_case,
                                 upload_arena)
from test_scatter_forms import expected_launches                            # the table of DESIGN.md §5b
import test_gpu_gather_var as var

pytestmark = pytest.mark.gpu

SEED = 0x5CA70000
SHAPES = [(10, 3), (20, 5), (4, 2), (6, 3), (12, 9)]                         # three compiled, runtime k in one and in two passes
SIZES = [16, 17, 260, 1025, 1200, 2100]


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# What a call must write, and where
# ------------------------------------------------------------------------------------------
def rebuilt_rows(c):
    """(g, j, m) of every row the call rebuilds: data shard j of a recoverable group g, its m-th lost."""
    lost_d = c.lost[:, :c.k]
    gi, ji = np.nonzero(lost_d & (c.status == 0)[:, None])
    return gi, ji, (np.cumsum(lost_d, axis=1) - 1)[gi, ji]


def symbol_lengths(c, with_lens):
    """L_g: the largest clamped length of the present entries; without a length table P when any is present."""
    if with_lens:
        return c.sym_rec.astype(np.int64)
    return np.where((~c.lost).any(axis=1), c.P, 0).astype(np.int64)


def padded_layout(seed):
    """Exactly L bytes per destination, in a seeded random order, a pad of 1..37 bytes before each."""
    def place(c, gi, ji, mi, L):
        rng = np.random.default_rng(seed)
        offs = np.zeros(len(gi), dtype=np.int64)
        fill = GUARD
        for i, pad in zip(rng.permutation(len(gi)), rng.integers(1, 38, size=len(gi))):
            fill += int(pad)
            offs[i] = fill
            fill += int(L[i])
        return fill + GUARD, offs
    return place


def slot_layout(c, gi, ji, mi, L):
    """The slot layout of the gather recovers: row m of group g at (g * r + m) * P."""
    return GUARD + c.G * c.r * c.P + GUARD, GUARD + (gi * c.r + mi) * c.P


def packed_layout(c, gi, ji, mi, L):
    """Back to back in (g, m) order, no byte between two destinations."""
    return GUARD + int(L.sum()) + GUARD, GUARD + np.concatenate([[0], np.cumsum(L)[:-1]]).astype(np.int64)


def make_scatter(torch, c, seed, layout, with_lens=True, unwanted=None, want_sym=True):
    """Arena, tables, destination allocation and pre-filled outputs of one scatter recover of case c.
    unwanted: bool per rebuilt row, True = its destination entry is 0.  Everything is uploaded on
    torch's stream: synchronise before launching on a side stream."""
    arenas, where, lens = build_arena(c, seed)
    b = SimpleNamespace(c=c, with_lens=with_lens)
    dev, b.table, b.lens = upload_arena(torch, arenas, where, lens)
    if not with_lens:
        assert (c.lens[~c.lost] == c.P).all()                                # NULL table = every present shard has P
        b.lens = None
    gi, ji, mi = rebuilt_rows(c)
    b.sym = symbol_lengths(c, with_lens)
    L = b.sym[gi]
    nbytes, offs = layout(c, gi, ji, mi, L)
    wanted = np.ones(len(gi), dtype=bool) if unwanted is None else ~unwanted
    image = np.full(nbytes, 0x5A, dtype=np.uint8)
    for i in np.nonzero(wanted)[0]:
        assert (image[offs[i]:offs[i] + L[i]] == 0x5A).all()                  # destinations do not overlap
        image[offs[i]:offs[i] + L[i]] = c.data[gi[i], ji[i], :L[i]]
    b.dest = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    b.canary = torch.full((GUARD + c.P + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    tab = np.full((c.G, c.k), b.canary.data_ptr() + GUARD, dtype=np.uint64)  # ignored entries: a valid address
    tab[gi, ji] = np.where(wanted, np.uint64(b.dest.data_ptr()) + offs.astype(np.uint64), np.uint64(0))
    b.offs, b.rows = offs, (gi, ji, mi)
    b.dtab = torch.from_numpy(tab.reshape(-1).view(np.int64)).to("cuda")
    b.images = list(zip(dev, arenas)) + [(b.dest, image), (b.canary, np.full(GUARD + c.P + GUARD, 0xC3, dtype=np.uint8))]
    b.st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
    b.mo = torch.full((c.G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    b.so = torch.full((c.G,), 0x77777777, dtype=torch.int32, device="cuda") if want_sym else None
    return b


def launch_scatter(ctx, b, stream=None, masks=True):
    """masks=False: d_masks_out NULL (a device-plan shape then keeps its masks in the stream's workspace)."""
    c = b.c
    ctx.recover_scatter_dev(b.table, b.lens, b.dtab, c.G, c.k, c.r, c.P, b.st, b.mo if masks else None, b.so, stream=stream)


def check_scatter(b, what="", masks=True):
    """masks=False: the call was given no d_masks_out, so b.mo still holds its fill."""
    c = b.c
    what = (what, c.k, c.r, c.P, c.G, b.with_lens)
    for n, (d, image) in enumerate(b.images):
        got = d.cpu().numpy()
        bad = np.nonzero(got != image)[0]
        assert bad.size == 0, (what, "buffer", n, "of", len(b.images), "first wrong bytes at", bad[:8], got[bad[:8]])
    assert np.array_equal(b.st.cpu().numpy(), c.status), what
    if masks:
        assert np.array_equal(b.mo.cpu().numpy().view(np.uint64), c.masks), what
    else:
        assert (b.mo.cpu().numpy() == 0x3C3C3C3C3C3C3C3C).all(), what
    if b.so is not None:
        assert np.array_equal(b.so.cpu().numpy().view(np.uint32), b.sym.astype(np.uint32)), what


def run_scatter(torch, ctx, c, seed, layout, what="", **kw):
    b = make_scatter(torch, c, seed, layout, **kw)
    launch_scatter(ctx, b)
    ctx.synchronize()
    check_scatter(b, what)
    return b


def full_case(oracle, k, r, P, G, seed):
    """Every length P (the inputs of the fixed-length call), permutation masks with the planted groups."""
    full = np.full((G, k + r), P)
    c = make_case(oracle, k, r, P, perm_masks(k, r, G, seed), full[:, :k], full[:, k:], seed + 1)
    assert c.rows > 0
    return c


# ------------------------------------------------------------------------------------------
# 1. Every cut
# ------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cut_case(oracle, k, r, P):
    """G = 67.  Groups 0..4 are the planted ones (untouched, parity-only loss, unrecoverable, the XOR
    path, the GF path with e = 1) under dealt lengths.  From group 5 on a cap cycles through the edge
    lengths within [0, P]: every length of the group is clamped to the cap and its first surviving data
    shard sits exactly at it, so L_g = cap.  The first cycle loses one data shard (odd groups parity
    row 0 too, r >= 2), the second two (r >= 2), the groups after that up to min(r, 3)."""
    caps = edge_lengths(P)
    caps = caps[caps <= P]
    n = len(caps)
    assert 5 + 2 * n <= G_MAIN
    masks = np.zeros(G_MAIN, dtype=np.uint64)
    masks[:5] = _planted(k, r)
    dl = dealt_lengths(P, G_MAIN, k)
    pl = dealt_lengths(P, G_MAIN, r, shift=k)
    for g in range(5, G_MAIN):
        i = g - 5
        cycle, cap = i // n, int(caps[i % n])
        first = g % k
        if cycle == 0:
            m = (1 << first) | ((1 << k) if (g % 2 == 1 and r >= 2) else 0)
        else:
            lose = 1 if r < 2 else 2 if cycle == 1 else min(r, 3)
            m = sum(1 << ((first + 2 * t) % k) for t in range(lose))
        masks[g] = m
        dl[g] = np.minimum(dl[g], cap)
        pl[g] = np.minimum(pl[g], cap)
        dl[g, [j for j in range(k) if not (m >> j) & 1][0]] = cap
    c = make_case(oracle, k, r, P, masks, dl, pl, SEED + k * 100000 + r * 10000 + P)
    e = c.lost[:, :k].sum(axis=1) * (c.status == 0)
    assert c.masks[0] == 0 and e[1] == 0 and c.masks[1] != 0 and c.status[2] == 1 and e[3] == 1 and e[4] == 1
    assert not c.lost[3, k] and (r < 2 or c.lost[4, k])                      # XOR path; GF path with e = 1
    for cap in caps:                                                          # every cut, in one row and in two
        assert ((e == 1) & (c.sym_rec == cap)).any(), (k, r, P, cap)
        assert r < 2 or ((e == 2) & (c.sym_rec == cap)).any(), (k, r, P, cap)
    return c


def test_destinations_take_every_residue_and_exactly_the_symbol_length(oracle_mod):
    """On the CPU: the padded layout gives each destination exactly L_g bytes, pads of 1..37 between
    them, and offsets at every residue mod 16 (device allocations are at least 16-B aligned)."""
    c = cut_case(oracle_mod, 10, 3, 1200)
    gi, ji, mi = rebuilt_rows(c)
    L = symbol_lengths(c, True)[gi]
    nbytes, offs = padded_layout(SEED + 1200)(c, gi, ji, mi, L)
    assert set((offs % 16).tolist()) == set(range(16))
    order = np.argsort(offs, kind="stable")
    gaps = offs[order][1:] - (offs[order] + L[order])[:-1]
    assert gaps.min() >= 1 and gaps.max() <= 37 and offs.min() > GUARD and (offs + L).max() + GUARD == nbytes


@pytest.mark.parametrize("k,r", SHAPES)
def test_every_cut(quicfec_mod, oracle_mod, torch_cuda, k, r):
    with product_ctx(quicfec_mod) as ctx:
        for P in SIZES:
            run_scatter(torch_cuda, ctx, cut_case(oracle_mod, k, r, P), SEED + P, padded_layout(SEED + P))


# ------------------------------------------------------------------------------------------
# 2. NULL length table, destinations on the slot layout: the fixed-length gather recover
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", SHAPES)
def test_null_length_table_on_slots_equals_the_gather_recover(quicfec_mod, oracle_mod, torch_cuda, k, r):
    torch = torch_cuda
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 17):
            c = full_case(oracle_mod, k, r, P, G_MAIN, SEED + P + k)
            b = make_scatter(torch, c, SEED + 5, slot_layout, with_lens=False)
            launch_scatter(ctx, b)
            whole, out = guarded(torch, c.G * r * P, 0x5A)
            st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
            mo = torch.full((c.G,), -1, dtype=torch.int64, device="cuda")
            ctx.recover_gather_dev(b.table, c.G, k, r, P, out, st, mo)
            ctx.synchronize()
            check_scatter(b, "NULL lens on slots")
            assert torch.equal(whole, b.dest) and torch.equal(st, b.st) and torch.equal(mo, b.mo), (k, r, P)


# ------------------------------------------------------------------------------------------
# 3. Length table, destinations on the slot layout: the first L_g bytes of the var recover's slots
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", SHAPES)
def test_length_table_on_slots_is_the_var_recover_cut_at_the_symbol_length(quicfec_mod, oracle_mod, torch_cuda, k, r):
    torch = torch_cuda
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 17):
            c = main_case(oracle_mod, k, r, P)
            b = make_scatter(torch, c, SEED + 6, slot_layout)
            launch_scatter(ctx, b)
            whole, out = guarded(torch, c.G * r * P, 0x5A)
            ctx.recover_gather_var_dev(b.table, b.lens, c.G, k, r, P, out)
            ctx.synchronize()
            check_scatter(b, "lens on slots")
            got, full = b.dest.cpu().numpy(), whole.cpu().numpy()
            keep = np.zeros(len(got), dtype=bool)                             # the first L_g bytes of each rebuilt slot
            for off, g in zip(b.offs, b.rows[0]):
                keep[off:off + b.sym[g]] = True
            assert np.array_equal(got[keep], full[keep]) and (got[~keep] == 0x5A).all(), (k, r, P)


# ------------------------------------------------------------------------------------------
# 4. In place: destinations are holes in the source arenas
# ------------------------------------------------------------------------------------------
def make_in_place(torch, c, seed):
    """build_arena's arenas with a hole of exactly L_g bytes (0xEE) reserved for every packet the call
    rebuilds, between live packets: the source entry of a hole is 0, its destination entry the hole."""
    k, r, P, G = c.k, c.r, c.P, c.G
    rng = np.random.default_rng(seed)
    sym = symbol_lengths(c, True)
    hg, hj, _ = rebuilt_rows(c)
    hole = np.zeros((G, k + r), dtype=bool)
    hole[hg, hj] = True
    size = np.where(hole, sym[:, None], c.lens)
    gi, si = np.nonzero(~c.lost | hole)
    where = np.full((G, k + r, 2), -1, dtype=np.int64)
    where[:, :, 1] = 0
    fill = [37, 37]
    for i, pad, a in zip(rng.permutation(len(gi)), rng.integers(1, 38, size=len(gi)), rng.integers(0, 2, size=len(gi))):
        where[gi[i], si[i]] = (a, fill[a])
        fill[a] += int(size[gi[i], si[i]]) + int(pad)
    before = [np.full(fill[a] + P + 38, 0xEE, dtype=np.uint8) for a in (0, 1)]
    for g, s in zip(gi, si):
        a, off = where[g, s]
        ln = int(size[g, s])
        if not hole[g, s]:
            before[a][off:off + ln] = c.raw[g, s, :ln] if s < k else c.praw[g, s - k, :ln]
    after = [a.copy() for a in before]
    for g, j in zip(hg, hj):
        a, off = where[g, j]
        after[a][off:off + sym[g]] = c.data[g, j, :sym[g]]
    assert len(hg) > 0 and any(not np.array_equal(x, y) for x, y in zip(before, after))
    src = where.copy()
    src[hole] = (-1, 0)
    b = SimpleNamespace(c=c, with_lens=True, sym=sym)
    dev, b.table, b.lens = upload_arena(torch, before, src, np.where(~c.lost, c.lens, JUNK_LEN).astype(np.uint32))
    b.canary = torch.full((GUARD + P + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    base = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    tab = np.full((G, k), b.canary.data_ptr() + GUARD, dtype=np.uint64)
    tab[hg, hj] = base[where[hg, hj, 0]] + where[hg, hj, 1].astype(np.uint64)
    b.dtab = torch.from_numpy(tab.reshape(-1).view(np.int64)).to("cuda")
    b.images = list(zip(dev, after)) + [(b.canary, np.full(GUARD + P + GUARD, 0xC3, dtype=np.uint8))]
    b.st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
    b.mo = torch.full((G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    b.so = torch.full((G,), 0x77777777, dtype=torch.int32, device="cuda")
    return b


@pytest.mark.parametrize("k,r", [(10, 3), (12, 9)])
def test_in_place_into_holes_of_the_arena(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """After the call both arenas hold every data packet of every recoverable group at its place and
    every other byte as before."""
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 260):
            for c in (main_case(oracle_mod, k, r, P), cut_case(oracle_mod, k, r, P)):
                b = make_in_place(torch_cuda, c, SEED + 31 + P)
                launch_scatter(ctx, b)
                ctx.synchronize()
                check_scatter(b, "in place")


# ------------------------------------------------------------------------------------------
# 5. Back to back: packed output
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", SHAPES)
def test_back_to_back_is_packed_output(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """No byte between two destinations; without d_symbol_len_out (the kernel's L_g then lives in the
    stream's workspace) and with it."""
    with product_ctx(quicfec_mod) as ctx:
        for P, want_sym in ((1200, False), (17, True), (1025, False)):
            run_scatter(torch_cuda, ctx, cut_case(oracle_mod, k, r, P), SEED + 41, packed_layout, "packed", want_sym=want_sym)
        run_scatter(torch_cuda, ctx, full_case(oracle_mod, k, r, 260, G_MAIN, SEED + 42), SEED + 43, packed_layout,
                    "packed, NULL lens", with_lens=False, want_sym=False)


# ------------------------------------------------------------------------------------------
# 6. Not wanted: a destination entry of 0
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", [(10, 3), (20, 5), (4, 2), (6, 3), (12, 9)])
def test_a_zero_destination_is_not_stored(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """In the groups that rebuild two rows one destination is 0 (the first row in even groups, the
    second in odd ones): the other row is written, nothing else changes, the status stays 0.  The
    NULL path itself is covered without a GPU (test_scatter_forms.test_store_cut_plain_and_under_sanitizers)."""
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 17):
            c = cut_case(oracle_mod, k, r, P)
            gi, ji, mi = rebuilt_rows(c)
            two = np.bincount(gi, minlength=c.G)[gi] == 2
            unwanted = two & (mi == gi % 2)
            assert unwanted.sum() >= 10 and (c.status[gi[unwanted]] == 0).all()
            b = run_scatter(torch_cuda, ctx, c, SEED + 51, padded_layout(SEED + 52), "not wanted", unwanted=unwanted)
            assert (b.dtab.cpu().numpy().reshape(c.G, k)[gi[unwanted], ji[unwanted]] == 0).all()


# ------------------------------------------------------------------------------------------
# 7. Launch trace
# ------------------------------------------------------------------------------------------
def _launch_text(rec):
    if rec["form"] == "classify_scatter":
        return rec["form"]
    return f"{rec['form']} k={rec['k']} r={rec['r']} first={rec['first']} pol={rec['pol']} aux={rec['aux']}"


@pytest.mark.parametrize("k,r", SHAPES)
def test_launches_only_the_scatter_kernels(quicfec_mod, oracle_mod, torch_cuda, k, r):
    lib = quicfec_mod.load_test_library()
    with hooks_ctx(quicfec_mod) as ctx:
        for P, with_lens in ((17, True), (1200, True), (1200, False)):
            c = cut_case(oracle_mod, k, r, P) if with_lens else full_case(oracle_mod, k, r, P, G_MAIN, SEED + 61)
            b = make_scatter(torch_cuda, c, SEED + 62, padded_layout(SEED + 63), with_lens=with_lens)
            quicfec_mod.launch_trace(lib)                                    # clear: fills and uploads are torch's
            launch_scatter(ctx, b)
            ctx.synchronize()
            trace = quicfec_mod.launch_trace(lib)
            assert [_launch_text(t) for t in trace] == expected_launches(k, r, P, with_lens), (k, r, P)
            assert {t["form"] for t in trace} == {"classify_scatter", "recover_scatter"}
            assert len(trace) == 1 + (r + 7) // 8 if (k, r) == (12, 9) else len(trace) == 2
            assert all(t["items"] == c.G and t["first_item"] == 0 and t["block"] == 256 for t in trace)
            assert trace[0]["grid"] == 1 and all(t["grid"] == (c.G + 3) // 4 for t in trace[1:])
            check_scatter(b, "hooks")


def test_chunked_launches(quicfec_mod, oracle_mod, torch_cuda, monkeypatch):
    """The test library's launch limits split the call into several launches of each kernel: every
    chunk takes its own part of the three tables."""
    lib = quicfec_mod.load_test_library()
    c = cut_case(oracle_mod, 12, 9, 260)
    with hooks_ctx(quicfec_mod) as ctx:
        b = make_scatter(torch_cuda, c, SEED + 65, padded_layout(SEED + 66))
        monkeypatch.setenv("QUICFEC_MAX_WAVE_BLOCKS", "5")
        monkeypatch.setenv("QUICFEC_MAX_LAUNCH_THREADS", "32")
        quicfec_mod.launch_trace(lib)
        launch_scatter(ctx, b)
        ctx.synchronize()
        trace = quicfec_mod.launch_trace(lib)
    assert [t["first_item"] for t in trace if t["form"] == "classify_scatter"] == list(range(0, c.G, 32))
    assert [t["first_item"] for t in trace if t["form"] == "recover_scatter"] == 2 * list(range(0, c.G, 20))
    check_scatter(b, "chunked")


# ------------------------------------------------------------------------------------------
# 8. Refusals: the documented code, a message, nothing launched, nothing written
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,k,r,P,null,code,word", [
    ("NULL address table", 10, 3, 1200, "table", "NULL", "d_shard_addrs"),
    ("NULL destination table", 10, 3, 1200, "dests", "NULL", "d_dest_addrs"),
    ("P = 15", 10, 3, 15, "", "RANGE", "packet_size"),
    ("k + r = 65", 60, 5, 1200, "", "RANGE", "exceeds"),
    ("sparse-plan shape", 16, 16, 1200, "", "RANGE", "sparse-plan")])
@pytest.mark.parametrize("with_lens", [True, False])
def test_refusals(quicfec_mod, torch_cuda, what, k, r, P, null, code, word, with_lens):
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    G, n = 5, k + r
    arena = torch.full((G * n * (P + 40),), 0xEE, dtype=torch.uint8, device="cuda")
    addr = np.uint64(arena.data_ptr()) + np.arange(G * n, dtype=np.uint64) * np.uint64(P + 40)   # all readable
    addr[::n] = 0                                                             # data shard 0 of every group lost
    table = None if null == "table" else torch.from_numpy(addr.view(np.int64)).to("cuda")
    lens = torch.full((G * n,), P, dtype=torch.int32, device="cuda") if with_lens else None
    out = torch.full((G * k * (P + 40),), 0x5A, dtype=torch.uint8, device="cuda")
    daddr = np.uint64(out.data_ptr()) + np.arange(G * k, dtype=np.uint64) * np.uint64(P + 40)    # all writable
    dests = None if null == "dests" else torch.from_numpy(daddr.view(np.int64)).to("cuda")
    st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
    mo = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    sym = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(lib)
        with pytest.raises(quicfec_mod.FecError) as ei:
            ctx.recover_scatter_dev(table, lens, dests, G, k, r, P, st, mo, sym)
        assert ei.value.code == getattr(quicfec_mod, "FEC_ERR_" + code)
        assert word in quicfec_mod.last_error(lib) and word in ctx.last_error(), quicfec_mod.last_error(lib)
        ctx.synchronize()
        assert quicfec_mod.launch_trace(lib) == []
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (st == 7).all().item() and (mo == -1).all().item() and (sym == -1).all().item()
    assert (arena == 0xEE).all().item()


def test_null_context_and_zero_groups_are_refused(quicfec_mod, torch_cuda):
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    table = torch.zeros(13, dtype=torch.int64, device="cuda")
    lens = torch.zeros(13, dtype=torch.int32, device="cuda")
    out = torch.full((10 * 1200,), 0x5A, dtype=torch.uint8, device="cuda")
    dests = torch.from_numpy((np.uint64(out.data_ptr()) + np.arange(10, dtype=np.uint64) * np.uint64(1200)).view(np.int64)).to("cuda")
    st = torch.full((1,), 7, dtype=torch.uint8, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        quicfec_mod.launch_trace(lib)
        assert lib.fec_recover_scatter_rs_dev(None, table.data_ptr(), lens.data_ptr(), dests.data_ptr(), 1, 10, 3, 1200,
                                              st.data_ptr(), None, None, None) == quicfec_mod.FEC_ERR_NULL
        assert "context" in quicfec_mod.last_error(lib)
        assert lib.fec_recover_scatter_rs_dev(ctx.handle, table.data_ptr(), lens.data_ptr(), dests.data_ptr(), 0, 10, 3,
                                              1200, st.data_ptr(), None, None, None) == quicfec_mod.FEC_ERR_RANGE
        assert "num_groups" in ctx.last_error()
        ctx.synchronize()
        assert quicfec_mod.launch_trace(lib) == []
    assert (out == 0x5A).all().item() and (st == 7).all().item()


# ------------------------------------------------------------------------------------------
# 9. One side stream, no host synchronise until the end; a context freed with calls in flight
# ------------------------------------------------------------------------------------------
def test_queue_on_one_side_stream(quicfec_mod, oracle_mod, torch_cuda):
    """In order on one non-blocking side stream: a scatter recover with lengths, a var gather recover,
    a scatter recover without lengths, one without d_symbol_len_out and a last one with more groups
    (the workspace grows under queued work); one synchronise at the end, then every result is checked."""
    torch = torch_cuda
    k, r, P = 20, 5, 1025
    s1 = make_scatter(torch, cut_case(oracle_mod, k, r, P), SEED + 71, padded_layout(SEED + 72))
    v = var.make_recover(torch, main_case(oracle_mod, k, r, P), SEED + 73)
    s2 = make_scatter(torch, full_case(oracle_mod, k, r, 1200, G_MAIN, SEED + 74), SEED + 75, slot_layout, with_lens=False)
    s3 = make_scatter(torch, main_case(oracle_mod, k, r, P), SEED + 76, packed_layout, want_sym=False)
    G2 = 1500
    rng = np.random.default_rng(SEED + 77)
    c2 = make_case(oracle_mod, k, r, P, iid_masks(k, r, G2, 0.1, rng), rng.integers(0, P + 9, size=(G2, k)),
                   rng.integers(0, P + 9, size=(G2, r)), SEED + 78)
    assert c2.rows > 0
    s4 = make_scatter(torch, c2, SEED + 79, padded_layout(SEED + 80), want_sym=False)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        launch_scatter(ctx, s1, stream.cuda_stream)
        var.launch_recover(ctx, v, stream.cuda_stream)
        launch_scatter(ctx, s2, stream.cuda_stream)
        launch_scatter(ctx, s3, stream.cuda_stream)
        launch_scatter(ctx, s4, stream.cuda_stream)
        torch.cuda.synchronize()
    check_scatter(s1, "first")
    var.check_recover(v, "var gather")
    check_scatter(s2, "NULL lens")
    check_scatter(s3, "no symbol lengths")
    check_scatter(s4, "grown")


def test_free_with_scatter_calls_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """Two scatter recovers queued on a side stream, and the context freed at once: fec_encoder_free
    drains them, so both are complete and right after it."""
    torch = torch_cuda
    k, r, P, G = 10, 3, 1200, 4096
    rng = np.random.default_rng(SEED + 81)
    c = make_case(oracle_mod, k, r, P, perm_masks(k, r, G, SEED + 82), rng.integers(0, P + 9, size=(G, k)),
                  np.zeros((G, r), dtype=np.int64), SEED + 83)
    a = make_scatter(torch, c, SEED + 84, padded_layout(SEED + 85))
    b = make_scatter(torch, c, SEED + 86, packed_layout, want_sym=False)
    stream = torch.cuda.Stream()
    ctx = product_ctx(quicfec_mod)
    torch.cuda.synchronize()
    launch_scatter(ctx, a, stream.cuda_stream)
    launch_scatter(ctx, b, stream.cuda_stream)
    ctx.close()
    assert stream.query()                                                    # the free drained the stream
    torch.cuda.synchronize()
    check_scatter(a, "in flight")
    check_scatter(b, "in flight, packed")


# ------------------------------------------------------------------------------------------
# 10. Random sweep
# ------------------------------------------------------------------------------------------
def test_random_sweep(quicfec_mod, oracle_mod, torch_cuda):
    """40 seeded cases (as test_gpu_gather_var's sweep) over shape, P in 16..2100, G in 1..40, iid loss
    of 1%, 10% or 30%, a length table with independent lengths in 0..P + 8 or none, and the three
    layouts.  Group 0 of every case loses exactly one data shard, so every case rebuilds a row."""
    shapes = [(10, 3), (10, 2), (10, 1), (4, 2), (20, 5), (6, 3), (12, 6), (16, 4), (12, 9)]
    rng = np.random.default_rng(SEED + 91)
    rebuilt = unrec = nulls = 0
    with product_ctx(quicfec_mod) as ctx:
        for i in range(40):
            k, r = shapes[rng.integers(len(shapes))]
            P, G = int(rng.integers(16, 2101)), int(rng.integers(1, 41))
            loss = (0.01, 0.10, 0.30)[rng.integers(3)]
            with_lens = bool(rng.integers(2))
            masks = iid_masks(k, r, G, loss, rng)
            masks[0] = np.uint64(1) << np.uint64(int(rng.integers(k)))
            dl, pl = rng.integers(0, P + 9, size=(G, k)), rng.integers(0, P + 9, size=(G, r))
            if not with_lens:
                dl[:], pl[:] = P, P
            c = make_case(oracle_mod, k, r, P, masks, dl, pl, SEED + 1000 + i)
            assert c.rows >= 1 and c.status[0] == 0
            layout = (padded_layout(SEED + 3000 + i), slot_layout, packed_layout)[rng.integers(3)]
            run_scatter(torch_cuda, ctx, c, SEED + 2000 + i, layout, (i, loss), with_lens=with_lens,
                        want_sym=bool(rng.integers(2)))
            rebuilt += c.rows
            unrec += int(c.status.sum())
            nulls += not with_lens
    assert rebuilt > 40 and unrec > 0 and 5 < nulls < 35                      # rebuilt, refused, both kinds of table
