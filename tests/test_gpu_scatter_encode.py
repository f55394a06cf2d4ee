"""fec_encode_scatter_rs_dev on the GPU: the address-table encode that writes every parity row to a
table of destinations, exactly the group's symbol length L_g of it.  Expected parity comes from the
oracle on zero-padded packets (test_gpu_gather_var.make_case with present=...), and row 0
additionally from oracle.go_generate_redundancy on the true packets.  Bit-exact, no tolerance.

Packets sit in test_gpu_gather_var.build_arena's arenas: true lengths, pads of 1..37 bytes of 0xEE,
every residue mod 16, a length-0 packet pointing at pad bytes, an absent packet as address 0 with a
junk length.  Destinations live in a separate allocation pre-filled 0x5A with a guard of 256 bytes at
each end; each destination has exactly L_g bytes, so a byte written before a destination or at or
past destination + L_g changes a byte that must stay 0x5A.  The entries of a group with L_g = 0
point into that allocation too: a valid address, so a wrong kernel fails a comparison instead of
faulting.

After every call: the packet arenas are byte-identical to before; the whole destination allocation
equals the expected image (rows in place, 0x5A everywhere else); the symbol lengths equal the
expected ones.
"""
import os
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_gather import GUARD, guarded, hooks_ctx, product_ctx
from test_gpu_gather_var import JUNK_LEN, build_arena, dealt_lengths, make_case, upload_arena
from test_gpu_scatter import packed_layout, padded_layout, slot_layout
from test_scatter_encode_forms import expected_launches                     # the table of DESIGN.md §5b

pytestmark = pytest.mark.gpu

SEED = 0x5CE70000
SHAPES = [(10, 3), (20, 5), (4, 2), (6, 3), (12, 9)]                         # r = 9: one full and one partial row pass
SIZES = [16, 17, 260, 1025, 1200, 2100]
G_MAIN = 67
HDR = 11                                                                     # bytes of the repair header before a hole


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases: one batch and what the oracle says about it, computed once and never modified
# ------------------------------------------------------------------------------------------
def enc_case(oracle, k, r, P, dlens, present, seed):
    """make_case for an encode: no losses, absent packets count as zeros.  Row 0 of every group with a
    packet present is also the reference encoder's repair payload on the true packets (cut at P)."""
    dlens = np.asarray(dlens, dtype=np.int64)
    G = len(dlens)
    c = make_case(oracle, k, r, P, [0] * G, dlens, np.zeros((G, r), dtype=np.int64), seed, present=present)
    for g in range(G):
        if c.sym_enc[g] == 0:                                                # the reference emits no repair packet
            assert not c.par[g].any()
            continue
        pk = [np.ascontiguousarray(c.raw[g, j, :min(int(c.lens[g, j]), P)]) for j in range(k) if c.present[g, j]]
        pay = oracle.go_generate_redundancy(pk, group_id=g)[HDR:]
        assert len(pay) == c.sym_enc[g]
        assert np.array_equal(c.par[g, 0, :len(pay)], pay) and not c.par[g, 0, len(pay):].any()
    return c


def symbol_lengths(c, with_lens):
    """L_g: the largest clamped length of the present packets; without a length table P when any is present."""
    if with_lens:
        return c.sym_enc.astype(np.int64)
    return np.where(c.present.any(axis=1), c.P, 0).astype(np.int64)


@lru_cache(maxsize=None)
def cut_case(oracle, k, r, P):
    """G = P + 1, and group g's longest packet has length g, so the call meets every L_g in 0..P.  The
    other packets have edge lengths (test_gpu_gather_var.edge_lengths: 0 among them, 2P cut down)
    capped at g; about one in seven is absent."""
    G = P + 1
    g = np.arange(G)
    dl = np.minimum(dealt_lengths(P, G, k), g[:, None])
    present = np.random.default_rng(SEED + k * 100000 + r * 10000 + P).random((G, k)) < 0.85
    present[g, g % k] = True
    dl[g, g % k] = g
    c = enc_case(oracle, k, r, P, dl, present, SEED + k * 100000 + r * 10000 + P + 1)
    assert np.array_equal(c.sym_enc, g)
    assert (~c.present).any() and (c.lens[:, :k][c.present] == 0).sum() > 1
    return c


@lru_cache(maxsize=None)
def mixed_case(oracle, k, r, P, G=G_MAIN):
    """Edge lengths dealt over the packets; group 1 has one packet present, group 2 all but one,
    group 3 none, the others about 85%; group 5 all lengths P, group 6 all lengths 0."""
    dl = dealt_lengths(P, G, k)
    present = np.ones((G, k), dtype=bool)
    present[4:] = np.random.default_rng(SEED + k + P).random((G - 4, k)) < 0.85
    present[1] = False
    present[1, k // 2] = True
    present[2, 0] = k == 1
    present[3] = False
    dl[5] = P
    dl[6] = 0
    c = enc_case(oracle, k, r, P, dl, present, SEED + 7 * P + k)
    assert c.sym_enc[3] == 0 and c.sym_enc[6] == 0 and c.sym_enc[5] == (P if present[5].any() else 0)
    return c


@lru_cache(maxsize=None)
def full_case(oracle, k, r, P, G=G_MAIN, absent=False):
    """Every length P (the inputs of the fixed-length gather encode); absent: about 85% present,
    group 3 with none."""
    present = np.ones((G, k), dtype=bool)
    if absent:
        present = np.random.default_rng(SEED + 3 * k + P).random((G, k)) < 0.85
        present[min(3, G - 1)] = False
    return enc_case(oracle, k, r, P, np.full((G, k), P), present, SEED + 11 * P + k + absent)


# ------------------------------------------------------------------------------------------
# Destinations and one call
# ------------------------------------------------------------------------------------------
def residue_layout(c, gi, ji, ii, L):
    """In (g, i) order, exactly L_g bytes per destination and 1..16 guard bytes before each, chosen so
    that the destination of row i of group g starts at residue (g + g // 16 + 7 i + P + k) mod 16
    (g // 16: the groups whose L_g is a multiple of 16 take every residue too)."""
    offs = np.zeros(len(gi), dtype=np.int64)
    fill = GUARD
    for n, (g, i) in enumerate(zip(gi, ii)):
        fill += 1 + (int(g) + int(g) // 16 + 7 * int(i) + c.P + c.k - (fill + 1)) % 16
        offs[n] = fill
        fill += int(L[n])
    return fill + GUARD, offs


def make_encode(torch, c, seed, layout, with_lens=True, unwanted=None, want_sym=True):
    """Arena, tables, destination allocation and pre-filled output of one scatter encode of case c.
    unwanted (G, r) bool: True = the row's destination entry is 0.  Everything is uploaded on torch's
    stream: synchronise before launching on a side stream."""
    k, r, P, G = c.k, c.r, c.P, c.G
    arenas, where, lens = build_arena(c, seed, encode=True)
    b = SimpleNamespace(c=c, with_lens=with_lens)
    dev, b.table, b.lens = upload_arena(torch, arenas, where, lens)
    if not with_lens:
        assert (c.lens[:, :k][c.present] == P).all()                         # NULL table = every present packet has P
        b.lens = None
    b.sym = symbol_lengths(c, with_lens)
    gi, ii = np.repeat(np.arange(G), r), np.tile(np.arange(r), G)
    L = b.sym[gi]
    nbytes, offs = layout(c, gi, None, ii, L)
    wanted = np.ones(G * r, dtype=bool) if unwanted is None else ~np.asarray(unwanted).reshape(-1)
    image = np.full(nbytes, 0x5A, dtype=np.uint8)
    used = np.zeros(nbytes, dtype=bool)
    for n in np.nonzero(wanted & (L > 0))[0]:
        assert not used[offs[n]:offs[n] + L[n]].any()                        # destinations do not overlap
        used[offs[n]:offs[n] + L[n]] = True
        image[offs[n]:offs[n] + L[n]] = c.par[gi[n], ii[n], :L[n]]
    b.dest = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    tab = np.where(wanted, np.uint64(b.dest.data_ptr()) + offs.astype(np.uint64), np.uint64(0))
    b.offs, b.image = offs, image
    b.dtab = torch.from_numpy(tab.view(np.int64)).to("cuda")
    b.images = list(zip(dev, arenas)) + [(b.dest, image)]
    b.so = torch.full((G,), 0x77777777, dtype=torch.int32, device="cuda") if want_sym else None
    return b


def launch_encode(ctx, b, stream=None):
    c = b.c
    ctx.encode_scatter_dev(b.table, b.lens, b.dtab, c.G, c.k, c.r, c.P, b.so, stream=stream)


def check_encode(b, what=""):
    c = b.c
    what = (what, c.k, c.r, c.P, c.G, b.with_lens)
    for n, (d, image) in enumerate(b.images):
        got = d.cpu().numpy()
        bad = np.nonzero(got != image)[0]
        assert bad.size == 0, (what, "buffer", n, "of", len(b.images), "first wrong bytes at", bad[:8], got[bad[:8]])
    if b.so is not None:
        assert np.array_equal(b.so.cpu().numpy().view(np.uint32), b.sym.astype(np.uint32)), what


def run_encode(torch, ctx, c, seed, layout, what="", **kw):
    b = make_encode(torch, c, seed, layout, **kw)
    launch_encode(ctx, b)
    ctx.synchronize()
    check_encode(b, what)
    return b


# ------------------------------------------------------------------------------------------
# 1. Every cut
# ------------------------------------------------------------------------------------------
def test_destinations_take_every_residue_and_exactly_the_symbol_length(oracle_mod):
    """On the CPU: the residue layout gives each destination exactly L_g bytes, 1..16 guard bytes
    between two, and every start residue mod 16 (device allocations are at least 16-B aligned)."""
    c = cut_case(oracle_mod, 10, 3, 260)
    gi, ii = np.repeat(np.arange(c.G), c.r), np.tile(np.arange(c.r), c.G)
    L = symbol_lengths(c, True)[gi]
    nbytes, offs = residue_layout(c, gi, None, ii, L)
    assert set((offs % 16).tolist()) == set(range(16)) and np.array_equal(offs % 16, (gi + gi // 16 + 7 * ii + c.P + c.k) % 16)
    gaps = offs[1:] - (offs + L)[:-1]
    assert gaps.min() >= 1 and gaps.max() <= 16 and offs.min() > GUARD and (offs + L).max() + GUARD == nbytes
    for res in range(16):                                                    # dword cuts and column cuts at every residue
        seen = L[offs % 16 == res]
        assert ((seen >= 4) & (seen < 16)).any() and ((seen >= 16) & (seen % 16 != 0)).any() and (seen % 16 == 0).any()
    assert len(set((offs % 16)[(L > 0) & (L < 4)].tolist())) >= 6            # byte cuts at several (three groups have them)


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("k,r", SHAPES)
def test_every_cut(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    with product_ctx(quicfec_mod) as ctx:
        run_encode(torch_cuda, ctx, cut_case(oracle_mod, k, r, P), SEED + P, residue_layout)


# ------------------------------------------------------------------------------------------
# 2. No length table, destinations on the slot layout: the fixed-length gather encode
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", SHAPES)
def test_no_length_table_on_slots_equals_the_gather_encode(quicfec_mod, oracle_mod, torch_cuda, k, r):
    torch = torch_cuda
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 17):
            c = full_case(oracle_mod, k, r, P)
            b = make_encode(torch, c, SEED + 5, slot_layout, with_lens=False)
            launch_encode(ctx, b)
            whole, out = guarded(torch, c.G * r * P, 0x5A)
            ctx.encode_gather_dev(b.table, c.G, k, r, P, out)
            ctx.synchronize()
            check_encode(b, "no lens on slots")
            assert torch.equal(whole, b.dest), (k, r, P)
            # absent packets (address 0), one group with none present: its rows keep their pre-fill
            c = full_case(oracle_mod, k, r, P, absent=True)
            b = run_encode(torch, ctx, c, SEED + 6, slot_layout, "no lens, absent packets", with_lens=False)
            assert b.sym[3] == 0 and (b.image[GUARD + 3 * r * P:GUARD + 4 * r * P] == 0x5A).all()
            assert (b.so.cpu().numpy()[3] == 0) and (~c.present).sum() > c.k


# ------------------------------------------------------------------------------------------
# 3. Length table, destinations on the slot layout: the first L_g bytes of the var encode's rows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", SHAPES)
def test_length_table_on_slots_is_the_var_encode_cut_at_the_symbol_length(quicfec_mod, oracle_mod, torch_cuda, k, r):
    torch = torch_cuda
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 17):
            c = mixed_case(oracle_mod, k, r, P)
            b = make_encode(torch, c, SEED + 7, slot_layout)
            launch_encode(ctx, b)
            whole, out = guarded(torch, c.G * r * P, 0x5A)
            sym = torch.full((c.G,), 0x77777777, dtype=torch.int32, device="cuda")
            ctx.encode_gather_var_dev(b.table, b.lens, c.G, k, r, P, out, sym)
            ctx.synchronize()
            check_encode(b, "lens on slots")
            assert torch.equal(sym, b.so), (k, r, P)
            got, full = b.dest.cpu().numpy(), whole.cpu().numpy()
            keep = np.zeros(len(got), dtype=bool)                             # the first L_g bytes of every row
            for off, n in zip(b.offs, np.repeat(b.sym, r)):
                keep[off:off + n] = True
            assert np.array_equal(got[keep], full[keep]) and (got[~keep] == 0x5A).all(), (k, r, P)


# ------------------------------------------------------------------------------------------
# 4. Into the send ring: destinations are the holes behind the headers in the packets' own arenas
# ------------------------------------------------------------------------------------------
def make_in_ring(torch, c, seed):
    """build_arena's two arenas holding, in one seeded random order with pads of 1..37 bytes, every
    present packet at its true length and, per parity row, a header of 11 bytes (0xB7) followed by a
    hole of exactly L_g bytes (0xEE): the row's destination is the hole."""
    k, r, P, G = c.k, c.r, c.P, c.G
    rng = np.random.default_rng(seed)
    sym = c.sym_enc.astype(np.int64)
    pg, pj = np.nonzero(c.present)
    rg, ri = np.repeat(np.arange(G), r), np.tile(np.arange(r), G)
    n_p = len(pg)
    size = np.concatenate([c.lens[pg, pj], HDR + sym[rg]]).astype(np.int64)
    n = len(size)
    ar, off = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    fill = [37, 37]
    for i, pad, a in zip(rng.permutation(n), rng.integers(1, 38, size=n), rng.integers(0, 2, size=n)):
        ar[i], off[i] = a, fill[a]
        fill[a] += int(size[i]) + int(pad)
    before = [np.full(fill[a] + P + 38, 0xEE, dtype=np.uint8) for a in (0, 1)]
    for i in range(n_p):
        ln = int(size[i])
        before[ar[i]][off[i]:off[i] + ln] = c.raw[pg[i], pj[i], :ln]
    for i in range(n_p, n):
        before[ar[i]][off[i]:off[i] + HDR] = 0xB7
    after = [a.copy() for a in before]
    for i in range(n_p, n):
        g, row = rg[i - n_p], ri[i - n_p]
        after[ar[i]][off[i] + HDR:off[i] + HDR + sym[g]] = c.par[g, row, :sym[g]]
    assert any(not np.array_equal(x, y) for x, y in zip(before, after))
    where = np.full((G, k, 2), -1, dtype=np.int64)
    where[:, :, 1] = 0
    where[pg, pj, 0], where[pg, pj, 1] = ar[:n_p], off[:n_p]
    b = SimpleNamespace(c=c, with_lens=True, sym=sym)
    dev, b.table, b.lens = upload_arena(torch, before, where, np.where(c.present, c.lens[:, :k], JUNK_LEN).astype(np.uint32))
    base = np.array([d.data_ptr() for d in dev], dtype=np.uint64)
    b.dtab = torch.from_numpy((base[ar[n_p:]] + (off[n_p:] + HDR).astype(np.uint64)).view(np.int64)).to("cuda")
    b.images = list(zip(dev, after))
    b.so = torch.full((G,), 0x77777777, dtype=torch.int32, device="cuda")
    return b


@pytest.mark.parametrize("k,r", [(10, 3), (12, 9)])
def test_into_the_send_ring_and_packed(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """After the call both arenas hold every repair payload behind its header and every other byte as
    before.  Packed: row i's destination is the previous one plus L_g, no byte between two."""
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 260):
            for c in (mixed_case(oracle_mod, k, r, P), cut_case(oracle_mod, k, r, P)):
                b = make_in_ring(torch_cuda, c, SEED + 31 + P)
                launch_encode(ctx, b)
                ctx.synchronize()
                check_encode(b, "send ring")
                run_encode(torch_cuda, ctx, c, SEED + 32, packed_layout, "packed")
        run_encode(torch_cuda, ctx, full_case(oracle_mod, k, r, 260, absent=True), SEED + 33, packed_layout,
                   "packed, no lens", with_lens=False)


# ------------------------------------------------------------------------------------------
# 5. Not wanted: a destination entry of 0
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", SHAPES)
def test_a_zero_destination_is_not_stored(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """Every third group does not want row g mod r, every fifth wants none; the other rows are written
    and nothing else changes.  At k=12 r=9 a second case wants no row of the second pass (row 8) in
    any group.  Both without d_symbol_len_out too.  The NULL path itself is covered without a GPU
    (test_scatter_encode_forms.test_store_cut_plain_and_under_sanitizers)."""
    with product_ctx(quicfec_mod) as ctx:
        for P, want_sym in ((1200, True), (17, False)):
            c = mixed_case(oracle_mod, k, r, P)
            g = np.arange(c.G)
            unwanted = np.zeros((c.G, r), dtype=bool)
            unwanted[g[g % 3 == 0], g[g % 3 == 0] % r] = True
            unwanted[g % 5 == 0] = True
            b = run_encode(torch_cuda, ctx, c, SEED + 51, padded_layout(SEED + 52), "not wanted", unwanted=unwanted,
                           want_sym=want_sym)
            assert (b.dtab.cpu().numpy().reshape(c.G, r)[unwanted] == 0).all() and unwanted.sum() > c.G // 3
            assert (b.dtab.cpu().numpy().reshape(c.G, r)[~unwanted] != 0).all()
            if r > 8:
                unwanted = np.zeros((c.G, r), dtype=bool)
                unwanted[:, 8:] = True
                run_encode(torch_cuda, ctx, c, SEED + 53, padded_layout(SEED + 54), "second pass not wanted",
                           unwanted=unwanted, want_sym=not want_sym)


# ------------------------------------------------------------------------------------------
# 6. Launch trace
# ------------------------------------------------------------------------------------------
def _launch_text(rec):
    return (f"{rec['form']} k={rec['k']} r={rec['r']} first={rec['first']} pol={rec['pol']} direct={rec['direct']} "
            f"aux={rec['aux']}")


@pytest.mark.parametrize("k,r", SHAPES)
def test_launches_only_the_scatter_encode_kernel(quicfec_mod, oracle_mod, torch_cuda, k, r):
    lib = quicfec_mod.load_test_library()
    with hooks_ctx(quicfec_mod) as ctx:
        for P, with_lens in ((17, True), (1200, True), (1200, False)):
            c = mixed_case(oracle_mod, k, r, P) if with_lens else full_case(oracle_mod, k, r, P, absent=True)
            b = make_encode(torch_cuda, c, SEED + 62, padded_layout(SEED + 63), with_lens=with_lens)
            quicfec_mod.launch_trace(lib)                                    # clear: fills and uploads are torch's
            launch_encode(ctx, b)
            ctx.synchronize()
            trace = quicfec_mod.launch_trace(lib)
            assert [_launch_text(t) for t in trace] == expected_launches(k, r, P, with_lens), (k, r, P)
            assert {t["form"] for t in trace} == {"encode_scatter"}
            assert len(trace) == (2 if r == 9 else 1)
            cpp = (P + 15) // 16
            assert all(t["items"] == c.G and t["first_item"] == 0 and t["block"] == 256 and
                       t["grid"] == (c.G * cpp + 255) // 256 for t in trace)
            check_encode(b, "hooks")


def test_chunked_launches(quicfec_mod, oracle_mod, torch_cuda, monkeypatch):
    """The test library's launch limit splits every pass into several launches: every chunk takes its
    own part of the four tables (addresses, lengths, destinations, symbol lengths)."""
    lib = quicfec_mod.load_test_library()
    k, r, P = 12, 9, 260
    c = mixed_case(oracle_mod, k, r, P)
    per = max(1, 32 // ((P + 15) // 16))                                     # groups per launch of 32 work items
    with hooks_ctx(quicfec_mod) as ctx:
        b = make_encode(torch_cuda, c, SEED + 65, padded_layout(SEED + 66))
        monkeypatch.setenv("QUICFEC_MAX_LAUNCH_THREADS", "32")
        quicfec_mod.launch_trace(lib)
        launch_encode(ctx, b)
        ctx.synchronize()
        trace = quicfec_mod.launch_trace(lib)
    assert {t["form"] for t in trace} == {"encode_scatter"} and len(trace) > 2 * 4
    assert [t["first_item"] for t in trace] == 2 * list(range(0, c.G, per))
    assert [t["aux"] for t in trace] == [0] * (len(trace) // 2) + [8] * (len(trace) // 2)
    assert all(t["items"] == min(per, c.G - t["first_item"]) for t in trace)
    check_encode(b, "chunked")


# ------------------------------------------------------------------------------------------
# 7. The limit shapes of the gather encodes (tests/test_gpu_address_limits.py)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", [(63, 1), (1, 63), (32, 32), (48, 16), (1, 1)])
def test_limit_shapes(quicfec_mod, oracle_mod, torch_cuda, k, r):
    G = 37
    with product_ctx(quicfec_mod) as ctx:
        for P in (16, 260, 1200):
            for with_lens in (True, False):
                rng = np.random.default_rng(SEED + 70 + k * 64 + r + P)
                dl = rng.integers(0, P + 9, size=(G, k)) if with_lens else np.full((G, k), P)
                present = rng.random((G, k)) < 0.85
                present[0], present[1] = True, False
                c = enc_case(oracle_mod, k, r, P, dl, present, SEED + 71 + P + with_lens)
                run_encode(torch_cuda, ctx, c, SEED + 72, padded_layout(SEED + 73 + P), "limits", with_lens=with_lens)


# ------------------------------------------------------------------------------------------
# 8. Refusals: the documented code, a message, nothing launched, nothing written
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,k,r,P,G,null,code,word", [
    ("NULL address table", 10, 3, 1200, 5, "table", "NULL", "d_packet_addrs"),
    ("NULL destination table", 10, 3, 1200, 5, "dests", "NULL", "d_dest_addrs"),
    ("P = 15", 10, 3, 15, 5, "", "RANGE", "packet_size"),
    ("k + r = 65", 60, 5, 1200, 5, "", "RANGE", "exceeds"),
    ("num_groups = 0", 10, 3, 1200, 0, "", "RANGE", "num_groups")])
@pytest.mark.parametrize("with_lens", [True, False])
def test_refusals(quicfec_mod, torch_cuda, what, k, r, P, G, null, code, word, with_lens):
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    n = 5                                                                    # the tables hold five groups whatever G says
    arena = torch.full((n * k * (P + 40),), 0xEE, dtype=torch.uint8, device="cuda")
    addr = np.uint64(arena.data_ptr()) + np.arange(n * k, dtype=np.uint64) * np.uint64(P + 40)   # all readable
    table = None if null == "table" else torch.from_numpy(addr.view(np.int64)).to("cuda")
    lens = torch.full((n * k,), P, dtype=torch.int32, device="cuda") if with_lens else None
    out = torch.full((n * r * (P + 40),), 0x5A, dtype=torch.uint8, device="cuda")
    daddr = np.uint64(out.data_ptr()) + np.arange(n * r, dtype=np.uint64) * np.uint64(P + 40)    # all writable
    dests = None if null == "dests" else torch.from_numpy(daddr.view(np.int64)).to("cuda")
    sym = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(lib)
        with pytest.raises(quicfec_mod.FecError) as ei:
            ctx.encode_scatter_dev(table, lens, dests, G, k, r, P, sym)
        assert ei.value.code == getattr(quicfec_mod, "FEC_ERR_" + code)
        assert word in quicfec_mod.last_error(lib) and word in ctx.last_error(), quicfec_mod.last_error(lib)
        ctx.synchronize()
        assert quicfec_mod.launch_trace(lib) == []
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (sym == -1).all().item() and (arena == 0xEE).all().item()


# ------------------------------------------------------------------------------------------
# 9. A caller's stream, no host synchronise until the end; a context freed with calls in flight
# ------------------------------------------------------------------------------------------
def test_queue_on_a_side_stream_behind_a_fill(quicfec_mod, oracle_mod, torch_cuda):
    """On one non-blocking side stream: the fill that gives the destination allocation its 0x5A (it
    holds 0x00 before), then the scatter encode into it; the same for a second call without a length
    table, and a var gather encode between them.  One synchronise at the end.  A call that ran ahead
    of its fill would have its rows overwritten."""
    import test_gpu_gather_var as var
    torch = torch_cuda
    k, r, P = 20, 5, 1025
    s1 = make_encode(torch, mixed_case(oracle_mod, k, r, P), SEED + 81, padded_layout(SEED + 82))
    s2 = make_encode(torch, full_case(oracle_mod, k, r, 1200, absent=True), SEED + 83, packed_layout, with_lens=False,
                     want_sym=False)
    big = np.random.default_rng(SEED + 84)
    G2 = 1500
    c3 = enc_case(oracle_mod, k, r, P, big.integers(0, P + 9, size=(G2, k)), big.random((G2, k)) < 0.9, SEED + 85)
    s3 = make_encode(torch, c3, SEED + 86, padded_layout(SEED + 87))
    for s in (s1, s2, s3):
        s.dest.zero_()
    vc = var.encode_case(oracle_mod, 10, 3, 260)
    arenas, where, lens = build_arena(vc, SEED + 88, encode=True)
    e = SimpleNamespace(c=vc, arenas=arenas)
    e.dev, e.table, e.lens = upload_arena(torch, arenas, where, lens)
    e.whole, e.par = guarded(torch, vc.G * vc.r * vc.P, 0x5A)
    e.sym = torch.full((vc.G,), 0x77777777, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            s1.dest.fill_(0x5A)
        launch_encode(ctx, s1, stream.cuda_stream)
        ctx.encode_gather_var_dev(e.table, e.lens, vc.G, vc.k, vc.r, vc.P, e.par, e.sym, stream=stream.cuda_stream)
        with torch.cuda.stream(stream):
            s2.dest.fill_(0x5A)
            s3.dest.fill_(0x5A)
        launch_encode(ctx, s2, stream.cuda_stream)
        launch_encode(ctx, s3, stream.cuda_stream)
        torch.cuda.synchronize()
    check_encode(s1, "first")
    var.check_encode(e, "var gather encode")
    check_encode(s2, "no lens, no symbol lengths")
    check_encode(s3, "more groups")


def test_free_with_scatter_encodes_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """Two scatter encodes queued on a side stream, and the context freed at once: fec_encoder_free
    drains them, so both are complete and right after it."""
    torch = torch_cuda
    k, r, P, G = 10, 3, 1200, 4096
    rng = np.random.default_rng(SEED + 91)
    c = enc_case(oracle_mod, k, r, P, rng.integers(0, P + 9, size=(G, k)), rng.random((G, k)) < 0.9, SEED + 92)
    a = make_encode(torch, c, SEED + 93, padded_layout(SEED + 94))
    b = make_encode(torch, c, SEED + 95, packed_layout, want_sym=False)
    stream = torch.cuda.Stream()
    ctx = product_ctx(quicfec_mod)
    torch.cuda.synchronize()
    launch_encode(ctx, a, stream.cuda_stream)
    launch_encode(ctx, b, stream.cuda_stream)
    ctx.close()
    assert stream.query()                                                    # the free drained the stream
    torch.cuda.synchronize()
    check_encode(a, "in flight")
    check_encode(b, "in flight, packed")


# ------------------------------------------------------------------------------------------
# 10. Random sweep
# ------------------------------------------------------------------------------------------
def test_random_sweep(quicfec_mod, oracle_mod, torch_cuda):
    """200 seeded cases over k in 1..20, r in 1..9, P in 16..2100, G in 1..40: a length table with
    independent lengths in 0..P + 8 or none, 0%, 10% or 50% of the packets absent, 0% or 25% of the
    rows not wanted, the padded, slot and packed layouts at whatever alignment they give, with and
    without d_symbol_len_out.  Every case is checked."""
    rng = np.random.default_rng(SEED + 101)
    checked = rows = unwanted_rows = empty = nulls = 0
    with product_ctx(quicfec_mod) as ctx:
        for i in range(200):
            k, r = int(rng.integers(1, 21)), int(rng.integers(1, 10))
            P, G = int(rng.integers(16, 2101)), int(rng.integers(1, 41))
            with_lens = bool(rng.integers(2))
            dl = rng.integers(0, P + 9, size=(G, k)) if with_lens else np.full((G, k), P)
            present = rng.random((G, k)) >= (0.0, 0.10, 0.50)[rng.integers(3)]
            unwanted = rng.random((G, r)) < (0.0, 0.25)[rng.integers(2)]
            c = enc_case(oracle_mod, k, r, P, dl, present, SEED + 1000 + i)
            layout = (padded_layout(SEED + 3000 + i), slot_layout, packed_layout)[rng.integers(3)]
            b = run_encode(torch_cuda, ctx, c, SEED + 2000 + i, layout, i, with_lens=with_lens, unwanted=unwanted,
                           want_sym=bool(rng.integers(2)))
            checked += 1
            rows += int(((b.sym > 0)[:, None] & ~unwanted).sum())
            unwanted_rows += int(unwanted.sum())
            empty += int((b.sym == 0).sum())
            nulls += not with_lens
    assert checked == 200 and rows > 1000 and unwanted_rows > 100 and empty > 0 and 50 < nulls < 150
