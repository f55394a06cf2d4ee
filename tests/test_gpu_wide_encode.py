"""fec_encode_scatter_wide_rs_dev on the GPU: the scatter encode for k + r <= 256 with no cap on
min(k, r), packets taken through a table of addresses (with or without a length per packet, address
0 = absent), every parity row written to a table of destinations, cut at the group's symbol length.

Truth is oracle.rs_encode (it serves k + r <= 256) on the packets zero-padded to P, cut at L_g; row 0
of every group with a packet present is also oracle.go_generate_redundancy's repair payload on the
true packets.  Bit-exact, no tolerance.  test_gpu_gather_var.make_case goes through the one-word
decode, so the wide cases are built here (wide_case) with the attributes build_arena and
test_gpu_scatter_encode.make_encode read: packets at their true lengths in two arenas with pads of
1..37 bytes of 0xEE, every residue mod 16, a length-0 packet pointing at pad bytes, an absent packet
as address 0 with a junk length entry.  Destinations are in an allocation of their own, 0x5A with
256-byte guards; after each call the whole allocation equals the expected image and both arenas are
unchanged.  The entries of a group with L_g = 0 point at valid memory.  G = 67 unless said.
"""
import os
import threading
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_gather import GUARD, hooks_ctx, product_ctx
from test_gpu_gather_var import JUNK_LEN, dealt_lengths, padded
from test_gpu_scatter import packed_layout, slot_layout
from test_gpu_scatter_encode import HDR, check_encode, make_encode, residue_layout

pytestmark = pytest.mark.gpu

SEED = 0x71DE0000
G_MAIN = 67
POL = 1 | 2 | 4 | 1024                                                        # fec_forms.hpp kWideEncodePol
# k at and across the 64-lane stride, r at and across the 8-row pass, the two shapes the wide recover
# refuses (33+33, 128+128), and a size with whole 1-KiB passes plus a tail
SHAPES = [(65, 3, (16, 272, 1200)),
          (64, 9, (17,)),
          (129, 17, (260,)),
          (224, 32, (16, 1200)),
          (32, 224, (48,)),
          (128, 128, (48,)),
          (33, 33, (1025,)),
          (255, 1, (16,)),
          (1, 255, (16,)),
          (100, 20, (1037, 2100))]
SHAPE_CASES = [(k, r, P) for k, r, sizes in SHAPES for P in sizes]


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases: one batch and what the oracle says about it, computed once and never modified
# ------------------------------------------------------------------------------------------
def wide_case(oracle, k, r, P, dlens, present, seed):
    """dlens (G, k): the packets' true lengths; present (G, k) bool: an absent packet counts as zeros."""
    dlens = np.asarray(dlens, dtype=np.int64)
    present = np.asarray(present, dtype=bool)
    G = len(dlens)
    L = int(max(dlens.max(), P))
    raw = oracle.splitmix_bytes(G * k * L, seed).reshape(G, k, L)
    data = padded(raw, np.where(present, dlens, 0), P)                       # (G, k, P)
    par = oracle.rs_encode(np.ascontiguousarray(data).reshape(-1), G, k, r, P, nthreads=8).reshape(G, r, P)
    sym = np.where(present, np.minimum(dlens, P), 0).max(axis=1)
    assert not (par * (np.arange(P)[None, None, :] >= sym[:, None, None])).any()     # zero past L_g
    for g in range(G):
        if sym[g] == 0:                                                      # the reference emits no repair packet
            assert not par[g].any()
            continue
        pk = [np.ascontiguousarray(raw[g, j, :min(int(dlens[g, j]), P)]) for j in range(k) if present[g, j]]
        pay = oracle.go_generate_redundancy(pk, group_id=g)[HDR:]
        assert len(pay) == sym[g]
        assert np.array_equal(par[g, 0, :len(pay)], pay)
    c = SimpleNamespace(k=k, r=r, P=P, G=G, present=present, raw=raw, lens=dlens, data=data, par=par,
                        sym_enc=sym.astype(np.uint32))
    for a in (c.present, c.raw, c.lens, c.data, c.par, c.sym_enc):
        a.setflags(write=False)
    return c


def _salt(k, r, P):
    return k * 1000000 + r * 10000 + P


@lru_cache(maxsize=None)
def mixed_case(oracle, k, r, P, G=G_MAIN):
    """Edge lengths (0 and 2P among them) dealt over the packets; group 1 has one packet present, group 3
    none, group 5 all present with every length P, group 6 all lengths 0, the others about 85% present."""
    dl = dealt_lengths(P, G, k).copy()
    present = np.ones((G, k), dtype=bool)
    present[4:] = np.random.default_rng(SEED + _salt(k, r, P)).random((G - 4, k)) < 0.85
    present[1] = False
    present[1, k // 2] = True
    present[3] = False
    present[5] = True
    dl[5] = P
    dl[6] = 0
    if not (present[7:] & (dl[7:] == 0)).any():                               # k = 1 may have drawn them all absent
        g0 = 7 + int(np.flatnonzero((dl[7:] == 0).any(axis=1))[0])
        present[g0, int(np.flatnonzero(dl[g0] == 0)[0])] = True
    if not (present[7:] & (dl[7:] == 2 * P)).any():
        g2 = 7 + int(np.flatnonzero((dl[7:] == 2 * P).any(axis=1))[0])
        present[g2, int(np.flatnonzero(dl[g2] == 2 * P)[0])] = True
    if present[7:].all():
        present[8, 0] = False
    c = wide_case(oracle, k, r, P, dl, present, SEED + _salt(k, r, P) + 1)
    # the composition, on the CPU
    assert (~c.present).any(), "no absent packet"
    assert (c.present & (c.lens == 0))[7:].any(), "no present packet of length 0"
    assert (c.present & (c.lens == 2 * P)).any(), "no length of 2P"
    assert c.present[1].sum() == 1 and not c.present[3].any() and c.present[5].all() and (c.lens[5] == P).all()
    assert c.sym_enc[3] == 0 and c.sym_enc[6] == 0 and c.sym_enc[5] == P and c.sym_enc.max() == P
    return c


@lru_cache(maxsize=None)
def full_case(oracle, k, r, P, G=G_MAIN, absent=True):
    """Every length P (the inputs of a NULL length table).  absent: every fourth group whole, group 3
    with no packet, the others about 85% present."""
    present = np.ones((G, k), dtype=bool)
    if absent:
        present = np.random.default_rng(SEED + _salt(k, r, P) + 2).random((G, k)) < 0.85
        present[::4] = True
        present[3] = False
        present[1] = False
        present[1, k - 1] = True
        if present[5].all():
            present[5, 0] = False
        assert present[4].all() and not present[5].all() and present[1].sum() == 1
    return wide_case(oracle, k, r, P, np.full((G, k), P), present, SEED + _salt(k, r, P) + 3 + absent)


@lru_cache(maxsize=None)
def cut_case(oracle, k, r, P):
    """G = P + 1 and group g's longest packet has length g, so L_g takes every value 0..P; the other
    packets have edge lengths capped at g; about one packet in seven is absent."""
    G = P + 1
    g = np.arange(G)
    dl = np.minimum(dealt_lengths(P, G, k), g[:, None])
    present = np.random.default_rng(SEED + _salt(k, r, P) + 5).random((G, k)) < 6.0 / 7.0
    present[g, g % k] = True
    dl[g, g % k] = g
    c = wide_case(oracle, k, r, P, dl, present, SEED + _salt(k, r, P) + 6)
    assert np.array_equal(c.sym_enc, g)                                      # every cut 0..P
    share = 1.0 - c.present.mean()
    assert 0.10 < share < 0.18, share
    return c


# ------------------------------------------------------------------------------------------
# One call
# ------------------------------------------------------------------------------------------
def launch(ctx, b, stream=None, wide=True):
    c = b.c
    call = ctx.encode_scatter_wide_dev if wide else ctx.encode_scatter_dev
    call(b.table, b.lens, b.dtab, c.G, c.k, c.r, c.P, b.so, stream=stream)


def check_tables(b):
    """On the CPU, before a launch: an absent packet is address 0 with a junk length entry; a present
    packet of length 0 has a non-zero address that points at pad bytes."""
    c = b.c
    table = b.table.cpu().numpy().view(np.uint64).reshape(c.G, c.k)
    assert np.array_equal(table == 0, ~c.present)
    if b.lens is None:
        return
    lens = b.lens.cpu().numpy().view(np.uint32).reshape(c.G, c.k)
    assert (lens[~c.present] == JUNK_LEN).all()
    for g, j in zip(*np.nonzero(c.present & (c.lens == 0))):
        hit = [img[int(table[g, j]) - d.data_ptr()] for d, img in b.images[:-1]
               if d.data_ptr() <= int(table[g, j]) < d.data_ptr() + d.numel()]
        assert hit == [0xEE], (g, j, hit)


def run(torch, ctx, c, seed, layout, what="", stream=None, **kw):
    b = make_encode(torch, c, seed, layout, **kw)
    check_tables(b)
    torch.cuda.synchronize()
    launch(ctx, b, stream)
    ctx.synchronize()
    torch.cuda.synchronize()
    check_encode(b, what)
    return b


# ------------------------------------------------------------------------------------------
# 1. Shapes and sizes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", [False, True], ids=["fixed", "lens"])
@pytest.mark.parametrize("k,r,P", SHAPE_CASES)
def test_shapes_and_sizes(quicfec_mod, oracle_mod, torch_cuda, k, r, P, var):
    """Every shape and size with the length table (the mixed case) and without it (every length P, absent
    packets): destinations at every start residue mod 16 with 1..16 guard bytes between two rows."""
    c = mixed_case(oracle_mod, k, r, P) if var else full_case(oracle_mod, k, r, P)
    with product_ctx(quicfec_mod) as ctx:
        b = run(torch_cuda, ctx, c, SEED + 11, residue_layout, with_lens=var)
    assert b.dest.data_ptr() % 16 == 0 and set((b.offs % 16).tolist()) == set(range(16))
    gaps = b.offs[1:] - (b.offs[:-1] + b.sym[np.repeat(np.arange(c.G), r)][:-1])
    assert gaps.min() >= 1 and gaps.max() <= 16


# ------------------------------------------------------------------------------------------
# 2. The mixed case
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(65, 3, 272), (100, 20, 1037), (33, 33, 1025)])
def test_mixed_case_packed(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """An absent packet with a junk length, a present packet of length 0 pointing at pad bytes, a length
    of 2P, a group with one packet, one with none and one with all lengths P (asserted in mixed_case and
    check_tables), the rows packed back to back."""
    c = mixed_case(oracle_mod, k, r, P)
    with product_ctx(quicfec_mod) as ctx:
        run(torch_cuda, ctx, c, SEED + 12, packed_layout)


# ------------------------------------------------------------------------------------------
# 3. Every cut
# ------------------------------------------------------------------------------------------
def test_every_cut(quicfec_mod, oracle_mod, torch_cuda):
    """(65, 3) at P = 272 with G = 273: L_g takes every value 0..P, destinations back to back, so a byte
    stored before a destination or at or past destination + L_g lands in a neighbour's row."""
    c = cut_case(oracle_mod, 65, 3, 272)
    assert c.G == 273 and set(c.sym_enc.tolist()) == set(range(273))
    with product_ctx(quicfec_mod) as ctx:
        run(torch_cuda, ctx, c, SEED + 13, packed_layout)


# ------------------------------------------------------------------------------------------
# 4. Unwanted rows
# ------------------------------------------------------------------------------------------
def test_unwanted_rows(quicfec_mod, oracle_mod, torch_cuda):
    """(100, 20): a quarter of the destination entries 0, group 7 with the whole second pass (rows 8..15)
    unwanted, group 9 with every row unwanted: the stored rows are right, everything else stays 0x5A and
    L_g is still written; once more without d_symbol_len_out."""
    k, r, P = 100, 20, 1037
    c = mixed_case(oracle_mod, k, r, P)
    unwanted = np.random.default_rng(SEED + 14).random((c.G, r)) < 0.25
    unwanted[7] = False
    unwanted[7, 8:16] = True
    unwanted[9] = True
    assert 0.2 < unwanted.mean() < 0.3 and c.sym_enc[7] > 0 and c.sym_enc[9] > 0
    assert unwanted[7, 8:16].all() and not unwanted[7, :8].any() and unwanted[9].all()
    with product_ctx(quicfec_mod) as ctx:
        for with_lens in (True, False):
            cc = c if with_lens else full_case(oracle_mod, k, r, P)
            b = run(torch_cuda, ctx, cc, SEED + 15, residue_layout, with_lens=with_lens, unwanted=unwanted)
            assert b.so is not None                                           # check_encode compared L_g of every group
        b = run(torch_cuda, ctx, c, SEED + 16, packed_layout, unwanted=unwanted, want_sym=False)
        assert b.so is None


# ------------------------------------------------------------------------------------------
# 5. / 6. Equivalences
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", [False, True], ids=["fixed", "lens"])
@pytest.mark.parametrize("k,r,P", [(10, 3, 1200), (12, 9, 260), (32, 32, 16)])
def test_one_word_shapes_equal_the_scatter_encode(quicfec_mod, oracle_mod, torch_cuda, k, r, P, var):
    """k + r <= 64: the destination allocation and the symbol lengths byte for byte those of
    fec_encode_scatter_rs_dev on the same tables."""
    torch = torch_cuda
    c = mixed_case(oracle_mod, k, r, P) if var else full_case(oracle_mod, k, r, P)
    unwanted = np.random.default_rng(SEED + 17).random((c.G, r)) < 0.1
    with product_ctx(quicfec_mod) as ctx:
        wide = make_encode(torch, c, SEED + 18, residue_layout, with_lens=var, unwanted=unwanted)
        narrow = make_encode(torch, c, SEED + 18, residue_layout, with_lens=var, unwanted=unwanted)
        torch.cuda.synchronize()
        launch(ctx, wide)
        launch(ctx, narrow, wide=False)
        ctx.synchronize()
        torch.cuda.synchronize()
    check_encode(wide)
    check_encode(narrow)
    assert np.array_equal(wide.dest.cpu().numpy(), narrow.dest.cpu().numpy())
    assert np.array_equal(wide.so.cpu().numpy(), narrow.so.cpu().numpy())


@pytest.mark.parametrize("k,r,P", [(224, 32, 1200), (128, 128, 48)])
def test_slot_layout_equals_the_contiguous_encode(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """All lengths P, every packet present, destinations at d_parity + (g*r + i)*P: byte for byte
    fec_encode_batch_rs_dev on the same packets laid contiguously."""
    torch = torch_cuda
    c = full_case(oracle_mod, k, r, P, absent=False)
    assert c.present.all() and (c.lens == P).all()
    with product_ctx(quicfec_mod) as ctx:
        b = make_encode(torch, c, SEED + 19, slot_layout, with_lens=False)
        d = torch.from_numpy(c.data.reshape(-1).copy()).cuda()                 # the case itself is read-only
        par = torch.full((GUARD + c.G * r * P + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        launch(ctx, b)
        ctx.encode_dev(d, c.G, k, r, P, par[GUARD:GUARD + c.G * r * P])
        ctx.synchronize()
        torch.cuda.synchronize()
    check_encode(b)
    assert np.array_equal(b.dest.cpu().numpy(), par.cpu().numpy())
    assert np.array_equal(d.cpu().numpy(), c.data.reshape(-1))


# ------------------------------------------------------------------------------------------
# 7. Round trip with the wide recover
# ------------------------------------------------------------------------------------------
def test_round_trip_with_the_wide_recover(quicfec_mod, oracle_mod, torch_cuda):
    """(224, 32) at 272: parity encoded into the holes of the arena that holds the packets, then
    min(k, r) data addresses per group zeroed and fec_recover_scatter_wide_rs_dev run on the arena: the
    rebuilt packets are the originals."""
    torch = torch_cuda
    k, r, P, G = 224, 32, 272, G_MAIN
    n, e = k + r, min(k, r)
    c = full_case(oracle_mod, k, r, P, absent=False)
    S = P + 23                                                                # odd stride: every residue
    off = 1 + np.arange(G * n, dtype=np.int64).reshape(G, n) * S
    arena_in = np.full(1 + G * n * S + 64, 0x5A, dtype=np.uint8)
    slots = arena_in[1:1 + G * n * S].reshape(G, n, S)
    slots[:, :k, :P] = c.data
    arena = torch.from_numpy(arena_in).cuda()
    at = (arena.data_ptr() + off).astype(np.uint64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).cuda()
    rng = np.random.default_rng(SEED + 20)
    lost = np.zeros((G, n), dtype=bool)
    for g in range(G):
        lost[g, rng.choice(k, size=e, replace=False)] = True
    assert (lost[:, :k].sum(axis=1) == e).all()
    out = torch.full((GUARD + G * e * P + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    dests = np.zeros((G, k), dtype=np.uint64)
    expect = np.full(out.numel(), 0x5A, dtype=np.uint8)
    for g in range(G):
        for m, j in enumerate(np.flatnonzero(lost[g, :k])):
            dests[g, j] = out.data_ptr() + GUARD + (g * e + m) * P
            expect[GUARD + (g * e + m) * P:GUARD + (g * e + m + 1) * P] = c.data[g, j]
    st = torch.full((G,), 0xAA, dtype=torch.uint8, device="cuda")
    sym = torch.full((G,), 0x77777777, dtype=torch.int32, device="cuda")
    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        ctx.encode_scatter_wide_dev(up(at[:, :k]), None, up(at[:, k:]), G, k, r, P, sym)
        ctx.synchronize()
        filled = arena.cpu().numpy()
        image = arena_in.copy()
        image[1:1 + G * n * S].reshape(G, n, S)[:, k:, :P] = c.par
        assert np.array_equal(filled, image) and (sym.cpu().numpy() == P).all()
        ctx.recover_scatter_wide_dev(up(np.where(lost, np.uint64(0), at)), None, up(dests), G, k, r, P, st)
        ctx.synchronize()
        torch.cuda.synchronize()
    assert not st.cpu().numpy().any()
    assert np.array_equal(out.cpu().numpy(), expect)
    assert np.array_equal(arena.cpu().numpy(), image)


# ------------------------------------------------------------------------------------------
# 8. Chunked launches and the trace
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", [False, True], ids=["fixed", "lens"])
def test_chunked_launches_and_the_trace(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, var):
    """The test library with 3 workgroups (12 groups) per launch at (100, 20): the same bytes, and the
    trace is, for each pass in order, one encode_scatter_wide launch per chunk, the chunks covering
    [0, G) once, in order; every chunk takes its own part of the four tables."""
    torch = torch_cuda
    q = quicfec_mod
    lib = q.load_test_library()
    k, r, P = 100, 20, 1037
    c = mixed_case(oracle_mod, k, r, P) if var else full_case(oracle_mod, k, r, P)
    G = c.G
    with hooks_ctx(q) as ctx:
        b = make_encode(torch, c, SEED + 21, residue_layout, with_lens=var)
        monkeypatch.setenv("QUICFEC_MAX_WAVE_BLOCKS", "3")
        torch.cuda.synchronize()
        q.launch_trace(lib)
        launch(ctx, b)
        ctx.synchronize()
        torch.cuda.synchronize()
        records = q.launch_trace(lib)
    trace = [(t["form"], t["first_item"], t["items"], t["aux"], t["pol"]) for t in records]
    check_encode(b)
    chunks = [(g0, min(12, G - g0)) for g0 in range(0, G, 12)]
    assert chunks[0][0] == 0 and sum(n for _, n in chunks) == G and len(chunks) == 6
    want = [("encode_scatter_wide", g0, gn, 8 * p, POL) for p in range(-(-r // 8)) for g0, gn in chunks]
    assert trace == want
    assert {t["first"] for t in records} == {int(var)} and {t["grid"] for t in records} == {3, 2}


def test_trace_names_the_length_table_form(quicfec_mod, oracle_mod, torch_cuda):
    """At the library's defaults one launch per pass; `first` is 1 with a length table, 0 without."""
    torch = torch_cuda
    q = quicfec_mod
    lib = q.load_test_library()
    with hooks_ctx(q) as ctx:
        for var in (True, False):
            c = mixed_case(oracle_mod, 65, 3, 272) if var else full_case(oracle_mod, 65, 3, 272)
            b = make_encode(torch, c, SEED + 22, packed_layout, with_lens=var)
            torch.cuda.synchronize()
            q.launch_trace(lib)
            launch(ctx, b)
            ctx.synchronize()
            torch.cuda.synchronize()
            trace = q.launch_trace(lib)
            check_encode(b, var)
            assert [(t["form"], t["first_item"], t["items"], t["aux"], t["pol"], t["first"], t["k"], t["r"], t["grid"], t["block"])
                    for t in trace] == [("encode_scatter_wide", 0, c.G, 0, POL, int(var), 0, 8, (c.G + 3) // 4, 256)]


# ------------------------------------------------------------------------------------------
# 9. State across calls
# ------------------------------------------------------------------------------------------
def test_three_shapes_queued_on_one_stream(quicfec_mod, oracle_mod, torch_cuda):
    """Three calls of different shapes back to back on one side stream with no host synchronise between
    them (each shape's coefficient table is uploaded at its first call), then the first shape again."""
    torch = torch_cuda
    cases = [(mixed_case(oracle_mod, 65, 3, 272), True), (full_case(oracle_mod, 100, 20, 1037), False),
             (mixed_case(oracle_mod, 33, 33, 1025), True), (full_case(oracle_mod, 65, 3, 272), False)]
    stream = torch.cuda.Stream()
    with product_ctx(quicfec_mod) as ctx:
        calls = [make_encode(torch, c, SEED + 30 + i, residue_layout, with_lens=var) for i, (c, var) in enumerate(cases)]
        torch.cuda.synchronize()
        for b in calls:
            launch(ctx, b, stream.cuda_stream)
        torch.cuda.synchronize()
    for i, b in enumerate(calls):
        check_encode(b, i)


def test_two_threads_on_two_streams(quicfec_mod, oracle_mod, torch_cuda):
    """Two host threads, each with its own side stream and its own shape, six calls each on one context
    from a barrier."""
    torch = torch_cuda
    cases = [mixed_case(oracle_mod, 65, 3, 272), mixed_case(oracle_mod, 100, 20, 1037)]
    layouts = (residue_layout, packed_layout)
    work = [[make_encode(torch, cases[t], SEED + 40 + j, layouts[j % 2]) for j in range(6)] for t in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2)
    errors = []

    def go(t, ctx):
        try:
            barrier.wait(timeout=60)
            for b in work[t]:
                launch(ctx, b, streams[t].cuda_stream)
        except BaseException as e:                                             # re-raised in the test
            errors.append((t, e))

    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        threads = [threading.Thread(target=go, args=(t, ctx)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
    if errors:
        raise errors[0][1]
    for t in range(2):
        for j, b in enumerate(work[t]):
            check_encode(b, (t, j))


def test_free_with_a_call_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """Two calls queued on a side stream and the context freed at once: fec_encoder_free drains the
    stream (the kernels read the context's coefficient table), so both outputs are complete."""
    torch = torch_cuda
    calls = [make_encode(torch, mixed_case(oracle_mod, 100, 20, 2100), SEED + 50, residue_layout),
             make_encode(torch, full_case(oracle_mod, 100, 20, 2100), SEED + 51, slot_layout, with_lens=False)]
    stream = torch.cuda.Stream()
    ctx = product_ctx(quicfec_mod)
    torch.cuda.synchronize()
    for b in calls:
        launch(ctx, b, stream.cuda_stream)
    ctx.close()
    assert stream.query()                                                      # the free drained the stream
    torch.cuda.synchronize()
    for b in calls:
        check_encode(b)


# ------------------------------------------------------------------------------------------
# 10. Refusals
# ------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(quicfec_mod, oracle_mod, torch_cuda):
    """k = 0, r = 0, 200+57, P = 15, G = 0, G = 2^32 and each required NULL pointer: the code, a message
    naming the case, nothing launched, every buffer untouched; the same buffers then serve a good call.
    33+33 and 128+128 are served.  fec_encode_scatter_rs_dev still refuses 60+5 in its own words."""
    torch = torch_cuda
    q = quicfec_mod
    lib = q.load_test_library()
    name = "fec_encode_scatter_wide_rs_dev"
    c = mixed_case(oracle_mod, 100, 20, 1037)
    G = c.G
    with hooks_ctx(q) as ctx:
        b = make_encode(torch, c, SEED + 60, residue_layout)
        torch.cuda.synchronize()
        q.launch_trace(lib)
        p = lambda t: t.data_ptr()
        for (k, r, P, groups), text in (((0, 20, 1037, G), "k>0"), ((100, 0, 1037, G), "r>0"), ((200, 57, 1037, G), "k+r<=256"),
                                        ((100, 20, 15, G), "below 16"), ((100, 20, 1037, 0), "num_groups is 0"),
                                        ((100, 20, 1037, 2**32), "32-bit group indices")):
            rc = getattr(lib, name)(ctx.handle, p(b.table), p(b.lens), p(b.dtab), groups, k, r, P, p(b.so), None)
            assert rc == q.FEC_ERR_RANGE and text in q.last_error(lib), (k, r, P, groups, q.last_error(lib))
            assert name in q.last_error(lib)
        args = [ctx.handle, p(b.table), p(b.lens), p(b.dtab)]
        for i, word in ((0, "context"), (1, "d_packet_addrs"), (3, "d_dest_addrs")):
            bad = list(args)
            bad[i] = None
            assert getattr(lib, name)(*bad, G, 100, 20, 1037, p(b.so), None) == q.FEC_ERR_NULL
            assert word in q.last_error(lib) and name in q.last_error(lib)
        # the narrow call's bound and message are as they were
        rc = lib.fec_encode_scatter_rs_dev(ctx.handle, p(b.table), p(b.lens), p(b.dtab), G, 60, 5, 1037, p(b.so), None)
        assert rc == q.FEC_ERR_RANGE
        assert "scatter encode: k=60 r=5: k + r exceeds 64 shards per group" in q.last_error(lib)
        ctx.synchronize()
        torch.cuda.synchronize()
        assert q.launch_trace(lib) == []
        assert (b.dest == 0x5A).all().item() and (b.so == 0x77777777).all().item()
        for d, image in b.images[:-1]:
            assert np.array_equal(d.cpu().numpy(), image)
        launch(ctx, b)                                                         # and the same buffers are served
        ctx.synchronize()
        torch.cuda.synchronize()
        check_encode(b)
        assert len(q.launch_trace(lib)) == 3
        # no min(k, r) cap
        for k, r, P in ((33, 33, 1025), (128, 128, 48)):
            ok = run(torch, ctx, mixed_case(oracle_mod, k, r, P), SEED + 61, packed_layout)
            assert {t["form"] for t in q.launch_trace(lib)} == {"encode_scatter_wide"} and ok.so is not None
