"""fec_recover_scatter_wide_rs_dev on the GPU: the scatter recover for k + r <= 256, shards taken
through a table of addresses (with or without a length per entry), rebuilt packets written to a table
of destinations, cut at the group's symbol length.

The oracle's decode stops at 64 shards, so the truth for a rebuilt row is the original data, as in
test_gpu_wide.py: data is seeded (each data shard real up to its own length, zeros up to P), parity
is oracle.rs_encode's of the zero-padded shards, the roles come from wide_masks.roles over the mask
the zero addresses imply, and seeded junk fills every parity row the rule does not read and the
length entry of every lost shard.  Shards lie at odd byte offsets in an arena with 0x5A guard bytes
between them; with a length table, seeded junk sits directly after each shard's `len` bytes, so a
load past `len` that reached the arithmetic would corrupt a row.  Destinations lie in a buffer
prefilled 0x5A between 256-byte guards (or are the arena's holes); the entry of every shard the call
does not rebuild points into a trap region that must stay 0x5A.  Status is prefilled 0xAA, masks and
symbol lengths with junk.  One case serves the run without and the run with the length table: without
it every present shard is its zero-padded P bytes.  G = 67 unless said otherwise.
"""
import os
import threading
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import unread_shards as us
import wide_masks as wm
from test_gpu_gather import hooks_ctx, product_ctx
from test_gpu_wide import check_kinds, drawn_group, planted_groups
from test_gpu_wide import main_case as contiguous_case

pytestmark = pytest.mark.gpu

SEED = 0x7AB1E000
G_MAIN = 67
GUARD = 256
TRAP = 4096
# (k, r, sizes): the word boundaries, the extremes, the pass counts and the walks
SHAPES = [(60, 5, (16, 272, 1200)),
          (64, 2, (16,)),
          (127, 3, (272,)),
          (190, 5, (48,)),
          (224, 32, (16, 1200)),
          (32, 224, (48,)),
          (255, 1, (16,)),
          (1, 255, (16,)),
          (100, 20, (1037, 4096))]
L_VALUES = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1025)
LENGTH_KINDS = ("all_P", "L", "longer", "L", "zero_shard", "L", "parity_long", "L")
DEST_MODES = ("holes", "packed", "slots", "odd")
POL = 1 | 2 | 4 | 1024                                                        # fec_forms.hpp kWideTablePol


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases
# ------------------------------------------------------------------------------------------
def l_values(P):
    return [x for x in L_VALUES + (P - 1,) if x <= P]


def draw_lengths(k, r, P, ro, rng):
    """Per group: the true length of each data shard (G, k), the length of its parity rows (G,), the
    table entry that is longer than P ((g, s) or none) and the kind drawn."""
    G = len(ro.ok)
    tl = np.full((G, k), P, dtype=np.int64)
    plen = np.full(G, P, dtype=np.int64)
    longer, kinds = {}, []
    allowed = l_values(P)
    nth = 0
    for g in range(G):
        kind = LENGTH_KINDS[g % len(LENGTH_KINDS)]
        present_d = np.flatnonzero(~ro.lost_d[g])
        lost_d = np.flatnonzero(ro.lost_d[g])
        present = np.concatenate([present_d, k + np.flatnonzero(~ro.lost_p[g])])
        if kind == "longer" and len(present):
            longer[g] = int(rng.choice(present))
        elif kind == "L":
            D = allowed[nth % len(allowed)]
            nth += 1
            tl[g] = rng.integers(0, D + 1, size=k)
            tl[g, rng.integers(0, k)] = D
            plen[g] = D
        elif kind == "zero_shard":
            D = int(rng.choice([x for x in allowed if x >= 1]))
            tl[g] = rng.integers(1, D + 1, size=k)
            top = int(rng.integers(0, k))
            tl[g, top] = D
            others = [j for j in present_d if j != top]
            if others:
                tl[g, int(rng.choice(others))] = 0
            plen[g] = D
        elif kind == "parity_long":
            D = int(rng.choice([x for x in allowed if x >= 2]))
            tl[g] = rng.integers(0, D // 2 + 1, size=k)
            if len(lost_d):
                tl[g, lost_d] = rng.integers(0, D + 1, size=len(lost_d))
                tl[g, lost_d[0]] = D
            plen[g] = D
        kinds.append(kind)
    return tl, plen, longer, kinds


class Case:
    def __init__(self, oracle, k, r, P, bits, seed, planted=None):
        self.k, self.r, self.P, self.G, self.seed = k, r, P, len(bits), seed
        G, n = self.G, k + r
        self.n = n
        bits = np.asarray(bits, dtype=bool).copy()
        bits[:, n:] = False
        self.masks = wm.from_bits(bits)                                        # every bit at and above k + r zero
        self.ro = ro = wm.roles(self.masks, k, r)
        self.e = ro.lost_d.sum(axis=1)
        self.rebuilds = ro.ok & (self.e >= 1)
        self.status = wm.status(ro)
        self.lost = np.concatenate([ro.lost_d, ro.lost_p], axis=1)             # (G, n)
        rng = np.random.default_rng([SEED, seed & 0xFFFFFFFF, 1])
        self.tl, self.plen, self.longer, self.kinds = draw_lengths(k, r, P, ro, rng)
        raw = oracle.splitmix_bytes(G * k * P, seed).reshape(G, k, P)
        self.orig = np.where(np.arange(P)[None, None, :] < self.tl[:, :, None], raw, 0).astype(np.uint8)
        self.par = oracle.rs_encode(np.ascontiguousarray(self.orig).reshape(-1), G, k, r, P, 8).reshape(G, r, P)
        # the length table: present data its own length, present rows the repair payload's, one entry past
        # P where drawn, junk for every lost entry
        lens = np.concatenate([self.tl, np.repeat(self.plen[:, None], r, axis=1)], axis=1).astype(np.uint32)
        for g, s in self.longer.items():
            lens[g, s] = (P + 1, P + 4096, 0xFFFFFFFF)[g % 3]
        junk = np.random.default_rng([SEED, seed & 0xFFFFFFFF, 2]).integers(0, 2**32, size=lens.shape, dtype=np.uint32)
        self.lens = np.where(self.lost, junk, lens).astype(np.uint32)
        eff = np.where(self.lost, 0, np.minimum(self.lens, P)).astype(np.int64)
        self.eff = eff                                                         # readable bytes per entry, 0 where lost
        self.symlen_var = eff.max(axis=1).astype(np.uint32)                    # L_g by numpy
        self.symlen_fixed = np.where((~self.lost).any(axis=1), P, 0).astype(np.uint32)
        # the shards as the arena holds them: (G, n, P); unread parity rows are junk throughout
        true = np.concatenate([self.orig, self.par], axis=1)
        unread = np.concatenate([np.zeros_like(ro.lost_d), ro.unread_p & ~ro.lost_p], axis=1)
        fill = us.junk(G * n * P, seed + 3).reshape(G, n, P) | 1                # never zero
        self.shards_fixed = np.where(unread[:, :, None], fill, true)
        past = np.arange(P)[None, None, :] >= eff[:, :, None]
        self.shards_var = np.where(unread[:, :, None] | past, fill, true)      # junk directly after len bytes
        # on the CPU, before anything is launched
        assert (np.where(past, 0, true) == true)[~self.lost].all(), "a present shard has bytes past its length"
        assert (self.symlen_var[self.rebuilds] >= self.tl.max(axis=1)[self.rebuilds]).all()
        if planted is not None:
            for kind, groups in planted.items():
                for g, want in groups:
                    assert np.array_equal(bits[g, :n], want[:n]), kind
            assert self.rebuilds.sum() * 4 >= 3 * G, "fewer than three quarters of the groups are rebuilt"

    def symlen(self, var):
        return self.symlen_var if var else self.symlen_fixed


@lru_cache(maxsize=None)
def main_case(oracle, k, r, P, G=G_MAIN):
    salt = k * 1000000 + r * 10000 + P
    rng = np.random.default_rng([SEED, salt])
    kinds = planted_groups(k, r)
    bits, planted = [], {}
    for kind, groups in kinds.items():
        planted[kind] = [(len(bits) + i, b) for i, b in enumerate(groups)]
        bits += groups
    assert len(bits) <= G // 3
    bits += [drawn_group(k, r, rng) for _ in range(G - len(bits))]
    c = Case(oracle, k, r, P, np.array(bits), SEED + salt, planted)
    check_kinds(c, planted)
    # every kind of length, and every L the size allows, in a group that is rebuilt
    seen_kinds = {c.kinds[g] for g in np.flatnonzero(c.rebuilds)}
    assert seen_kinds == set(LENGTH_KINDS), seen_kinds
    seen = set(c.symlen_var[c.rebuilds].tolist())
    assert set(l_values(P)) <= seen, sorted(set(l_values(P)) - seen)
    assert any(c.rebuilds[g] for g in c.longer) and (c.lens[~c.lost] > P).any()
    zero = (c.eff == 0) & ~c.lost
    zero[:, k:] &= c.ro.chosen                                                 # a row the rule reads
    if k >= 2:                                                                 # k = 1: the survivors are rows of L_g bytes
        assert (zero.any(axis=1) & c.rebuilds & (c.symlen_var > 0)).any(), "no present shard of length 0 among the survivors"
    only_parity = c.rebuilds & (c.eff[:, :k].max(axis=1) < c.symlen_var)
    assert only_parity.any(), "no group whose only long shard is a parity row"
    return c


# ------------------------------------------------------------------------------------------
# Device buffers of one call
# ------------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(torch, init):
    """`init` (u8) on the device between two guards of its own kind of fill."""
    whole = torch.full((GUARD + len(init) + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    whole[GUARD:GUARD + len(init)].copy_(_dev(torch, init))
    return whole, whole[GUARD:GUARD + len(init)]


def slot_stride(P):
    return P + 23 if P % 2 == 0 else P + 22                                    # odd: the addresses take every residue


def make_call(torch, c, var, dest_mode, seed=0):
    """The arena, the tables and the outputs of one call; `expect`: what the destination buffer holds
    afterwards, by numpy."""
    k, r, P, G, n = c.k, c.r, c.P, c.G, c.n
    b = SimpleNamespace(c=c, var=var, dest_mode=dest_mode)
    S = slot_stride(P)
    shard_off = 1 + np.arange(G * n, dtype=np.int64).reshape(G, n) * S         # odd offsets
    arena = np.full(1 + G * n * S + 64, 0x5A, dtype=np.uint8)
    rows = arena[1:1 + G * n * S].reshape(G * n, S)
    content = (c.shards_var if var else c.shards_fixed).reshape(G * n, P)
    present = ~c.lost.reshape(-1)
    rows[present, :P] = content[present]                                       # a lost shard's place stays a hole of 0x5A
    b.arena_in = arena
    b.arena = _dev(torch, arena)
    b.addrs_np = np.where(c.lost, 0, b.arena.data_ptr() + shard_off).astype(np.uint64)
    b.addrs = _dev(torch, b.addrs_np.view(np.int64).reshape(-1))
    b.lens = _dev(torch, c.lens.view(np.int32).reshape(-1)) if var else None
    L = c.symlen(var).astype(np.int64)
    # the rows the call rebuilds, in order: (g, j, m)
    rebuilt = [(g, int(j), m) for g in np.flatnonzero(c.rebuilds) for m, j in enumerate(np.flatnonzero(c.ro.lost_d[g]))]
    off = {}
    if dest_mode == "holes":
        size = 0
        for g, j, m in rebuilt:
            off[g, j] = int(shard_off[g, j])
    elif dest_mode == "packed":
        at = 1
        for g, j, m in rebuilt:
            off[g, j] = at
            at += int(L[g])
        size = at + 3
    elif dest_mode == "slots":
        for g, j, m in rebuilt:
            off[g, j] = (g * r + m) * P
        size = G * r * P
    else:                                                                      # "odd": gaps of 13, every alignment
        for i, (g, j, m) in enumerate(rebuilt):
            off[g, j] = 3 + i * (P + 13)
        size = 3 + len(rebuilt) * (P + 13)
    # "not wanted": the second lost shard of every third rebuilt group with two or more
    b.unwanted = set()
    for g in np.flatnonzero(c.rebuilds & (c.e >= 2))[::3]:
        b.unwanted.add((int(g), int(np.flatnonzero(c.ro.lost_d[g])[1])))
    if min(k, r) >= 2:
        assert b.unwanted
    if dest_mode == "holes":
        b.owhole = b.out = b.arena
        out_in = arena
        base = 0
    else:
        out_in = np.full(size, 0x5A, dtype=np.uint8)
        b.owhole, b.out = _guarded(torch, out_in)
        base = GUARD
        out_in = b.owhole.cpu().numpy()
    b.trap = torch.full((TRAP + P,), 0x5A, dtype=torch.uint8, device="cuda")
    dests = np.full((G, k), b.trap.data_ptr() + 1027, dtype=np.uint64)         # every entry the call must not use
    expect = out_in.copy()
    for g, j, m in rebuilt:
        if (g, j) in b.unwanted:
            dests[g, j] = 0
            continue
        dests[g, j] = b.owhole.data_ptr() + base + off[g, j]
        expect[base + off[g, j]:base + off[g, j] + int(L[g])] = c.orig[g, j, :int(L[g])]
    b.expect = expect
    b.dests_np = dests
    b.dests = _dev(torch, dests.view(np.int64).reshape(-1))
    rng = np.random.default_rng([SEED, 9, seed])
    b.swhole, b.st = _guarded(torch, np.full(G, 0xAA, dtype=np.uint8))
    b.masks_in = rng.integers(0, 256, size=G * 32, dtype=np.uint8)
    b.mwhole, mo = _guarded(torch, b.masks_in)
    b.masks_out = mo.view(torch.int64)
    b.symlen_in = rng.integers(0, 256, size=G * 4, dtype=np.uint8)
    b.lwhole, lo = _guarded(torch, b.symlen_in)
    b.symlen_out = lo.view(torch.int32)
    return b


def launch(ctx, b, stream=None, st=True, masks=True, symlen=True, wide=True):
    c, s = b.c, stream.cuda_stream if stream is not None else None
    call = ctx.recover_scatter_wide_dev if wide else ctx.recover_scatter_dev
    call(b.addrs, b.lens, b.dests, c.G, c.k, c.r, c.P, b.st if st else None, b.masks_out if masks else None,
         b.symlen_out if symlen else None, stream=s)


def _guards_intact(whole):
    w = whole.cpu().numpy()
    return (w[:GUARD] == 0x5A).all() and (w[-GUARD:] == 0x5A).all()


def _first_wrong(b, got):
    c = b.c
    bad = np.flatnonzero(got != b.expect)
    if not len(bad):
        return "equal"
    return f"{len(bad)} bytes differ, the first at {int(bad[0])} of {len(got)}; dest_mode {b.dest_mode} var {b.var} k {c.k} r {c.r} P {c.P}"


def check(b, what="", st=True, masks=True, symlen=True):
    c = b.c
    what = (what, b.dest_mode, b.var, c.k, c.r, c.P)
    got_st = b.st.cpu().numpy()
    assert np.array_equal(got_st, c.status if st else np.full(c.G, 0xAA, dtype=np.uint8)), (what, "status")
    got_m = b.masks_out.cpu().numpy().view(np.uint8)
    assert np.array_equal(got_m, c.masks.view(np.uint8).reshape(-1) if masks else b.masks_in), (what, "masks")
    got_l = b.symlen_out.cpu().numpy().view(np.uint8)
    assert np.array_equal(got_l, c.symlen(b.var).view(np.uint8) if symlen else b.symlen_in), (what, "symbol lengths")
    assert _guards_intact(b.swhole) and _guards_intact(b.mwhole) and _guards_intact(b.lwhole), what
    # rebuilt rows are the original bytes [0, L_g); every guard, every unwanted destination and every
    # destination of an unrecoverable or untouched group as it was
    got = b.owhole.cpu().numpy()
    assert np.array_equal(got, b.expect), (what, _first_wrong(b, got))
    if b.dest_mode != "holes":
        assert np.array_equal(b.arena.cpu().numpy(), b.arena_in), (what, "the arena changed")
    assert (b.trap == 0x5A).all().item(), (what, "a destination entry the call must not read was stored to")
    assert np.array_equal(b.addrs.cpu().numpy().view(np.uint64).reshape(c.G, -1), b.addrs_np), what
    assert np.array_equal(b.dests.cpu().numpy().view(np.uint64).reshape(c.G, -1), b.dests_np), what
    if b.var:
        assert np.array_equal(b.lens.cpu().numpy().view(np.uint32).reshape(c.G, -1), c.lens), what


def run(torch, ctx, c, var, dest_mode, what=""):
    b = make_call(torch, c, var, dest_mode)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    launch(ctx, b, stream)
    torch.cuda.synchronize()
    check(b, what)
    return b


# ------------------------------------------------------------------------------------------
# 1. Shapes and sizes, lengths
# ------------------------------------------------------------------------------------------
SHAPE_CASES = [(k, r, P) for k, r, sizes in SHAPES for P in sizes]


@pytest.mark.parametrize("var", [False, True], ids=["fixed", "lens"])
@pytest.mark.parametrize("k,r,P", SHAPE_CASES)
def test_shapes_and_sizes(quicfec_mod, oracle_mod, torch_cuda, k, r, P, var):
    """Every shape and size without and with the length table: rebuilt bytes [0, L_g) equal the
    original data, every status byte, the four mask words, L_g, guards, holes, tables."""
    c = main_case(oracle_mod, k, r, P)
    mode = DEST_MODES[(SHAPE_CASES.index((k, r, P)) + var) % len(DEST_MODES)]
    with product_ctx(quicfec_mod) as ctx:
        run(torch_cuda, ctx, c, var, mode)


@pytest.mark.parametrize("var", [False, True], ids=["fixed", "lens"])
@pytest.mark.parametrize("mode", DEST_MODES)
@pytest.mark.parametrize("k,r,P", [(60, 5, 272), (100, 20, 1037)])
def test_destinations(quicfec_mod, oracle_mod, torch_cuda, k, r, P, mode, var):
    """The arena's holes (in place), packed back to back, the slot layout and odd alignments; one
    destination of 0 in groups with two or more rows: the others are stored, the status is 0."""
    c = main_case(oracle_mod, k, r, P)
    with product_ctx(quicfec_mod) as ctx:
        b = run(torch_cuda, ctx, c, var, mode)
    assert all(c.status[g] == 0 for g, _ in b.unwanted)


# ------------------------------------------------------------------------------------------
# 2. Equivalences
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", [False, True], ids=["fixed", "lens"])
@pytest.mark.parametrize("k,r,P", [(10, 3, 16), (10, 3, 1200), (20, 5, 16), (20, 5, 1200), (32, 32, 16), (32, 32, 1200)])
def test_one_word_shapes_equal_the_scatter_recover(quicfec_mod, oracle_mod, torch_cuda, k, r, P, var):
    """k + r <= 64: outputs, statuses, symbol lengths and word 0 of the masks byte for byte those of
    fec_recover_scatter_rs_dev on the same tables; words 1..3 zero."""
    torch = torch_cuda
    q = quicfec_mod
    c = main_case(oracle_mod, k, r, P)
    with product_ctx(q) as ctx:
        if (k, r) == (32, 32):
            ctx.decode_plan_mode(q.FEC_PLAN_DEVICE)
        wide, narrow = make_call(torch, c, var, "odd"), make_call(torch, c, var, "odd")
        narrow_masks = torch.full((c.G,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        launch(ctx, wide)
        ctx.recover_scatter_dev(narrow.addrs, narrow.lens, narrow.dests, c.G, k, r, P, narrow.st, narrow_masks, narrow.symlen_out)
        ctx.synchronize()
        torch.cuda.synchronize()
    check(wide)
    assert np.array_equal(wide.owhole.cpu().numpy(), narrow.owhole.cpu().numpy())
    assert np.array_equal(wide.swhole.cpu().numpy(), narrow.swhole.cpu().numpy())
    assert np.array_equal(wide.lwhole.cpu().numpy(), narrow.lwhole.cpu().numpy())
    words = wide.masks_out.cpu().numpy().view(np.uint64).reshape(c.G, 4)
    assert np.array_equal(words[:, 0], narrow_masks.cpu().numpy().view(np.uint64)) and not words[:, 1:].any()


@pytest.mark.parametrize("k,r,P", [(224, 32, 16), (60, 5, 272)])
def test_contiguous_tables_equal_the_wide_recover(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """Tables that point into the contiguous layout, slot destinations, no lengths: byte for byte the
    output and the statuses of fec_recover_wide_rs_dev, and its masks below k + r."""
    torch = torch_cuda
    c = contiguous_case(oracle_mod, k, r, P)
    G, n = c.G, k + r
    dd, dp = _dev(torch, c.d_in), _dev(torch, c.p_in)
    dm = _dev(torch, c.masks.view(np.int64).reshape(-1))
    outs = [torch.full((GUARD + G * r * P + GUARD,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(2)]
    sts = [torch.full((G,), 0xAA, dtype=torch.uint8, device="cuda") for _ in range(2)]
    lost = wm.to_bits(c.masks)[:, :n]
    at = np.concatenate([dd.data_ptr() + np.arange(G * k, dtype=np.uint64).reshape(G, k) * P,
                         dp.data_ptr() + np.arange(G * r, dtype=np.uint64).reshape(G, r) * P], axis=1)
    addrs = _dev(torch, np.where(lost, 0, at).astype(np.uint64).view(np.int64).reshape(-1))
    dests = np.zeros((G, k), dtype=np.uint64)
    for g in range(G):
        for m, j in enumerate(np.flatnonzero(lost[g, :k])):
            if m < r:                                                          # an unrecoverable group may lose more than r
                dests[g, j] = outs[0].data_ptr() + GUARD + (g * r + m) * P
    dests = _dev(torch, dests.view(np.int64).reshape(-1))
    masks_out = torch.full((G * 4,), -1, dtype=torch.int64, device="cuda")
    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        ctx.recover_scatter_wide_dev(addrs, None, dests, G, k, r, P, sts[0], masks_out)
        ctx.recover_wide_dev(dd, dp, dm, G, k, r, P, outs[1][GUARD:GUARD + G * r * P], sts[1])
        ctx.synchronize()
        torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), outs[1].cpu().numpy())
    assert np.array_equal(outs[1].cpu().numpy()[GUARD:-GUARD].reshape(G, r, P), c.slots)
    assert np.array_equal(sts[0].cpu().numpy(), sts[1].cpu().numpy()) and np.array_equal(sts[0].cpu().numpy(), c.status)
    below = wm.to_bits(c.masks)
    below[:, n:] = False
    assert np.array_equal(masks_out.cpu().numpy().view(np.uint64).reshape(G, 4), wm.from_bits(below))
    assert np.array_equal(dd.cpu().numpy(), c.d_in) and np.array_equal(dp.cpu().numpy(), c.p_in)


# ------------------------------------------------------------------------------------------
# 3. Nullable outputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", [False, True], ids=["fixed", "lens"])
def test_outputs_are_nullable(quicfec_mod, oracle_mod, torch_cuda, var):
    """d_status, d_masks_out and d_symbol_len_out NULL in turn, then all at once: the rebuilt bytes and
    the outputs that are given as ever, the ones not given untouched."""
    torch = torch_cuda
    c = main_case(oracle_mod, 60, 5, 272)
    given = [dict(st=False), dict(masks=False), dict(symlen=False), dict(st=False, masks=False, symlen=False)]
    with product_ctx(quicfec_mod) as ctx:
        calls = [make_call(torch, c, var, "packed", seed=i) for i in range(len(given))]
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        for b, kw in zip(calls, given):
            launch(ctx, b, stream, **kw)
        torch.cuda.synchronize()
    for b, kw in zip(calls, given):
        check(b, kw, **kw)


# ------------------------------------------------------------------------------------------
# 4. Chunks and the launch trace
# ------------------------------------------------------------------------------------------
def _stride(k, r):
    return 512 + min(k, r) * k * 32                                            # fec_forms.hpp wide_slot_stride


def expected_trace(G, per_chunk, passes, wave_groups, var):
    """One classify over [0, G); per plan chunk the build (id 28), then wide_passes(k, r) passes of
    recover_scatter_wide (id 31); each wave-per-group launch at most wave_groups groups.
    (form, first group, groups, aux, pol, first)."""
    out = [("classify_table_wide", 0, G, -1, -1, -1)]
    for c0 in range(0, G, per_chunk):
        cn = min(per_chunk, G - c0)
        pieces = [(g0, min(wave_groups, cn - g0)) for g0 in range(0, cn, wave_groups)]
        out += [("build_records_wide", c0 + g0, gn, g0, -1, -1) for g0, gn in pieces]
        for p in range(passes):
            out += [("recover_scatter_wide", c0 + g0, gn, 8 * p, POL, int(var)) for g0, gn in pieces]
    return out


@pytest.mark.parametrize("k,r,P", [(224, 32, 16), (60, 5, 272)])
def test_chunked_walk(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P):
    """The test library at its defaults, with 12 groups per wave-per-group launch, and with the arena
    lowered to three strides and to one: the same bytes, and the launches DESIGN §5b names."""
    torch = torch_cuda
    q = quicfec_mod
    lib = q.load_test_library()
    assert q.WIDE_LAUNCH_FORMS[28] == "build_records_wide" and q.WIDE_TABLE_LAUNCH_FORMS[31] == "recover_scatter_wide"
    c = main_case(oracle_mod, k, r, P)
    G, passes = c.G, -(-min(k, r) // 8)
    settings = [({}, G, 1 << 40), ({"QUICFEC_MAX_WAVE_BLOCKS": "3"}, G, 12),
                ({"QUICFEC_MAX_WAVE_BLOCKS": "3", "QUICFEC_PLAN_ARENA_BYTES": str(3 * _stride(k, r))}, 3, 12),
                ({"QUICFEC_MAX_WAVE_BLOCKS": "3", "QUICFEC_PLAN_ARENA_BYTES": str(_stride(k, r))}, 1, 12)]
    with hooks_ctx(q) as ctx:
        for i, (env, per_chunk, wave_groups) in enumerate(settings):
            for name in ("QUICFEC_MAX_WAVE_BLOCKS", "QUICFEC_PLAN_ARENA_BYTES"):
                monkeypatch.delenv(name, raising=False)
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            var = i % 2 == 1
            calls = [make_call(torch, c, var, "odd"), make_call(torch, c, not var, "holes")]
            torch.cuda.synchronize()
            q.launch_trace(lib)
            for b in calls:
                launch(ctx, b, torch.cuda.current_stream())
            ctx.synchronize()
            torch.cuda.synchronize()
            trace = [(t["form"], t["first_item"], t["items"], t["aux"], t["pol"], t["first"]) for t in q.launch_trace(lib)]
            for b in calls:
                check(b, env)
            want = expected_trace(G, per_chunk, passes, wave_groups, var) + expected_trace(G, per_chunk, passes, wave_groups, not var)
            assert trace == want, env
            builds = [(t[1], t[2]) for t in trace[:len(trace) // 2] if t[0] == "build_records_wide"]
            assert builds[0][0] == 0 and sum(n for _, n in builds) == G
            assert all(a[0] + a[1] == b[0] for a, b in zip(builds, builds[1:]))


# ------------------------------------------------------------------------------------------
# 5. State across calls
# ------------------------------------------------------------------------------------------
def test_three_shapes_queued_on_one_stream(quicfec_mod, oracle_mod, torch_cuda):
    """Three calls of different shapes back to back on one side stream, no host synchronise between
    them, each needing a larger workspace than the one before; then a small one again."""
    torch = torch_cuda
    cases = [main_case(oracle_mod, 60, 5, 16), main_case(oracle_mod, 100, 20, 1037), main_case(oracle_mod, 224, 32, 16)]
    assert _stride(60, 5) < _stride(100, 20) < _stride(224, 32)
    stream = torch.cuda.Stream()
    with product_ctx(quicfec_mod) as ctx:
        calls = [make_call(torch, c, var, mode) for c, var, mode in zip(cases, (True, False, True), ("packed", "holes", "slots"))]
        calls.append(make_call(torch, cases[0], False, "odd"))
        torch.cuda.synchronize()
        for b in calls:
            launch(ctx, b, stream, masks=b.var, symlen=not b.var)               # the workspace holds what the caller does not
        torch.cuda.synchronize()
    for i, b in enumerate(calls):
        check(b, i, masks=b.var, symlen=not b.var)


def test_two_threads_on_two_streams(quicfec_mod, oracle_mod, torch_cuda):
    """Two host threads, each with its own side stream and a different shape, six calls each on one
    context from a barrier: each stream's masks, lengths and records are its own workspace's."""
    torch = torch_cuda
    cases = [main_case(oracle_mod, 60, 5, 272), main_case(oracle_mod, 100, 20, 1037)]
    work = [[make_call(torch, cases[t], j % 2 == 0, DEST_MODES[j % 4], seed=j) for j in range(6)] for t in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2)
    errors = []

    def go(t, ctx):
        try:
            barrier.wait(timeout=60)
            for b in work[t]:
                launch(ctx, b, streams[t], st=True, masks=False, symlen=False)
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
            check(b, (t, j), masks=False, symlen=False)


def test_free_with_calls_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """Two calls queued on a side stream and the context freed at once: fec_encoder_free drains them
    (they read the context's parity matrix and the stream's workspace), so both outputs are complete."""
    torch = torch_cuda
    c = main_case(oracle_mod, 100, 20, 4096)
    calls = [make_call(torch, c, True, "slots"), make_call(torch, c, False, "holes")]
    stream = torch.cuda.Stream()
    ctx = product_ctx(quicfec_mod)
    torch.cuda.synchronize()
    for b in calls:
        launch(ctx, b, stream, masks=False, symlen=False)
    ctx.close()
    assert stream.query()                                                      # the free drained the stream
    torch.cuda.synchronize()
    for b in calls:
        check(b, masks=False, symlen=False)


# ------------------------------------------------------------------------------------------
# 6. Refusals
# ------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(quicfec_mod, oracle_mod, torch_cuda):
    """k = 0, r = 0, k + r = 257, 33+33, P = 15, G = 0, G = 2^32 and each required NULL pointer: the
    code, a message naming the case, nothing launched, every buffer untouched."""
    torch = torch_cuda
    q = quicfec_mod
    lib = q.load_test_library()
    c = main_case(oracle_mod, 60, 5, 16)
    G = c.G
    with hooks_ctx(q) as ctx:
        b = make_call(torch, c, True, "packed")
        before = b.owhole.cpu().numpy().copy()
        torch.cuda.synchronize()
        q.launch_trace(lib)
        p = lambda t: t.data_ptr()
        outs = [p(b.st), p(b.masks_out), p(b.symlen_out), None]
        for (k, r, P, groups), text in (((0, 5, 16, G), "k>0"), ((60, 0, 16, G), "r>0"), ((200, 57, 16, G), "k+r<=256"),
                                        ((33, 33, 16, G), "min(k, r)"), ((60, 5, 15, G), "below 16"),
                                        ((60, 5, 16, 0), "num_groups is 0"), ((60, 5, 16, 2**32), "32-bit group indices")):
            rc = lib.fec_recover_scatter_wide_rs_dev(ctx.handle, p(b.addrs), p(b.lens), p(b.dests), groups, k, r, P, *outs)
            assert rc == q.FEC_ERR_RANGE and text in q.last_error(lib), (k, r, P, groups, q.last_error(lib))
            assert "fec_recover_scatter_wide_rs_dev" in q.last_error(lib)
        args = [ctx.handle, p(b.addrs), p(b.lens), p(b.dests)]
        for i, name in ((0, "context"), (1, "d_shard_addrs"), (3, "d_dest_addrs")):
            bad = list(args)
            bad[i] = None
            assert lib.fec_recover_scatter_wide_rs_dev(*bad, G, 60, 5, 16, *outs) == q.FEC_ERR_NULL
            assert name in q.last_error(lib)
        ctx.synchronize()
        torch.cuda.synchronize()
        assert q.launch_trace(lib) == []
        assert np.array_equal(b.owhole.cpu().numpy(), before) and (b.swhole.cpu().numpy()[GUARD:-GUARD] == 0xAA).all()
        assert np.array_equal(b.masks_out.cpu().numpy().view(np.uint8), b.masks_in)
        assert np.array_equal(b.symlen_out.cpu().numpy().view(np.uint8), b.symlen_in)
        assert np.array_equal(b.arena.cpu().numpy(), b.arena_in) and (b.trap == 0x5A).all().item()
        launch(ctx, b)                                                         # and the same buffers are served
        ctx.synchronize()
    check(b)
