"""The five address-table calls (fec_recover_gather_rs_dev, fec_encode_gather_rs_dev,
fec_recover_gather_var_rs_dev, fec_encode_gather_var_rs_dev, fec_recover_scatter_rs_dev) at the
limits the contiguous calls meet in test_gpu_limits.py and test_gpu_forms.py:

  1. the largest and the smallest shapes (k + r = 64: bit 63 of the derived mask, 63 entries of the
     runtime-k LDS slices, the survivor bytes of a record right before its erased-id bytes; k = 1;
     r = 1; eight row passes);
  2. jumbo packets (4096, 9000 and 65535 B) with the shortest survivor and the symbol length inside,
     at the start of and at the end of a late 1-KiB pass and of the tail passes;
  3. more than one classify workgroup (G = 589 = 2 * 256 + 77), also with the launches chunked;
  4. every record of the dense codebook once, and every erasure mask.

The cases, arenas, guards and checks are those of test_gpu_gather.py, test_gpu_gather_var.py and
test_gpu_scatter.py, taken by import: 0xEE in the arenas and the holes, 0x5A and guard bytes in the
outputs, 7 in the statuses, JUNK_LEN in the length entries of lost shards; every comparison is
bit-exact against the oracle on the contiguous equivalent, and the arenas are byte-identical after
each call.  Every address in a table is readable for its stated length and every destination
writable for the group's symbol length; "never read" is checked through unchanged arenas and guards.

What each case holds is asserted on the CPU before anything is launched, and again by the tests
of this file that carry no gpu mark.
"""
import os
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_gather as fx
import test_gpu_gather_var as var
import test_gpu_scatter as sc
from test_gpu_forms import record_masks
from test_gpu_gather import GUARD, guarded, hooks_ctx, perm_masks, product_ctx
from test_gpu_gather_var import JUNK_LEN, dealt_lengths, edge_lengths

gpu = pytest.mark.gpu

SEED = 0xADD20000
G_MAIN = 67                                           # more than one wave-block, no multiple of 4, an odd tail


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


def _bits(shards):
    return sum(1 << int(s) for s in shards)


def _u64(values):
    return np.array([int(v) for v in values], dtype=np.uint64)


# ------------------------------------------------------------------------------------------
# 0. The arena without a Python loop per shard
# ------------------------------------------------------------------------------------------
PAD_MAX = 37


def fast_arena(c, seed, encode=False, at_length=False):
    """build_arena of test_gpu_gather.py (at_length=False: every present shard has its P bytes, case
    of fx.make_case) and of test_gpu_gather_var.py (at_length=True: every present shard sits at
    exactly its table length, case of var.make_case) in numpy alone.  The same layout properties:
    two allocations filled with 0xEE, a seeded random placement order, a pad of 1..37 bytes before
    each shard, P + 38 bytes of 0xEE at the end of each arena, lost / absent shards placed nowhere
    ((-1, 0) in `where`, entry 0 in the table).  Every arena is one boolean-masked copy out of a
    matrix of [37 pad bytes | shard] rows in placement order; the offsets are cumulative sums.
    Returns (arenas, where) as the builders it stands in for (the length table is the caller's)."""
    k, r, P, G = c.k, c.r, c.P, c.G
    n = k if encode else k + r
    rng = np.random.default_rng(seed)
    here = (c.present if hasattr(c, "present") else np.ones((G, k), dtype=bool)) if encode else ~c.lost
    gi, si = np.nonzero(here[:, :n])
    order = rng.permutation(len(gi))                                         # placement i puts shard order[i]
    pads = rng.integers(1, PAD_MAX + 1, size=len(gi))
    side = rng.integers(0, 2, size=len(gi))
    size = c.lens[gi, si].astype(np.int64) if at_length else np.full(len(gi), P, dtype=np.int64)
    width = int(size.max()) if len(gi) else 0
    if at_length:
        data, par = c.raw, c.praw
    else:
        data, par = c.data.reshape(G, k, P), c.par_in.reshape(G, r, P)       # junk in the rows the rule does not read
    cols = np.arange(PAD_MAX + width)
    where = np.full((G, n, 2), -1, dtype=np.int64)
    where[:, :, 1] = 0
    arenas = []
    for a in (0, 1):
        mine = side == a
        g, s, pad, sz = gi[order[mine]], si[order[mine]], pads[mine], size[order[mine]]
        rows = np.full((len(g), PAD_MAX + width), 0xEE, dtype=np.uint8)
        d = s < k
        rows[d, PAD_MAX:] = data[g[d], s[d], :width]
        rows[~d, PAD_MAX:] = par[g[~d], s[~d] - k, :width]
        keep = (cols[None, :] >= PAD_MAX - pad[:, None]) & (cols[None, :] < PAD_MAX + sz[:, None])
        where[g, s, 0] = a
        where[g, s, 1] = np.cumsum(pad + sz) - sz                            # the pads and shards before it, and its pad
        arenas.append(np.concatenate([rows[keep], np.full(P + PAD_MAX + 1, 0xEE, dtype=np.uint8)]))
    return arenas, where


def lens_table(c, encode=False):
    """The length table of a var case: JUNK_LEN where the entry is lost / absent."""
    n = c.k if encode else c.k + c.r
    return np.where(c.present if encode else ~c.lost, c.lens[:, :n], JUNK_LEN).astype(np.uint32)


def check_fast_arena(c, at_length):
    """What test_arena_addresses_take_every_residue and
    test_arena_puts_shards_at_their_length_at_every_residue assert of the old builders, and that
    nothing overlaps and nothing else is written."""
    k, r, P, G = c.k, c.r, c.P, c.G
    arenas, where = fast_arena(c, 1, at_length=at_length)
    assert ((where[:, :, 0] < 0) == c.lost).all() and (where[c.lost][:, 1] == 0).all()
    for a in (0, 1):
        for part in (where[:, :k], where[:, k:]):                            # data and parity, in both arenas
            assert set((part[..., 1][part[..., 0] == a] % 16).tolist()) == set(range(16))
    used = [np.zeros(len(a), dtype=np.int32) for a in arenas]
    for g, s in zip(*np.nonzero(~c.lost)):
        a, off = where[g, s]
        if at_length:
            ln = int(c.lens[g, s])
            want = c.raw[g, s, :ln] if s < k else c.praw[g, s - k, :ln]
        else:
            ln = P
            want = c.data.reshape(G, k, P)[g, s] if s < k else c.par_in.reshape(G, r, P)[g, s - k]
        assert np.array_equal(arenas[a][off:off + ln], want), (g, s)
        assert (arenas[a][off - 1] == 0xEE) and arenas[a][off + ln] == 0xEE  # a pad before it, 0xEE right after it
        used[a][off:off + ln] += 1
    size = np.where(c.lost, 0, c.lens if at_length else P)
    for a in (0, 1):
        assert used[a].max() == 1                                            # no two shards overlap
        assert (arenas[a][used[a] == 0] == 0xEE).all()                       # every byte outside a shard
        assert (arenas[a][-(P + PAD_MAX + 1):] == 0xEE).all() and used[a][-(P + PAD_MAX + 1):].max() == 0
        mine = where[:, :, 0] == a
        off, ln = where[:, :, 1][mine], size[mine]
        order = np.argsort(off, kind="stable")
        pads = off[order] - np.concatenate([[0], (off + ln)[order][:-1]])     # 1..37 bytes before every shard
        assert pads.min() >= 1 and pads.max() <= PAD_MAX and set(pads.tolist()) == set(range(1, PAD_MAX + 1))
        assert (off + ln).max() + P + PAD_MAX + 1 == len(arenas[a])


def test_fast_arena_keeps_the_layout_properties(oracle_mod):
    """On the CPU, a k=10 r=3 1200 B G = 67 case in both modes: addresses at every residue mod 16 in
    both arenas for data and for parity, no two shards overlap, every shard's bytes in place, every
    byte outside a shard 0xEE."""
    check_fast_arena(fx.main_case(oracle_mod, 10, 3, 1200), at_length=False)
    c = var.main_case(oracle_mod, 10, 3, 1200)
    check_fast_arena(c, at_length=True)
    assert (lens_table(c)[c.lost] == JUNK_LEN).all() and np.array_equal(lens_table(c)[~c.lost], c.lens[~c.lost])


# The calls on a fast arena: the make_* of the three files with fast_arena for build_arena and a
# vectorised destination image; launched and checked by the three files' own functions.
def make_fixed(torch, c, seed):
    arenas, where = fast_arena(c, seed)
    b = SimpleNamespace(c=c, arenas=arenas)
    b.dev, b.table = fx.upload_arena(torch, arenas, where)
    b.whole, b.out = guarded(torch, c.G * c.r * c.P, 0x5A)
    b.st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
    b.mo = torch.full((c.G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    return b


def make_var(torch, c, seed):
    arenas, where = fast_arena(c, seed, at_length=True)
    b = SimpleNamespace(c=c, arenas=arenas)
    b.dev, b.table, b.lens = var.upload_arena(torch, arenas, where, lens_table(c))
    b.whole, b.out = guarded(torch, c.G * c.r * c.P, 0x5A)
    b.st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
    b.mo = torch.full((c.G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    b.sym = torch.full((c.G,), 0x77777777, dtype=torch.int32, device="cuda")
    return b


def make_packed_scatter(torch, c, seed, want_sym=True):
    """sc.make_scatter with a length table and sc.packed_layout: every destination right behind the
    one before it, in (g, m) order, so one misplaced or mis-cut row shifts everything after it."""
    arenas, where = fast_arena(c, seed, at_length=True)
    b = SimpleNamespace(c=c, with_lens=True)
    dev, b.table, b.lens = var.upload_arena(torch, arenas, where, lens_table(c))
    gi, ji, mi = sc.rebuilt_rows(c)
    b.sym = sc.symbol_lengths(c, True)
    L = b.sym[gi]
    nbytes, offs = sc.packed_layout(c, gi, ji, mi, L)
    guard = np.full(GUARD, 0x5A, dtype=np.uint8)
    image = np.concatenate([guard, c.data[gi, ji][np.arange(c.P)[None, :] < L[:, None]], guard])
    assert len(image) == nbytes
    b.dest = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")
    b.canary = torch.full((GUARD + c.P + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    tab = np.full((c.G, c.k), b.canary.data_ptr() + GUARD, dtype=np.uint64)  # ignored entries: a valid address
    tab[gi, ji] = np.uint64(b.dest.data_ptr()) + offs.astype(np.uint64)
    b.offs, b.rows = offs, (gi, ji, mi)
    b.dtab = torch.from_numpy(tab.reshape(-1).view(np.int64)).to("cuda")
    b.images = list(zip(dev, arenas)) + [(b.dest, image), (b.canary, np.full(GUARD + c.P + GUARD, 0xC3, dtype=np.uint8))]
    b.st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
    b.mo = torch.full((c.G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    b.so = torch.full((c.G,), 0x77777777, dtype=torch.int32, device="cuda") if want_sym else None
    return b


def run_fixed_encode(torch, ctx, c, seed, what=""):
    """fec_encode_gather_rs_dev on the packets of c (all present), as test_gpu_gather.test_encode_gather:
    parity equals rs_encode, the guards hold, the arenas are unchanged."""
    arenas, where = fx.build_arena(c, seed, encode=True)
    dev, table = fx.upload_arena(torch, arenas, where)
    whole, par = guarded(torch, c.G * c.r * c.P, 0x5A)
    ctx.encode_gather_dev(table, c.G, c.k, c.r, c.P, par)
    ctx.synchronize()
    got = whole.cpu().numpy()
    what = (what, c.k, c.r, c.P, c.G)
    assert np.array_equal(got[GUARD:-GUARD], c.par), what
    assert (got[:GUARD] == 0x5A).all() and (got[-GUARD:] == 0x5A).all(), what
    for d, a in zip(dev, arenas):
        assert np.array_equal(d.cpu().numpy(), a), what


def run_var_encode(torch, ctx, c, seed, what=""):
    e = var.run_encode(torch, ctx, c, seed)
    ctx.synchronize()
    var.check_encode(e, what)


# ------------------------------------------------------------------------------------------
# 1. Limit shapes
# ------------------------------------------------------------------------------------------
LIMIT_RECOVER = [(63, 1), (1, 63), (62, 2), (2, 62), (3, 61), (1, 1)]
LIMIT_ENCODE = [(63, 1), (1, 63), (32, 32), (48, 16), (1, 1)]
LIMIT_RECOVER_SIZES = (16, 272, 1200)
LIMIT_ENCODE_SIZES = (16, 260, 1200)
G_ENCODE = 37


def rule_rows(c):
    """(G, r) bool: the parity rows the decode rule rebuilds group g from -- the e lowest alive ones
    of a recoverable group that lost e > 0 data shards."""
    e = c.lost[:, :c.k].sum(axis=1)
    alive = ~c.lost[:, c.k:]
    return alive & (np.cumsum(alive, axis=1) <= e[:, None]) & ((c.status == 0) & (e > 0))[:, None]


def limit_masks(k, r, seed):
    """perm_masks with its five planted groups, and in groups 5..9 what the permutations do not
    promise.  5: data shard 0 lost with every parity row but the top one, so the rule's one row is
    shard k + r - 1.  6: data shard k - 1 lost and (r >= 2) the top parity row, bit k + r - 1 of the
    mask.  7: e = min(k, r, 3) data shards lost, shards 0 and k - 1 among them, and every parity row
    but the top e.  8: shards 0 and k - 1 lost with every parity row alive (rows 0 and 1).  9: the
    top parity row alone."""
    masks = perm_masks(k, r, G_MAIN, seed)
    ends = list(dict.fromkeys([0, k - 1, k // 2]))[:min(k, r, 3)]
    ends2 = ends[:2] if min(k, r) >= 2 else ends[:1]
    masks[5:10] = _u64([_bits([0]) | _bits(range(k, k + r - 1)),
                        _bits([k - 1]) | (_bits([k + r - 1]) if r >= 2 else 0),
                        _bits(ends) | _bits(range(k, k + r - len(ends))),
                        _bits(ends2),
                        _bits([k + r - 1])])
    return masks


def check_limit_case(c):
    """What a limit case must hold, on the CPU."""
    k, r = c.k, c.r
    lost_d, ok = c.lost[:, :k], c.status == 0
    e = lost_d.sum(axis=1)
    assert (c.masks == 0).any() and (c.status == 1).any() and c.rows > 0
    assert ((c.masks >> np.uint64(k + r - 1)) & np.uint64(1)).any()          # the top bit of the derived mask
    assert rule_rows(c)[:, r - 1].any()                                      # shard k + r - 1 is a survivor of a rebuild
    assert (lost_d[:, k - 1] & ok).any() and (lost_d[:, 0] & ok).any()       # shards k - 1 and 0 are rebuilt
    assert ((e == min(k, r, 2)) & ok).any() and ((e == min(k, r, 3)) & ok).any()
    if k + r == 64:
        assert c.lost[:, 63].any() and rule_rows(c)[:, 63 - k].any()
    if (k, r) in ((62, 2), (2, 62)):
        assert ((e == 2) & ok & rule_rows(c)[:, r - 1]).any()                # two rows, shard 63 one of their sources


@lru_cache(maxsize=None)
def limit_cases(oracle, k, r, P):
    """The G = 67 cases of a limit shape and size on one set of masks: fixed-length shards, lengths
    dealt from edge_lengths(P) over data and parity, and every length P (the NULL length table)."""
    salt = k * 100000 + r * 10000 + P
    masks = limit_masks(k, r, salt)
    full = np.full((G_MAIN, k + r), P)
    cs = SimpleNamespace(
        fixed=fx.make_case(oracle, k, r, P, masks, SEED + salt),
        lens=var.make_case(oracle, k, r, P, masks, dealt_lengths(P, G_MAIN, k), dealt_lengths(P, G_MAIN, r, shift=k),
                           SEED + salt + 1),
        full=var.make_case(oracle, k, r, P, masks, full[:, :k], full[:, k:], SEED + salt + 2))
    for c in (cs.fixed, cs.lens, cs.full):
        check_limit_case(c)
    assert set(edge_lengths(P).tolist()) <= set(cs.lens.lens[:, :k].reshape(-1).tolist())
    return cs


@lru_cache(maxsize=None)
def limit_encode_cases(oracle, k, r, P):
    """G = 37: every packet present at P bytes (the fixed call), and test_gpu_gather_var.encode_case's
    dealing for the var call -- one packet present, k - 1 present, none present, then 85% present
    under edge lengths -- with row 0 checked against the reference encoder on the true packets."""
    G = G_ENCODE
    fixed = fx.make_case(oracle, k, r, P, [0] * G, SEED + 5 * P + k)
    dl = dealt_lengths(P, G, k)
    present = np.ones((G, k), dtype=bool)
    present[1] = False
    present[1, k // 2] = True
    present[2, 0] = False
    present[3] = False
    present[4:] = np.random.default_rng(SEED + k + P).random((G - 4, k)) < 0.85
    dl[5] = P
    dl[6] = 0
    c = var.make_case(oracle, k, r, P, [0] * G, dl, np.zeros((G, r), dtype=np.int64), SEED + 7 * P + k, present=present)
    assert not present[3].any() and c.sym_enc[3] == 0 and not c.par[3].any() and c.sym_enc[6] == 0
    assert (~c.present).any() and c.present[4:].any()
    for g in range(G):
        pk = [np.ascontiguousarray(c.raw[g, j, :min(int(c.lens[g, j]), P)]) for j in range(k) if present[g, j]]
        if c.sym_enc[g] == 0:                                                # the reference emits no repair packet
            assert not c.par[g].any()
        else:
            pay = oracle.go_generate_redundancy(pk, group_id=g)[11:]
            assert len(pay) == c.sym_enc[g]
            assert np.array_equal(c.par[g, 0, :len(pay)], pay) and not c.par[g, 0, len(pay):].any()
    return SimpleNamespace(fixed=fixed, var=c)


@pytest.mark.parametrize("k,r", LIMIT_RECOVER)
def test_limit_cases_hold_what_they_are_for(oracle_mod, k, r):
    """On the CPU, every limit shape at its smallest size: bit k + r - 1 set in a mask, shard
    k + r - 1 a survivor of a rebuild, shards 0 and k - 1 rebuilt, e = 2 where the shape allows it
    (asserted inside limit_cases, which the GPU test builds its cases with)."""
    cs = limit_cases(oracle_mod, k, r, 16)
    assert cs.fixed.G == G_MAIN and np.array_equal(cs.fixed.masks, cs.lens.masks)
    assert (cs.full.lens == 16).all()


@gpu
@pytest.mark.parametrize("k,r", LIMIT_RECOVER)
def test_limit_shapes_recover(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """The dense-codebook shapes with k + r = 64, k = 1 and r = 1 at 16, 272 and 1200 B, G = 67:
    the fixed gather recover, the var gather recover, the scatter recover with a length table on
    padded destinations and the scatter recover without one on the slot layout."""
    torch = torch_cuda
    with product_ctx(quicfec_mod) as ctx:
        assert ctx.decode_prepare(k, r) > 0                                  # dense: a sparse-plan shape would be refused
        for P in LIMIT_RECOVER_SIZES:
            cs = limit_cases(oracle_mod, k, r, P)
            fx.run_recover(torch, ctx, cs.fixed, SEED + P, "fixed gather")
            var.run_recover(torch, ctx, cs.lens, SEED + P + 1, "var gather")
            sc.run_scatter(torch, ctx, cs.lens, SEED + P + 2, sc.padded_layout(SEED + P + 3), "scatter, lengths")
            sc.run_scatter(torch, ctx, cs.full, SEED + P + 4, sc.slot_layout, "scatter, NULL lengths", with_lens=False)


@gpu
@pytest.mark.parametrize("k,r", LIMIT_ENCODE)
def test_limit_shapes_encode(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """k + r = 64 (two of them sparse-plan shapes, legal for an encode), k = 1 and r = 1 at 16, 260
    and 1200 B, G = 37: both gather encodes.  k=1 r=63 runs eight row passes, the last of 7 rows."""
    with product_ctx(quicfec_mod) as ctx:
        for P in LIMIT_ENCODE_SIZES:
            cs = limit_encode_cases(oracle_mod, k, r, P)
            run_fixed_encode(torch_cuda, ctx, cs.fixed, SEED + P, "fixed encode")
            run_var_encode(torch_cuda, ctx, cs.var, SEED + P + 1, "var encode")


# ------------------------------------------------------------------------------------------
# 2. Jumbo packets
# ------------------------------------------------------------------------------------------
JUMBO = [(k, r, P) for (k, r) in ((10, 3), (6, 3)) for P in (4096, 9000, 65535)]
G_JUMBO = 9


def jumbo_targets(P):
    """Where the shortest survivor and the symbol length are put: around 2 KiB and 4 KiB, and around
    the start of the tail passes (the end of the last 1-KiB pass)."""
    main_end = P & ~1023
    return [2047, 2048, 2049, 4095, 4096, 4097, main_end - 1, main_end, main_end + 1]


def jumbo_pool(P):
    return np.array(list(dict.fromkeys(edge_lengths(P).tolist() + jumbo_targets(P))), dtype=np.int64)


@lru_cache(maxsize=None)
def jumbo_cases(oracle, k, r, P):
    """Three G = 9 cases, i = 0, 1, 2, each with three of the nine targets t.  Lengths are dealt from
    jumbo_pool(P).  Group 0: every present length below 4 (the byte-wise pass), one data shard lost.
    Group 1: every present length 0 (nothing dereferenced), a data shard and parity row 0 lost.
    Group 2: unrecoverable, untouched or parity-only loss by i.  Groups 3..5: every length raised to
    t and the first surviving data shard exactly t, so the shortest survivor is t.  Groups 6..8:
    every length cut at t and the first surviving data shard exactly t, so the symbol length is
    min(t, P).  Groups 3..8 lose one, two or three data shards, some with a parity row."""
    n, G = k + r, G_JUMBO
    pool, targets = jumbo_pool(P), jumbo_targets(P)
    rebuilds = [_bits([0]), _bits([1, k]), _bits([2, 3]), _bits([k - 1]), _bits([0, 1, 2]), _bits([4, k + 1])]
    out = []
    for i in range(3):
        masks = _u64([_bits([1]), _bits([0, k]), [_bits([0]) | _bits(range(k, n)), 0, _bits([k])][i]] + rebuilds)
        lens = pool[(np.arange(G)[:, None] * 7 + np.arange(n)[None, :] + 11 * i) % len(pool)]
        lens[0] = (np.arange(n) + i) % 4
        lens[1] = 0
        first = [[j for j in range(k) if not (int(m) >> j) & 1][0] for m in masks]
        for g in range(3, 9):
            t = targets[3 * i + (g - 3) % 3]
            lens[g] = np.maximum(lens[g], t) if g < 6 else np.minimum(lens[g], t)
            lens[g, first[g]] = t
        salt = k * 1000000 + P * 10 + i
        c = var.make_case(oracle, k, r, P, masks, lens[:, :k], lens[:, k:], SEED + salt)
        here = ~c.lost
        assert (c.lens[0][here[0]] < 4).all() and c.status[0] == 0 and c.lost[0, 1] and 0 < c.sym_rec[0] < 4
        assert (c.lens[1][here[1]] == 0).all() and c.status[1] == 0 and c.lost[1, 0] and c.sym_rec[1] == 0
        assert (c.status[3:] == 0).all() and c.lost[3:, :k].any(axis=1).all()
        for g in range(3, 9):
            t = targets[3 * i + (g - 3) % 3]
            if g < 6:
                assert c.lens[g][here[g]].min() == t and c.sym_rec[g] >= min(t, P)
            else:
                assert c.sym_rec[g] == min(t, P) and c.lens[g][here[g]].max() == t
        # under a floor some survivor is longer than the shortest, under a cut some is shorter than the symbol
        assert any(c.lens[g][here[g]].max() > c.lens[g][here[g]].min() for g in range(3, 6))
        assert any(c.lens[g][here[g]].min() < c.sym_rec[g] for g in range(6, 9))
        full = np.full((G, n), P)
        present = np.ones((G, k), dtype=bool)
        present[2, 0] = False
        present[5] = False
        present[5, k - 1] = True
        out.append(SimpleNamespace(
            lens=c, fixed=fx.make_case(oracle, k, r, P, masks, SEED + salt + 1),
            full=var.make_case(oracle, k, r, P, masks, full[:, :k], full[:, k:], SEED + salt + 2),
            enc_fixed=fx.make_case(oracle, k, r, P, [0] * G, SEED + salt + 3),
            enc=var.make_case(oracle, k, r, P, [0] * G, lens[:, :k], np.zeros((G, r), dtype=np.int64), SEED + salt + 4,
                              present=present)))
    return out


def test_jumbo_cases_hold_the_short_and_the_empty_group(oracle_mod):
    """On the CPU: the group with every present length below 4 and the one with every present length
    0 are in each jumbo case, and the targets sit where they are meant to (asserted inside
    jumbo_cases); the nine targets are spread over the three cases."""
    k, r, P = 6, 3, 4096
    cases = jumbo_cases(oracle_mod, k, r, P)
    assert len(cases) == 3 and all(cs.lens.G == G_JUMBO for cs in cases)
    floors = [int(cs.lens.lens[g][~cs.lens.lost[g]].min()) for cs in cases for g in (3, 4, 5)]
    assert floors == jumbo_targets(P)
    for Q in (4096, 9000, 65535):
        assert set(jumbo_targets(Q)) <= set(jumbo_pool(Q).tolist()) and jumbo_targets(Q)[7] % 1024 == 0


@gpu
@pytest.mark.parametrize("k,r,P", JUMBO)
def test_jumbo_packets(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """A compiled and a runtime-k shape at 4096, 9000 and 65535 B, G = 9, all five calls (the scatter
    recover with a length table on padded destinations, so the byte after each cut is a guard, and
    without one on the slot layout)."""
    torch = torch_cuda
    with product_ctx(quicfec_mod) as ctx:
        for i, cs in enumerate(jumbo_cases(oracle_mod, k, r, P)):
            fx.run_recover(torch, ctx, cs.fixed, SEED + i, ("fixed gather", i))
            var.run_recover(torch, ctx, cs.lens, SEED + 10 + i, ("var gather", i))
            sc.run_scatter(torch, ctx, cs.lens, SEED + 20 + i, sc.padded_layout(SEED + 30 + i), ("scatter, lengths", i))
            sc.run_scatter(torch, ctx, cs.full, SEED + 40 + i, sc.slot_layout, ("scatter, NULL lengths", i), with_lens=False)
            run_fixed_encode(torch, ctx, cs.enc_fixed, SEED + 50 + i, ("fixed encode", i))
            run_var_encode(torch, ctx, cs.enc, SEED + 60 + i, ("var encode", i))


# ------------------------------------------------------------------------------------------
# 3. More than one classify workgroup
# ------------------------------------------------------------------------------------------
G_MULTI = 589                                         # 2 * 256 + 77: three classify workgroups, no multiple of 4
MULTI = [(10, 3, 48), (10, 3, 1200), (62, 2, 48), (12, 9, 48)]              # compiled k; 256 * 64 entries; two passes
MULTI_ENCODE = {(10, 3), (12, 9)}
PLANTED_AT = (255, 256, 511, 512, 588)                # the last and the first group of a workgroup, and the last group
PLANTED_LEN = (5, 41, 17, 33, 29)                     # every present length of the planted group: its symbol length


def multi_planted_masks(k, r):
    return [_bits([0]), _bits([1]) | (_bits([k]) if r >= 2 else 0), _bits([k - 1]), _bits([0]) | _bits(range(k, k + r)),
            _bits([2, k + r - 1])]


@lru_cache(maxsize=None)
def multi_cases(oracle, k, r, P):
    """G = 589: permutation masks, independent random lengths in 0..P + 8 for every data and parity
    entry, and in groups 255, 256, 511, 512 and 588 masks and lengths found nowhere next to them."""
    G = G_MULTI
    salt = k * 100000 + r * 10000 + P
    rng = np.random.default_rng(SEED + salt)
    masks = perm_masks(k, r, G, SEED + salt)
    masks[list(PLANTED_AT)] = _u64(multi_planted_masks(k, r))
    dl, pl = rng.integers(0, P + 9, size=(G, k)), rng.integers(0, P + 9, size=(G, r))
    for g, ln in zip(PLANTED_AT, PLANTED_LEN):
        dl[g], pl[g] = ln, ln
    cs = SimpleNamespace(fixed=fx.make_case(oracle, k, r, P, masks, SEED + salt + 1),
                         lens=var.make_case(oracle, k, r, P, masks, dl, pl, SEED + salt + 2))
    if (k, r) in MULTI_ENCODE:
        cs.enc_fixed = fx.make_case(oracle, k, r, P, [0] * G, SEED + salt + 3)
        cs.enc = var.make_case(oracle, k, r, P, [0] * G, dl, np.zeros((G, r), dtype=np.int64), SEED + salt + 4,
                               present=rng.random((G, k)) < 0.85)
    check_multi_case(cs.lens)
    assert np.array_equal(cs.fixed.masks, cs.lens.masks) and np.array_equal(cs.fixed.status, cs.lens.status)
    return cs


def check_multi_case(c):
    """What a G = 589 case must hold, on the CPU."""
    at = list(PLANTED_AT)
    assert c.G == G_MULTI == 2 * 256 + 77 and c.G % 4 != 0
    assert c.masks[at].tolist() == multi_planted_masks(c.k, c.r) and len(set(c.masks[at].tolist())) == len(at)
    assert c.sym_rec[at].tolist() == list(PLANTED_LEN)
    assert c.status[at].tolist() == [0, 0, 0, 1, 0]
    for g in at:                                                              # the neighbours differ in mask and length
        for h in (g - 1, g + 1):
            if h < c.G and h not in at:
                assert c.masks[h] != c.masks[g] and c.sym_rec[h] != c.sym_rec[g], (g, h)
    # every classify workgroup rebuilds, refuses and leaves groups alone; parity lengths are not all 0
    for lo in (0, 256, 512):
        part = slice(lo, min(lo + 256, c.G))
        assert (c.status[part] == 1).any() and (c.masks[part] == 0).any()
        assert ((c.status[part] == 0) & c.lost[part, :c.k].any(axis=1)).any()
    assert (c.lens[:, c.k:] > 0).any() and len(set(c.lens.reshape(-1).tolist())) > c.P // 2


@pytest.mark.parametrize("k,r,P", [(10, 3, 48), (62, 2, 48)])
def test_multi_workgroup_cases_hold_the_planted_groups(oracle_mod, k, r, P):
    """On the CPU: the planted masks and lengths at groups 255, 256, 511, 512 and 588 (asserted
    inside multi_cases, which the GPU tests build their cases with)."""
    cs = multi_cases(oracle_mod, k, r, P)
    check_multi_case(cs.lens)
    assert (k + r) * 256 <= 256 * 64                                          # k=62 r=2: the documented maximum per workgroup


def run_multi(torch, ctx, cs, traced=None):
    """The three recovers (the scatter with d_symbol_len_out on padded destinations and without it
    back to back, its L_g then in the workspace) and, where the case has them, the two encodes.
    traced(name, launch): runs launch() and looks at what it launched."""
    c = cs.lens

    def go(name, b, launch, check):
        if traced is None:
            launch(ctx, b)
        else:
            traced(name, lambda: launch(ctx, b))
        ctx.synchronize()
        check(b, name)

    go("recover_gather", fx.make_recover(torch, cs.fixed, SEED + 1), fx.launch_recover, fx.check_recover)
    go("recover_gather_var", var.make_recover(torch, c, SEED + 2), var.launch_recover, var.check_recover)
    go("recover_scatter", sc.make_scatter(torch, c, SEED + 3, sc.padded_layout(SEED + 4)), sc.launch_scatter, sc.check_scatter)
    go("recover_scatter", sc.make_scatter(torch, c, SEED + 5, sc.packed_layout, want_sym=False), sc.launch_scatter,
       sc.check_scatter)
    if hasattr(cs, "enc"):
        for name, run, case in (("encode_v16", run_fixed_encode, cs.enc_fixed), ("encode_gather_var", run_var_encode, cs.enc)):
            if traced is None:
                run(torch, ctx, case, SEED + 6, name)
            else:
                traced(name, lambda: run(torch, ctx, case, SEED + 6, name))


@gpu
@pytest.mark.parametrize("k,r,P", MULTI)
def test_more_than_one_classify_workgroup(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """G = 589 in one launch of each kernel: every masks_out, status and symbol_len_out entry and
    every rebuilt byte against the CPU's."""
    with product_ctx(quicfec_mod) as ctx:
        run_multi(torch_cuda, ctx, multi_cases(oracle_mod, k, r, P))


def chunk_runs(trace, G):
    """The launches of a call as the runs of its chunk loops: a run starts at item 0, every further
    launch of it starts where the one before ended, and it ends at G.  [[(first_item, items, grid)]]"""
    runs = []
    for t in trace:
        if t["first_item"] == 0:
            runs.append([t])
        else:
            prev = runs[-1][-1]
            assert (t["form"], t["aux"]) == (prev["form"], prev["aux"]), (prev, t)
            assert t["first_item"] == prev["first_item"] + prev["items"], (prev, t)
            runs[-1].append(t)
    assert all(run[-1]["first_item"] + run[-1]["items"] == G for run in runs)
    return runs


@gpu
@pytest.mark.parametrize("k,r,P", MULTI)
def test_more_than_one_classify_workgroup_chunked(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P):
    """The same cases on the test library with at most 300 items per classify launch (300 + 289
    groups: two workgroups each, the second partial, the second launch at a non-zero base) and 40
    workgroups per recover launch (160 groups): the bytes are the same, and the chunks of each
    kernel cover [0, G) once, in order."""
    lib = quicfec_mod.load_test_library()
    G = G_MULTI
    passes = 1 if (k, r) == (10, 3) else (r + 7) // 8

    def traced(name, launch):
        quicfec_mod.launch_trace(lib)                                        # clear: fills and uploads are torch's
        launch()
        ctx.synchronize()
        trace = quicfec_mod.launch_trace(lib)
        runs = chunk_runs(trace, G)
        shape = [[(t["first_item"], t["items"], t["grid"]) for t in run] for run in runs]
        if name.startswith("recover"):
            classify = name.replace("recover", "classify")
            assert [run[0]["form"] for run in runs] == [classify] + [name] * passes, (name, k, r, P)
            assert shape[0] == [(0, 300, 2), (300, 289, 2)]
            assert shape[1:] == passes * [[(0, 160, 40), (160, 160, 40), (320, 160, 40), (480, 109, 28)]]
            assert [run[0]["aux"] for run in runs[1:]] == [8 * p for p in range(passes)]
        else:
            assert {t["form"] for t in trace} == {name} and all(len(run) > 1 for run in runs), (name, k, r, P)

    with hooks_ctx(quicfec_mod) as ctx:
        torch_cuda.cuda.synchronize()
        monkeypatch.setenv("QUICFEC_MAX_LAUNCH_THREADS", "300")
        monkeypatch.setenv("QUICFEC_MAX_WAVE_BLOCKS", "40")
        run_multi(torch_cuda, ctx, multi_cases(oracle_mod, k, r, P), traced)


# ------------------------------------------------------------------------------------------
# 4. Every codebook record, every mask
# ------------------------------------------------------------------------------------------
RECORDS = [(20, 5, 53_129, 48)] + [(k, r, n, P) for (k, r, n) in ((10, 3, 285), (10, 2, 65), (10, 1, 10), (4, 2, 14), (7, 4, 329))
                                   for P in (48, 272)]


def record_lengths(P, G, n, shift=0):
    """dealt_lengths; past 10,000 groups (k=20 r=5) without the edge lengths above 2 P.  The call
    clamps a length at P, so those (255..1025 at 48 B) are to it what P + 1 and 2 P are, which stay;
    a shard holds its unclamped length, so with them the 1.3 million shards of that case would be
    1.4 GB of packets instead of 100 MB.  Trimmed there: these lengths, no group and no record."""
    if G <= 10_000:
        return dealt_lengths(P, G, n, shift)
    e = edge_lengths(P)
    e = e[e <= 2 * P]
    return e[(np.arange(G)[:, None] + np.arange(n)[None, :] + shift) % len(e)]


@lru_cache(maxsize=None)
def record_cases(oracle, k, r, P):
    """One group per (E, R) record of the dense codebook (test_gpu_forms.record_masks), fixed-length
    and with lengths dealt from edge_lengths(P) (record_lengths).  Every group is recoverable."""
    masks = record_masks(k, r, k * 100 + r)
    G = len(masks)
    salt = k * 100000 + r * 10000 + P
    cs = SimpleNamespace(fixed=fx.make_case(oracle, k, r, P, masks, SEED + salt + 7),
                         lens=var.make_case(oracle, k, r, P, masks, record_lengths(P, G, k), record_lengths(P, G, r, shift=k),
                                            SEED + salt + 8))
    rows = int(sum(bin(int(m) & ((1 << k) - 1)).count("1") for m in masks))
    for c in (cs.fixed, cs.lens):
        assert (c.status == 0).all() and c.rows == rows                      # a wrong rank cannot hide as 'unrecoverable'
    return cs


def test_record_cases_are_all_recoverable(oracle_mod):
    """On the CPU: one group per record, every status 0, as many rebuilt rows as lost data shards
    (asserted inside record_cases), and the rule's rows are exactly the record's R."""
    cs = record_cases(oracle_mod, 7, 4, 48)
    assert cs.fixed.G == 329 and len(set(cs.fixed.masks.tolist())) == 329
    used = rule_rows(cs.fixed)
    e = cs.fixed.lost[:, :7].sum(axis=1)
    assert (used.sum(axis=1) == e).all() and len({(int(m) & 127, tuple(u)) for m, u in zip(cs.fixed.masks, used)}) == 329


@gpu
@pytest.mark.parametrize("k,r,records,P", RECORDS)
def test_every_codebook_record(quicfec_mod, oracle_mod, torch_cuda, k, r, records, P):
    """Every (erased set, parity rows) record once through the table-indexed loads ga[rec_byte(rw, s)]
    of the fixed gather recover and through those and the destinations gd[rec_byte(rw, 64 + m)] of
    the scatter recover, its destinations back to back.  k=20 r=5 runs at 48 B only (53,129 groups,
    64 MB of shards); its arenas come from fast_arena."""
    torch = torch_cuda
    cs = record_cases(oracle_mod, k, r, P)
    assert cs.fixed.G == records
    with product_ctx(quicfec_mod) as ctx:
        b = make_fixed(torch, cs.fixed, SEED + 71)
        fx.launch_recover(ctx, b)
        ctx.synchronize()
        fx.check_recover(b, "every record, fixed gather")
        del b
        s = make_packed_scatter(torch, cs.lens, SEED + 72)
        sc.launch_scatter(ctx, s)
        ctx.synchronize()
        sc.check_scatter(s, "every record, scatter")
        assert len(s.rows[0]) == cs.lens.rows


@lru_cache(maxsize=None)
def mask_cases(oracle, k, r):
    """All 2^(k+r) masks, shuffled, at 272 B."""
    P = 272
    masks = np.arange(1 << (k + r), dtype=np.uint64)
    np.random.default_rng(k + r).shuffle(masks)
    G = len(masks)
    salt = k * 100000 + r * 10000 + P
    cs = SimpleNamespace(fixed=fx.make_case(oracle, k, r, P, masks, SEED + salt + 9),
                         lens=var.make_case(oracle, k, r, P, masks, dealt_lengths(P, G, k), dealt_lengths(P, G, r, shift=k),
                                            SEED + salt + 10))
    cs.none = int(np.flatnonzero(masks == 0)[0])
    cs.all = int(np.flatnonzero(masks == np.uint64((1 << (k + r)) - 1))[0])
    for c in (cs.fixed, cs.lens):
        assert c.status[cs.none] == 0 and not c.lost[cs.none].any()
        assert c.status[cs.all] == 1 and c.lost[cs.all].all() and (c.slots[cs.all] == 0x5A).all()
    assert cs.lens.sym_rec[cs.all] == 0 and (lens_table(cs.lens)[cs.all] == JUNK_LEN).all()
    return cs


def test_mask_cases_hold_the_empty_and_the_full_mask(oracle_mod):
    """On the CPU: mask 0 and the all-ones mask are in the set, the latter with every entry lost and
    symbol length 0 (asserted inside mask_cases)."""
    cs = mask_cases(oracle_mod, 4, 2)
    assert cs.fixed.G == 64 and sorted(cs.fixed.masks.tolist()) == list(range(64))
    _, where = fast_arena(cs.lens, 1, at_length=True)
    assert (where[cs.all, :, 0] == -1).all()                                 # every table entry of that group is 0


@gpu
@pytest.mark.parametrize("k,r", [(10, 3), (10, 2), (10, 1), (4, 2)])
def test_every_mask(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """All 2^(k+r) masks at 272 B through the fixed gather, the var gather and the scatter recover:
    statuses, derived masks, symbol lengths and rows equal the oracle's.  The group with every entry
    0 leaves its slots and every destination untouched and reports L = 0."""
    torch = torch_cuda
    cs = mask_cases(oracle_mod, k, r)
    with product_ctx(quicfec_mod) as ctx:
        b = make_fixed(torch, cs.fixed, SEED + 81)
        fx.launch_recover(ctx, b)
        ctx.synchronize()
        fx.check_recover(b, "every mask, fixed gather")
        v = make_var(torch, cs.lens, SEED + 82)
        var.launch_recover(ctx, v)
        ctx.synchronize()
        var.check_recover(v, "every mask, var gather")
        assert (v.table.cpu().numpy().reshape(-1, k + r)[cs.all] == 0).all()
        assert (v.out.cpu().numpy().reshape(-1, r, 272)[cs.all] == 0x5A).all() and v.sym.cpu().numpy()[cs.all] == 0
        assert v.st.cpu().numpy()[cs.all] == 1 and v.st.cpu().numpy()[cs.none] == 0
        s = make_packed_scatter(torch, cs.lens, SEED + 83)
        sc.launch_scatter(ctx, s)
        ctx.synchronize()
        sc.check_scatter(s, "every mask, scatter")                           # the canary its entries point at is intact
        assert cs.all not in s.rows[0] and s.so.cpu().numpy()[cs.all] == 0 and s.st.cpu().numpy()[cs.all] == 1
