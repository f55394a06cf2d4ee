"""fec_recover_gather_var_rs_dev and fec_encode_gather_var_rs_dev on the GPU: the address-table
calls with a length per entry.  Expected bytes come from the oracle on zero-padded inputs
(oracle.rs_encode, oracle.rs_decode) and, for parity row 0, from oracle.go_generate_redundancy on
the true variable-length packets.  Bit-exact, no tolerance.

The arena (build_arena): two separate allocations filled with 0xEE.  Every present shard sits at
its true length (the table's length, unclamped: a shard of length 2P has 2P bytes there), in a
seeded random order, each followed by a pad of 1..37 bytes of 0xEE and then the next shard, so
addresses take every residue mod 16; each arena ends with P + 38 bytes of 0xEE.  A read past a
shard's length therefore changes the output and never leaves the allocation.  A present shard of
length 0 points at pad bytes.  A lost / absent entry is address 0 and its length entry is garbage.
A present parity row the erasure rule does not read (a row past the e lowest surviving ones, every
row of a group that rebuilds nothing: tests/unread_shards.py) keeps its address and its length
entry -- the group's symbol length is taken over every present entry -- and holds seeded junk.

After every call: both arenas byte-identical to before; the output (pre-filled 0x5A, with guard
bytes before and after) equals the oracle's and still holds 0x5A everywhere else; status
(pre-filled 7), the derived masks and the symbol lengths equal the expected ones.
"""
import os
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import unread_shards as us
from test_gather_var_forms import expected_encode_launches, expected_recover_launches   # the table of DESIGN.md §5b
from test_gpu_gather import GUARD, _planted, guarded, hooks_ctx, iid_masks, perm_masks, product_ctx

pytestmark = pytest.mark.gpu

SEED = 0x7A4E0000
G_MAIN = 67                                           # more than one wave-block, no multiple of 4, an odd tail
RECOVER_SHAPES = [(10, 3), (20, 5), (4, 2), (6, 3), (12, 9)]     # three compiled, runtime k in one and in two passes
ENCODE_SHAPES = [(10, 3), (10, 1), (4, 2), (20, 5), (7, 3)]
RECOVER_SIZES = [16, 17, 260, 1025, 1200, 2100]
ENCODE_SIZES = [16, 260, 1200]
JUNK_LEN = 0xFFFFFFFF                                 # the length entry of a lost / absent shard: ignored


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


def edge_lengths(P):
    """The lengths at every piece edge of the walk and of the mask, without the negative ones."""
    vals = [0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, P - 17, P - 16, P - 15, P - 5, P - 4, P - 3,
            P - 1, P, P + 1, 2 * P]
    return np.array(list(dict.fromkeys(v for v in vals if v >= 0)), dtype=np.int64)


def dealt_lengths(P, G, n, shift=0):
    """Edge lengths dealt cyclically over the n entries of a group, the dealing offset by one per
    group: with G >= the number of edge lengths every position meets every length."""
    e = edge_lengths(P)
    return e[(np.arange(G)[:, None] + np.arange(n)[None, :] + shift) % len(e)]


# ------------------------------------------------------------------------------------------
# Cases: one batch and what the oracle says about it, computed once and never modified
# ------------------------------------------------------------------------------------------
def padded(raw, lens, P):
    """Shards (.., L >= P) cut at min(len, P) and zero-padded to P."""
    return np.where(np.arange(P) < np.minimum(lens, P)[..., None], raw[..., :P], 0).astype(np.uint8)


def make_case(oracle, k, r, P, masks, dlens, plens_min, seed, present=None):
    """masks: lost shards (recover).  dlens (G, k): the data packets' true lengths.  plens_min
    (G, r): wanted parity shard lengths, raised to the group's symbol length (a repair packet
    carries at least that).  present (G, k) bool, encode only: absent packets count as zeros."""
    masks = np.asarray(masks, dtype=np.uint64)
    G = len(masks)
    dlens = np.asarray(dlens, dtype=np.int64)
    L = int(max(dlens.max(), np.max(plens_min), P))
    raw = oracle.splitmix_bytes(G * k * L, seed).reshape(G, k, L)
    here = np.ones((G, k), dtype=bool) if present is None else present
    data = padded(raw, np.where(here, dlens, 0), P)                          # (G, k, P)
    par = oracle.rs_encode(data.reshape(-1), G, k, r, P, nthreads=8).reshape(G, r, P)
    sym_enc = np.where(here, np.minimum(dlens, P), 0).max(axis=1)
    # the code is column-wise, so parity is zero past the group's symbol length: a parity shard
    # truncated there is the same symbol, which is what makes truncated repair packets legal inputs
    assert not (par * (np.arange(P)[None, None, :] >= sym_enc[:, None, None])).any()
    plens = np.maximum(np.asarray(plens_min, dtype=np.int64), sym_enc[:, None])
    praw = np.full((G, r, L), 0xA5, dtype=np.uint8)                          # bytes past P of an over-long repair packet
    praw[:, :, :P] = par
    assert np.array_equal(padded(praw, plens, P), par)
    lost = ((masks[:, None] >> np.arange(k + r, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    lost_d = lost[:, :k]
    # what a recover is given: junk in every parity row the rule does not read, over the row's whole
    # length (praw is what the arenas place; `par` stays true for the encode comparisons), and in
    # every lost data shard of the contiguous image the oracle decodes
    ro = us.roles(masks, k, r)
    assert np.array_equal(ro.lost_d, lost_d) and np.array_equal(ro.lost_p, lost[:, k:])
    praw[ro.unread_p] = us.junk(int(ro.unread_p.sum()) * L, seed).reshape(-1, L)
    praw[ro.unread_p & (padded(praw, plens, P) == par).all(axis=2)] ^= 0xFF      # a row of a few bytes drew the truth
    par_in = padded(praw, plens, P)
    assert np.array_equal(par_in[ro.chosen], par[ro.chosen])
    assert ((par_in != par).any(axis=2) | (plens == 0))[ro.unread_p].all()
    broken, _ = us.inputs(data, par, masks, k, r, P, seed, need_lost_below=False, need_unchosen_alive=False)
    ref = broken.copy()
    _, status = oracle.rs_decode(ref, par_in.reshape(-1), masks, G, k, r, P, nthreads=8)
    ok = status == 0
    assert np.array_equal(ref.reshape(G, k, P)[ok], data[ok])               # rebuilt = the zero-padded originals
    gi, ji = np.nonzero(lost_d & ok[:, None])
    mi = (np.cumsum(lost_d, axis=1) - 1)[gi, ji]
    slots = np.full((G, r, P), 0x5A, dtype=np.uint8)
    slots[gi, mi] = data[gi, ji]
    lens = np.concatenate([dlens, plens], axis=1)
    sym_rec = np.where(lost, 0, np.minimum(lens, P)).max(axis=1)
    c = SimpleNamespace(k=k, r=r, P=P, G=G, masks=masks, lost=lost, present=here, raw=raw, praw=praw, data=data, par=par,
                        par_in=par_in, chosen=ro.chosen, lens=lens, status=status, slots=slots, rows=len(gi),
                        sym_enc=sym_enc.astype(np.uint32), sym_rec=sym_rec.astype(np.uint32))
    for a in (c.masks, c.lost, c.present, c.raw, c.praw, c.data, c.par, c.par_in, c.chosen, c.lens, c.status, c.slots,
              c.sym_enc, c.sym_rec):
        a.setflags(write=False)
    return c


def main_masks(k, r, n_edges):
    """Groups 0..4: untouched, parity lost only, unrecoverable, a single loss with parity row 0 alive
    (the XOR path) and one with it lost (test_gpu_gather's planted ones); 5..7 are set by main_case.
    From group 8 on every group rebuilds: two whole cycles of the dealt lengths, the first losing data
    shard 0 and the second data shard 1, so every other shard position is a survivor under every
    length in both and positions 0 and 1 in one; odd groups also lose parity row 0 (the GF path with a
    higher row) where r >= 2.  The groups after the two cycles lose two data shards (one if r = 1)."""
    masks = np.zeros(G_MAIN, dtype=np.uint64)
    masks[:5] = _planted(k, r)
    assert 8 + 2 * n_edges <= G_MAIN
    for g in range(8, G_MAIN):
        cycle = (g - 8) // n_edges
        m = 1 << cycle if cycle < 2 else (1 << 2) | ((1 << 3) if r >= 2 else 0)
        if cycle < 2 and g % 2 == 1 and r >= 2:
            m |= 1 << k
        masks[g] = m
    return masks


@lru_cache(maxsize=None)
def main_case(oracle, k, r, P):
    """The G = 67 case of a shape and size: main_masks, edge lengths dealt over data and parity, and
    the planted groups 3..7."""
    salt = k * 100000 + r * 10000 + P
    edges = edge_lengths(P)
    masks = main_masks(k, r, len(edges))
    dl = dealt_lengths(P, G_MAIN, k)
    pl = dealt_lengths(P, G_MAIN, r, shift=k)
    two = r >= 2
    dl[3] = P                                                   # all lengths P (one data loss, the XOR path)
    pl[3] = P
    dl[4] = 0                                                   # all lengths 0: the rebuilt row is P zeros
    pl[4] = 0
    dl[5] = np.arange(k) % 7 + 1                                # one full packet among short ones, a short one lost
    dl[5, 0] = P
    masks[5] = (1 << 2) | ((1 << (k + 1)) if two else 0)
    dl[6] = np.arange(k) * 3 % max(1, P - 3)                    # the lost packet is the longest: its tail comes
    dl[6, 0] = P - 3                                            # from parity alone
    pl[6] = 0
    masks[6] = 1 | ((1 << (k - 1)) if two else 0)
    dl[7] = np.minimum(dl[7], P // 2)                           # parity truncated to the symbol length,
    pl[7] = 0                                                   # one row left at full P
    pl[7, r - 1] = P
    masks[7] = 1 | ((1 << k) if two else 0)
    c = make_case(oracle, k, r, P, masks, dl, pl, SEED + salt)
    e = c.lost[:, :k].sum(axis=1) * (c.status == 0)
    assert c.masks[0] == 0 and e[1] == 0 and c.status[2] == 1 and (e[3:] >= 1).all() and (r < 2 or (e >= 2).any())
    assert (c.lens[3] == P).all() and (c.lens[4] == 0).all() and c.sym_rec[4] == 0
    assert c.lens[6, 0] == c.lens[6, :k].max() and (c.lens[6, k:] == P - 3).all() and c.lost[6, 0]
    assert (c.lens[7, k:k + r - 1] == c.sym_enc[7]).all() and c.lens[7, k + r - 1] == P and c.sym_enc[7] <= P // 2
    # every data shard position is a survivor of a rebuilding group under every edge length
    for s in range(k):
        assert set(edges.tolist()) <= set(c.lens[8:][~c.lost[8:, s], s].tolist()), (k, r, P, s)
    # a rebuilding group with a surviving row it does not read, junk of P bytes in the arena (group 3)
    if two:
        assert e[3] == 1 and (~c.lost[3, k:] & ~c.chosen[3]).any() and (c.lens[3, k:] == P).all()
    return c


# ------------------------------------------------------------------------------------------
# The arena and one call on it
# ------------------------------------------------------------------------------------------
def build_arena(c, seed, encode=False, par_rows=None):
    """Host image of the two arenas and, per table entry, (arena, offset) or (-1, 0) for a lost /
    absent one.  encode: the k data packets only.  par_rows (G, r, P): other parity bytes than the
    oracle's in the rows the rule reads (the round trip places the encode call's own rows); a present
    row it does not read holds the case's junk either way."""
    k, r, P, G = c.k, c.r, c.P, c.G
    n = k if encode else k + r
    rng = np.random.default_rng(seed)
    here = c.present if encode else ~c.lost
    gi, si = np.nonzero(here)
    order = rng.permutation(len(gi))
    pads = rng.integers(1, 38, size=len(gi))
    side = rng.integers(0, 2, size=len(gi))
    where = np.full((G, n, 2), -1, dtype=np.int64)
    where[:, :, 1] = 0
    fill = [37, 37]
    for i, pad, a in zip(order, pads, side):
        where[gi[i], si[i]] = (a, fill[a])
        fill[a] += int(c.lens[gi[i], si[i]]) + int(pad)
    arenas = [np.full(fill[a] + P + 38, 0xEE, dtype=np.uint8) for a in (0, 1)]
    for g, s in zip(gi, si):
        a, off = where[g, s]
        ln = int(c.lens[g, s])
        if s < k:
            arenas[a][off:off + ln] = c.raw[g, s, :ln]
        else:
            arenas[a][off:off + ln] = c.praw[g, s - k, :ln]
            if par_rows is not None and c.chosen[g, s - k]:
                arenas[a][off:off + min(ln, P)] = par_rows[g, s - k, :min(ln, P)]
    lens = np.where(here, c.lens[:, :n], JUNK_LEN).astype(np.uint32)
    return arenas, where, lens


def upload_arena(torch, arenas, where, lens):
    dev = [torch.from_numpy(a).to("cuda") for a in arenas]
    base = np.array([d.data_ptr() for d in dev] + [0], dtype=np.uint64)      # [-1] -> 0: lost / absent
    table = base[where[:, :, 0]] + where[:, :, 1].astype(np.uint64)
    assert ((table == 0) == (where[:, :, 0] < 0)).all()
    return (dev, torch.from_numpy(table.reshape(-1).view(np.int64)).to("cuda"),
            torch.from_numpy(lens.reshape(-1).view(np.int32)).to("cuda"))


def make_recover(torch, c, seed, par_rows=None):
    arenas, where, lens = build_arena(c, seed, par_rows=par_rows)
    b = SimpleNamespace(c=c, arenas=arenas)
    b.dev, b.table, b.lens = upload_arena(torch, arenas, where, lens)
    b.whole, b.out = guarded(torch, c.G * c.r * c.P, 0x5A)
    b.st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
    b.mo = torch.full((c.G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    b.sym = torch.full((c.G,), 0x77777777, dtype=torch.int32, device="cuda")
    return b


def launch_recover(ctx, b, stream=None):
    c = b.c
    ctx.recover_gather_var_dev(b.table, b.lens, c.G, c.k, c.r, c.P, b.out, b.st, b.mo, b.sym, stream=stream)


def check_recover(b, what=""):
    c = b.c
    what = (what, c.k, c.r, c.P, c.G)
    for d, a in zip(b.dev, b.arenas):
        assert np.array_equal(d.cpu().numpy(), a), what                      # the arenas are only read
    whole = b.whole.cpu().numpy()
    assert (whole[:GUARD] == 0x5A).all() and (whole[GUARD + c.slots.size:] == 0x5A).all(), what
    got = whole[GUARD:GUARD + c.slots.size].reshape(c.G, c.r, c.P)
    bad = np.nonzero((got != c.slots).any(axis=2))
    assert np.array_equal(got, c.slots), (what, "first wrong (g, m):", bad[0][:4], bad[1][:4],
                                          us.mismatch(c.masks, c.k, c.r, got, c.slots))
    assert np.array_equal(b.st.cpu().numpy(), c.status), what
    assert np.array_equal(b.mo.cpu().numpy().view(np.uint64), c.masks), what
    assert np.array_equal(b.sym.cpu().numpy().view(np.uint32), c.sym_rec), what


def run_recover(torch, ctx, c, seed, what=""):
    b = make_recover(torch, c, seed)
    launch_recover(ctx, b)
    ctx.synchronize()
    check_recover(b, what)
    return b


# ------------------------------------------------------------------------------------------
# 1. Lengths at every piece edge
# ------------------------------------------------------------------------------------------
def test_arena_puts_shards_at_their_length_at_every_residue(oracle_mod):
    """On the CPU: shards of the main case sit at every address residue mod 16, each followed by
    0xEE, and each arena ends with more than P bytes of 0xEE."""
    c = main_case(oracle_mod, 10, 3, 1200)
    arenas, where, lens = build_arena(c, 1)
    assert set((where[..., 1][where[..., 0] >= 0] % 16).tolist()) == set(range(16))
    for g, s in zip(*np.nonzero(~c.lost)):
        a, off = where[g, s]
        assert arenas[a][off + int(c.lens[g, s])] == 0xEE
    assert all((a[-(c.P + 38):] == 0xEE).all() for a in arenas)
    assert (lens[c.lost] == JUNK_LEN).all() and np.array_equal(lens[~c.lost], c.lens[~c.lost])


@pytest.mark.parametrize("k,r", RECOVER_SHAPES)
def test_lengths_at_every_piece_edge(quicfec_mod, oracle_mod, torch_cuda, k, r):
    with product_ctx(quicfec_mod) as ctx:
        for P in RECOVER_SIZES:
            run_recover(torch_cuda, ctx, main_case(oracle_mod, k, r, P), SEED + P)


# ------------------------------------------------------------------------------------------
# 2. All lengths = P: the fixed-length call
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", RECOVER_SHAPES)
def test_all_lengths_full_equals_the_fixed_call(quicfec_mod, oracle_mod, torch_cuda, k, r):
    torch = torch_cuda
    with product_ctx(quicfec_mod) as ctx:
        for P in (1200, 17):
            full = np.full((G_MAIN, k + r), P)
            c = make_case(oracle_mod, k, r, P, perm_masks(k, r, G_MAIN, SEED + P + k), full[:, :k], full[:, k:], SEED + 3 * P + r)
            b = make_recover(torch, c, SEED + 5)
            launch_recover(ctx, b)
            whole, out = guarded(torch, c.G * r * P, 0x5A)
            st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
            mo = torch.full((c.G,), -1, dtype=torch.int64, device="cuda")
            ctx.recover_gather_dev(b.table, c.G, k, r, P, out, st, mo)
            ctx.synchronize()
            check_recover(b, "all full")
            assert torch.equal(whole, b.whole) and torch.equal(st, b.st) and torch.equal(mo, b.mo), (k, r, P)


# ------------------------------------------------------------------------------------------
# 3. Launch trace
# ------------------------------------------------------------------------------------------
def _launch_text(rec):
    if rec["form"] == "classify_gather_var":
        return rec["form"]
    first = f" first={rec['first']}" if rec["form"] == "encode_gather_var" else ""
    return f"{rec['form']} k={rec['k']} r={rec['r']}{first} pol={rec['pol']} aux={rec['aux']}"


@pytest.mark.parametrize("k,r", RECOVER_SHAPES)
def test_recover_launches_only_the_var_kernels(quicfec_mod, oracle_mod, torch_cuda, k, r):
    lib = quicfec_mod.load_test_library()
    with hooks_ctx(quicfec_mod) as ctx:
        for P in (17, 1200):
            c = main_case(oracle_mod, k, r, P)
            b = make_recover(torch_cuda, c, SEED + 11)
            quicfec_mod.launch_trace(lib)                                    # clear: fills and uploads are torch's
            launch_recover(ctx, b)
            ctx.synchronize()
            trace = quicfec_mod.launch_trace(lib)
            assert [_launch_text(t) for t in trace] == expected_recover_launches(k, r, P), (k, r, P)
            assert {t["form"] for t in trace} == {"classify_gather_var", "recover_gather_var"}
            assert all(t["items"] == c.G and t["first_item"] == 0 and t["block"] == 256 for t in trace)
            assert trace[0]["grid"] == 1 and all(t["grid"] == (c.G + 3) // 4 for t in trace[1:])
            check_recover(b, "hooks")


# ------------------------------------------------------------------------------------------
# 4. Encode
# ------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def encode_case(oracle, k, r, P):
    G = G_MAIN
    dl = dealt_lengths(P, G, k)
    present = np.ones((G, k), dtype=bool)
    present[1] = False                                                       # partial groups: one present,
    present[1, k // 2] = True
    present[2, 0] = False                                                    # k - 1 present,
    present[3] = False                                                       # none present
    present[4:] = np.random.default_rng(SEED + k + P).random((G - 4, k)) < 0.85
    dl[5] = P
    dl[6] = 0
    c = make_case(oracle, k, r, P, [0] * G, dl, np.zeros((G, r), dtype=np.int64), SEED + 7 * P + k, present=present)
    assert c.sym_enc[3] == 0 and not c.par[3].any() and c.sym_enc[6] == 0 and c.sym_enc[5] == (P if present[5].any() else 0)
    # row 0 is the reference encoder's repair payload on the true packets (cut at P, as padTo cuts)
    for g in range(G):
        pk = [np.ascontiguousarray(c.raw[g, j, :min(int(c.lens[g, j]), P)]) for j in range(k) if present[g, j]]
        if c.sym_enc[g] == 0:                                                # the reference emits no repair packet
            assert not c.par[g].any()
        else:
            pay = oracle.go_generate_redundancy(pk, group_id=g)[11:]
            assert len(pay) == c.sym_enc[g]
            assert np.array_equal(c.par[g, 0, :len(pay)], pay) and not c.par[g, 0, len(pay):].any()
    return c


def make_encode(torch, c, seed):
    """Arena, tables and pre-filled outputs of one var gather encode of case c.  Everything is uploaded
    on torch's stream: synchronise before launching on a side stream."""
    arenas, where, lens = build_arena(c, seed, encode=True)
    e = SimpleNamespace(c=c, arenas=arenas)
    e.dev, e.table, e.lens = upload_arena(torch, arenas, where, lens)
    e.whole, e.par = guarded(torch, c.G * c.r * c.P, 0x5A)
    e.sym = torch.full((c.G,), 0x77777777, dtype=torch.int32, device="cuda")
    return e


def launch_encode(ctx, e, stream=None):
    c = e.c
    ctx.encode_gather_var_dev(e.table, e.lens, c.G, c.k, c.r, c.P, e.par, e.sym, stream=stream)


def run_encode(torch, ctx, c, seed, stream=None):
    e = make_encode(torch, c, seed)
    if stream is not None:
        torch.cuda.synchronize()
    launch_encode(ctx, e, stream)
    return e


def check_encode(e, what=""):
    c = e.c
    what = (what, c.k, c.r, c.P)
    got = e.whole.cpu().numpy()
    assert np.array_equal(got[GUARD:-GUARD].reshape(c.G, c.r, c.P)[:, 0], c.par[:, 0]), what      # the reference's row
    assert np.array_equal(got[GUARD:-GUARD].reshape(c.G, c.r, c.P), c.par), what
    assert (got[:GUARD] == 0x5A).all() and (got[-GUARD:] == 0x5A).all(), what
    assert np.array_equal(e.sym.cpu().numpy().view(np.uint32), c.sym_enc), what
    for d, a in zip(e.dev, e.arenas):
        assert np.array_equal(d.cpu().numpy(), a), what


@pytest.mark.parametrize("k,r", ENCODE_SHAPES)
def test_encode(quicfec_mod, oracle_mod, torch_cuda, k, r):
    with product_ctx(quicfec_mod) as ctx:
        for P in ENCODE_SIZES:
            e = run_encode(torch_cuda, ctx, encode_case(oracle_mod, k, r, P), SEED + P)
            ctx.synchronize()
            check_encode(e)


@pytest.mark.parametrize("k,r", [(10, 3), (12, 9)])
def test_encode_launches_only_the_var_passes(quicfec_mod, oracle_mod, torch_cuda, k, r):
    lib = quicfec_mod.load_test_library()
    P = 260
    c = encode_case(oracle_mod, 10, 3, P) if (k, r) == (10, 3) else make_case(
        oracle_mod, k, r, P, [0] * 9, dealt_lengths(P, 9, k), np.zeros((9, r), dtype=np.int64), SEED + 9)
    with hooks_ctx(quicfec_mod) as ctx:
        torch_cuda.cuda.synchronize()
        arenas, where, lens = build_arena(c, SEED + 12, encode=True)
        dev, table, dlens = upload_arena(torch_cuda, arenas, where, lens)
        whole, par = guarded(torch_cuda, c.G * r * P, 0x5A)
        quicfec_mod.launch_trace(lib)
        ctx.encode_gather_var_dev(table, dlens, c.G, k, r, P, par)           # no symbol lengths asked for
        ctx.synchronize()
        trace = quicfec_mod.launch_trace(lib)
    assert [_launch_text(t) for t in trace] == expected_encode_launches(k, r, P)
    cpp = (P + 15) // 16
    assert all(t["items"] == c.G and t["block"] == 256 and t["grid"] == (c.G * cpp + 255) // 256 for t in trace)
    assert np.array_equal(whole.cpu().numpy()[GUARD:-GUARD].reshape(c.G, r, P), c.par)


# ------------------------------------------------------------------------------------------
# 5. Round trip
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(10, 3, 1200), (7, 3, 260), (20, 5, 1025)])
def test_round_trip(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """The var encode's rows, cut at the symbol length it reports, go into an arena with the data;
    shards are erased; the var recover rebuilds the original packets."""
    torch = torch_cuda
    G = G_MAIN
    rng = np.random.default_rng(SEED + k + P)
    dl = np.where(rng.random((G, k)) < 0.5, P, rng.integers(0, P, size=(G, k)))
    enc = make_case(oracle_mod, k, r, P, [0] * G, dl, np.zeros((G, r), dtype=np.int64), SEED + 21 + P)
    with product_ctx(quicfec_mod) as ctx:
        e = run_encode(torch, ctx, enc, SEED + 22)
        ctx.synchronize()
        check_encode(e, "round trip")
        rows = e.par.cpu().numpy().reshape(G, r, P)
        sym = e.sym.cpu().numpy().view(np.uint32)
        # the same packets (same seed), now with losses; the repair shards carry sym bytes of the encode's rows
        c = make_case(oracle_mod, k, r, P, perm_masks(k, r, G, SEED + 23), dl, np.zeros((G, r), dtype=np.int64), SEED + 21 + P)
        assert np.array_equal(c.lens[:, k:], np.repeat(sym[:, None], r, axis=1)) and c.rows > 0
        b = make_recover(torch, c, SEED + 24, par_rows=rows)
        launch_recover(ctx, b)
        ctx.synchronize()
        check_recover(b, "round trip")                                       # slots = the zero-padded original packets


# ------------------------------------------------------------------------------------------
# 6. Refusals: the documented code, a message, nothing launched, nothing written
# ------------------------------------------------------------------------------------------
REFUSALS = [("k + r = 65", 60, 5, 1200, "", "exceeds"), ("P = 15", 10, 3, 15, "", "packet_size"),
            ("NULL length table", 10, 3, 1200, "lens", "length table"), ("NULL table", 10, 3, 1200, "table", "addrs")]


@pytest.mark.parametrize("call,what,k,r,P,null,word",
                         [("recover", *x) for x in REFUSALS] + [("encode", *x) for x in REFUSALS] +
                         # the codebook cap is the recover's alone: the encode serves k=16 r=16
                         [("recover", "sparse-plan shape", 16, 16, 1200, "", "sparse-plan")])
def test_refusals(quicfec_mod, torch_cuda, call, what, k, r, P, null, word):
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    G = 5
    n = k + r if call == "recover" else k
    arena = torch.full((G * n * (P + 40),), 0xEE, dtype=torch.uint8, device="cuda")
    addr = np.uint64(arena.data_ptr()) + np.arange(G * n, dtype=np.uint64) * np.uint64(P + 40)   # all readable
    table = None if null == "table" else torch.from_numpy(addr.view(np.int64)).to("cuda")
    lens = None if null == "lens" else torch.full((G * n,), P, dtype=torch.int32, device="cuda")
    out = torch.full((G * r * P + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
    mo = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    sym = torch.full((G,), -1, dtype=torch.int32, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(lib)
        with pytest.raises(quicfec_mod.FecError) as ei:
            if call == "recover":
                ctx.recover_gather_var_dev(table, lens, G, k, r, P, out, st, mo, sym)
            else:
                ctx.encode_gather_var_dev(table, lens, G, k, r, P, out, sym)
        assert ei.value.code == (quicfec_mod.FEC_ERR_NULL if null else quicfec_mod.FEC_ERR_RANGE)
        assert word in quicfec_mod.last_error(lib) and word in ctx.last_error(), quicfec_mod.last_error(lib)
        ctx.synchronize()
        assert quicfec_mod.launch_trace(lib) == []
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (st == 7).all().item() and (mo == -1).all().item() and (sym == -1).all().item()
    assert (arena == 0xEE).all().item()


def test_zero_groups_are_refused(quicfec_mod, torch_cuda):
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    table = torch.zeros(13, dtype=torch.int64, device="cuda")
    lens = torch.zeros(13, dtype=torch.int32, device="cuda")
    out = torch.full((3 * 1200,), 0x5A, dtype=torch.uint8, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        quicfec_mod.launch_trace(lib)
        assert lib.fec_recover_gather_var_rs_dev(ctx.handle, table.data_ptr(), lens.data_ptr(), 0, 10, 3, 1200,
                                                 out.data_ptr(), None, None, None, None) == quicfec_mod.FEC_ERR_RANGE
        assert "num_groups" in ctx.last_error()
        assert lib.fec_encode_gather_var_rs_dev(ctx.handle, table.data_ptr(), lens.data_ptr(), 0, 10, 3, 1200,
                                                out.data_ptr(), None, None) == quicfec_mod.FEC_ERR_RANGE
        assert "num_groups" in ctx.last_error()
        assert quicfec_mod.launch_trace(lib) == []
    assert (out == 0x5A).all().item()


# ------------------------------------------------------------------------------------------
# 7. One side stream, no host synchronise until the end
# ------------------------------------------------------------------------------------------
def _contiguous(torch, oracle, k, r, P, G, seed):
    """A contiguous slot recover (recover_dev) of a record-addressed form: its classify writes the
    stream's workspace too."""
    from test_gpu_gather import make_case as fixed_case
    c = fixed_case(oracle, k, r, P, perm_masks(k, r, G, seed), seed + 1)
    d = SimpleNamespace(c=c, dd=torch.from_numpy(np.array(c.broken)).to("cuda"),
                        dp=torch.from_numpy(np.array(c.par_in)).to("cuda"),
                        dm=torch.from_numpy(np.array(c.masks).view(np.int64)).to("cuda"),
                        st=torch.full((G,), 7, dtype=torch.uint8, device="cuda"))
    d.whole, d.out = guarded(torch, G * r * P, 0x5A)
    return d


def test_queue_on_one_side_stream(quicfec_mod, oracle_mod, torch_cuda):
    """In order on one non-blocking side stream: a var recover, a fixed gather recover, a contiguous
    recover_dev and a second var recover with more groups (the workspace grows under queued work);
    one synchronise at the end, then every result is checked."""
    import test_gpu_gather as fixed
    torch = torch_cuda
    k, r, P = 20, 5, 1025
    v1 = make_recover(torch, main_case(oracle_mod, k, r, P), SEED + 41)
    f = fixed.make_recover(torch, fixed.main_case(oracle_mod, k, r, 1200), SEED + 42)
    d = _contiguous(torch, oracle_mod, k, r, 700, 33, SEED + 43)
    G2 = 1500
    rng = np.random.default_rng(SEED + 44)
    c2 = make_case(oracle_mod, k, r, P, iid_masks(k, r, G2, 0.1, rng), rng.integers(0, P + 9, size=(G2, k)),
                   rng.integers(0, P + 9, size=(G2, r)), SEED + 45)
    v2 = make_recover(torch, c2, SEED + 46)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        launch_recover(ctx, v1, stream.cuda_stream)
        fixed.launch_recover(ctx, f, stream.cuda_stream)
        ctx.recover_dev(d.dd, d.dp, d.dm, d.c.G, d.c.k, d.c.r, d.c.P, d.out, d.st, stream=stream.cuda_stream)
        launch_recover(ctx, v2, stream.cuda_stream)
        torch.cuda.synchronize()
    check_recover(v1, "first")
    fixed.check_recover(f, "fixed")
    assert np.array_equal(d.whole.cpu().numpy()[GUARD:-GUARD].reshape(d.c.slots.shape), d.c.slots)
    assert np.array_equal(d.st.cpu().numpy(), d.c.status)
    check_recover(v2, "second")


def test_free_with_var_calls_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """A var encode and a var recover queued on a side stream, and the context freed at once:
    fec_encoder_free drains them, so both outputs are complete and right after it."""
    torch = torch_cuda
    k, r, P, G = 10, 3, 1200, 4096
    rng = np.random.default_rng(SEED + 51)
    c = make_case(oracle_mod, k, r, P, perm_masks(k, r, G, SEED + 52), rng.integers(0, P + 9, size=(G, k)),
                  np.zeros((G, r), dtype=np.int64), SEED + 53)
    b = make_recover(torch, c, SEED + 54)
    stream = torch.cuda.Stream()
    ctx = product_ctx(quicfec_mod)
    e = run_encode(torch, ctx, c, SEED + 55, stream=stream.cuda_stream)
    launch_recover(ctx, b, stream.cuda_stream)
    ctx.close()
    assert stream.query()                                                    # the free drained the stream
    torch.cuda.synchronize()
    check_encode(e, "in flight")
    check_recover(b, "in flight")


# ------------------------------------------------------------------------------------------
# 8. Random sweep
# ------------------------------------------------------------------------------------------
def test_random_sweep(quicfec_mod, oracle_mod, torch_cuda):
    """40 seeded cases over shape, P in 16..2100, G in 1..40, iid loss of 1%, 10% or 30% and
    independent lengths in 0..P + 8 for every data and parity shard."""
    shapes = [(10, 3), (10, 2), (10, 1), (4, 2), (20, 5), (6, 3), (12, 6), (16, 4), (12, 9)]
    rng = np.random.default_rng(SEED + 77)
    rebuilt = unrec = 0
    with product_ctx(quicfec_mod) as ctx:
        for i in range(40):
            k, r = shapes[rng.integers(len(shapes))]
            P, G = int(rng.integers(16, 2101)), int(rng.integers(1, 41))
            loss = (0.01, 0.10, 0.30)[rng.integers(3)]
            c = make_case(oracle_mod, k, r, P, iid_masks(k, r, G, loss, rng), rng.integers(0, P + 9, size=(G, k)),
                          rng.integers(0, P + 9, size=(G, r)), SEED + 1000 + i)
            run_recover(torch_cuda, ctx, c, SEED + 2000 + i, (i, loss))
            rebuilt += c.rows
            unrec += int(c.status.sum())
    assert rebuilt > 40 and unrec > 0                                        # the sweep rebuilt and refused
