"""fec_recover_gather_rs_dev and fec_encode_gather_rs_dev on the GPU: shards scattered over two
device allocations at arbitrary byte offsets, reached through a table of absolute addresses
(0 = lost), against the oracle on the contiguous equivalent.  Bit-exact, no tolerance.

The arena (build_arena): two separate allocations filled with 0xEE; the surviving shards of every
group, data and parity mixed, placed in a seeded random order at a stride of P + pad with pad drawn
from 1..37 per shard, so shard addresses take every residue mod 16.  A lost shard is placed nowhere
and its table entry is 0; every other entry is a readable address.  A surviving parity row the
erasure rule does not read (a row past the e lowest surviving ones, every row of a group that
rebuilds nothing: tests/unread_shards.py) is placed like any other, with seeded junk for contents.

After every call: both arenas byte-identical to before; the rebuilt buffer (pre-filled 0x5A, with
guard bytes before and after) equals the oracle's slots and still holds 0x5A everywhere else;
status (pre-filled 7) equals the oracle's; the derived masks equal the masks the arena was built
from.
"""
import os
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import unread_shards as us
from test_gather_forms import expected_launches      # the table written from DESIGN.md §5b

pytestmark = pytest.mark.gpu

SEED = 0x6A7E0000
GUARD = 256                                           # guard bytes on each side of an output buffer
G_MAIN = 67                                           # more than one wave-block, no multiple of 4, an odd tail
COMPILED = [(10, 3), (10, 2), (10, 1), (4, 2), (20, 5)]
RUNTIME = [(6, 3), (12, 6), (16, 4)]
SHAPES = COMPILED + RUNTIME
# the piece-walk edges: one 16-B piece, the 256-B and 1-KiB pass boundaries, the shifted-back tail
SIZES = [16, 17, 31, 255, 256, 257, 1023, 1024, 1025, 1200, 1279, 1280, 2047, 2048, 2100]


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases: one batch and what the oracle says about it, computed once and never modified
# ------------------------------------------------------------------------------------------
def _planted(k, r):
    """Untouched, parity lost only, unrecoverable (a data shard and every parity row lost); then the
    two single-loss rebuilds: one data shard lost with parity row 0 alive (the XOR path), and one
    data shard lost with parity row 0 lost too (the GF path with e = 1; r = 1 has no such group
    and gets a second XOR group)."""
    return [0, 1 << k, 1 | (((1 << r) - 1) << k), 1 << 1, (1 << 2) | (1 << k) if r >= 2 else 1 << (k - 1)]


def perm_masks(k, r, G, seed):
    rng = np.random.default_rng(seed)
    masks = np.zeros(G, dtype=np.uint64)
    for g in range(G):
        for s in rng.permutation(k + r)[: rng.integers(0, r + 2)]:
            masks[g] |= np.uint64(1) << np.uint64(int(s))
    planted = _planted(k, r)[:G]
    masks[:len(planted)] = planted
    return masks


def rebuild_kinds(masks, k, r):
    """Per group: the number of data shards it rebuilds (0 when none lost or unrecoverable), and
    whether parity row 0 is lost."""
    masks = np.asarray(masks, dtype=np.uint64)
    bits = ((masks[:, None] >> np.arange(k + r, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    e = bits[:, :k].sum(axis=1)
    e[e + bits[:, k:].sum(axis=1) > r] = 0
    return e, bits[:, k]


def iid_masks(k, r, G, loss, rng):
    w = np.left_shift(np.uint64(1), np.arange(k + r, dtype=np.uint64))
    return ((rng.random((G, k + r)) < loss) * w).sum(axis=1, dtype=np.uint64)


def make_case(oracle, k, r, P, masks, seed):
    masks = np.asarray(masks, dtype=np.uint64)
    G = len(masks)
    data = oracle.splitmix_bytes(G * k * P, seed)
    par = oracle.rs_encode(data, G, k, r, P, nthreads=8)
    lost = ((masks[:, None] >> np.arange(k + r, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    lost_d = lost[:, :k]
    # junk in every lost data shard and every parity row the rule does not read.  A lost row has
    # address 0 in a table, so which groups have one below a chosen row does not matter here, and
    # make_case also serves encode cases and edge masks: main_case asserts the mix of its own cases.
    broken, par_in = us.inputs(data, par, masks, k, r, P, seed, need_lost_below=False, need_unchosen_alive=False)
    ref = broken.copy()
    _, status = oracle.rs_decode(ref, par_in, masks, G, k, r, P, nthreads=8)
    ok = status == 0
    # the oracle's rebuilt packets are the original ones
    assert np.array_equal(ref.reshape(G, k, P)[ok], data.reshape(G, k, P)[ok])
    gi, ji = np.nonzero(lost_d & ok[:, None])               # (g, j ascending)
    mi = (np.cumsum(lost_d, axis=1) - 1)[gi, ji]
    slots = np.full((G, r, P), 0x5A, dtype=np.uint8)
    slots[gi, mi] = ref.reshape(G, k, P)[gi, ji]
    c = SimpleNamespace(k=k, r=r, P=P, G=G, masks=masks, lost=lost, data=data, par=par, par_in=par_in, broken=broken,
                        status=status, slots=slots, rows=len(gi))
    for a in (c.masks, c.lost, c.data, c.par, c.par_in, c.broken, c.status, c.slots):
        a.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def main_case(oracle, k, r, P):
    """The G = 67 case of a shape and size: permutation masks with the five planted groups, and the
    mix checked on the CPU before anything runs."""
    salt = k * 100000 + r * 10000 + P
    c = make_case(oracle, k, r, P, perm_masks(k, r, G_MAIN, salt), SEED + salt)
    kmask = np.uint64((1 << k) - 1)
    assert (c.masks == 0).any() and (c.status != 0).any() and c.rows > 0
    assert ((c.masks != 0) & ((c.masks & kmask) == 0)).any()
    assert c.masks[0] == 0 and c.status[2] == 1 and c.status[1] == 0
    # the single-loss XOR path, the GF path with e = 1, and more than one row (r >= 2)
    e, row0_lost = rebuild_kinds(c.masks, k, r)
    assert ((e == 1) & ~row0_lost).any()
    if r >= 2:
        assert ((e == 1) & row0_lost).any() and (e >= 2).any()
    assert np.array_equal(e > 0, (c.status == 0) & ((c.masks & kmask) != 0))
    # a surviving row that a rebuilding group does not read (junk in the arena), and with r >= 2 a
    # lost row below a chosen one
    ro = us.roles(c.masks, k, r)
    assert us.has_unchosen_alive_row(ro).any()
    if r >= 2:
        assert (us.has_unchosen_alive_row(ro) & (e > 0)).any() and us.has_lost_row_below_chosen(ro).any()
    return c


# ------------------------------------------------------------------------------------------
# The arena and one call on it
# ------------------------------------------------------------------------------------------
def build_arena(c, seed, encode=False):
    """Host image of the two arenas and, per table entry, (arena, offset) or (-1, 0) for a lost shard.
    encode: only the k data packets of every group, all present (the encode call's table).  A present
    parity row holds c.par_in: true parity where the rule reads it, junk where it does not."""
    k, r, P, G = c.k, c.r, c.P, c.G
    n = k if encode else k + r
    rng = np.random.default_rng(seed)
    present = np.ones((G, k), dtype=bool) if encode else ~c.lost
    gi, si = np.nonzero(present)
    order = rng.permutation(len(gi))
    pads = rng.integers(1, 38, size=len(gi))
    side = rng.integers(0, 2, size=len(gi))
    where = np.full((G, n, 2), -1, dtype=np.int64)
    where[:, :, 1] = 0
    fill = [0, 0]
    for i, pad, a in zip(order, pads, side):
        fill[a] += int(pad)
        where[gi[i], si[i]] = (a, fill[a])
        fill[a] += P
    arenas = [np.full(fill[a] + 38, 0xEE, dtype=np.uint8) for a in (0, 1)]
    shards = np.concatenate([c.data.reshape(G, k, P), c.par_in.reshape(G, r, P)], axis=1)
    for g, s in zip(gi, si):
        a, off = where[g, s]
        arenas[a][off:off + P] = shards[g, s]
    return arenas, where


def upload_arena(torch, arenas, where):
    """The arenas as two separate device allocations and the table of absolute addresses."""
    dev = [torch.from_numpy(a).to("cuda") for a in arenas]
    base = np.array([d.data_ptr() for d in dev] + [0], dtype=np.uint64)      # [-1] -> 0: lost
    table = base[where[:, :, 0]] + where[:, :, 1].astype(np.uint64)
    assert ((table == 0) == (where[:, :, 0] < 0)).all()
    return dev, torch.from_numpy(table.reshape(-1).view(np.int64)).to("cuda")


def guarded(torch, nbytes, fill):
    """A device buffer of nbytes between two guards, everything pre-filled; (whole, the buffer)."""
    whole = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def make_recover(torch, c, seed):
    """Arena, table and pre-filled outputs of one gather recover of case c.  Everything is uploaded
    on torch's stream: synchronise before launching on a side stream."""
    arenas, where = build_arena(c, seed)
    b = SimpleNamespace(c=c, arenas=arenas)
    b.dev, b.table = upload_arena(torch, arenas, where)
    b.whole, b.out = guarded(torch, c.G * c.r * c.P, 0x5A)
    b.st = torch.full((c.G,), 7, dtype=torch.uint8, device="cuda")
    b.mo = torch.full((c.G,), 0x3C3C3C3C3C3C3C3C, dtype=torch.int64, device="cuda")
    return b


def launch_recover(ctx, b, stream=None):
    c = b.c
    ctx.recover_gather_dev(b.table, c.G, c.k, c.r, c.P, b.out, b.st, b.mo, stream=stream)


def check_recover(b, what=""):
    """After the synchronise: everything the call must write, and everything it must not."""
    c = b.c
    what = (what, c.k, c.r, c.P, c.G)
    for d, a in zip(b.dev, b.arenas):
        assert np.array_equal(d.cpu().numpy(), a), what                      # the arenas are only read
    whole = b.whole.cpu().numpy()
    assert (whole[:GUARD] == 0x5A).all() and (whole[GUARD + c.slots.size:] == 0x5A).all(), what
    # the oracle's slots; 0x5A in slots m >= e and in every slot of an unrecoverable group
    assert np.array_equal(whole[GUARD:GUARD + c.slots.size].reshape(c.G, c.r, c.P), c.slots), \
        (what, us.mismatch(c.masks, c.k, c.r, whole[GUARD:GUARD + c.slots.size], c.slots))
    assert np.array_equal(b.st.cpu().numpy(), c.status), what
    assert np.array_equal(b.mo.cpu().numpy().view(np.uint64), c.masks), what


def run_recover(torch, ctx, c, seed, what=""):
    b = make_recover(torch, c, seed)
    launch_recover(ctx, b)
    ctx.synchronize()
    check_recover(b, what)
    return b


def product_ctx(quicfec):
    return quicfec.Context(device=0, lib=quicfec.load_library())


def hooks_ctx(quicfec):
    return quicfec.Context(device=0, lib=quicfec.load_test_library())


# ------------------------------------------------------------------------------------------
# 1. Shapes and sizes
# ------------------------------------------------------------------------------------------
def test_arena_addresses_take_every_residue():
    """On the CPU: the arena of a main case puts shards at every residue mod 16 (allocations are
    at least 16-B aligned, so offsets decide), in both arenas, data and parity mixed."""
    c = SimpleNamespace(k=10, r=3, P=1200, G=G_MAIN, lost=np.zeros((G_MAIN, 13), dtype=bool),
                        data=np.zeros(G_MAIN * 10 * 1200, dtype=np.uint8), par_in=np.zeros(G_MAIN * 3 * 1200, dtype=np.uint8))
    _, where = build_arena(c, 1)
    for a in (0, 1):
        for part in (where[:, :10], where[:, 10:]):
            assert set((part[..., 1][part[..., 0] == a] % 16).tolist()) == set(range(16))


@pytest.mark.parametrize("k,r", SHAPES)
def test_shapes_and_sizes(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """Every compiled shape and three runtime-k shapes at the piece-walk edges, G = 67."""
    with product_ctx(quicfec_mod) as ctx:
        for P in SIZES:
            run_recover(torch_cuda, ctx, main_case(oracle_mod, k, r, P), SEED + P)


# ------------------------------------------------------------------------------------------
# 2. Identity table: the contiguous buffers through the address table
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r", [(10, 3), (20, 5)])
def test_identity_table_equals_contiguous_recover(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """Addresses into ordinary contiguous data / parity buffers (0 where the mask says lost):
    output, status and masks byte-identical to fec_recover_batch_rs_dev on the same buffers."""
    torch = torch_cuda
    P = 1200
    c = main_case(oracle_mod, k, r, P)
    G = c.G
    dd = torch.from_numpy(np.array(c.broken)).to("cuda")
    dp = torch.from_numpy(np.array(c.par_in)).to("cuda")
    dm = torch.from_numpy(np.array(c.masks).view(np.int64)).to("cuda")
    s = np.arange(k + r, dtype=np.uint64)
    addr = np.where(s < k, np.uint64(dd.data_ptr()) + (np.arange(G, dtype=np.uint64)[:, None] * np.uint64(k) + s) * np.uint64(P),
                    np.uint64(dp.data_ptr()) + (np.arange(G, dtype=np.uint64)[:, None] * np.uint64(r) + (s - np.uint64(k))) * np.uint64(P))
    addr[c.lost] = 0
    table = torch.from_numpy(addr.reshape(-1).view(np.int64)).to("cuda")
    outs = []
    with product_ctx(quicfec_mod) as ctx:
        for gather in (False, True):
            whole, out = guarded(torch, G * r * P, 0x5A)
            st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
            if gather:
                mo = torch.full((G,), -1, dtype=torch.int64, device="cuda")
                ctx.recover_gather_dev(table, G, k, r, P, out, st, mo)
            else:
                ctx.recover_dev(dd, dp, dm, G, k, r, P, out, st)
            ctx.synchronize()
            outs.append((whole.cpu().numpy(), st.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[1][0][GUARD:-GUARD].reshape(G, r, P), c.slots)
    assert np.array_equal(outs[1][1], c.status)
    assert np.array_equal(mo.cpu().numpy().view(np.uint64), c.masks)
    assert np.array_equal(dd.cpu().numpy(), c.broken) and np.array_equal(dp.cpu().numpy(), c.par_in)


# ------------------------------------------------------------------------------------------
# 3. Edge masks
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all_survive", "all_unrecoverable", "one_group", "three_groups"])
@pytest.mark.parametrize("k,r,P", [(10, 3, 1200), (20, 5, 300), (6, 3, 48)])
def test_edge_masks(quicfec_mod, oracle_mod, torch_cuda, k, r, P, kind):
    unrec = 1 | (((1 << r) - 1) << k)
    masks = {"all_survive": [0] * G_MAIN, "all_unrecoverable": [unrec] * G_MAIN,
             "one_group": [0b110 | (1 << k)], "three_groups": _planted(k, r)[:3]}[kind]
    c = make_case(oracle_mod, k, r, P, masks, SEED + len(masks) + k)
    if kind == "all_survive":
        assert (c.status == 0).all() and c.rows == 0
    if kind == "all_unrecoverable":
        assert (c.status == 1).all() and c.rows == 0
    if kind == "one_group":
        assert c.rows == 2 and c.status[0] == 0
    with product_ctx(quicfec_mod) as ctx:
        b = run_recover(torch_cuda, ctx, c, SEED + 5, kind)
    if c.rows == 0:                                                          # nothing at all was written
        assert (b.whole.cpu().numpy() == 0x5A).all()


# ------------------------------------------------------------------------------------------
# 4. Launch trace
# ------------------------------------------------------------------------------------------
def _launch_text(rec):
    if rec["form"] == "classify_gather":
        return "classify_gather"
    return f"{rec['form']} k={rec['k']} r={rec['r']} pol={rec['pol']} aux={rec['aux']}"


@pytest.mark.parametrize("k,r", SHAPES)
def test_recover_launches_only_the_gather_kernels(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """On the test library: a gather recover launches classify_gather and the recover_gather form
    of gather_form's table, nothing else -- no decode_* and no classify."""
    lib = quicfec_mod.load_test_library()
    with hooks_ctx(quicfec_mod) as ctx:
        for P in SIZES:
            c = main_case(oracle_mod, k, r, P)
            b = make_recover(torch_cuda, c, SEED + 11)
            quicfec_mod.launch_trace(lib)                                    # clear: fills and uploads are torch's
            launch_recover(ctx, b)
            ctx.synchronize()
            trace = quicfec_mod.launch_trace(lib)
            assert [_launch_text(t) for t in trace] == expected_launches(k, r, P), (k, r, P)
            assert {t["form"] for t in trace} == {"classify_gather", "recover_gather"}
            assert all(t["items"] == c.G and t["first_item"] == 0 and t["block"] == 256 for t in trace)
            assert trace[0]["grid"] == 1 and trace[1]["grid"] == (c.G + 3) // 4
            check_recover(b, "hooks")


@pytest.mark.parametrize("k,r", [(10, 3), (10, 1), (20, 5), (7, 3)])
def test_encode_launches_the_address_passes(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """A gather encode runs encode_v16 instantiated for absolute addresses (off = 3), no new form."""
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    P, G = 1200, 19
    c = make_case(oracle_mod, k, r, P, [0] * G, SEED + 13)
    dev, table = upload_arena(torch, *build_arena(c, SEED + 14, encode=True))
    par = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        quicfec_mod.launch_trace(lib)
        ctx.encode_gather_dev(table, G, k, r, P, par)
        ctx.synchronize()
        trace = quicfec_mod.launch_trace(lib)
    assert trace and all(t["form"] == "encode_v16" and t["off"] == 3 for t in trace)
    assert all(t["k"] == (10 if (k, r) == (10, 1) else 0) for t in trace)    # the compiled k=10 r=1, else runtime k
    assert np.array_equal(par.cpu().numpy(), c.par)


# ------------------------------------------------------------------------------------------
# 5. Caller stream
# ------------------------------------------------------------------------------------------
def test_queue_on_one_side_stream(quicfec_mod, oracle_mod, torch_cuda):
    """Eight gather recovers of differing G and shape queued on one non-blocking side stream,
    interleaved with contiguous recovers whose record offsets share the stream's workspace (it
    grows under queued work); one synchronise at the end, then every output is checked."""
    torch = torch_cuda
    queue = [(10, 3, 1200, 67), (6, 3, 48, 5), (20, 5, 300, 300), (16, 4, 700, 33), (10, 2, 255, 131), (4, 2, 2100, 3),
             (12, 6, 1025, 257), (10, 1, 17, 19)]
    gathers, contig = [], []
    for i, (k, r, P, G) in enumerate(queue):
        c = make_case(oracle_mod, k, r, P, perm_masks(k, r, G, SEED + i), SEED + 100 + i)
        gathers.append(make_recover(torch, c, SEED + 200 + i))
        # a contiguous slot recover of a record-addressed form (its classify writes the workspace too)
        d = SimpleNamespace(c=c, dd=torch.from_numpy(np.array(c.broken)).to("cuda"),
                            dp=torch.from_numpy(np.array(c.par_in)).to("cuda"),
                            dm=torch.from_numpy(np.array(c.masks).view(np.int64)).to("cuda"),
                            st=torch.full((G,), 7, dtype=torch.uint8, device="cuda"))
        d.whole, d.out = guarded(torch, G * r * P, 0x5A)
        contig.append(d)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        for b, d in zip(gathers, contig):
            launch_recover(ctx, b, stream.cuda_stream)
            ctx.recover_dev(d.dd, d.dp, d.dm, d.c.G, d.c.k, d.c.r, d.c.P, d.out, d.st, stream=stream.cuda_stream)
        torch.cuda.synchronize()
    for q, b, d in zip(queue, gathers, contig):
        check_recover(b, q)
        assert np.array_equal(d.whole.cpu().numpy()[GUARD:-GUARD].reshape(d.c.slots.shape), d.c.slots), q
        assert np.array_equal(d.st.cpu().numpy(), d.c.status), q


def test_free_with_gather_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """A gather recover (its record offsets in the stream's workspace, its records in the plan's
    codebook) and a gather encode queued on a side stream, and the context freed at once:
    fec_encoder_free drains them, so both outputs are complete and right after it."""
    torch = torch_cuda
    k, r, P = 10, 3, 1200
    c = make_case(oracle_mod, k, r, P, perm_masks(k, r, 4096, SEED + 31), SEED + 32)
    b = make_recover(torch, c, SEED + 33)
    edev, etable = upload_arena(torch, *build_arena(c, SEED + 34, encode=True))
    par = torch.full((c.G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    ctx = product_ctx(quicfec_mod)
    torch.cuda.synchronize()
    ctx.encode_gather_dev(etable, c.G, k, r, P, par, stream=stream.cuda_stream)
    launch_recover(ctx, b, stream.cuda_stream)
    ctx.close()
    assert stream.query()                                                    # the free drained the stream
    torch.cuda.synchronize()
    assert np.array_equal(par.cpu().numpy(), c.par)
    check_recover(b)


# ------------------------------------------------------------------------------------------
# 6. Encode gather
# ------------------------------------------------------------------------------------------
def make_encode(torch, c, seed):
    """Arena, table and pre-filled parity buffer of one gather encode of case c (no losses).  Everything
    is uploaded on torch's stream: synchronise before launching on a side stream."""
    arenas, where = build_arena(c, seed, encode=True)
    e = SimpleNamespace(c=c, arenas=arenas)
    e.dev, e.table = upload_arena(torch, arenas, where)
    e.whole, e.par = guarded(torch, c.G * c.r * c.P, 0x5A)
    return e


def launch_encode(ctx, e, stream=None):
    c = e.c
    ctx.encode_gather_dev(e.table, c.G, c.k, c.r, c.P, e.par, stream=stream)


def check_encode(e, what=""):
    c = e.c
    what = (what, c.k, c.r, c.P)
    got = e.whole.cpu().numpy()
    assert np.array_equal(got[GUARD:-GUARD], c.par), what
    assert (got[:GUARD] == 0x5A).all() and (got[-GUARD:] == 0x5A).all(), what
    for d, a in zip(e.dev, e.arenas):
        assert np.array_equal(d.cpu().numpy(), a), what


@pytest.mark.parametrize("k,r", [(10, 3), (4, 2), (20, 5), (7, 3)])
def test_encode_gather(quicfec_mod, oracle_mod, torch_cuda, k, r):
    """Packets scattered like the recover's shards; parity equals rs_encode, the arena is unchanged
    and the guard bytes around the parity buffer hold."""
    torch = torch_cuda
    G = 37
    with product_ctx(quicfec_mod) as ctx:
        for P in (16, 17, 1200, 2048, 8193):
            e = make_encode(torch, make_case(oracle_mod, k, r, P, [0] * G, SEED + P + k), SEED + P)
            launch_encode(ctx, e)
            ctx.synchronize()
            check_encode(e)


# ------------------------------------------------------------------------------------------
# 7. Errors: the documented code, a message, nothing launched, nothing written
# ------------------------------------------------------------------------------------------
REFUSALS = [("k + r = 65", 60, 5, 1200, False), ("P = 15", 10, 3, 15, False), ("NULL table", 10, 3, 1200, True)]


@pytest.mark.parametrize("call,what,k,r,P,null_table",
                         [("recover", *x) for x in REFUSALS] + [("encode", *x) for x in REFUSALS] +
                         # the codebook cap is the recover's alone: the encode serves k=16 r=16
                         [("recover", "sparse-plan shape", 16, 16, 1200, False)])
def test_refusals(quicfec_mod, torch_cuda, call, what, k, r, P, null_table):
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    G = 5
    arena = torch.full((G * (k + r) * (P + 40),), 0xEE, dtype=torch.uint8, device="cuda")
    addr = np.uint64(arena.data_ptr()) + np.arange(G * (k + r), dtype=np.uint64) * np.uint64(P + 40)   # all readable
    table = None if null_table else torch.from_numpy(addr.view(np.int64)).to("cuda")
    out = torch.full((G * r * P + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
    mo = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(lib)
        with pytest.raises(quicfec_mod.FecError) as ei:
            if call == "recover":
                ctx.recover_gather_dev(table, G, k, r, P, out, st, mo)
            else:
                ctx.encode_gather_dev(table, G, k, r, P, out)
        assert ei.value.code == (quicfec_mod.FEC_ERR_NULL if null_table else quicfec_mod.FEC_ERR_RANGE)
        assert quicfec_mod.last_error(lib) != "" and ctx.last_error() != ""
        ctx.synchronize()
        assert quicfec_mod.launch_trace(lib) == []
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (st == 7).all().item() and (mo == -1).all().item()
    assert (arena == 0xEE).all().item()


def test_zero_groups_and_null_output_are_refused(quicfec_mod, torch_cuda):
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    table = torch.zeros(13, dtype=torch.int64, device="cuda")
    out = torch.full((3 * 1200,), 0x5A, dtype=torch.uint8, device="cuda")
    with hooks_ctx(quicfec_mod) as ctx:
        quicfec_mod.launch_trace(lib)
        for fn, args in ((lib.fec_recover_gather_rs_dev, (0, 10, 3, 1200, out.data_ptr(), None, None, None)),
                         (lib.fec_encode_gather_rs_dev, (0, 10, 3, 1200, out.data_ptr(), None)),):
            assert fn(ctx.handle, table.data_ptr(), *args) == quicfec_mod.FEC_ERR_RANGE
            assert "num_groups" in ctx.last_error()
        assert lib.fec_recover_gather_rs_dev(ctx.handle, table.data_ptr(), 1, 10, 3, 1200, None, None, None,
                                             None) == quicfec_mod.FEC_ERR_NULL
        assert lib.fec_encode_gather_rs_dev(ctx.handle, table.data_ptr(), 1, 10, 3, 1200, None, None) == quicfec_mod.FEC_ERR_NULL
        assert "NULL" in ctx.last_error()
        assert quicfec_mod.launch_trace(lib) == []
    assert (out == 0x5A).all().item()


# ------------------------------------------------------------------------------------------
# 8. Random sweep
# ------------------------------------------------------------------------------------------
def test_random_sweep(quicfec_mod, oracle_mod, torch_cuda):
    """300 seeded cases over the eight shapes: P in 16..2100, G in 1..40, iid loss of 1%, 10% or 30%."""
    rng = np.random.default_rng(SEED + 77)
    rebuilt = unrec = 0
    with product_ctx(quicfec_mod) as ctx:
        for i in range(300):
            k, r = SHAPES[rng.integers(len(SHAPES))]
            P, G = int(rng.integers(16, 2101)), int(rng.integers(1, 41))
            loss = (0.01, 0.10, 0.30)[rng.integers(3)]
            c = make_case(oracle_mod, k, r, P, iid_masks(k, r, G, loss, rng), SEED + 1000 + i)
            run_recover(torch_cuda, ctx, c, SEED + 2000 + i, (i, loss))
            rebuilt += c.rows
            unrec += int(c.status.sum())
    assert rebuilt > 300 and unrec > 10                                      # the sweep rebuilt and refused
