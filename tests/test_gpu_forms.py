"""Which kernel form ran, and every compiled form at its edges.

Every other GPU test checks the bytes a call produced; a call that quietly fell back to another
correct form would pass them all.  These run through libfec_hip_test.so (gpu_ctx_hooks), whose
launchers record every kernel launch (csrc/fec_knobs.hpp LaunchRecord, quicfec.launch_trace), and
check two things per case: the bytes, statuses, row starts and totals against the oracle (seeded junk in
every shard and in every mask bit the erasure rule does not read -- tests/unread_shards.py -- 0x5A in
unwritten output, 7 in unwritten status), and the launches against the table below.

The table (expected_decode / expected_encode) is written from the dispatch rules as documented --
DESIGN.md §5b, include/fec_hip.h and the comments of the lists and rules in csrc/fec_forms.hpp
-- not from what the code was seen to do.  A trace that differs from it means either the
dispatch or its documentation changed.  The CPU tests at the end check the same table against
the deciding code itself (fec_forms.hpp, through tests/csrc/forms_dump.cpp) at every packet size.

Masks are permutation(k + r)[:0..r+1] per group (untouched and unrecoverable groups and lost
parity in every case) unless a test says otherwise.
"""
import itertools
import os
import subprocess
from functools import lru_cache
from math import comb
from pathlib import Path

import numpy as np
import pytest

import unread_shards as us

gpu = pytest.mark.gpu

SEED = 0x5EEDF000

# `pol` bits of a launch record (csrc/fec_forms.hpp)
NT_LOAD, NT_STORE, NO_BRANCH, LDS_TABS, COMPACT, COEF_BYTES, PAIR_MAC, STAGE = 1, 2, 4, 64, 1024, 2048, 4096, 8192

# Shapes with compiled decode forms (the lists of csrc/fec_forms.hpp, restated independently)
MASK_SHAPES = {(10, 3), (10, 1), (10, 2), (4, 2)}      # mask-addressed decode_fused + recover_runs
TILED_SHAPES = {(10, 3), (10, 1), (4, 2)}              # decode_tiled that auto takes (P <= 256)
WAVE_SHAPES = {(10, 3), (10, 1), (20, 5), (4, 2)}      # compile-time-k decode_wave
LAYOUTS = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2), (1, 3), (1, 4)]
FUSED_MAX_P = 2047                                     # the last packet size with a piece layout
SCAN = 8                                               # kDecodeScanGroups
SCAN_MAX_SHARE = 0.25                                  # kDecodeScanMaxShare

_FIELDS = ("k", "r", "nm", "nt", "off", "first", "pol", "direct", "scan", "aux")
# aux tells instantiations (or passes) apart only for these forms
_AUX_FORMS = {"encode_v16", "encode_bits", "decode_wave"}


def form(name, **kw):
    """An expected launch: the form and the template parameters that tell instantiations apart."""
    return (name,) + tuple(kw.get(f, -1) for f in _FIELDS)


def sig_of(rec):
    return (rec["form"],) + tuple(rec[f] if (f != "aux" or rec["form"] in _AUX_FORMS) else -1 for f in _FIELDS)


def layout(P):
    return P // 1024, (P % 1024 + 255) // 256


# ------------------------------------------------------------------------------------------
# The expected-form table
# ------------------------------------------------------------------------------------------
def packed_accepts(k, r, P):
    """include/fec_hip.h, fec_recover_batch_rs_dev_packed: mask-addressed shapes, 256 < P < 2048,
    and below that where the shape has no tiled form (k=10 r=2, 16 <= P <= 256)."""
    return (k, r) in MASK_SHAPES and 16 <= P <= FUSED_MAX_P and (P > 256 or (k, r) not in TILED_SHAPES)


def expected_decode(api, k, r, P, scan=False, runs=False):
    """Launches of one decode call, in order; None = refused with FEC_ERR_RANGE, nothing launched.
    api: in_place (fec_decode_batch_rs_dev), slots (fec_recover_batch_rs_dev), packed
    (fec_recover_batch_rs_dev_packed).  scan: QUICFEC_DECODE_SCAN=8 (or a sparse loss share);
    runs: QUICFEC_PACKED_RUNS=1."""
    compact = 0 if api == "in_place" else COMPACT
    nm, nt = layout(P)
    classify = [form("classify")]
    if api == "packed":
        if not packed_accepts(k, r, P):
            return None
        # sparse loss (the scan share) or the switch: one launch, recover_runs
        if runs or scan:
            return [form("recover_runs", k=k, r=r, nm=nm, nt=nt, pol=NT_LOAD | NT_STORE)]
        prefix = [form("rows_block_sums"), form("rows_write", direct=1)]
    else:
        prefix = []
    if P < 16:
        return classify + [form("decode_bytes", k=0, pol=compact)]
    passes = (r + 7) // 8
    runtime_wave = [form("decode_wave", k=0, r=8, pol=NT_STORE | NO_BRANCH | compact, aux=8 * p) for p in range(passes)]
    if (k, r) == (20, 5):
        # record-addressed, tables through LDS from the compact codebook, wherever a layout exists
        if P <= FUSED_MAX_P:
            return classify + [form("decode_fused", k=20, r=5, nm=nm, nt=nt, direct=0, scan=0,
                                    pol=NT_STORE | NT_LOAD | LDS_TABS | COEF_BYTES | compact)]
        return classify + ([form("decode_wave", k=20, r=5, pol=NT_STORE, aux=0)] if not compact else runtime_wave)
    if (k, r) in MASK_SHAPES:
        if P <= 256 and (k, r) in TILED_SHAPES:
            return classify + [form("decode_tiled", k=k, r=r, pol=NT_STORE | compact)]
        if P <= FUSED_MAX_P and (P > 256 or compact):
            # mask-addressed: one launch, classifies inline; k=10 r=3 also in the scan form
            s = SCAN if (scan and (k, r) == (10, 3)) else 0
            return prefix + [form("decode_fused", k=k, r=r, nm=nm, nt=nt, direct=1, scan=s,
                                  pol=NT_STORE | NT_LOAD | compact)]
        if P <= 256:
            # known slow path: k=10 r=2 in place has no tiled form and the in-place
            # route does not try the mask-addressed (0,1) form: one wave per group
            return classify + runtime_wave
        if compact or (k, r) not in WAVE_SHAPES:
            return classify + runtime_wave
        return classify + [form("decode_wave", k=k, r=r, pol=NT_STORE, aux=0)]
    # runtime k: one wave per group at every size (P <= 256 in place: the same known slow path)
    return classify + runtime_wave


def pick_tile(cpp, k, P):
    """Groups per workgroup of the tiled mapping (fec_forms.hpp pick_tile: fewest idle lanes of
    whole waves, +0.05 when the tile's bytes are no multiple of 128, +0.02 below 256 lanes;
    0 = flat, more than 512 columns per packet)."""
    if cpp == 0 or cpp > 512:
        return 0
    best, best_score = 1, 1e9
    for t in range(1, 512 // cpp + 1):
        lanes = t * cpp
        bs = (lanes + 63) // 64 * 64
        score = (bs - lanes) / bs + (0.05 if (t * k * P) % 128 else 0.0) + (0.02 if bs < 256 else 0.0)
        if score < best_score - 1e-9:
            best, best_score = t, score
    return best


def expected_encode(k, r, P, off=0):
    """Launches of one encode call (launch_encode's rules), with the mapping (tile or flat).
    off: 0 contiguous, 1 legacy u32 offsets, 2 u64 offsets."""
    if P < 16:
        return [(form("encode_bytes", k=0, off=off), None)]
    cpp = (P + 15) // 16
    tile = pick_tile(cpp, k, P)
    mapping = "tile" if tile else "flat"

    def staged(groups_per_block):  # use_stage_rows: P % 16 == 0 and the window fits 64 KiB
        return STAGE if (P % 16 == 0 and groups_per_block * r * P <= 64 * 1024) else 0

    if off == 0:
        if (k, r) == (20, 5) and P <= 8192:   # bit-sliced for r >= 4 while a workgroup holds whole groups
            return [(form("encode_bits", k=20, r=5, off=0, pol=NT_STORE | staged(2 * tile), aux=4), mapping)]
        if (k, r) in ((10, 3), (10, 2)):
            return [(form("encode_v16", k=k, r=r, off=0, first=1, pol=NT_STORE | PAIR_MAC | staged(tile), aux=0), mapping)]
        if (k, r) == (20, 5):
            return [(form("encode_v16", k=20, r=5, off=0, first=1, pol=NT_STORE | PAIR_MAC, aux=0), mapping)]
        if (k, r) in ((10, 1), (4, 2)):       # the XOR row and k=4 keep their direct stores
            return [(form("encode_v16", k=k, r=r, off=0, first=1, pol=NT_STORE, aux=0), mapping)]
    elif off == 1 and (k, r) == (10, 1):
        return [(form("encode_v16", k=10, r=1, off=1, first=1, pol=NT_STORE, aux=0), mapping)]
    # runtime k: one pass per 8 rows, the first owns the XOR row
    return [(form("encode_v16", k=0, r=min(8, r - row0), off=off, first=int(row0 == 0), pol=NT_STORE, aux=row0), mapping)
            for row0 in range(0, r, 8)]


# ------------------------------------------------------------------------------------------
# Trace checks
# ------------------------------------------------------------------------------------------
def _groups_per_block(rec):
    f = rec["form"]
    if f in ("decode_wave",):
        return 4
    if f == "decode_fused":
        return 4 * rec["scan"] if rec["scan"] > 0 else 4
    if f in ("decode_tiled", "recover_runs"):
        return rec["tile"]
    if f in ("encode_v16", "encode_bits") and rec["tile"] > 0:
        return rec["tile"] * (2 if f == "encode_bits" else 1)
    if f == "classify":
        return 256
    if f in ("rows_block_sums", "rows_write"):
        return 1024
    return None


def collapse(trace, G):
    """The trace as runs of launches of one instantiation (one run = the chunks of one pass),
    each run checked to cover groups [0, G) exactly once in increasing order with grids that fit
    their chunks.  Returns [(sig, mapping, launches)]."""
    runs = []
    for rec in trace:
        s = sig_of(rec)
        per = _groups_per_block(rec)
        if per:
            assert rec["grid"] == (rec["items"] + per - 1) // per, rec
        assert rec["items"] > 0 and rec["grid"] > 0, rec
        if runs and runs[-1][0] == s and runs[-1][3] < G:
            assert rec["first_item"] == runs[-1][3], ("chunks out of order or overlapping", rec)
            runs[-1][3] += rec["items"]
            runs[-1][2] += 1
        else:
            assert rec["first_item"] == 0, rec
            mapping = ("tile" if rec["tile"] > 0 else "flat") if rec["form"] in ("encode_v16", "encode_bits") else None
            runs.append([s, mapping, 1, rec["items"]])
    for s, _, _, covered in runs:
        assert covered == G, (s, covered, G)
    return [(s, m, n) for s, m, n, _ in runs]


def assert_forms(trace, G, expected):
    got = collapse(trace, G)
    assert [g[0] for g in got] == list(expected), (
        "launched:\n  " + "\n  ".join(map(str, (g[0] for g in got))) + "\nexpected:\n  " + "\n  ".join(map(str, expected)))
    return got


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    import os
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases against the oracle
# ------------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.array(a)).to("cuda")      # a copy: the case's arrays are read-only


def perm_masks(k, r, G, seed):
    rng = np.random.default_rng(seed)
    masks = np.zeros(G, dtype=np.uint64)
    for g in range(G):
        for s in rng.permutation(k + r)[: rng.integers(0, r + 2)]:
            masks[g] |= np.uint64(1) << np.uint64(int(s))
    return masks


class Case:
    """One batch and everything the oracle says about it, computed once and never modified."""

    def __init__(self, oracle, k, r, P, masks, need_unchosen_alive=True, need_full=True, need_short=True,
                 need_untouched=True, masks_in=None):
        G = len(masks)
        self.k, self.r, self.P, self.G, self.masks = k, r, P, G, masks
        # what a decode is given as masks: junk in the bits at and above k + r, which the rule ignores
        # (masks_in given: the caller's own pattern up there)
        if masks_in is None:
            masks_in = us.high_bits(masks, k, r, SEED + k * 31 + r * 7 + P, need_full=need_full, need_short=need_short,
                                    need_untouched=need_untouched)
        low = np.uint64((1 << (k + r)) - 1)
        assert masks_in.dtype == np.uint64 and np.array_equal(masks_in & low, masks)
        self.masks_in = masks_in
        data = oracle.splitmix_bytes(G * k * P, SEED + k * 31 + r * 7 + P)
        self.par = oracle.rs_encode(data, G, k, r, P, nthreads=8)          # true: what an encode must give
        lost = us.roles(masks, k, r).lost_d
        # what a decode is given: junk in every lost data shard and every parity row the rule does
        # not read (a lost row below the highest chosen one needs r > 1)
        self.broken, self.par_in = us.inputs(data, self.par, masks, k, r, P, SEED + k * 31 + r * 7 + P,
                                             need_lost_below=r > 1, need_unchosen_alive=need_unchosen_alive)
        ref = self.broken.copy()
        _, self.status = oracle.rs_decode(ref, self.par_in, masks_in, G, k, r, P, nthreads=8)
        self.ref = ref                                    # in-place result
        clean = self.broken.copy()                        # the oracle itself ignores those bits
        _, clean_status = oracle.rs_decode(clean, self.par_in, masks, G, k, r, P, nthreads=8)
        assert np.array_equal(clean, ref) and np.array_equal(clean_status, self.status)
        ok = self.status == 0
        # the oracle's rebuilt packets are the original ones
        assert np.array_equal(ref.reshape(G, k, P)[ok], data.reshape(G, k, P)[ok])
        gi, ji = np.nonzero(lost & ok[:, None])           # (g, j ascending)
        mi = (np.cumsum(lost, axis=1) - 1)[gi, ji]
        self.rows = ref.reshape(G, k, P)[gi, ji]          # packed rows
        self.slots = np.full((G, r, P), 0x5A, dtype=np.uint8)
        self.slots[gi, mi] = self.rows
        per_group = (lost & ok[:, None]).sum(axis=1)
        self.row_start = np.concatenate([[0], np.cumsum(per_group)[:-1]]).astype(np.uint32)
        for a in (self.par, self.par_in, self.broken, self.ref, self.status, self.rows, self.slots, self.row_start, self.masks,
                  self.masks_in):
            a.setflags(write=False)


@lru_cache(maxsize=2)
def _perm_case(oracle, k, r, P, G):
    return Case(oracle, k, r, P, perm_masks(k, r, G, k * 1000 + r * 100 + P))


def run_decode(ctx, quicfec, torch, c, api, expected):
    """One decode call of `api` on case c: bytes against the oracle, launches against `expected`
    (None: the call must be refused with FEC_ERR_RANGE and touch nothing)."""
    k, r, P, G = c.k, c.r, c.P, c.G
    dd, dp, dm = _dev(torch, c.broken), _dev(torch, c.par_in), _dev(torch, c.masks_in.view(np.int64))
    st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
    ctx.synchronize()
    quicfec.launch_trace(ctx.lib)                          # clear
    if api == "in_place":
        ctx.decode_dev(dd, dp, dm, G, k, r, P, st)
        ctx.synchronize()
        trace = quicfec.launch_trace(ctx.lib)
        assert np.array_equal(dd.cpu().numpy(), c.ref), us.mismatch(c.masks, k, r, dd.cpu().numpy(), c.ref)
    elif api == "slots":
        out = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
        ctx.recover_dev(dd, dp, dm, G, k, r, P, out, st)
        ctx.synchronize()
        trace = quicfec.launch_trace(ctx.lib)
        assert np.array_equal(out.cpu().numpy().reshape(G, r, P), c.slots), us.mismatch(c.masks, k, r, out.cpu().numpy(), c.slots)
        assert np.array_equal(dd.cpu().numpy(), c.broken)          # data untouched
    else:
        out = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
        rs = torch.full((G,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -5, dtype=torch.int64, device="cuda")
        if expected is None:
            with pytest.raises(quicfec.FecError) as ei:
                ctx.recover_packed_dev(dd, dp, dm, G, k, r, P, out, rs, tot, st)
            assert ei.value.code == quicfec.FEC_ERR_RANGE
            ctx.synchronize()
            assert quicfec.launch_trace(ctx.lib) == []             # refused before anything ran
            assert bool((out == 0x5A).all()) and bool((rs == 0x3C3C3C3C).all()) and int(tot.item()) == -5
            assert bool((st == 7).all())
            assert np.array_equal(dd.cpu().numpy(), c.broken) and np.array_equal(dp.cpu().numpy(), c.par_in)
            assert np.array_equal(dm.cpu().numpy().view(np.uint64), c.masks_in)
            return []
        ctx.recover_packed_dev(dd, dp, dm, G, k, r, P, out, rs, tot, st)
        ctx.synchronize()
        trace = quicfec.launch_trace(ctx.lib)
        n = len(c.rows)
        assert int(tot.item()) == n
        assert np.array_equal(rs.cpu().numpy().view(np.uint32), c.row_start)
        o = out.cpu().numpy().reshape(G * r, P)
        assert np.array_equal(o[:n], c.rows)
        assert (o[n:] == 0x5A).all()                               # nothing past the last row
        assert np.array_equal(dd.cpu().numpy(), c.broken)
    assert np.array_equal(st.cpu().numpy(), c.status), us.mismatch(c.masks, k, r, st.cpu().numpy(), c.status)
    assert np.array_equal(dp.cpu().numpy(), c.par_in)              # parity only read, junk rows included
    assert np.array_equal(dm.cpu().numpy().view(np.uint64), c.masks_in)   # masks only read, junk bits included
    return assert_forms(trace, G, expected)


# ---- a. decode matrix -----------------------------------------------------------------------
# both ends of every piece layout, 15 (byte kernel), 2048 and 2064 (past the fused layouts)
DECODE_P = [15, 16, 256, 257, 512, 513, 768, 769, 1023, 1024, 1025, 1280, 1281, 1536, 1537, 1792, 1793, 2047,
            2048, 2064]
DECODE_SHAPES = [(10, 3), (10, 2), (10, 1), (4, 2), (20, 5)]


def _apis(k, r):
    """(name, api, switches) of the decode matrix: every API, packed also in one launch, and
    k=10 r=3 (the shape with a scan form) each API again with the scan switch."""
    apis = [("in_place", "in_place", {}), ("slots", "slots", {}), ("packed", "packed", {}),
            ("packed_runs", "packed", {"QUICFEC_PACKED_RUNS": "1"})]
    if (k, r) == (10, 3):
        apis += [(n + "+scan", a, dict(e, QUICFEC_DECODE_SCAN="8")) for n, a, e in list(apis)]
    return apis


@gpu
@pytest.mark.parametrize("P", DECODE_P)
@pytest.mark.parametrize("k,r", DECODE_SHAPES)
def test_decode_matrix(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P):
    """Every compiled decode shape at both ends of every piece layout, through every API: bytes
    equal the oracle's and the launches are the documented form's.  G = 1031: more than one
    workgroup of every form (4 or 32 groups per workgroup, 512 per recover_runs tile) and a
    partial last one."""
    G = 261 if (k, r) == (20, 5) else 1031
    c = _perm_case(oracle_mod, k, r, P, G)
    for name, api, env in _apis(k, r):
        with monkeypatch.context() as mp:
            for key, val in env.items():
                mp.setenv(key, val)
            exp = expected_decode(api, k, r, P, scan="QUICFEC_DECODE_SCAN" in env, runs="QUICFEC_PACKED_RUNS" in env)
            got = run_decode(gpu_ctx_hooks, quicfec_mod, torch_cuda, c, api, exp)
            assert all(n == 1 for _, _, n in got), (name, got)     # no chunking at this size


@gpu
@pytest.mark.parametrize("P", [48, 272, 2064])
def test_decode_runtime_k(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, P):
    """A shape without compiled forms (k=6 r=3): the runtime-k wave kernel at every size, in
    place and in slots; the packed call refuses it."""
    k, r, G = 6, 3, 261
    c = _perm_case(oracle_mod, k, r, P, G)
    for api in ("in_place", "slots", "packed"):
        run_decode(gpu_ctx_hooks, quicfec_mod, torch_cuda, c, api, expected_decode(api, k, r, P))


@gpu
@pytest.mark.parametrize("loss", [0.01, 0.30])
def test_host_decode_scan_choice(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, loss):
    """A small host-pointer decode measures the share of groups to rebuild from the masks and
    takes the scan form (8 groups per wave) below kDecodeScanMaxShare, else one wave per group."""
    k, r, P, G = 10, 3, 1200, 131          # 2 MB: under the zero-copy limit of pageable buffers
    rng = np.random.default_rng(int(loss * 100))
    w = np.left_shift(np.uint64(1), np.arange(k + r, dtype=np.uint64))
    masks = ((rng.random((G, k + r)) < loss) * w).sum(axis=1, dtype=np.uint64)
    masks[0] = 1 | 1 << k                  # planted: row 0 lost, row 1 chosen, row 2 survives unread
    # 1 % iid loss over 131 groups leaves too few groups that use every surviving row, or are one short
    c = Case(oracle_mod, k, r, P, masks, need_full=loss > 0.1, need_short=loss > 0.1)
    lost = (masks & np.uint64((1 << k) - 1)) != 0
    share = float((lost & (c.status == 0)).sum()) / G
    assert share > 0 and (share < SCAN_MAX_SHARE) == (loss < 0.1), share   # the two cases sit on either side
    ctx = gpu_ctx_hooks
    data, st = c.broken.copy(), np.full(G, 7, dtype=np.uint8)
    quicfec_mod.launch_trace(ctx.lib)
    par_in = c.par_in.copy()
    masks_in = c.masks_in.copy()
    bad = ctx.decode(data, par_in, masks_in, k, r, P, st)   # the loss share must not count the junk bits
    trace = quicfec_mod.launch_trace(ctx.lib)
    assert np.array_equal(par_in, c.par_in) and np.array_equal(masks_in, c.masks_in)
    assert np.array_equal(data, c.ref) and np.array_equal(st, c.status) and bad == int((c.status != 0).sum())
    assert_forms(trace, G, expected_decode("in_place", k, r, P, scan=share < SCAN_MAX_SHARE))


# ---- b. packed boundaries ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k,r", sorted(MASK_SHAPES))
def test_packed_bounds(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r):
    """The packed call's documented range (include/fec_hip.h): 2047 B is the last size accepted,
    2048 is refused with FEC_ERR_RANGE and nothing written; at 16..256 B it is accepted exactly
    for the shape without a tiled form (k=10 r=2), in both of its forms."""
    assert packed_accepts(k, r, 2047) and not packed_accepts(k, r, 2048)
    assert packed_accepts(k, r, 256) == ((k, r) == (10, 2))
    G = 1031
    for P in (16, 200, 256, 2047, 2048):
        c = _perm_case(oracle_mod, k, r, P, G)
        for runs in (False, True):
            with monkeypatch.context() as mp:
                if runs:
                    mp.setenv("QUICFEC_PACKED_RUNS", "1")
                run_decode(gpu_ctx_hooks, quicfec_mod, torch_cuda, c, "packed", expected_decode("packed", k, r, P, runs=runs))


# ---- c. encode matrix ---------------------------------------------------------------------------
ENCODE_P = [15, 16, 1200, 1201, 8192, 8208]
ENCODE_SHAPES = [(10, 3), (10, 2), (10, 1), (4, 2), (20, 5), (12, 9)]


def run_encode(ctx, quicfec, torch, oracle, k, r, P, G, seed):
    data = oracle.splitmix_bytes(G * k * P, seed)
    exp = oracle.rs_encode(data, G, k, r, P, nthreads=8).reshape(-1)
    dd = _dev(torch, data)
    guard = 67
    dp = torch.full((G * r * P + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.synchronize()
    quicfec.launch_trace(ctx.lib)
    ctx.encode_dev(dd, G, k, r, P, dp[guard:guard + G * r * P])
    ctx.synchronize()
    trace = quicfec.launch_trace(ctx.lib)
    got = dp.cpu().numpy()
    assert np.array_equal(got[guard:guard + G * r * P], exp)
    assert (got[:guard] == 0xA5).all() and (got[guard + G * r * P:] == 0xA5).all()
    return trace


@gpu
@pytest.mark.parametrize("P", ENCODE_P)
@pytest.mark.parametrize("k,r", ENCODE_SHAPES)
def test_encode_matrix(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """Contiguous encodes with no switch set: parity equals the oracle's and the launch is the
    form launch_encode documents -- the tables for k=10 r=3, the bit-sliced form for k=20 r=5 up
    to 8192 B (what test_bits_is_the_default_for_c4 claims), rows staged where the window fits,
    one pass per 8 rows for a runtime k, the byte kernel below 16 B, the flat mapping past 8192 B."""
    G = 53
    trace = run_encode(gpu_ctx_hooks, quicfec_mod, torch_cuda, oracle_mod, k, r, P, G, SEED + 131 * P + k)
    exp = expected_encode(k, r, P)
    got = collapse(trace, G)
    assert [(s, m) for s, m, _ in got] == [(s, m) for s, m in exp], (got, exp)
    if (k, r) == (20, 5) and 16 <= P <= 8192:
        assert got[0][0][0] == "encode_bits"
    if (k, r) == (10, 3) and P >= 16:
        assert got[0][0][0] == "encode_v16"


@gpu
def test_encode_gathered_offsets(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda):
    """Gathered packets: u64 offsets run the runtime-k kernel's OFF=2 instantiation, the legacy
    call (u32 offsets, k = 10, one XOR row) its own compile-time one (OFF=1)."""
    torch, ctx = torch_cuda, gpu_ctx_hooks
    k, r, P, G = 7, 3, 1201, 53
    rng = np.random.default_rng(99)
    slab = oracle_mod.splitmix_bytes(G * k * P + 4096, SEED + 5)
    order = rng.permutation(G * k)
    offs = (order.astype(np.uint64) * np.uint64(P) + np.uint64(13))      # every packet at an odd address
    data = np.concatenate([slab[int(o):int(o) + P] for o in offs])
    exp = oracle_mod.rs_encode(data, G, k, r, P, nthreads=8).reshape(-1)
    ds, do = _dev(torch, slab), _dev(torch, offs.view(np.int64))
    dp = torch.full((G * r * P,), 0xA5, dtype=torch.uint8, device="cuda")
    ctx.synchronize()
    quicfec_mod.launch_trace(ctx.lib)
    ctx.encode(ds, k, r, P, dp, num_groups=G, offsets=do)
    trace = quicfec_mod.launch_trace(ctx.lib)
    assert np.array_equal(dp.cpu().numpy(), exp)
    assert [(s, m) for s, m, _ in collapse(trace, G)] == expected_encode(k, r, P, off=2)
    # the legacy call, device-resident slab / offsets / output
    k, P = 10, 1200
    order = rng.permutation(G * k)
    offs32 = (order * P + 16).astype(np.uint32)
    slab = oracle_mod.splitmix_bytes(G * k * P + 4096, SEED + 6)
    rc, exp = oracle_mod.encode_batch_legacy(slab, offs32, G, P)
    assert rc == 0
    ds, do = _dev(torch, slab), _dev(torch, offs32.view(np.int32))
    dp = torch.full((G * P,), 0xA5, dtype=torch.uint8, device="cuda")
    quicfec_mod.launch_trace(ctx.lib)
    assert ctx.encode_batch_legacy(ds, do, G, P, dp) == 0
    trace = quicfec_mod.launch_trace(ctx.lib)
    assert np.array_equal(dp.cpu().numpy(), exp)
    assert [(s, m) for s, m, _ in collapse(trace, G)] == expected_encode(10, 1, P, off=1)


# ---- d. split launches --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k,r,P,G,form_name,chunks", [
    (10, 3, 1200, 261, "encode_v16", [66, 66, 66, 63]),      # tiled: 75 columns per group, 5000 // 75 groups
    (10, 3, 8208, 53, "encode_v16", [9, 9, 9, 9, 9, 8]),     # flat: 513 columns per group
    (5, 2, 15, 1031, "encode_bytes", [333, 333, 333, 32]),   # one lane per byte
])
def test_split_encode_launches(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P, G, form_name,
                               chunks):
    """QUICFEC_MAX_LAUNCH_THREADS lowers the 2^30 work items per launch, so the encode loops that
    split past it run: the chunks cover the groups once, in order, and the parity is the oracle's."""
    monkeypatch.setenv("QUICFEC_MAX_LAUNCH_THREADS", "5000")
    trace = run_encode(gpu_ctx_hooks, quicfec_mod, torch_cuda, oracle_mod, k, r, P, G, SEED + 7 * P + G)
    assert [t["form"] for t in trace] == [form_name] * len(chunks)
    assert [t["items"] for t in trace] == chunks
    got = collapse(trace, G)
    assert [(s, m) for s, m, _ in got] == expected_encode(k, r, P) and got[0][2] == len(chunks)


@gpu
@pytest.mark.parametrize("k,r,P,api", [(10, 3, 64, "in_place"), (10, 3, 64, "slots"), (10, 3, 15, "in_place"),
                                       (10, 3, 15, "slots")])
def test_split_decode_launches(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P, api):
    """The same switch on the decode side: classify (400 groups per launch), the tiled decode
    (whole workgroups per launch) and the byte kernel (400 // 15 groups per launch)."""
    G = 1031
    monkeypatch.setenv("QUICFEC_MAX_LAUNCH_THREADS", "400")
    c = _perm_case(oracle_mod, k, r, P, G)
    got = run_decode(gpu_ctx_hooks, quicfec_mod, torch_cuda, c, api, expected_decode(api, k, r, P))
    assert got[0][0][0] == "classify" and got[0][2] == 3            # 400 + 400 + 231
    if P == 15:
        assert got[1][0][0] == "decode_bytes" and got[1][2] == (G + 25) // 26
    else:
        tile = pick_tile(4, k, P)
        per_launch = max(1, 400 // ((tile * 4 + 63) // 64 * 64)) * tile
        assert got[1][0][0] == "decode_tiled" and got[1][2] == (G + per_launch - 1) // per_launch >= 3
        assert G % per_launch != 0                                     # a partial last chunk


@gpu
@pytest.mark.parametrize("k,r,P,api", [(6, 3, 1200, "in_place"), (12, 9, 64, "in_place"), (10, 3, 2064, "in_place"),
                                       (10, 3, 2064, "slots")])
def test_split_wave_launches(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P, api):
    """QUICFEC_MAX_WAVE_BLOCKS=7 (28 groups per launch) on the wave-per-group kernel, which
    test_chunked_launches reaches only through decode_fused: runtime k, r > 8 (two passes, each in
    chunks) and the compile-time-k kernel, in place and in slots."""
    G = 261
    monkeypatch.setenv("QUICFEC_MAX_WAVE_BLOCKS", "7")
    c = _perm_case(oracle_mod, k, r, P, G)
    got = run_decode(gpu_ctx_hooks, quicfec_mod, torch_cuda, c, api, expected_decode(api, k, r, P))
    waves = [g for g in got if g[0][0] == "decode_wave"]
    assert len(waves) == (r + 7) // 8 and all(n == (G + 27) // 28 for _, _, n in waves), got


@gpu
def test_split_fill_and_copy_launches(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, monkeypatch):
    """The fill and copy kernels' loops under the same switch: 16-B words in chunks of 5000, then
    the tail bytes; the bytes are the oracle's splitmix stream and the copy is exact."""
    torch, ctx = torch_cuda, gpu_ctx_hooks
    monkeypatch.setenv("QUICFEC_MAX_LAUNCH_THREADS", "5000")
    words, tail, seed, off = 12_345, 7, SEED + 77, 24
    n = words * 16 + tail
    buf = torch.full((n + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.synchronize()
    quicfec_mod.launch_trace(ctx.lib)
    ctx.fill_random_dev(buf[16:16 + n], n, seed, off)
    ctx.synchronize()
    trace = quicfec_mod.launch_trace(ctx.lib)
    got = buf.cpu().numpy()
    assert np.array_equal(got[16:16 + n], oracle_mod.splitmix_bytes(n, seed, off))
    assert (got[:16] == 0x5A).all() and (got[16 + n:] == 0x5A).all()
    assert [(t["form"], t["aux"], t["first_item"], t["items"]) for t in trace] == \
        [("fill", 16, 0, 5000), ("fill", 16, 5000, 5000), ("fill", 16, 10000, 2345), ("fill", 1, words * 16, tail)]
    dst = torch.full((words * 16 + 32,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.copy_dev(buf[16:16 + words * 16], dst[16:16 + words * 16], words * 16)
    ctx.synchronize()
    trace = quicfec_mod.launch_trace(ctx.lib)
    out = dst.cpu().numpy()
    assert np.array_equal(out[16:-16], got[16:16 + words * 16]) and (out[:16] == 0x5A).all() and (out[-16:] == 0x5A).all()
    assert [(t["form"], t["first_item"], t["items"]) for t in trace] == \
        [("copy", 0, 5000), ("copy", 5000, 5000), ("copy", 10000, 2345)]


# ---- e. every codebook record once, and every mask ----------------------------------------------
def record_masks(k, r, seed):
    """One mask per record (E, R) of the dense codebook: the data bits are E; the parity rows
    below max(R) that are not in R are lost, so the decoder's rows (the first |E| alive ones) are
    exactly R; rows above max(R) are lost or alive by a seeded coin.  Shuffled."""
    rng = np.random.default_rng(seed)
    masks = []
    for e in range(1, min(k, r) + 1):
        for E in itertools.combinations(range(k), e):
            mE = sum(1 << j for j in E)
            for R in itertools.combinations(range(r), e):
                m = mE
                for i in range(r):
                    if (i < R[-1] and i not in R) or (i > R[-1] and rng.random() < 0.5):
                        m |= 1 << (k + i)
                masks.append(m)
    masks = np.array(masks, dtype=np.uint64)
    rng.shuffle(masks)
    assert len(masks) == sum(comb(k, e) * comb(r, e) for e in range(1, min(k, r) + 1))
    return masks


@gpu
@pytest.mark.parametrize("P", [48, 272])
@pytest.mark.parametrize("k,r,records", [(20, 5, 53_129), (10, 3, 285), (10, 2, 65), (10, 1, 10), (4, 2, 14), (7, 4, 329)])
def test_every_codebook_record(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, k, r, records, P):
    """Every (erased set, parity rows) record of the dense codebook decodes once, in place and
    into slots.  Every group is recoverable, so every status is 0: a wrong rank would otherwise
    hide as an 'unrecoverable' group."""
    masks = record_masks(k, r, k * 100 + r)
    assert len(masks) == records
    # every group rebuilds: with one parity row none survives unchosen, and no group is one row short or untouched
    c = Case(oracle_mod, k, r, P, masks, need_unchosen_alive=r > 1, need_short=False, need_untouched=False)
    assert (c.status == 0).all() and len(c.rows) == int(sum(bin(int(m) & ((1 << k) - 1)).count("1") for m in masks))
    for api in ("in_place", "slots"):
        run_decode(gpu_ctx_hooks, quicfec_mod, torch_cuda, c, api, expected_decode(api, k, r, P))


@gpu
@pytest.mark.parametrize("k,r", [(10, 3), (10, 2), (10, 1), (4, 2)])
def test_every_mask(gpu_ctx_hooks, quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r):
    """All 2^(k+r) erasure masks, shuffled, at 272 B through every API and form: statuses, rows,
    row starts and the total equal the oracle's.  Four passes: the bits at and above k + r clean,
    all set, only bit k + r set, and the helper's draw."""
    P = 272
    masks = np.arange(1 << (k + r), dtype=np.uint64)
    np.random.default_rng(k + r).shuffle(masks)
    every = np.uint64(((1 << (64 - k - r)) - 1) << (k + r))
    cases = [Case(oracle_mod, k, r, P, masks, masks_in=masks_in)
             for masks_in in (masks.copy(), masks | every, masks | np.uint64(1 << (k + r)))] + [Case(oracle_mod, k, r, P, masks)]
    for (name, api, env), c in itertools.product([("in_place", "in_place", {}), ("slots", "slots", {}), ("packed", "packed", {}),
                           ("packed_runs", "packed", {"QUICFEC_PACKED_RUNS": "1"}),
                           ("scan", "in_place", {"QUICFEC_DECODE_SCAN": "8"}),
                           ("slots+scan", "slots", {"QUICFEC_DECODE_SCAN": "8"})], cases):
        with monkeypatch.context() as mp:
            for key, val in env.items():
                mp.setenv(key, val)
            exp = expected_decode(api, k, r, P, scan="QUICFEC_DECODE_SCAN" in env, runs="QUICFEC_PACKED_RUNS" in env)
            run_decode(gpu_ctx_hooks, quicfec_mod, torch_cuda, c, api, exp)


# ---- the table against the list of compiled instantiations (no GPU) -----------------------------
CSRC = Path(__file__).resolve().parent.parent / "quic-test_amd" / "csrc"


@pytest.fixture(scope="module")
def forms_dump(tmp_path_factory):
    """tests/csrc/forms_dump.cpp, which asks csrc/fec_forms.hpp -- the code that decides the forms
    -- with no GPU: run(*args, **env) -> its output lines.  Built twice like the libraries: plain
    (every switch at its default) and with -DQUICFEC_TEST_HOOKS (switches read from the
    environment); a call with env runs the latter."""
    d = tmp_path_factory.mktemp("forms_dump")
    for exe, flags in (("plain", []), ("hooks", ["-DQUICFEC_TEST_HOOKS"])):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", *flags, "-I", str(CSRC),
                        str(Path(__file__).parent / "csrc" / "forms_dump.cpp"), str(CSRC / "fec_knobs.cpp"),
                        "-o", str(d / exe)], check=True)

    def run(*args, **env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("QUICFEC_")}
        out = subprocess.run([str(d / ("hooks" if env else "plain")), *args], capture_output=True, text=True,
                             check=True, timeout=120, env=dict(clean, **env))
        return out.stdout.splitlines()
    return run


def _parse_launch(text):
    """'decode_fused k=10 r=3 ...' -> a launch record like quicfec.launch_trace's (-1 = not set)."""
    name, *fields = text.split()
    rec = dict({f: -1 for f in _FIELDS + ("tile",)}, form=name)
    rec.update((key, int(val)) for key, val in (f.split("=") for f in fields))
    return rec


def compiled_instantiations(forms_dump):
    """The kernel instantiations libfec_hip.so carries: the decode forms and recover_runs as
    forms_dump --compiled expands them from the lists of csrc/fec_forms.hpp that launch_decode and
    launch_recover_runs dispatch on; the encodes and the rest from the lists in fec_forms.hpp /
    fec_encode.hip (QFEC_ENCODE_*_FORMS, run_encode_generic)."""
    out = {sig_of(_parse_launch(line)) for line in forms_dump("--compiled")}
    for off in range(4):
        out.add(form("encode_bytes", k=0, off=off))
        for rows in range(1, 9):
            for first in (0, 1):
                out.add(form("encode_v16", k=0, r=rows, off=off, first=first, pol=NT_STORE))
    for (k, r) in ((10, 3), (10, 2)):
        for s in (0, STAGE):
            out.add(form("encode_v16", k=k, r=r, off=0, first=1, pol=NT_STORE | PAIR_MAC | s))
    out.add(form("encode_v16", k=20, r=5, off=0, first=1, pol=NT_STORE | PAIR_MAC))
    out.add(form("encode_v16", k=10, r=1, off=0, first=1, pol=NT_STORE))
    out.add(form("encode_v16", k=4, r=2, off=0, first=1, pol=NT_STORE))
    out.add(form("encode_v16", k=10, r=1, off=1, first=1, pol=NT_STORE))
    out.add(form("encode_v16", k=10, r=1, off=3, first=1, pol=NT_STORE))
    for (k, r) in ((20, 5), (10, 3)):
        for s in (0, STAGE):
            out.add(form("encode_bits", k=k, r=r, off=0, pol=NT_STORE | s))
    for name in ("classify", "rows_block_sums", "rows_scan_blocks", "fill", "copy", "legacy_server"):
        out.add(form(name))
    out.add(form("rows_write", direct=0))
    out.add(form("rows_write", direct=1))
    return out


def _strip_aux(s):
    return s[:-1] + (-1,) if s[0] != "decode_wave" else s[:-1] + (0,)


def launched_by_this_file():
    """Instantiations the tables above expect this file's cases to launch."""
    got = set()
    for (k, r) in DECODE_SHAPES:
        for P in DECODE_P:
            for _, api, env in _apis(k, r):
                got.update(expected_decode(api, k, r, P, scan="QUICFEC_DECODE_SCAN" in env,
                                           runs="QUICFEC_PACKED_RUNS" in env) or [])
    for P in (48, 272, 2064):
        for api in ("in_place", "slots"):
            got.update(expected_decode(api, 6, 3, P))
    for (k, r) in sorted(MASK_SHAPES):
        for P in (16, 200, 256):
            for runs in (False, True):
                got.update(expected_decode("packed", k, r, P, runs=runs) or [])
    for (k, r) in ENCODE_SHAPES:
        for P in ENCODE_P:
            got.update(s for s, _ in expected_encode(k, r, P))
    got.update(s for s, _ in expected_encode(7, 3, 1201, off=2))
    got.update(s for s, _ in expected_encode(10, 1, 1200, off=1))
    got.update(s for s, _ in expected_encode(5, 2, 15))
    return {_strip_aux(s) for s in got}


# Compiled but launched by no case here, each with its reason.
NOT_LAUNCHED_HERE = {
    "decode_fused mask-addressed (0,1): all but k=10 r=2 compact; recover_runs (0,1): all but k=10 r=2":
        "P <= 256 takes the tiled form for k=10 r=3, k=10 r=1 and k=4 r=2, and the wave kernel for k=10 r=2 in place: "
        "compiled, but no call reaches them",
    "decode_fused record-addressed k=10 r=3 (1,1)": "reached only with host-built records or a probe's variant; "
                                                     "the library's dense k=10 r=3 plan always takes the mask-addressed form",
    "decode_tiled k=20 r=5 (both layouts)": "auto leaves k=20 r=5 to the LDS-table fused form; only a probe's variant selects it",
    "encode_bits k=10 r=3 (both)": "only with QUICFEC_ENCODE_BITS=1 (tests/test_gpu_bits.py)",
    "encode_v16 runtime k, OFF=1 and OFF=3, and the row counts not used here": "u32 offsets reach the library only "
        "through the legacy call (k=10 r=1, its own instantiation); OFF=3 is the coalescer's (tests/test_gpu_coalesce*.py) "
        "and the address-table encode's (tests/test_gpu_gather.py; tests/test_gpu_address_limits.py runs its passes of 1, 7 "
        "and 8 rows: k=63 r=1, k=1 r=63, k=32 r=32, k=48 r=16, k=12 r=9)",
    "encode_bytes OFF=1..3": "gathered packets shorter than 16 B (tests/test_gpu_parity.py offsets cases)",
    "rows_scan_blocks / rows_write<false>": "past 4096 prefix blocks or QUICFEC_ROWS_DIRECT_BLOCKS (tests/test_gpu_packed.py)",
    "fill, copy, legacy_server": "not dispatch forms; covered by their own tests",
}


DUMP_P = list(range(1, 2101)) + [4096, 8192, 8193, 9000]
DUMP_SHAPES = DECODE_SHAPES + [(6, 3), (7, 4), (12, 6), (12, 9), (16, 4)]


def _dump_queries(lines, kind):
    """(query fields, launches or None) of the dump's lines of one kind."""
    for line in lines:
        query, _, launches = line.partition(" | ")
        if query.split()[0] == kind:
            q = dict(f.split("=") for f in query.split()[1:])
            yield q, (None if launches == "refused" else [t.strip() for t in launches.split(";")])


def _check_decode_lines(lines, runs):
    prefix = [form("rows_block_sums"), form("rows_write", direct=1)]     # the packed prefix the table names
    seen = set()
    for q, launches in _dump_queries(lines, "decode"):
        api, k, r, P, scan = q["api"], int(q["k"]), int(q["r"]), int(q["P"]), int(q["scan"])
        assert int(q["runs"]) == (1 if runs else -1)
        exp = expected_decode(api, k, r, P, scan=scan == SCAN, runs=runs)
        if launches is not None:
            launches = [s for t in launches for s in (prefix if t == "rows_prefix" else [sig_of(_parse_launch(t))])]
        assert launches == exp, (q, launches, exp)
        seen.add((api, k, r, P, scan))
    return seen


def test_decided_decode_forms_equal_the_table(forms_dump):
    """The deciding code (csrc/fec_forms.hpp decode_form / packed_form, asked by forms_dump)
    against the table, for every packet size 1..2100 and four larger ones, the compiled shapes and
    five runtime-k ones, every API, scan 1 and 8; the packed call also with QUICFEC_PACKED_RUNS=1."""
    lines = forms_dump()
    seen = _check_decode_lines(lines, runs=False)
    assert seen == {(api, k, r, P, scan) for api in ("in_place", "slots", "packed") for (k, r) in DUMP_SHAPES
                    for P in DUMP_P for scan in (1, SCAN)}
    seen = _check_decode_lines(forms_dump("--packed", QUICFEC_PACKED_RUNS="1"), runs=True)
    assert seen == {("packed", k, r, P, scan) for (k, r) in DUMP_SHAPES for P in DUMP_P for scan in (1, SCAN)}


def test_decided_encode_forms_equal_the_table(forms_dump):
    """csrc/fec_forms.hpp encode_form (and the launcher's passes of 8 rows) against the table: the
    same sizes and shapes, contiguous packets, u32 and u64 offsets."""
    seen = set()
    for q, launches in _dump_queries(forms_dump(), "encode"):
        k, r, P, off = int(q["k"]), int(q["r"]), int(q["P"]), int(q["off"])
        recs = [_parse_launch(t) for t in launches]
        got = [(sig_of(t), None if t["tile"] < 0 else "tile" if t["tile"] > 0 else "flat") for t in recs]
        assert got == expected_encode(k, r, P, off=off), (q, got)
        seen.add((k, r, P, off))
    assert seen == {(k, r, P, off) for (k, r) in DUMP_SHAPES for P in DUMP_P for off in (0, 1, 2)}


def test_table_covers_the_compiled_dispatch_forms(forms_dump):
    """The cases of this file, by the table, launch every instantiation of the decode forms that
    the library's own choice can reach -- 81 of the 90 mask-addressed decode_fused, all 18
    LDS-table ones, 33 of the 36 recover_runs, the 6 tiled and 6 wave ones -- and name nothing
    that is not compiled; what is left is listed with its reason (NOT_LAUNCHED_HERE)."""
    compiled = {_strip_aux(s) for s in compiled_instantiations(forms_dump)}
    launched = launched_by_this_file()
    assert launched <= compiled, sorted(launched - compiled)
    missing = compiled - launched

    def n(pred):
        return sum(1 for s in compiled if pred(s)), sum(1 for s in missing if pred(s))

    # the (0,1) layout (P <= 256) is reachable only for k=10 r=2 into slots or packed rows: the
    # three tiled shapes decode such packets in the tiled form and every in-place call of k=10 r=2
    # lands in the wave kernel, so 9 of the 90 and 3 of the 36 cannot be launched by the library
    unreachable = {s for s in missing if s[0] in ("decode_fused", "recover_runs") and s[8] != 0 and (s[3], s[4]) == (0, 1)}
    assert all((s[1], s[2]) != (10, 2) or not s[7] & COMPACT for s in unreachable if s[0] == "decode_fused")
    assert n(lambda s: s[0] == "decode_fused" and s[8] == 1) == (90, 9)
    assert sum(1 for s in unreachable if s[0] == "decode_fused") == 9
    assert n(lambda s: s[0] == "decode_fused" and s[8] == 0 and s[1] == 20) == (18, 0)
    assert n(lambda s: s[0] == "recover_runs") == (36, 3)
    assert sum(1 for s in unreachable if s[0] == "recover_runs") == 3
    assert n(lambda s: s[0] == "decode_wave") == (6, 0)
    assert n(lambda s: s[0] == "decode_tiled") == (8, 2)            # k=20 r=5: NOT_LAUNCHED_HERE
    assert n(lambda s: s[0] == "decode_bytes") == (2, 0)
    assert n(lambda s: s[0] == "decode_fused" and s[8] == 0 and s[1] == 10) == (1, 1)
    assert n(lambda s: s[0] == "encode_v16" and s[1] > 0) == (9, 1)  # OFF=3: the coalescer's
    assert n(lambda s: s[0] == "encode_bits") == (4, 2)
