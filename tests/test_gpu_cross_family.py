"""One context across call families: the caller streams' workspaces, the lazily built plans and tables
and the two modes are shared by every device entry point (csrc/fec_shim.cpp), and every other GPU test
file drives one family.  Here the calls of all families meet on one context, in sequences chosen so
that each call finds another family's state underneath it: a wide or deep record arena under a
gather's record offsets, a plan arena under the wide table's 32-B masks, block sums under record
offsets, a mode switched while another family's call is still queued.

Nothing is new about the truth.  Cases, device buffers, launches and checks are the per-family
modules', taken by import: rebuilt bytes against oracle.rs_decode (one-word shapes) or the original
data (wide and deep shapes), encodes against oracle.rs_encode, junk in every shard, parity row and mask
bit the erasure rule does not read, guard bytes around every output, pre-filled statuses, inputs
unchanged.  Bit-exact, no tolerance.  A call the context's modes refuse must report FEC_ERR_RANGE with
its words and leave every buffer of the call as it was.

REPRESENTATIVES has one row per way of carving the workspace; tests/test_cross_family_layout.py
asserts on the CPU, from tests/csrc/workspace_dump.cpp, that these rows really put one family's
regions over another's.  Every row has two cases of different G, so a pair of rows meets both with the
buffer growing and with a larger buffer reused.
"""
import os
import threading
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import cross_family as xf
import test_gpu_device_plan as dp
import test_gpu_gather as fx
import test_gpu_gather_var as var
import test_gpu_scatter as sc
import test_gpu_scatter_encode as se
import test_gpu_streams as st
import test_gpu_wide as tw
import test_gpu_wide_deep as wd
import test_gpu_wide_encode as we
import test_gpu_wide_table as tt
from cross_family import PLAN_CODEBOOK, PLAN_DEVICE, ROWS_ALL, ROWS_CAPPED, Rep

pytestmark = pytest.mark.gpu

SEED = 0xC2055F00
# QUICFEC_XFAM_SEED / QUICFEC_XFAM_BLOCKS widen test_random_sequences for a long run (the default is
# the committed 6 blocks of 24 calls)
XFAM_SEED = int(os.environ.get("QUICFEC_XFAM_SEED", str(SEED)), 0)
XFAM_BLOCKS = int(os.environ.get("QUICFEC_XFAM_BLOCKS", "6"))

# id, call, k, r, P, (G, the other G), workspace layout, own masks, own symbol lengths, plan mode, rows mode
REPRESENTATIVES = [
    Rep("prefix", "fec_recover_batch_rs_dev_packed", 10, 3, 700, (3000, 131), "prefix", False, False, None, None),
    Rep("tiled", "fec_decode_batch_rs_dev", 10, 3, 64, (1031, 131), "offsets", False, False, None, None),
    Rep("book_slots", "fec_recover_batch_rs_dev", 20, 5, 272, (261, 131), "offsets", False, False, None, None),
    Rep("plan_dev", "fec_decode_batch_rs_dev", 16, 16, 32, (67, 131), "plan", False, False, PLAN_DEVICE, None),
    Rep("plan_host", "fec_decode_batch_rs_dev", 16, 16, 32, (67, 131), "offsets", False, False, PLAN_CODEBOOK, None),
    Rep("gather", "fec_recover_gather_rs_dev", 20, 5, 1025, (67, 131), "offsets", False, False, None, None),
    Rep("scatter_own", "fec_recover_scatter_rs_dev", 10, 3, 1200, (67, 131), "offsets2", False, True, None, None),
    Rep("scatter_plan", "fec_recover_scatter_rs_dev", 12, 12, 45, (67, 131), "plan", True, True, PLAN_DEVICE, None),
    Rep("wide", "fec_recover_wide_rs_dev", 224, 32, 16, (67, 9), "wide", False, False, None, None),
    Rep("wide_table", "fec_recover_scatter_wide_rs_dev", 100, 20, 1037, (67, 9), "wide_table", True, True, None, None),
    Rep("deep", "fec_decode_wide_rs_dev", 33, 33, 16, (67, 131), "deep", False, False, None, ROWS_ALL),
    Rep("deep_table", "fec_recover_scatter_wide_rs_dev", 128, 128, 16, (9, 67), "deep_table", True, False, None, ROWS_ALL),
]
BY_ID = {rep.id: rep for rep in REPRESENTATIVES}
# the riders: no workspace, but the encode plans, the wide encode tables and the streams are shared
ENCODES = ("enc_batch", "enc_gather", "enc_gather_var", "enc_scatter", "enc_scatter_wide")
# test_small_arena_walks_across_families: the calls that build records, and the slots each gets
ARENA_WALK = (("plan_dev", 5), ("scatter_plan", 5), ("wide", 5), ("wide_table", 5), ("deep", 5), ("deep_table", 4))
BUILD_FORM = {"plan": "build_records", "wide": "build_records_wide", "wide_table": "build_records_wide",
              "deep": "build_records_deep", "deep_table": "build_records_deep"}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


def cases_of(family):
    return 2


# ------------------------------------------------------------------------------------------
# Cases: the per-family modules', computed once and never modified
# ------------------------------------------------------------------------------------------
def _salt(k, r, P, G):
    return k * 1000000 + r * 10000 + P * 7 + G


@lru_cache(maxsize=None)
def _prefix_case(oracle, k, r, P, G):
    salt = _salt(k, r, P, G)
    return st.Case(oracle, k, r, P, st.perm_masks(k, r, G, salt), SEED + salt)


def _lens_case(oracle, k, r, P, G):
    """test_gpu_scatter's queue case: permutation masks with the planted groups, independent lengths in 0..P + 8."""
    salt = _salt(k, r, P, G)
    rng = np.random.default_rng([SEED, salt])
    c = var.make_case(oracle, k, r, P, fx.perm_masks(k, r, G, salt), rng.integers(0, P + 9, size=(G, k)),
                      rng.integers(0, P + 9, size=(G, r)), SEED + salt)
    assert c.rows > 0 and (c.status == 1).any() and (c.masks == 0).any()
    return c


SMALL_TABLE_KINDS = ("xor", "single_row_0_lost", "first_and_last", "full_lowest_rows", "full_highest_rows", "full_spread",
                     "untouched", "parity_only", "short_by_one")


def _small_wide_case(oracle, Case, k, r, P):
    """Nine groups, all planted (test_gpu_wide.planted_groups), for a shape within the rows cap; Case is
    test_gpu_wide's (contiguous) or test_gpu_wide_table's."""
    kinds = tw.planted_groups(k, r)
    bits = np.array([kinds[kind][0] for kind in SMALL_TABLE_KINDS])
    c = Case(oracle, k, r, P, bits, SEED + _salt(k, r, P, len(bits)))
    assert c.rebuilds.sum() == 6 and (c.e[c.rebuilds] == min(k, r)).sum() == 3 and (c.status == 1).sum() == 1
    return c


@lru_cache(maxsize=None)
def case(oracle, family, i):
    """Case i (0: the table's G, 1: the other G) of a representative or a rider."""
    if family in BY_ID:
        rep = BY_ID[family]
        k, r, P, G = rep.k, rep.r, rep.P, rep.groups[i]
        if family == "prefix":
            c = _prefix_case(oracle, k, r, P, max(rep.groups)).head(G)
            st._check_mix(c)
            return c
        if family in ("tiled", "book_slots"):
            return st._case(oracle, k, r, P, G)
        if family in ("plan_dev", "plan_host"):
            return dp.contiguous_case(oracle, k, r, P) if G == dp.G_MAIN else st._case(oracle, k, r, P, G)
        if family == "gather":
            if G == fx.G_MAIN:
                return fx.main_case(oracle, k, r, P)
            c = fx.make_case(oracle, k, r, P, fx.perm_masks(k, r, G, _salt(k, r, P, G)), SEED + _salt(k, r, P, G))
            assert c.rows > 0 and (c.status == 1).any()
            return c
        if family == "scatter_own":
            return var.main_case(oracle, k, r, P) if G == var.G_MAIN else _lens_case(oracle, k, r, P, G)
        if family == "scatter_plan":
            return dp.table_cases(oracle, k, r, P).lens if G == dp.G_MAIN else _lens_case(oracle, k, r, P, G)
        if family == "wide":
            return tw.main_case(oracle, k, r, P) if G == tw.G_MAIN else _small_wide_case(oracle, tw.Case, k, r, P)
        if family == "wide_table":
            return tt.main_case(oracle, k, r, P) if G == tt.G_MAIN else _small_wide_case(oracle, tt.Case, k, r, P)
        if family == "deep":
            return wd.wide_case(oracle, k, r, P, G)
        if family == "deep_table":
            return wd.table_case(oracle, k, r, P, G)
    if family == "enc_batch":
        return st._case(oracle, 20, 5, 272, (261, 131)[i])
    if family == "enc_gather":
        G, P = ((67, 1025), (37, 272))[i]
        return fx.make_case(oracle, 20, 5, P, [0] * G, SEED + P)
    if family == "enc_gather_var":
        return var.encode_case(oracle, 20, 5, (272, 1025)[i])
    if family == "enc_scatter":
        return se.mixed_case(oracle, 20, 5, 272) if i == 0 else se.full_case(oracle, 20, 5, 1025, absent=True)
    if family == "enc_scatter_wide":
        return we.mixed_case(oracle, 60, 5, 272) if i == 0 else we.mixed_case(oracle, 33, 33, 1025)
    raise KeyError(family)


# ------------------------------------------------------------------------------------------
# One call of a family: the module's buffers, its launch on a stream, its check after the last synchronise
# ------------------------------------------------------------------------------------------
def _handle(stream):
    return stream.cuda_stream if stream is not None else None


def _make_encode_batch(torch, c, seed):
    b = SimpleNamespace(c=c)
    b.dd = st._dev(torch, c.data)
    b.whole, b.par = fx.guarded(torch, c.G * c.r * c.P, 0x5A)
    return b


def _check_encode_batch(b, what=""):
    c = b.c
    got = b.whole.cpu().numpy()
    assert np.array_equal(got[fx.GUARD:-fx.GUARD], c.par), what
    assert (got[:fx.GUARD] == 0x5A).all() and (got[-fx.GUARD:] == 0x5A).all(), what
    assert np.array_equal(b.dd.cpu().numpy(), c.data), what


def _contiguous(api, status_fill=None):
    """inputs: device copies shared with other read-only calls of the case (st.make_call); the caller
    then checks them once itself (st.check_inputs)."""
    make = (lambda torch, c, seed, inputs=None: st.make_call(torch, c, api, inputs=inputs)) if status_fill is None else \
        (lambda torch, c, seed: dp.make_call(torch, c, api))
    return SimpleNamespace(make=make, launch=lambda ctx, b, s: st.launch(ctx, b, s), check=st.check)


KINDS = {
    "prefix": _contiguous("packed"),
    "tiled": _contiguous("in_place"),
    "book_slots": _contiguous("slots"),
    "plan_dev": _contiguous("in_place", 0xAA),
    "plan_host": _contiguous("in_place", 0xAA),
    "gather": SimpleNamespace(make=fx.make_recover, launch=lambda ctx, b, s: fx.launch_recover(ctx, b, _handle(s)),
                              check=fx.check_recover),
    "var_gather": SimpleNamespace(make=var.make_recover, launch=lambda ctx, b, s: var.launch_recover(ctx, b, _handle(s)),
                                  check=var.check_recover),
    "scatter": SimpleNamespace(make=lambda torch, c, seed: sc.make_scatter(torch, c, seed, sc.padded_layout(seed + 1)),
                               launch=lambda ctx, b, s: sc.launch_scatter(ctx, b, _handle(s)), check=sc.check_scatter),
    # the symbol lengths the kernel cuts its stores at live behind the record offsets
    "scatter_own": SimpleNamespace(
        make=lambda torch, c, seed: sc.make_scatter(torch, c, seed, sc.padded_layout(seed + 1), want_sym=False),
        launch=lambda ctx, b, s: sc.launch_scatter(ctx, b, _handle(s)), check=sc.check_scatter),
    # and the masks build_records reads: both optional outputs NULL
    "scatter_plan": SimpleNamespace(
        make=lambda torch, c, seed: sc.make_scatter(torch, c, seed, sc.padded_layout(seed + 1), want_sym=False),
        launch=lambda ctx, b, s: sc.launch_scatter(ctx, b, _handle(s), masks=False),
        check=lambda b, what="": sc.check_scatter(b, what, masks=False)),
    "wide": SimpleNamespace(make=lambda torch, c, seed: tw.make_call(torch, c, "slots"), launch=tw.launch, check=tw.check),
    "wide_table": SimpleNamespace(
        make=lambda torch, c, seed: tt.make_call(torch, c, True, "odd", seed=seed & 0xFFFF),
        launch=lambda ctx, b, s: tt.launch(ctx, b, s, masks=False, symlen=False),
        check=lambda b, what="": tt.check(b, what, masks=False, symlen=False)),
    "deep": SimpleNamespace(make=lambda torch, c, seed: tw.make_call(torch, c, "in_place"), launch=tw.launch, check=tw.check),
    "deep_table": SimpleNamespace(
        make=lambda torch, c, seed: tt.make_call(torch, c, True, "packed", seed=seed & 0xFFFF),
        launch=lambda ctx, b, s: tt.launch(ctx, b, s, masks=False),
        check=lambda b, what="": tt.check(b, what, masks=False)),
    "enc_batch": SimpleNamespace(
        make=_make_encode_batch,
        launch=lambda ctx, b, s: ctx.encode_dev(b.dd, b.c.G, b.c.k, b.c.r, b.c.P, b.par, stream=_handle(s)),
        check=_check_encode_batch),
    "enc_gather": SimpleNamespace(make=fx.make_encode, launch=lambda ctx, b, s: fx.launch_encode(ctx, b, _handle(s)),
                                  check=fx.check_encode),
    "enc_gather_var": SimpleNamespace(make=var.make_encode, launch=lambda ctx, b, s: var.launch_encode(ctx, b, _handle(s)),
                                      check=var.check_encode),
    "enc_scatter": SimpleNamespace(
        make=lambda torch, c, seed: se.make_encode(torch, c, seed, se.residue_layout,
                                                   with_lens=bool((c.lens[:, :c.k][c.present] != c.P).any())),
        launch=lambda ctx, b, s: se.launch_encode(ctx, b, _handle(s)), check=se.check_encode),
    "enc_scatter_wide": SimpleNamespace(make=lambda torch, c, seed: se.make_encode(torch, c, seed, se.residue_layout),
                                        launch=lambda ctx, b, s: we.launch(ctx, b, _handle(s)), check=se.check_encode),
}
assert set(KINDS) >= set(BY_ID) | set(ENCODES)


def _tensors(b):
    """Every device buffer of a call: the attributes that are tensors, and those in lists of them."""
    for name, v in sorted(vars(b).items()):
        items = v if isinstance(v, (list, tuple)) else [v]
        for n, x in enumerate(items):
            x = x[0] if isinstance(x, tuple) else x
            if hasattr(x, "data_ptr"):
                yield f"{name}[{n}]", x


def make(torch, oracle, family, i, seed, kind=None, refused=None, **kw):
    """One call of `family` on its case i.  refused: the words of the refusal it is to meet; every
    buffer is then copied to the host now, to be compared after the last synchronise."""
    c = case(oracle, family, i) if isinstance(i, int) else i
    call = SimpleNamespace(family=family, kind=KINDS[kind or family], refused=refused, what=(family, c.k, c.r, c.P, c.G))
    call.b = call.kind.make(torch, c, SEED + seed, **kw)
    if refused:
        call.before = {name: x.cpu().numpy().copy() for name, x in _tensors(call.b)}
        assert len(call.before) >= 4
    return call


def launch(q, ctx, call, stream):
    """Queue the call (None: on the context's own stream), or see it refused with its code and words."""
    if not call.refused:
        call.kind.launch(ctx, call.b, stream)
        return
    with pytest.raises(q.FecError) as ei:
        call.kind.launch(ctx, call.b, stream)
    assert ei.value.code == q.FEC_ERR_RANGE and call.refused in ctx.last_error(), (call.what, ctx.last_error())


def check(call, what=""):
    if not call.refused:
        call.kind.check(call.b, (what, call.what))
        return
    for name, x in _tensors(call.b):                                           # nothing launched, nothing written
        assert np.array_equal(x.cpu().numpy(), call.before[name]), (what, call.what, "refused, yet changed", name)


def set_modes(ctx, rep):
    """The mode the representative needs, set right before its call."""
    if rep.plan is not None:
        ctx.decode_plan_mode(rep.plan)
    if rep.rows is not None:
        ctx.wide_rows_mode(rep.rows)


def test_constants_are_the_bindings(quicfec_mod):
    q = quicfec_mod
    assert (q.FEC_PLAN_CODEBOOK, q.FEC_PLAN_DEVICE) == (PLAN_CODEBOOK, PLAN_DEVICE)
    assert (q.FEC_WIDE_ROWS_CAPPED, q.FEC_WIDE_ROWS_ALL) == (ROWS_CAPPED, ROWS_ALL)


@pytest.mark.parametrize("family", [rep.id for rep in REPRESENTATIVES] + list(ENCODES))
def test_cases_hold_what_the_sequences_need(oracle_mod, family):
    """On the CPU, ahead of every launch (and once for the whole file: the cases are shared by every
    test below and never modified): both cases of a family have the table's shape and G; a recover case
    has a group it rebuilds, an untouched one and an unrecoverable one, an encode case parity to compare."""
    rep = BY_ID.get(family)
    for i in range(cases_of(family)):
        c = case(oracle_mod, family, i)
        assert case(oracle_mod, family, i) is c
        if rep is None:
            assert c.par.any() and c.G >= 37
            continue
        assert (c.k, c.r, c.P, c.G) == (rep.k, rep.r, rep.P, rep.groups[i])
        status = np.asarray(c.status)
        assert (status == 1).any() and (status == 0).sum() >= 3
        lost = np.asarray(c.ro.lost_d if hasattr(c, "ro") else
                          (c.masks[:, None] >> np.arange(c.k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
        assert (lost.any(axis=1) & (status == 0)).any() and (~lost.any(axis=1) & (status == 0)).any()


# ------------------------------------------------------------------------------------------
# a. Every ordered pair of representatives on one stream
# ------------------------------------------------------------------------------------------
PAIR_STREAMS = 3
HALVES = ("even_rows", "odd_rows")


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("first", [rep.id for rep in REPRESENTATIVES])
def test_every_ordered_pair_on_one_stream(quicfec_mod, oracle_mod, torch_cuda, first, half):
    """For each B of the table, `first` itself included: A, then B, then A at its other G, queued on a
    side stream with the mode each needs set right before it and no host synchronise of the test's own
    (plan_host synchronises inside its call: part of what is tested).  The twelve B of an A are split by
    parameter into the table's even and odd rows, six pairs on one context each; three side streams take
    the six pairs in turn, so the last three pairs land on the workspaces the first three left behind.
    One synchronise after the last pair, then all 18 calls are checked."""
    torch, q = torch_cuda, quicfec_mod
    A = BY_ID[first]
    seconds = REPRESENTATIVES[HALVES.index(half)::2]
    assert len(seconds) == 6 and len(REPRESENTATIVES) == 12
    # the packed recover only reads its inputs: one upload per case serves all of A's calls
    shared = {i: st.upload(torch, case(oracle_mod, first, i)) for i in range(2)} if first == "prefix" else None
    make_a = lambda i, seed: make(torch, oracle_mod, first, i, seed, **({"inputs": shared[i]} if shared else {}))
    trios = []
    for n, B in enumerate(seconds):
        trios.append([(A, make_a(0, 100 * n)), (B, make(torch, oracle_mod, B.id, 0, 100 * n + 1)), (A, make_a(1, 100 * n + 2))])
    streams = [torch.cuda.Stream() for _ in range(PAIR_STREAMS)]
    assert len({s.cuda_stream for s in streams} - {0}) == PAIR_STREAMS
    with st.fresh_context(q, q.load_library()) as ctx:
        torch.cuda.synchronize()
        for n, trio in enumerate(trios):
            for rep, call in trio:
                set_modes(ctx, rep)
                launch(q, ctx, call, streams[n % PAIR_STREAMS])
        torch.cuda.synchronize()
    assert sum(len(trio) for trio in trios) == 18
    for n, trio in enumerate(trios):
        for pos, (rep, call) in enumerate(trio):
            check(call, (first, half, "pair", n, "call", pos))
    for i, inputs in (shared or {}).items():
        st.check_inputs(case(oracle_mod, first, i), *inputs)


# ------------------------------------------------------------------------------------------
# b. Modes switched between queued calls
# ------------------------------------------------------------------------------------------
def test_mode_switches_between_queued_calls(quicfec_mod, oracle_mod, torch_cuda):
    """One side stream, nothing synchronised by the test until the end: a mode is read when a call
    starts, so a switch must neither reach back into a call already queued nor be missed by the next.
    deep in ROWS_ALL; CAPPED, and the same 33 + 33 call is refused; wide; PLAN_DEVICE and scatter_plan;
    PLAN_CODEBOOK, and the same scatter call is refused while the served one is queued; plan_host (it
    drains the stream inside the call); PLAN_DEVICE and plan_dev; ROWS_ALL and deep_table; a loss hint of
    0.001 and tiled; no hint and prefix."""
    torch, q = torch_cuda, quicfec_mod
    mk = lambda family, n, **kw: make(torch, oracle_mod, family, 0, 7000 + n, **kw)
    plan, rows, hint = (lambda m: lambda ctx: ctx.decode_plan_mode(m)), (lambda m: lambda ctx: ctx.wide_rows_mode(m)), \
        (lambda h: lambda ctx: ctx.decode_loss_hint(h))
    steps = [(rows(ROWS_ALL), mk("deep", 0)),
             (rows(ROWS_CAPPED), mk("deep", 1, refused="min(k, r)")),
             (None, mk("wide", 2)),
             (plan(PLAN_DEVICE), mk("scatter_plan", 3)),
             (plan(PLAN_CODEBOOK), mk("scatter_plan", 4, refused="sparse-plan")),
             (None, mk("plan_host", 5)),
             (plan(PLAN_DEVICE), mk("plan_dev", 6)),
             (rows(ROWS_ALL), mk("deep_table", 7)),
             (hint(0.001), mk("tiled", 8)),
             (hint(-1.0), mk("prefix", 9))]
    stream = torch.cuda.Stream()
    with st.fresh_context(q, q.load_library()) as ctx:
        torch.cuda.synchronize()
        for switch, call in steps:
            if switch:
                switch(ctx)
            launch(q, ctx, call, stream)
        torch.cuda.synchronize()
    for n, (_, call) in enumerate(steps):
        check(call, ("step", n + 1))


# ------------------------------------------------------------------------------------------
# c. Families race to build the shared plans and tables
# ------------------------------------------------------------------------------------------
def test_families_race_to_build_shared_state(quicfec_mod, oracle_mod, torch_cuda):
    """Four host threads, each with its own side stream and eight calls, start from a barrier on a fresh
    context in ROWS_ALL and PLAN_DEVICE: the first calls race for the decode and encode plans of 20 + 5
    (and its compact book), the wide matrix and the wide encode tables of 60 + 5 -- one (k, r) entry of
    each map for three calls -- those of 33 + 33 and the device plan's matrix of 16 + 16, all under the
    context's lock, while the workspace list is shared."""
    torch, q = torch_cuda, quicfec_mod
    o = oracle_mod
    mk = lambda t, j, family, c, kind=None: make(torch, o, family, c, 9000 + 10 * t + j, kind=kind)
    c205 = st._case(o, 20, 5, 272, 261)
    v205 = var.main_case(o, 20, 5, 1025)
    plans = [
        [("book_slots", c205, None), ("enc_batch", 0, None), ("tiled", c205, None), ("enc_batch", 1, None)],
        [("gather", 0, None), ("enc_gather", 0, None), ("var_gather", v205, "var_gather"), ("enc_gather_var", 0, None),
         ("scatter", v205, "scatter"), ("enc_scatter", 0, None), ("gather", 1, None), ("enc_scatter", 1, None)],
        [("wide", tw.main_case(o, 60, 5, 16), None), ("wide_table", tt.main_case(o, 60, 5, 16), None),
         ("enc_scatter_wide", 0, None)],
        [("deep", 0, None), ("enc_scatter_wide", 1, None), ("plan_dev", 0, None)],
    ]
    assert case(o, "enc_scatter_wide", 0).k == 60 and case(o, "enc_scatter_wide", 1).k == 33
    work = [[mk(t, j, *plan[j % len(plan)]) for j in range(8)] for t, plan in enumerate(plans)]
    streams = [torch.cuda.Stream() for _ in work]
    barrier = threading.Barrier(len(work))
    errors = []

    def run(t, ctx):
        try:
            barrier.wait(timeout=60)
            for call in work[t]:
                launch(q, ctx, call, streams[t])
        except BaseException as e:                                             # re-raised in the test
            errors.append((t, e))

    with st.fresh_context(q, q.load_library()) as ctx:
        ctx.wide_rows_mode(ROWS_ALL)
        ctx.decode_plan_mode(PLAN_DEVICE)
        torch.cuda.synchronize()
        threads = [threading.Thread(target=run, args=(t, ctx)) for t in range(len(work))]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
    if errors:
        raise errors[0][1]
    for t, mine in enumerate(work):
        for j, call in enumerate(mine):
            check(call, ("thread", t, "call", j))


# ------------------------------------------------------------------------------------------
# d. A small arena walked chunk after chunk by six families
# ------------------------------------------------------------------------------------------
def arena_budget(rep, slots):
    """QUICFEC_PLAN_ARENA_BYTES for `slots` records of the representative's shape per chunk."""
    header = 128 if rep.layout == "plan" else 512          # fec_forms.hpp plan_slot_stride; wide_slot_stride, wide_deep_slot_stride
    return slots * (header + min(rep.k, rep.r) * rep.k * 32)


def test_small_arena_walks_across_families(quicfec_mod, oracle_mod, torch_cuda, monkeypatch):
    """The test library with the arena lowered per call to five slots (four for deep_table's nine groups):
    plan_dev, scatter_plan, wide, wide_table, deep and deep_table queued on one side stream, so each arena
    is reused chunk after chunk and then by the next family at another stride.  Every result is checked,
    and the trace of each call shows its builds: ceil(G / per_chunk) of them, the first at group 0, each
    beginning where the one before ended, G groups in all."""
    torch, q = torch_cuda, quicfec_mod
    lib = q.load_test_library()
    calls = [(BY_ID[family], slots, make(torch, oracle_mod, family, 0, 11000 + n)) for n, (family, slots) in enumerate(ARENA_WALK)]
    for rep, slots, _ in calls:
        assert 2 <= slots < rep.groups[0]                                      # per_chunk = slots: several chunks, none of one group
    stream = torch.cuda.Stream()
    traces = []
    with st.fresh_context(q, lib) as ctx:
        ctx.wide_rows_mode(ROWS_ALL)
        ctx.decode_plan_mode(PLAN_DEVICE)
        torch.cuda.synchronize()
        q.launch_trace(lib)                                                    # clear: fills and uploads are torch's
        for rep, slots, call in calls:
            with monkeypatch.context() as mp:                                  # the test library reads its switches per call
                mp.setenv("QUICFEC_PLAN_ARENA_BYTES", str(arena_budget(rep, slots)))
                launch(q, ctx, call, stream)
            traces.append(q.launch_trace(lib))                                 # written at launch: no wait for the stream
        torch.cuda.synchronize()
    for rep, slots, call in calls:
        check(call, ("arena of", slots))
    total = 0
    for (rep, slots, call), trace in zip(calls, traces):
        G = rep.groups[0]
        builds = [(t["first_item"], t["items"]) for t in trace if t["form"] == BUILD_FORM[rep.layout]]
        assert {t["form"] for t in trace if t["form"].startswith("build_records")} == {BUILD_FORM[rep.layout]}, rep.id
        assert len(builds) == -(-G // slots), (rep.id, builds)
        assert builds[0][0] == 0 and sum(n for _, n in builds) == G, (rep.id, builds)
        assert all(a[0] + a[1] == b[0] for a, b in zip(builds, builds[1:])), (rep.id, builds)
        assert all(n == slots for _, n in builds[:-1]) and 1 <= builds[-1][1] <= slots, (rep.id, builds)
        total += len(builds)
    assert total == sum(-(-BY_ID[family].groups[0] // slots) for family, slots in ARENA_WALK)    # six builds' worth, no more


# ------------------------------------------------------------------------------------------
# e. More caller streams than workspaces
# ------------------------------------------------------------------------------------------
def test_more_streams_than_workspaces_across_families(quicfec_mod, oracle_mod, torch_cuda):
    """20 caller streams on one context, two rounds, no host synchronise between them: from the 17th
    stream on a workspace last laid out by one family is dropped (after the library's device
    synchronise), and in the second round its stream comes back with another family and the other G.
    plan_host is left out: the context stays in PLAN_DEVICE and ROWS_ALL."""
    torch, q = torch_cuda, quicfec_mod
    reps = [rep for rep in REPRESENTATIVES if rep.id != "plan_host"]
    nstreams, rounds = 20, 2
    assert nstreams > st.MAX_STREAM_WORKSPACES and len(reps) == 11
    calls = []
    for rnd in range(rounds):
        for s in range(nstreams):
            rep = reps[(s + 4 * rnd) % len(reps)]
            calls.append((s, make(torch, oracle_mod, rep.id, rnd, 13000 + 100 * rnd + s)))
    for s in range(nstreams):                                                  # another family when the stream comes back
        assert calls[s][1].family != calls[nstreams + s][1].family
    assert {call.family for _, call in calls} == {rep.id for rep in reps}
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    assert len({s.cuda_stream for s in streams}) == nstreams
    with st.fresh_context(q, q.load_library()) as ctx:
        ctx.wide_rows_mode(ROWS_ALL)
        ctx.decode_plan_mode(PLAN_DEVICE)
        torch.cuda.synchronize()
        for s, call in calls:
            launch(q, ctx, call, streams[s])
        torch.cuda.synchronize()
    for n, (s, call) in enumerate(calls):
        check(call, ("call", n, "stream", s))


# ------------------------------------------------------------------------------------------
# f. Freeing a context with calls of four families in flight
# ------------------------------------------------------------------------------------------
def test_free_with_mixed_families_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """wide_table and scatter_own on one side stream, deep and prefix on another, and the context freed
    at once: fec_encoder_free waits for calls queued on caller streams, which read the workspaces, the
    wide matrices and the codebook it frees, so both streams are drained and all four results complete."""
    torch, q = torch_cuda, quicfec_mod
    calls = [(n % 2, make(torch, oracle_mod, family, 0, 15000 + n))
             for n, family in enumerate(("wide_table", "deep", "scatter_own", "prefix"))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctx = st.fresh_context(q, q.load_library())
    ctx.wide_rows_mode(ROWS_ALL)
    torch.cuda.synchronize()
    for s, call in calls:
        launch(q, ctx, call, streams[s])
    ctx.close()
    assert streams[0].query() and streams[1].query()                           # the free drained both streams
    torch.cuda.synchronize()
    for s, call in calls:
        check(call, ("in flight on stream", s))


# ------------------------------------------------------------------------------------------
# g. Random sequences
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", range(XFAM_BLOCKS))
def test_random_sequences(quicfec_mod, oracle_mod, torch_cuda, block):
    """24 seeded calls on one context: each draws a family from the twelve representatives and the five
    encodes, one of its cases, a stream from {the context's own, two side streams} and, one time in six,
    a switch of the plan mode, the rows mode or the loss hint first.  A call the modes of its moment
    refuse is expected to be refused, with its code, its words and every buffer untouched.  One
    synchronise per block, then every check.  The block's seed is the first whose draw holds ten
    families, both directions of each mode switch, a refusal and three calls per stream (cross_family.py),
    asserted here before anything is launched."""
    torch, q = torch_cuda, quicfec_mod
    seed = xf.block_seed(XFAM_SEED, block, REPRESENTATIVES, ENCODES, cases_of)
    seq = xf.draw_block(seed, REPRESENTATIVES, ENCODES, cases_of)
    assert len(seq) == xf.CALLS_PER_BLOCK and xf.block_problems(seq) == []
    calls = [make(torch, oracle_mod, d.family, d.case, 17000 + 100 * block + n, refused=d.refused) for n, d in enumerate(seq)]
    streams = [None, torch.cuda.Stream(), torch.cuda.Stream()]
    switches = {"plan": lambda ctx, v: ctx.decode_plan_mode(v), "rows": lambda ctx, v: ctx.wide_rows_mode(v),
                "hint": lambda ctx, v: ctx.decode_loss_hint(v)}
    with st.fresh_context(q, q.load_library()) as ctx:
        torch.cuda.synchronize()
        for d, call in zip(seq, calls):
            if d.switch:
                switches[d.switch[0]](ctx, d.switch[1])
            launch(q, ctx, call, streams[d.stream])
        torch.cuda.synchronize()
    for n, (d, call) in enumerate(zip(seq, calls)):
        check(call, ("block", block, "seed", seed, "call", n, "stream", d.stream, "modes", d.plan, d.rows))
