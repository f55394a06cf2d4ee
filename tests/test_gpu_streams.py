"""The decode state a context keeps between calls: caller streams, per-stream workspaces, look-back
epochs, lazily built plans, and what freeing a context waits for (csrc/fec_shim.cpp).

Every other GPU test drives a context call by call, mostly on the context's own stream with a
host synchronise after each call.  Here calls are queued on side streams (non-blocking ones, so
nothing orders them against torch's default stream) with no host synchronise until the end, from
several streams and host threads of one context, and everything every call wrote is compared with
the oracle afterwards: rebuilt bytes, statuses, row starts, totals, `data` untouched by the recover
calls, the inputs of the recover calls as they were (seeded junk in every shard the erasure rule
does not read, tests/unread_shards.py), 0x5A wherever nothing may be written (slots m >= e,
everything past the last packed row), 7 in statuses never written.

Each test makes its own quicfec.Context, so no plan, workspace or epoch of another test is there
when it starts.  Expected bytes come from the oracle, once per shape (`_case`); a call of fewer
groups uses the head of its shape's case.  Masks are permutation(k + r)[:0..r+1] per group, or
iid loss where a test says so; the first three groups of every case are planted -- untouched,
parity lost only, unrecoverable -- so every call of every size has all three, and `_check_mix`
asserts it on the CPU before anything runs.
"""
import os
import re
import threading
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import unread_shards as us

pytestmark = pytest.mark.gpu

SEED = 0x5EED5700
REPO = Path(__file__).resolve().parent.parent

# fec_shim.cpp keeps this many per-stream workspaces and drops the least recently used (after a
# device synchronise) when one more stream arrives; test_more_streams_than_workspaces relies on 20
# being more.
MAX_STREAM_WORKSPACES = 16
RUN_TILE = 512                                     # groups per recover_runs workgroup (kRunGroups)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases against the oracle (the pattern of tests/test_gpu_forms.py)
# ------------------------------------------------------------------------------------------
def _planted(k, r):
    """Untouched, parity lost only, unrecoverable (a data shard and every parity row lost)."""
    return [0, 1 << k, 1 | (((1 << r) - 1) << k)]


def perm_masks(k, r, G, seed):
    rng = np.random.default_rng(seed)
    masks = np.zeros(G, dtype=np.uint64)
    for g in range(G):
        for s in rng.permutation(k + r)[: rng.integers(0, r + 2)]:
            masks[g] |= np.uint64(1) << np.uint64(int(s))
    masks[:3] = _planted(k, r)
    return masks


def iid_masks(k, r, G, loss, seed):
    rng = np.random.default_rng(seed)
    w = np.left_shift(np.uint64(1), np.arange(k + r, dtype=np.uint64))
    masks = ((rng.random((G, k + r)) < loss) * w).sum(axis=1, dtype=np.uint64)
    masks[:3] = _planted(k, r)
    return masks


class Case:
    """One batch and everything the oracle says about it, computed once and never modified."""

    def __init__(self, oracle, k, r, P, masks, seed):
        G = len(masks)
        self.k, self.r, self.P, self.G, self.masks, self.seed = k, r, P, G, masks, seed
        data = oracle.splitmix_bytes(G * k * P, seed)
        self.par = oracle.rs_encode(data, G, k, r, P, nthreads=8)          # true: what an encode must give
        lost = us.roles(masks, k, r).lost_d
        self.data = data
        # what a decode is given: junk in every lost data shard and every parity row the rule does
        # not read (every shape here has r > 1, so every case has a lost row below a chosen one)
        self.broken, self.par_in = us.inputs(data, self.par, masks, k, r, P, seed)
        # what a decode is given as masks: junk in the bits at and above k + r, which the rule ignores
        self.masks_in = us.high_bits(masks, k, r, seed)
        ref, clean = self.broken.copy(), self.broken.copy()
        _, self.status = oracle.rs_decode(ref, self.par_in, self.masks_in, G, k, r, P, nthreads=8)
        _, clean_status = oracle.rs_decode(clean, self.par_in, masks, G, k, r, P, nthreads=8)
        assert np.array_equal(clean, ref) and np.array_equal(clean_status, self.status)   # the oracle ignores them
        self.ref = ref                                    # in-place result
        ok = self.status == 0
        # the oracle's rebuilt packets are the original ones
        assert np.array_equal(ref.reshape(G, k, P)[ok], data.reshape(G, k, P)[ok])
        gi, ji = np.nonzero(lost & ok[:, None])           # (g, j ascending)
        mi = (np.cumsum(lost, axis=1) - 1)[gi, ji]
        self.rows = ref.reshape(G, k, P)[gi, ji]          # packed rows
        self.slots = np.full((G, r, P), 0x5A, dtype=np.uint8)
        self.slots[gi, mi] = self.rows
        per_group = (lost & ok[:, None]).sum(axis=1)
        self.row_end = np.cumsum(per_group)
        self.row_start = np.concatenate([[0], self.row_end[:-1]]).astype(np.uint32)
        for a in (self.data, self.par, self.par_in, self.broken, self.ref, self.status, self.rows, self.slots,
                  self.row_start, self.masks, self.masks_in):
            a.setflags(write=False)

    def head(self, G):
        """The first G groups as a case of their own (groups are independent and the packed rows of
        a head are the head of the rows): views, nothing recomputed."""
        if G == self.G:
            return self
        assert 3 <= G < self.G
        k, r, P = self.k, self.r, self.P
        n = int(self.row_end[G - 1])
        return SimpleNamespace(k=k, r=r, P=P, G=G, seed=self.seed, masks=self.masks[:G], masks_in=self.masks_in[:G],
                               data=self.data[:G * k * P],
                               par=self.par[:G * r * P], par_in=self.par_in[:G * r * P], broken=self.broken[:G * k * P],
                               ref=self.ref[:G * k * P],
                               status=self.status[:G], rows=self.rows[:n], slots=self.slots[:G],
                               row_start=self.row_start[:G])


# groups of each shape's one case: the most any test asks of it
CASE_GROUPS = {
    (10, 3, 700, "iid"): 5000, (4, 2, 513, "perm"): 5000, (10, 2, 200, "perm"): 5000,         # epoch wrap
    (10, 3, 700, "perm"): 9000, (10, 3, 700, "perm2"): 4096, (10, 3, 1200, "perm"): 4096, (10, 3, 1200, "perm2"): 4096,
    (6, 3, 48, "perm"): 5000, (20, 5, 272, "perm"): 517, (10, 3, 64, "perm"): 1031, (20, 5, 300, "perm"): 261,
    (16, 16, 32, "perm"): 131, (20, 5, 1200, "perm"): 1031,
}


@lru_cache(maxsize=None)
def _full_case(oracle, k, r, P, kind):
    G = CASE_GROUPS[(k, r, P, kind)]
    salt = k * 1000 + r * 100 + P + {"perm": 0, "perm2": 7777, "iid": 3333}[kind]
    masks = iid_masks(k, r, G, 0.06, salt) if kind == "iid" else perm_masks(k, r, G, salt)
    return Case(oracle, k, r, P, masks, SEED + salt)


def _case(oracle, k, r, P, G, kind="perm"):
    c = _full_case(oracle, k, r, P, kind).head(G)
    _check_mix(c)
    return c


def _check_mix(c):
    """On the CPU, before any GPU work: the case has an untouched group, an unrecoverable one and
    one that lost only parity (and, so the comparison says something, one to rebuild)."""
    kmask = np.uint64((1 << c.k) - 1)
    assert (c.masks == 0).any()
    assert (c.status != 0).any()
    assert ((c.masks != 0) & ((c.masks & kmask) == 0)).any()
    assert len(c.rows) > 0


# ------------------------------------------------------------------------------------------
# One call: its buffers, its launch on a stream, its check after the final synchronise
# ------------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.array(a)).to("cuda")      # a copy: the case's arrays are read-only


def upload(torch, c):
    """Fresh device copies of a case's inputs (junk in every shard and mask bit the rule does not read)."""
    return _dev(torch, c.broken), _dev(torch, c.par_in), _dev(torch, c.masks_in.view(np.int64))


def make_call(torch, c, api, inputs=None, env=None):
    """The buffers of one call of `api` (in_place, slots, packed) on case c: its inputs (fresh
    copies, or `inputs` shared with other read-only calls: a longer case's, used from the front)
    and its own pre-filled outputs.  Fills run on torch's stream: synchronise before launching on a
    side stream."""
    assert api in ("in_place", "slots", "packed") and not (api == "in_place" and inputs is not None)
    k, r, P, G = c.k, c.r, c.P, c.G
    b = SimpleNamespace(c=c, api=api, env=env or {}, shared=inputs is not None)
    b.dd, b.dp, b.dm = inputs if inputs is not None else upload(torch, c)
    b.st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
    if api != "in_place":
        b.out = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
    if api == "packed":
        b.rs = torch.full((G,), 0x3C3C3C3C, dtype=torch.int32, device="cuda")
        b.tot = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    return b


def launch(ctx, b, stream, monkeypatch=None):
    """Queue the call on `stream` (a torch stream; None: the context's own); returns without waiting
    for it."""
    c, s = b.c, stream.cuda_stream if stream is not None else None
    assert s != 0                                          # a side stream, not the default one
    if b.env:
        with monkeypatch.context() as mp:                  # the test library reads its switches per call
            for key, val in b.env.items():
                mp.setenv(key, val)
            return launch(ctx, SimpleNamespace(**dict(vars(b), env={})), stream)
    if b.api == "in_place":
        ctx.decode_dev(b.dd, b.dp, b.dm, c.G, c.k, c.r, c.P, b.st, stream=s)
    elif b.api == "slots":
        ctx.recover_dev(b.dd, b.dp, b.dm, c.G, c.k, c.r, c.P, b.out, b.st, stream=s)
    else:
        ctx.recover_packed_dev(b.dd, b.dp, b.dm, c.G, c.k, c.r, c.P, b.out, b.rs, b.tot, b.st, stream=s)


def check_inputs(c, dd, dp, dm):
    """The recover calls only read: data, parity (the junk of both included) and masks unchanged."""
    assert np.array_equal(dd.cpu().numpy()[:c.G * c.k * c.P], c.broken)
    assert np.array_equal(dp.cpu().numpy()[:c.G * c.r * c.P], c.par_in)
    assert np.array_equal(dm.cpu().numpy().view(np.uint64)[:c.G], c.masks_in)


def check(b, what=""):
    """After the final synchronise: everything the call wrote, and everything it must not write."""
    c = b.c
    k, r, P, G = c.k, c.r, c.P, c.G
    assert np.array_equal(b.st.cpu().numpy(), c.status), what
    assert np.array_equal(b.dm.cpu().numpy().view(np.uint64)[:G], c.masks_in), what       # masks only read, junk bits included
    if b.api == "in_place":
        assert np.array_equal(b.dd.cpu().numpy(), c.ref), (what, us.mismatch(c.masks, k, r, b.dd.cpu().numpy(), c.ref))
        assert np.array_equal(b.dp.cpu().numpy(), c.par_in), what
    elif b.api == "slots":
        assert np.array_equal(b.out.cpu().numpy().reshape(G, r, P), c.slots), \
            (what, us.mismatch(c.masks, k, r, b.out.cpu().numpy(), c.slots))              # slots m >= e still 0x5A
    else:
        n = len(c.rows)
        assert int(b.tot.item()) == n, what
        assert np.array_equal(b.rs.cpu().numpy().view(np.uint32), c.row_start), what
        o = b.out.cpu().numpy().reshape(G * r, P)
        assert np.array_equal(o[:n], c.rows), what
        assert (o[n:] == 0x5A).all(), what                 # nothing past the last rebuilt row
    if b.api != "in_place" and not b.shared:
        check_inputs(c, b.dd, b.dp, b.dm)


def fresh_context(quicfec, lib):
    return quicfec.Context(device=0, lib=lib)


def _libs(quicfec):
    return {"product": quicfec.load_library, "hooks": quicfec.load_test_library}


# ------------------------------------------------------------------------------------------
# a. Look-back epochs of the one-launch packed recover wrap
# ------------------------------------------------------------------------------------------
EPOCH_LIMIT = 16
WRAP_GROUPS = (5000, 300, 2049, 7, 4097, 1024)
WRAP_SHAPES = ((10, 3, 700, "iid"), (4, 2, 513, "perm"), (10, 2, 200, "perm"))


def _wrap_launches(G, blocks_per_launch):
    return -(-G // (blocks_per_launch * RUN_TILE))


def _wrap_plan(calls=24, streams=2, seed=3):
    """(stream, shape, G) per call: streams alternate, the first call of each is the largest (its
    workspace never grows later), the other sizes are drawn from WRAP_GROUPS; each stream's calls
    rotate over the shapes, so one workspace serves all three."""
    rng = np.random.default_rng(seed)
    plan = []
    for i in range(calls):
        G = max(WRAP_GROUPS) if i < streams else int(rng.choice(WRAP_GROUPS))
        plan.append((i % streams, WRAP_SHAPES[(i // streams) % len(WRAP_SHAPES)], G))
    return plan


def _predicted_trace(plan, streams, limit, blocks_per_launch):
    """The rule of csrc/fec_shim.cpp runs_workspace, restated: a stream's workspace counts the
    epochs its launches used since it was zeroed; a call of n launches that would bring the count
    to the limit or past it (count + n >= limit) zeroes the workspace first -- one runs_rezero
    record -- and counts from 0 again; the first call on a stream allocates (no record).  Returns
    the forms of the whole trace in call order and the re-zeroes per stream."""
    count = [0] * streams
    forms, rezeroes = [], [0] * streams
    for s, _, G in plan:
        n = _wrap_launches(G, blocks_per_launch)
        if count[s] + n >= limit:
            rezeroes[s] += 1
            count[s] = 0
            forms.append("runs_rezero")
        count[s] += n
        forms += ["recover_runs"] * n
    return forms, rezeroes


def test_runs_epochs_wrap(quicfec_mod, oracle_mod, torch_cuda, monkeypatch):
    """24 one-launch packed recovers on two side streams, no host synchronise in between, with the
    epoch limit at 16 instead of 2^30 and 1024 groups per launch (calls of 1, 3 and 5 launches):
    every stream's workspace is re-zeroed several times under queued work, serves three shapes,
    and every call's rows, row starts, total and statuses are the oracle's.  The trace shows a
    re-zero exactly where the rule predicts one (at least 5 in all)."""
    torch = torch_cuda
    assert [_wrap_launches(G, 2) for G in WRAP_GROUPS] == [5, 1, 3, 1, 5, 1]
    plan = _wrap_plan()
    forms, rezeroes = _predicted_trace(plan, 2, EPOCH_LIMIT, 2)
    assert sum(rezeroes) >= 5 and min(rezeroes) >= 2, rezeroes
    assert {G for _, _, G in plan} == set(WRAP_GROUPS)
    assert {sh for s, sh, _ in plan if s == 0} == {sh for s, sh, _ in plan if s == 1} == set(WRAP_SHAPES)
    for key, val in (("QUICFEC_PACKED_RUNS", "1"), ("QUICFEC_MAX_WAVE_BLOCKS", "2"),
                     ("QUICFEC_RUNS_EPOCH_LIMIT", str(EPOCH_LIMIT))):
        monkeypatch.setenv(key, val)
    full = {sh: _case(oracle_mod, *sh[:3], CASE_GROUPS[sh], sh[3]) for sh in WRAP_SHAPES}
    inputs = {sh: upload(torch, c) for sh, c in full.items()}          # read-only: shared by the shape's calls
    calls = [make_call(torch, _case(oracle_mod, *sh[:3], G, sh[3]), "packed", inputs=inputs[sh]) for _, sh, G in plan]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with fresh_context(quicfec_mod, quicfec_mod.load_test_library()) as ctx:
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(ctx.lib)                                # clear
        for (s, _, _), b in zip(plan, calls):
            launch(ctx, b, streams[s])
        torch.cuda.synchronize()
        trace = quicfec_mod.launch_trace(ctx.lib)
    assert [t["form"] for t in trace] == forms
    assert sum(t["form"] == "runs_rezero" for t in trace) == sum(rezeroes) >= 5
    runs = [t for t in trace if t["form"] == "recover_runs"]
    assert all(t["grid"] <= 2 and t["items"] <= 2 * RUN_TILE for t in runs)
    for i, ((s, sh, G), b) in enumerate(zip(plan, calls)):
        check(b, (i, s, sh, G))
    for sh, c in full.items():
        check_inputs(c, *inputs[sh])


# ------------------------------------------------------------------------------------------
# b. More caller streams than workspaces
# ------------------------------------------------------------------------------------------
# the forms that take a per-stream workspace: (k, r, P, api, switches)
WORKSPACE_FORMS = [
    (6, 3, 48, "in_place", {}),       # classify + the runtime-k wave kernel: record offsets
    (20, 5, 272, "slots", {}),        # record-addressed, tables through LDS: record offsets
    (10, 3, 64, "in_place", {}),      # classify + tiled: record offsets
    (10, 3, 700, "packed", {}),       # the row prefix: block sums
]
RUNS_FORM = (10, 3, 700, "packed", {"QUICFEC_PACKED_RUNS": "1"})          # recover_runs: the runs workspace


@pytest.mark.parametrize("which", ["product", "hooks"])
def test_more_streams_than_workspaces(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, which):
    """20 caller streams on one context, three rounds, no host synchronise between rounds: more
    streams than the 16 workspaces, so from the 17th on every new stream drops the least recently
    used one (after the library's device synchronise) and the streams of the next round find
    theirs gone.  The form rotates per (stream, round); all 60 calls equal the oracle."""
    torch = torch_cuda
    src = (REPO / "quic-test_amd" / "csrc" / "fec_shim.cpp").read_text()
    assert int(re.search(r"kMaxStreamWorkspaces = (\d+);", src).group(1)) == MAX_STREAM_WORKSPACES
    nstreams, rounds, G = 20, 3, 517
    assert nstreams > MAX_STREAM_WORKSPACES
    forms = WORKSPACE_FORMS + ([RUNS_FORM] if which == "hooks" else [])
    calls = []
    for rnd in range(rounds):
        for s in range(nstreams):
            k, r, P, api, env = forms[(s + rnd) % len(forms)]
            calls.append((s, make_call(torch, _case(oracle_mod, k, r, P, G), api, env=env)))   # fresh inputs per call
    assert len(calls) == 60
    streams = [torch.cuda.Stream() for _ in range(nstreams)]
    assert len({s.cuda_stream for s in streams}) == nstreams
    with fresh_context(quicfec_mod, _libs(quicfec_mod)[which]()) as ctx:
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(ctx.lib)
        for s, b in calls:
            launch(ctx, b, streams[s], monkeypatch)
        torch.cuda.synchronize()
        trace = quicfec_mod.launch_trace(ctx.lib)
    if which == "hooks":
        assert sum(t["form"] == "recover_runs" for t in trace) == sum(1 for _, b in calls if b.env)
        assert not any(t["form"] == "runs_rezero" for t in trace)      # first allocations only: no wrap
    for i, (s, b) in enumerate(calls):
        check(b, (i, s, b.api, b.c.k, b.c.r, b.c.P))


# ------------------------------------------------------------------------------------------
# c. Packed recover in flight on two streams
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,P,api,env", [
    ("product", 700, "packed", {}),                                    # row prefix: per-stream block sums
    ("hooks", 700, "packed", {"QUICFEC_PACKED_RUNS": "1"}),            # recover_runs: per-stream ticket and look-back words
    ("product", 1200, "slots", {}),                                    # mask-addressed: no workspace at all
], ids=["prefix", "runs", "slots_1200"])
def test_packed_recover_on_two_streams(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, which, P, api, env):
    """Two different batches of 4096 groups, each on its own stream, three rounds with no
    synchronise between the streams: each call's rows and row starts are its own batch's."""
    torch = torch_cuda
    k, r, G = 10, 3, 4096
    cases = [_case(oracle_mod, k, r, P, G, "perm"), _case(oracle_mod, k, r, P, G, "perm2")]
    assert not np.array_equal(cases[0].row_start, cases[1].row_start)
    inputs = [upload(torch, c) for c in cases]
    calls = [(s, make_call(torch, cases[s], api, inputs=inputs[s], env=env)) for _ in range(3) for s in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    with fresh_context(quicfec_mod, _libs(quicfec_mod)[which]()) as ctx:
        torch.cuda.synchronize()
        for s, b in calls:
            launch(ctx, b, streams[s], monkeypatch)
        torch.cuda.synchronize()
    for i, (s, b) in enumerate(calls):
        check(b, (i, s))
    for s in range(2):
        check_inputs(cases[s], *inputs[s])


# ------------------------------------------------------------------------------------------
# d. One stream, a mixed queue
# ------------------------------------------------------------------------------------------
def test_mixed_queue_on_one_stream(quicfec_mod, oracle_mod, torch_cuda):
    """Six calls of different forms queued on one side stream with no synchronise of the test's:
    the stream's one workspace serves block sums, then record offsets, grows under queued work
    (the slots call of 5000 groups), serves a larger prefix, the sparse plan's host-built records
    (k=16 r=16, which synchronises inside the call) and the tiled form."""
    torch = torch_cuda
    queue = [(10, 3, 700, 3000, "packed"), (20, 5, 300, 261, "in_place"), (6, 3, 48, 5000, "slots"),
             (10, 3, 700, 9000, "packed"), (16, 16, 32, 64, "in_place"), (10, 3, 64, 1031, "in_place")]
    calls = [make_call(torch, _case(oracle_mod, k, r, P, G), api) for k, r, P, G, api in queue]
    stream = torch.cuda.Stream()
    with fresh_context(quicfec_mod, quicfec_mod.load_library()) as ctx:
        assert ctx.decode_prepare(16, 16) == 0                         # over the dense cap: the sparse plan
        torch.cuda.synchronize()
        for b in calls:
            launch(ctx, b, stream)
        torch.cuda.synchronize()
    for q, b in zip(queue, calls):
        check(b, q)


# ------------------------------------------------------------------------------------------
# e. Several host threads on one context
# ------------------------------------------------------------------------------------------
def test_four_threads_on_one_context(quicfec_mod, oracle_mod, torch_cuda):
    """Four host threads, each with its own side stream and buffers, start from a barrier on a
    fresh context and make 12 calls each: the first calls race to build the decode plans (and the
    compact book of k=20 r=5) under the context's lock, the workspace list is shared, and one
    thread's sparse-plan calls synchronise and copy while the others wait for the lock."""
    torch = torch_cuda
    G, nthreads, ncalls = 517, 4, 12
    combos = [(6, 3, 48, "in_place"), (20, 5, 272, "slots"), (10, 3, 64, "in_place"), (10, 3, 700, "packed"),
              (6, 3, 48, "slots"), (20, 5, 272, "in_place"), (10, 3, 64, "slots"), (10, 3, 700, "slots"),
              (10, 3, 700, "in_place")]
    work = []
    for t in range(nthreads):
        mine = []
        for j in range(ncalls):
            if t == 0 and j % 4 == 1:
                mine.append(make_call(torch, _case(oracle_mod, 16, 16, 32, 64), "in_place"))      # the sparse plan
            else:
                k, r, P, api = combos[(5 * t + j) % len(combos)]
                mine.append(make_call(torch, _case(oracle_mod, k, r, P, G), api))
        work.append(mine)
    assert {b.api for mine in work for b in mine} == {"in_place", "slots", "packed"}
    streams = [torch.cuda.Stream() for _ in range(nthreads)]
    barrier = threading.Barrier(nthreads)
    errors = []

    def run(t, ctx):
        try:
            barrier.wait(timeout=60)
            for b in work[t]:
                launch(ctx, b, streams[t])
        except BaseException as e:                                     # re-raised in the test
            errors.append((t, e))

    with fresh_context(quicfec_mod, quicfec_mod.load_library()) as ctx:
        torch.cuda.synchronize()
        threads = [threading.Thread(target=run, args=(t, ctx)) for t in range(nthreads)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
    if errors:
        raise errors[0][1]
    for t, mine in enumerate(work):
        for j, b in enumerate(mine):
            check(b, (t, j, b.api, b.c.k, b.c.r, b.c.P))


# ------------------------------------------------------------------------------------------
# f. A pipeline queued on a side stream: stream order is the only order
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P,G", [(10, 3, 1200, 1031), (20, 5, 1200, 1031), (6, 3, 48, 1031), (16, 16, 32, 131)])
def test_queued_pipeline_on_side_stream(quicfec_mod, oracle_mod, torch_cuda, k, r, P, G):
    """fill -> encode -> every shard the rule does not read overwritten with the case's junk (a
    torch op) -> masks copied in (a torch copy) ->
    the decode calls, all queued on one non-blocking side stream with one synchronise at the end.
    Nothing but stream order makes a call see its producer's bytes: before the chain runs the data
    is 0x11, the parity 0x5A and the masks say "every shard lost".  The data are the oracle's
    splitmix bytes of the same seed (test_fill_random_matches_oracle pins the fill kernel to them).
    k=16 r=16 takes the sparse plan, whose call reads the masks on the host: it must have waited
    for the copy that produces them."""
    torch = torch_cuda
    c = _case(oracle_mod, k, r, P, G)
    sparse = (k, r) == (16, 16)
    packed_ok = (k, r) == (10, 3)                                      # the other shapes: refused, nothing written
    ro = us.roles(c.masks, k, r)
    d_junk_d, d_junk_p = _dev(torch, ro.lost_d), _dev(torch, ro.unread_p)       # which shards get junk
    d_broken, d_par_in = _dev(torch, c.broken).view(G, k, P), _dev(torch, c.par_in).view(G, r, P)   # where it comes from
    d_masks_src = _dev(torch, c.masks_in.view(np.int64))
    dd = torch.full((G * k * P,), 0x11, dtype=torch.uint8, device="cuda")
    par = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
    dm = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    slots = make_call(torch, c, "slots", inputs=(dd, par, dm))
    packed = make_call(torch, c, "packed", inputs=(dd, par, dm))
    st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with fresh_context(quicfec_mod, quicfec_mod.load_library()) as ctx:
        torch.cuda.synchronize()                                       # the fills above; nothing below waits on the host
        ctx.fill_random_dev(dd, G * k * P, c.seed, 0, stream=s)
        ctx.encode_dev(dd, G, k, r, P, par, stream=s)
        with torch.cuda.stream(stream):
            par_made = par.clone()
            dd.view(G, k, P).copy_(torch.where(d_junk_d[:, :, None], d_broken, dd.view(G, k, P)))     # no host wait
            par.view(G, r, P).copy_(torch.where(d_junk_p[:, :, None], d_par_in, par.view(G, r, P)))
            dm.copy_(d_masks_src, non_blocking=True)
        if not sparse:
            launch(ctx, slots, stream)
            if packed_ok:
                launch(ctx, packed, stream)
            else:
                with pytest.raises(quicfec_mod.FecError) as ei:
                    launch(ctx, packed, stream)
                assert ei.value.code == quicfec_mod.FEC_ERR_RANGE
            with torch.cuda.stream(stream):
                broken_seen = dd.clone()                               # what the recover calls read
        ctx.decode_dev(dd, par, dm, G, k, r, P, st, stream=s)
        torch.cuda.synchronize()
    assert np.array_equal(par_made.cpu().numpy(), c.par)
    assert np.array_equal(dm.cpu().numpy().view(np.uint64), c.masks_in)
    assert np.array_equal(st.cpu().numpy(), c.status)
    assert np.array_equal(dd.cpu().numpy(), c.ref)
    assert np.array_equal(par.cpu().numpy(), c.par_in)                 # chosen rows as encoded, the rest junk still
    if not sparse:
        assert np.array_equal(broken_seen.cpu().numpy(), c.broken)
        check(slots)
        if packed_ok:
            check(packed)
        else:
            assert bool((packed.out == 0x5A).all()) and bool((packed.rs == 0x3C3C3C3C).all())
            assert int(packed.tot.item()) == -5 and bool((packed.st == 7).all())


# ------------------------------------------------------------------------------------------
# g. Freeing a context with work queued on a caller stream
# ------------------------------------------------------------------------------------------
def test_free_with_work_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """An encode and a mask-addressed in-place decode (k=10 r=3 at 1200 B: neither takes a
    workspace, both read the plans' tables) queued on a side stream, and the context freed at once:
    fec_encoder_free waits for calls queued on caller streams (include/fec_hip.h), so both outputs
    are complete and right after it."""
    torch = torch_cuda
    k, r, P, G = 10, 3, 1200, 4096
    c = _case(oracle_mod, k, r, P, G)
    d_data = _dev(torch, c.data)
    d_par = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
    dec = make_call(torch, c, "in_place")
    stream = torch.cuda.Stream()
    ctx = fresh_context(quicfec_mod, quicfec_mod.load_library())
    torch.cuda.synchronize()
    ctx.encode_dev(d_data, G, k, r, P, d_par, stream=stream.cuda_stream)
    launch(ctx, dec, stream)
    ctx.close()
    assert stream.query()                                              # the free drained the stream
    torch.cuda.synchronize()
    assert np.array_equal(d_par.cpu().numpy(), c.par)
    assert np.array_equal(d_data.cpu().numpy(), c.data)
    check(dec)
