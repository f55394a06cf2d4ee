"""The wide calls on the GPU: fec_decode_wide_rs_dev (in place) and fec_recover_wide_rs_dev (slots)
for k + r <= 256 with four mask words per group.

The oracle's decode stops at 64 shards, so the truth for a rebuilt row is the original data: data is
seeded, parity is oracle.rs_encode's (which serves k + r <= 256), and then seeded junk goes into
every lost data shard and every parity row the rule does not read (tests/wide_masks.py assigns the
roles).  A decoder that picks a wrong row reads junk and fails; a correct one returns the original
bytes from any valid rows.  Every mask carries junk in the bits of the partial word above k + r and
all ones in every whole word above it.  Statuses are pre-filled 0xAA, outputs 0x5A between guard
bytes, every case goes through both calls on a side stream, G = 67 unless said otherwise.
"""
import os
import threading
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import wide_masks as wm
from test_gpu_gather import hooks_ctx, product_ctx

pytestmark = pytest.mark.gpu

SEED = 0x71DE0000
G_MAIN = 67
GUARD = 256
# (k, r, sizes): the word boundaries, the extremes and the pass counts
SHAPES = [(60, 5, (16, 272, 1200)),       # bit 64 is a parity row
          (64, 2, (16, 1200)),            # the data fills word 0
          (65, 3, (48,)),
          (127, 3, (272,)),               # the rows straddle bit 128
          (190, 5, (48,)),                # the rows straddle bit 192
          (224, 32, (16, 1200)),          # bit 255; e = 32, four row passes
          (32, 224, (48,)),               # the chosen rows reach into words 2-3
          (255, 1, (16,)),
          (1, 255, (16,)),
          (100, 20, (1037, 1200, 4096))]  # an odd size; four whole 1-KiB passes
BOUNDARY_BITS = (63, 64, 127, 128, 191, 192)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


# ------------------------------------------------------------------------------------------
# Cases
# ------------------------------------------------------------------------------------------
def _group(k, lost_data=(), lost_rows=()):
    b = np.zeros(256, dtype=bool)
    b[list(lost_data)] = True
    b[[k + i for i in lost_rows]] = True
    return b


def _spread(n, count):
    """`count` of range(n), evenly spread, first and last included when count >= 2."""
    return sorted({int(x) for x in np.linspace(0, n - 1, count).round()}) if count > 1 else [n // 2]


def planted_groups(k, r):
    """{kind: [256 bools]} of the groups every case plants (the module docstring of the issue's list);
    a kind the shape cannot hold (r = 1 has no 'row 0 lost' rebuild, k = 1 no pair) is absent."""
    emax = min(k, r)
    out = {"untouched": [_group(k)], "parity_only": [_group(k, (), [0])]}
    t = min(2, k, r)
    out["short_by_one"] = [_group(k, range(t), range(r - t + 1))]              # t lost, t - 1 rows alive
    # recoverable to a reader of word 0 alone: its losses above bit 63 are what refuses it
    out["short_above_word_0"] = [_group(k, [0], range(r))]
    out["xor"] = [_group(k, [k // 2])]
    if r >= 2:
        out["single_row_0_lost"] = [_group(k, [k // 3], [0])]
        out["single_top_row"] = [_group(k, [k - 1], range(r - 1))]
    if emax >= 2:
        out["first_and_last"] = [_group(k, [0, k - 1])]
    out["full_lowest_rows"] = [_group(k, range(emax))]
    out["full_highest_rows"] = [_group(k, range(k - emax, k), range(r - emax))]
    full_spread = _spread(k, emax)
    full_spread += [j for j in range(k) if j not in full_spread][:emax - len(full_spread)]
    alive = _spread(r, emax)
    alive += [i for i in range(r) if i not in alive][:emax - len(alive)]
    out["full_spread"] = [_group(k, full_spread, [i for i in range(r) if i not in alive])]
    at = [s for s in BOUNDARY_BITS if s < k]
    if at:
        out["boundary_data"] = [_group(k, at[i:i + emax]) for i in range(0, len(at), emax)]
    straddle = [B for B in (64, 128, 192) if k <= B - 1 and B <= k + r - 1] if emax >= 2 else []
    if straddle:                                                               # rows B-1-k and B-k, every lower row lost
        out["rows_straddle"] = [_group(k, [1, k - 2] if k >= 4 else [0, 1], range(B - 1 - k)) for B in straddle]
    return out


def drawn_group(k, r, rng):
    emax = min(k, r)
    e = int(rng.integers(1, emax + 1))
    lost_rows = int(rng.integers(0, r - e + 1))
    return _group(k, rng.choice(k, size=e, replace=False), rng.choice(r, size=lost_rows, replace=False))


class Case:
    def __init__(self, oracle, k, r, P, bits, seed, check_planted=None):
        self.k, self.r, self.P, self.G, self.seed = k, r, P, len(bits), seed
        G = self.G
        self.masks = wm.with_high_junk(wm.from_bits(bits), k, r, seed)
        self.ro = ro = wm.roles(self.masks, k, r)
        self.e = ro.lost_d.sum(axis=1)
        self.rebuilds = ro.ok & (self.e >= 1)
        self.status = wm.status(ro)
        self.data = oracle.splitmix_bytes(G * k * P, seed)
        self.par = oracle.rs_encode(self.data, G, k, r, P)
        self.d_in, self.p_in = wm.inputs(self.data, self.par, ro, P, seed + 1)
        # in place: a recoverable group ends as the original data, any other stays as it came
        keep = np.repeat(~ro.ok, k * P)
        self.ref = np.where(keep, self.d_in, self.data)
        self.slots = np.full((G, r, P), 0x5A, dtype=np.uint8)
        orig = self.data.reshape(G, k, P)
        for g in np.flatnonzero(self.rebuilds):
            lost = np.flatnonzero(ro.lost_d[g])
            self.slots[g, :len(lost)] = orig[g, lost]
        # on the CPU, before anything is launched
        top = -(-(k + r) // 64) * 64
        assert wm.to_bits(self.masks)[:, top:].all()
        if check_planted is not None:
            for kind, groups in check_planted.items():
                for g, want in groups:
                    assert np.array_equal(wm.to_bits(self.masks)[g, :k + r], want[:k + r]), kind
            assert self.rebuilds.sum() * 4 >= 3 * G, "fewer than three quarters of the groups are rebuilt"


def check_kinds(c, planted):
    """The planted kinds do what their names say, by the numpy rule."""
    k, r, ro, emax = c.k, c.r, c.ro, min(c.k, c.r)
    first = {kind: groups[0][0] for kind, groups in planted.items()}
    g = first["untouched"]
    assert not ro.lost_d[g].any() and not ro.lost_p[g].any()
    g = first["parity_only"]
    assert not ro.lost_d[g].any() and ro.lost_p[g].any() and c.status[g] == 0
    g = first["short_by_one"]
    assert c.status[g] == 1 and c.e[g] == (~ro.lost_p[g]).sum() + 1
    g = first["short_above_word_0"]
    assert c.status[g] == 1
    if k + r > 64:                                                             # word 0 alone says recoverable
        low = wm.to_bits(c.masks)[g].copy()
        low[64:] = False
        assert wm.roles(wm.from_bits(low[None, :]), k, r).ok[0]
    g = first["xor"]
    assert c.rebuilds[g] and c.e[g] == 1 and ro.chosen[g, 0]
    if "single_row_0_lost" in first:
        g = first["single_row_0_lost"]
        assert c.rebuilds[g] and c.e[g] == 1 and ro.lost_p[g, 0] and ro.chosen[g, 1]
        g = first["single_top_row"]
        assert c.rebuilds[g] and c.e[g] == 1 and ro.chosen[g].tolist() == [False] * (r - 1) + [True]
    if "first_and_last" in first:
        g = first["first_and_last"]
        assert c.rebuilds[g] and ro.lost_d[g, 0] and ro.lost_d[g, k - 1]
    for kind in ("full_lowest_rows", "full_highest_rows", "full_spread"):
        g = first[kind]
        assert c.rebuilds[g] and c.e[g] == emax, kind
    assert ro.chosen[first["full_lowest_rows"], :emax].all() and ro.chosen[first["full_highest_rows"], r - emax:].all()
    seen = set()
    for g, _ in planted.get("boundary_data", []):
        assert c.rebuilds[g]
        seen |= set(np.flatnonzero(ro.lost_d[g]).tolist())
    assert seen == {s for s in BOUNDARY_BITS if s < k}
    for g, _ in planted.get("rows_straddle", []):
        rows = np.flatnonzero(ro.chosen[g])
        assert c.rebuilds[g] and len(rows) == 2 and (k + rows[0]) % 64 == 63 and rows[1] == rows[0] + 1
        assert ro.lost_p[g, :rows[0]].all()


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
    if k + r > 64:
        assert {"untouched", "parity_only", "short_by_one", "short_above_word_0", "xor", "full_lowest_rows",
                "full_highest_rows", "full_spread"} <= set(planted)
    check_kinds(c, planted)
    return c


# ------------------------------------------------------------------------------------------
# Calls
# ------------------------------------------------------------------------------------------
def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(torch, nbytes, fill):
    whole = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def make_call(torch, c, api):
    """Device buffers of one call: in_place (the data between guards, rebuilt there) or slots."""
    b = SimpleNamespace(c=c, api=api)
    b.dwhole, b.dd = _guarded(torch, c.G * c.k * c.P, 0x5A)
    b.dd.copy_(_dev(torch, c.d_in))
    b.dp = _dev(torch, c.p_in)
    b.dm = _dev(torch, c.masks.view(np.int64).reshape(-1))
    b.swhole, b.st = _guarded(torch, c.G, 0xAA)
    if api == "slots":
        b.owhole, b.out = _guarded(torch, c.G * c.r * c.P, 0x5A)
    return b


def launch(ctx, b, stream=None, st=True):
    c, s = b.c, stream.cuda_stream if stream is not None else None
    if b.api == "slots":
        ctx.recover_wide_dev(b.dd, b.dp, b.dm, c.G, c.k, c.r, c.P, b.out, b.st if st else None, stream=s)
    else:
        ctx.decode_wide_dev(b.dd, b.dp, b.dm, c.G, c.k, c.r, c.P, b.st if st else None, stream=s)


def _guards_intact(whole, fill):
    w = whole.cpu().numpy()
    return (w[:GUARD] == fill).all() and (w[-GUARD:] == fill).all()


def _first_wrong(c, got, want):
    G = c.G
    wrong = (np.asarray(got).reshape(G, -1) != np.asarray(want).reshape(G, -1)).any(axis=1)
    if not wrong.any():
        return "equal"
    g = int(np.flatnonzero(wrong)[0])
    return (f"group {g} lost data {np.flatnonzero(c.ro.lost_d[g]).tolist()} lost rows {np.flatnonzero(c.ro.lost_p[g]).tolist()} "
            f"chosen {np.flatnonzero(c.ro.chosen[g]).tolist()} ok {bool(c.ro.ok[g])} ({int(wrong.sum())} groups differ)")


def check(b, what="", status=True):
    c = b.c
    what = (what, b.api, c.k, c.r, c.P)
    if status:
        st = b.st.cpu().numpy()
        assert np.array_equal(st, c.status), (what, "status", _first_wrong(c, st, c.status))
    else:
        assert (b.st.cpu().numpy() == 0xAA).all(), what
    assert _guards_intact(b.swhole, 0xAA) and _guards_intact(b.dwhole, 0x5A), what
    assert np.array_equal(b.dp.cpu().numpy(), c.p_in), (what, "parity changed")
    assert np.array_equal(b.dm.cpu().numpy().view(np.uint64).reshape(-1, 4), c.masks), (what, "masks changed")
    dd = b.dd.cpu().numpy()
    if b.api == "slots":
        out = b.out.cpu().numpy()
        # rebuilt rows are the original data; slots m >= e and unrecoverable groups' slots are still 0x5A
        assert np.array_equal(out.reshape(c.G, c.r, c.P), c.slots), (what, "slots", _first_wrong(c, out, c.slots))
        assert _guards_intact(b.owhole, 0x5A), what
        assert np.array_equal(dd, c.d_in), (what, "data changed")
    else:
        # rebuilt in place; surviving shards and an unrecoverable group's junk unchanged
        assert np.array_equal(dd, c.ref), (what, "in place", _first_wrong(c, dd, c.ref))


def run_both(torch, ctx, c, what=""):
    stream = torch.cuda.Stream()
    calls = [make_call(torch, c, "in_place"), make_call(torch, c, "slots")]
    torch.cuda.synchronize()
    for b in calls:
        launch(ctx, b, stream)
    torch.cuda.synchronize()
    for b in calls:
        check(b, what)
    return calls


# ------------------------------------------------------------------------------------------
# 1. Shapes and sizes
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,sizes", SHAPES)
def test_shapes_and_sizes(quicfec_mod, oracle_mod, torch_cuda, k, r, sizes):
    """Both calls at every size of the shape: rebuilt rows equal the original data, every status byte,
    untouched slots, guards, and the inputs each call only reads."""
    with product_ctx(quicfec_mod) as ctx:
        for P in sizes:
            run_both(torch_cuda, ctx, main_case(oracle_mod, k, r, P))


def test_status_is_nullable(quicfec_mod, oracle_mod, torch_cuda):
    torch = torch_cuda
    c = main_case(oracle_mod, 60, 5, 272)
    with product_ctx(quicfec_mod) as ctx:
        calls = [make_call(torch, c, "in_place"), make_call(torch, c, "slots")]
        for b in calls:
            launch(ctx, b, torch.cuda.Stream(), st=False)
        torch.cuda.synchronize()
    for b in calls:
        check(b, "no status", status=False)


# ------------------------------------------------------------------------------------------
# 2. Single and double losses
# ------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def losses_case(oracle, k, r, P, pairs):
    n = k + r
    sets = [()] + [(s,) for s in range(n)] + ([(a, b) for a in range(n) for b in range(a + 1, n)] if pairs else [])
    bits = np.zeros((len(sets), 256), dtype=bool)
    for g, lost in enumerate(sets):
        bits[g, list(lost)] = True
    return Case(oracle, k, r, P, bits, SEED + 77 * k + r)


@pytest.mark.parametrize("k,r,pairs,groups", [(60, 5, True, 2146), (224, 32, False, 257), (32, 224, False, 257),
                                              (255, 1, False, 257), (1, 255, False, 257)])
def test_every_single_loss(quicfec_mod, oracle_mod, torch_cuda, k, r, pairs, groups):
    """Every single lost shard (60+5: also none and every pair) at 16 B."""
    c = losses_case(oracle_mod, k, r, 16, pairs)
    assert c.G == groups and (c.status == 0).all()
    with product_ctx(quicfec_mod) as ctx:
        run_both(torch_cuda, ctx, c)


# ------------------------------------------------------------------------------------------
# 3. One-word shapes through the wide calls
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,P", [(10, 3, 1200), (16, 16, 32), (32, 32, 16)])
def test_one_word_shapes_equal_the_one_word_calls(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """k + r <= 64: byte-equal to fec_recover_batch_rs_dev and fec_decode_batch_rs_dev on the same case,
    words 1..3 holding junk (all ones) and word 0 junk above k + r."""
    torch = torch_cuda
    c = main_case(oracle_mod, k, r, P)
    assert (c.masks[:, 1:] == np.iinfo(np.uint64).max).all()
    with product_ctx(quicfec_mod) as ctx:
        wide = run_both(torch, ctx, c)
        narrow = [make_call(torch, c, "in_place"), make_call(torch, c, "slots")]
        for b in narrow:
            b.dm = _dev(torch, c.masks[:, 0].copy().view(np.int64))
        torch.cuda.synchronize()
        ctx.decode_dev(narrow[0].dd, narrow[0].dp, narrow[0].dm, c.G, k, r, P, narrow[0].st)
        ctx.recover_dev(narrow[1].dd, narrow[1].dp, narrow[1].dm, c.G, k, r, P, narrow[1].out, narrow[1].st)
        ctx.synchronize()
        torch.cuda.synchronize()
    for w, n in zip(wide, narrow):
        assert np.array_equal(w.dwhole.cpu().numpy(), n.dwhole.cpu().numpy()), (w.api, "data")
        assert np.array_equal(w.swhole.cpu().numpy(), n.swhole.cpu().numpy()), (w.api, "status")
    assert np.array_equal(wide[1].owhole.cpu().numpy(), narrow[1].owhole.cpu().numpy())


# ------------------------------------------------------------------------------------------
# 4. Chunks and the launch trace
# ------------------------------------------------------------------------------------------
def _stride(k, r):
    return 512 + min(k, r) * k * 32                                            # fec_forms.hpp wide_slot_stride


def expected_trace(G, per_chunk, passes, wave_groups, slots):
    """DESIGN §5b "Wide shapes": classify_wide over [0, G); per plan chunk build_records_wide, then
    ceil(min(k, r) / 8) passes of decode_wide; each wave-per-group launch at most wave_groups groups.
    (form, first group, groups, aux, pol)."""
    pol = 2 | 4 | (1024 if slots else 0)                                       # NT stores, no coefficient branch, slots
    out = [("classify_wide", 0, G, -1, -1)]
    for c0 in range(0, G, per_chunk):
        cn = min(per_chunk, G - c0)
        pieces = [(g0, min(wave_groups, cn - g0)) for g0 in range(0, cn, wave_groups)]
        out += [("build_records_wide", c0 + g0, gn, g0, -1) for g0, gn in pieces]
        for p in range(passes):
            out += [("decode_wide", c0 + g0, gn, 8 * p, pol) for g0, gn in pieces]
    return out


def _trace(quicfec, lib):
    return [(t["form"], t["first_item"], t["items"], t["aux"], t["pol"]) for t in quicfec.launch_trace(lib)]


@pytest.mark.parametrize("k,r,P", [(100, 20, 48), (224, 32, 16)])
def test_chunked_walk(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P):
    """The test library at its defaults, with 12 groups per wave-per-group launch, with the arena
    lowered to five groups per chunk and to below one stride (one per chunk): results as ever, and
    the launches the design's table names, the chunks covering [0, G) once, in order."""
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    c = main_case(oracle_mod, k, r, P)
    G, passes = c.G, -(-min(k, r) // 8)
    settings = [({}, G, 1 << 40), ({"QUICFEC_MAX_WAVE_BLOCKS": "3"}, G, 12),
                ({"QUICFEC_MAX_WAVE_BLOCKS": "3", "QUICFEC_PLAN_ARENA_BYTES": str(5 * _stride(k, r))}, 5, 12),
                ({"QUICFEC_MAX_WAVE_BLOCKS": "3", "QUICFEC_PLAN_ARENA_BYTES": str(_stride(k, r) - 1)}, 1, 12)]
    with hooks_ctx(quicfec_mod) as ctx:
        for env, per_chunk, wave_groups in settings:
            for name in ("QUICFEC_MAX_WAVE_BLOCKS", "QUICFEC_PLAN_ARENA_BYTES"):
                monkeypatch.delenv(name, raising=False)
            for name, value in env.items():
                monkeypatch.setenv(name, value)
            calls = [make_call(torch, c, "in_place"), make_call(torch, c, "slots")]
            torch.cuda.synchronize()
            quicfec_mod.launch_trace(lib)
            for b in calls:
                launch(ctx, b, torch.cuda.current_stream())
            ctx.synchronize()
            torch.cuda.synchronize()
            trace = _trace(quicfec_mod, lib)
            for b in calls:
                check(b, env)
            want = expected_trace(G, per_chunk, passes, wave_groups, False) + expected_trace(G, per_chunk, passes, wave_groups, True)
            assert trace == want, env
            builds = [(t[1], t[2]) for t in trace[:len(trace) // 2] if t[0] == "build_records_wide"]
            assert builds[0][0] == 0 and sum(n for _, n in builds) == G
            assert all(a[0] + a[1] == b[0] for a, b in zip(builds, builds[1:]))


# ------------------------------------------------------------------------------------------
# 5. State across calls
# ------------------------------------------------------------------------------------------
def test_three_shapes_queued_on_one_stream(quicfec_mod, oracle_mod, torch_cuda):
    """Three calls of different shapes back to back on one side stream, no host synchronise between
    them, each needing a larger workspace than the one before."""
    torch = torch_cuda
    cases = [main_case(oracle_mod, 60, 5, 16), main_case(oracle_mod, 100, 20, 1037), main_case(oracle_mod, 224, 32, 16)]
    assert _stride(60, 5) < _stride(100, 20) < _stride(224, 32)
    stream = torch.cuda.Stream()
    with product_ctx(quicfec_mod) as ctx:
        calls = [make_call(torch, c, api) for c, api in zip(cases, ("slots", "in_place", "slots"))]
        calls.append(make_call(torch, cases[0], "in_place"))                   # and a small one after the largest
        torch.cuda.synchronize()
        for b in calls:
            launch(ctx, b, stream)
        torch.cuda.synchronize()
    for i, b in enumerate(calls):
        check(b, i)


def test_two_threads_on_two_streams(quicfec_mod, oracle_mod, torch_cuda):
    """Two host threads, each with its own side stream and a different shape, six calls each on one
    context from a barrier: each stream's records are its own workspace's."""
    torch = torch_cuda
    cases = [main_case(oracle_mod, 60, 5, 272), main_case(oracle_mod, 100, 20, 1037)]
    work = [[make_call(torch, cases[t], ("in_place", "slots")[j % 2]) for j in range(6)] for t in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2)
    errors = []

    def run(t, ctx):
        try:
            barrier.wait(timeout=60)
            for b in work[t]:
                launch(ctx, b, streams[t])
        except BaseException as e:                                             # re-raised in the test
            errors.append((t, e))

    with product_ctx(quicfec_mod) as ctx:
        torch.cuda.synchronize()
        threads = [threading.Thread(target=run, args=(t, ctx)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        torch.cuda.synchronize()
    if errors:
        raise errors[0][1]
    for t in range(2):
        for j, b in enumerate(work[t]):
            check(b, (t, j))


def test_free_with_wide_calls_in_flight(quicfec_mod, oracle_mod, torch_cuda):
    """Both calls queued on a side stream and the context freed at once: fec_encoder_free drains them
    (they read the context's parity matrix and the stream's workspace), so both outputs are complete."""
    torch = torch_cuda
    c = main_case(oracle_mod, 100, 20, 4096)
    calls = [make_call(torch, c, "slots"), make_call(torch, c, "in_place")]
    stream = torch.cuda.Stream()
    ctx = product_ctx(quicfec_mod)
    torch.cuda.synchronize()
    for b in calls:
        launch(ctx, b, stream)
    ctx.close()
    assert stream.query()                                                      # the free drained the stream
    torch.cuda.synchronize()
    for b in calls:
        check(b)


# ------------------------------------------------------------------------------------------
# 6. Refusals
# ------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(quicfec_mod, oracle_mod, torch_cuda):
    """200+57, 33+33, 100+100, P = 15, G = 0 and each NULL pointer: the code, a message naming the
    case, nothing launched, outputs and statuses untouched.  The one-word calls still refuse 60+5."""
    torch = torch_cuda
    q = quicfec_mod
    lib = q.load_test_library()
    c = main_case(oracle_mod, 60, 5, 16)
    G = c.G
    with hooks_ctx(q) as ctx:
        b = make_call(torch, c, "slots")
        torch.cuda.synchronize()
        q.launch_trace(lib)
        p = lambda t: t.data_ptr()
        for (k, r, P, groups), text in (((200, 57, 16, G), "k+r<=256"), ((33, 33, 16, G), "min(k, r)"), ((100, 100, 16, G), "min(k, r)"),
                                        ((60, 5, 15, G), "below 16"), ((60, 5, 16, 0), "num_groups is 0")):
            for call in (lambda: ctx.decode_wide_dev(b.dd, b.dp, b.dm, groups, k, r, P, b.st),
                         lambda: ctx.recover_wide_dev(b.dd, b.dp, b.dm, groups, k, r, P, b.out, b.st)):
                with pytest.raises(q.FecError) as ei:
                    call()
                assert ei.value.code == q.FEC_ERR_RANGE and text in ctx.last_error(), (k, r, P, groups, ctx.last_error())
        args = [ctx.handle, p(b.dd), p(b.dp), p(b.dm), G, 60, 5, 16]
        for i, name in ((0, "context"), (1, "d_data"), (2, "d_parity"), (3, "d_erasure_masks")):
            bad = list(args)
            bad[i] = None
            assert lib.fec_decode_wide_rs_dev(*bad, p(b.st), None) == q.FEC_ERR_NULL
            assert name in q.last_error(lib)
            assert lib.fec_recover_wide_rs_dev(*bad, p(b.out), p(b.st), None) == q.FEC_ERR_NULL
            assert name in q.last_error(lib)
        assert lib.fec_recover_wide_rs_dev(*args, None, p(b.st), None) == q.FEC_ERR_NULL and "d_rebuilt" in q.last_error(lib)
        for call in (lambda: ctx.decode_dev(b.dd, b.dp, b.dm, G, 60, 5, 16, b.st),
                     lambda: ctx.recover_dev(b.dd, b.dp, b.dm, G, 60, 5, 16, b.out, b.st)):
            with pytest.raises(q.FecError) as ei:
                call()
            assert ei.value.code == q.FEC_ERR_RANGE
        ctx.synchronize()
        torch.cuda.synchronize()
        assert q.launch_trace(lib) == []
        assert (b.owhole == 0x5A).all().item() and (b.swhole == 0xAA).all().item()
        assert np.array_equal(b.dd.cpu().numpy(), c.d_in) and np.array_equal(b.dp.cpu().numpy(), c.p_in)
        launch(ctx, b)                                                         # and the same buffers are served
        ctx.synchronize()
    check(b)
