"""FEC_PLAN_DEVICE on the GPU: the shapes whose decode codebook is past the 2 GiB cap (12+12, 20+7,
16+16, 32+32, 60+4), their recovery records built on the device per call, through the two
contiguous device calls and the three address-table recovers.  Bit-exact against the oracle
(rs_decode) on the contiguous equivalent, no tolerance.

Contexts are product-library contexts switched to FEC_PLAN_DEVICE unless a test needs the launch
trace or a switch.  The table-recover cases, arenas, guards and checks are those of
test_gpu_gather.py, test_gpu_gather_var.py, test_gpu_scatter.py and test_gpu_address_limits.py,
taken by import (0xEE arenas, 0x5A outputs between guard bytes, 7 in the statuses); the contiguous
calls' are test_gpu_streams.py's, with the statuses pre-filled 0xAA and, like them, masks with junk
in the bits at and above k + r (12+12, 20+7 and 16+16 have such bits, and build_records reads the
masks on the device; the table recovers derive their masks from the tables).  Every case is G = 67 (more
than one workgroup of four waves, no multiple of 4) or G = 131.
"""
import os
import threading
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

import test_gpu_gather as fx
import test_gpu_gather_var as var
import test_gpu_scatter as sc
import test_gpu_streams as st
import unread_shards as us
from test_gpu_address_limits import G_MAIN, check_limit_case, limit_masks
from test_gpu_gather import hooks_ctx, product_ctx
from test_gpu_gather_var import dealt_lengths, edge_lengths

pytestmark = pytest.mark.gpu

SEED = 0xDE71CE00
# (k, r, sizes): one row pass (r <= 8), two (r = 12, 16), four at k + r = 64 with e = 32; 7 B is the byte kernel
SHAPES = [(12, 12, (7, 32, 45)), (20, 7, (48,)), (16, 16, (32, 1200)), (32, 32, (16,)), (60, 4, (16,))]
TABLE_SHAPES = [(k, r, tuple(P for P in sizes if P >= 16)) for k, r, sizes in SHAPES]


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    """Every case starts from the library's own choice: no test switch set."""
    for name in [n for n in os.environ if n.startswith("QUICFEC_")]:
        monkeypatch.delenv(name)


def device_plan(quicfec, ctx):
    ctx.decode_plan_mode(quicfec.FEC_PLAN_DEVICE)
    return ctx


def _bits(shards):
    return sum(1 << int(s) for s in shards)


def plan_masks(k, r, seed):
    """limit_masks (untouched, parity-only loss, unrecoverable, e = 1 with and without parity row 0,
    shards 0 and k - 1, the top parity row) and, in groups 10..12, e = min(k, r): the lowest data
    shards with the lowest rows alive; the highest data shards with (r > k) the lowest r - k rows
    lost, so the record's rows are the top ones; every other data shard from 0 and from k - 1."""
    masks = limit_masks(k, r, seed)
    e = min(k, r)
    spread = sorted(set(list(range(0, k, 2))[:(e + 1) // 2] + list(range(k - 1, -1, -2))[:e // 2]))
    spread += [j for j in range(k) if j not in spread][:e - len(spread)]
    masks[10:13] = np.array([_bits(range(e)), _bits(range(k - e, k)) | _bits(range(k, k + r - e)),
                             _bits(spread) | (_bits(range(k, k + r - e)))], dtype=np.uint64)
    return masks


def check_plan_masks(c):
    """What a device-plan case must hold, on the CPU before anything is launched."""
    k, r = c.k, c.r
    lost_d, ok = c.lost[:, :k], c.status == 0
    e, row0_lost = lost_d.sum(axis=1), c.lost[:, k]
    assert (c.masks == 0).any() and (c.status == 1).any()
    assert ((e == 0) & c.lost[:, k:].any(axis=1)).any()                      # parity-only loss
    assert ((e == 1) & ok & ~row0_lost).any() and ((e == 1) & ok & row0_lost).any()
    assert ((e == min(k, r)) & ok).sum() >= 3
    assert (lost_d[:, 0] & lost_d[:, k - 1] & ok).any()


@lru_cache(maxsize=None)
def contiguous_case(oracle, k, r, P):
    salt = k * 100000 + r * 10000 + P
    c = st.Case(oracle, k, r, P, plan_masks(k, r, salt), SEED + salt)
    c.lost = ((c.masks[:, None] >> np.arange(k + r, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    check_plan_masks(c)
    return c


@lru_cache(maxsize=None)
def table_cases(oracle, k, r, P):
    """limit_cases of test_gpu_address_limits.py on plan_masks: fixed-length shards, lengths dealt
    from edge_lengths(P), and every length P (the NULL length table)."""
    salt = k * 100000 + r * 10000 + P
    masks = plan_masks(k, r, salt)
    full = np.full((G_MAIN, k + r), P)
    cs = SimpleNamespace(
        fixed=fx.make_case(oracle, k, r, P, masks, SEED + salt),
        lens=var.make_case(oracle, k, r, P, masks, dealt_lengths(P, G_MAIN, k), dealt_lengths(P, G_MAIN, r, shift=k),
                           SEED + salt + 1),
        full=var.make_case(oracle, k, r, P, masks, full[:, :k], full[:, k:], SEED + salt + 2))
    for c in (cs.fixed, cs.lens, cs.full):
        check_limit_case(c)
        check_plan_masks(c)
    assert set(edge_lengths(P).tolist()) <= set(cs.lens.lens[:, :k].reshape(-1).tolist())
    return cs


def make_call(torch, c, api):
    b = st.make_call(torch, c, api)
    b.st.fill_(0xAA)                                                         # every status byte must be written
    return b


# ------------------------------------------------------------------------------------------
# 4. Contiguous calls
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,r,sizes", SHAPES)
def test_contiguous_calls(quicfec_mod, oracle_mod, torch_cuda, k, r, sizes):
    """fec_decode_batch_rs_dev in place and fec_recover_batch_rs_dev into slots, on a side stream:
    rebuilt bytes, every status byte (pre-filled 0xAA), slots m >= e still 0x5A, and in recover mode
    data, parity and masks unchanged."""
    torch = torch_cuda
    stream = torch.cuda.Stream()
    with device_plan(quicfec_mod, product_ctx(quicfec_mod)) as ctx:
        assert ctx.decode_prepare(k, r) == 0                                 # past the cap: no codebook in either mode
        for P in sizes:
            c = contiguous_case(oracle_mod, k, r, P)
            calls = [make_call(torch, c, "in_place"), make_call(torch, c, "slots")]
            torch.cuda.synchronize()
            for b in calls:
                st.launch(ctx, b, stream)
            torch.cuda.synchronize()
            for b in calls:
                st.check(b, (b.api, k, r, P))
            st.check_inputs(c, calls[1].dd, calls[1].dp, calls[1].dm)


# ------------------------------------------------------------------------------------------
# 5. Table recovers
# ------------------------------------------------------------------------------------------
def _refused(quicfec, ctx, launch, b):
    with pytest.raises(quicfec.FecError) as ei:
        launch(ctx, b)
    assert ei.value.code == quicfec.FEC_ERR_RANGE and "sparse-plan" in ctx.last_error()


@pytest.mark.parametrize("k,r,sizes", TABLE_SHAPES)
def test_table_recovers(quicfec_mod, oracle_mod, torch_cuda, k, r, sizes):
    """The fixed gather, the variable-length gather, the scatter with a length table on padded
    destinations and the scatter without one on the slot layout, d_masks_out (and the symbol
    lengths) given."""
    torch = torch_cuda
    with device_plan(quicfec_mod, product_ctx(quicfec_mod)) as ctx:
        for P in sizes:
            cs = table_cases(oracle_mod, k, r, P)
            fx.run_recover(torch, ctx, cs.fixed, SEED + P, "fixed gather")
            var.run_recover(torch, ctx, cs.lens, SEED + P + 1, "var gather")
            sc.run_scatter(torch, ctx, cs.lens, SEED + P + 2, sc.padded_layout(SEED + P + 3), "scatter, lengths")
            sc.run_scatter(torch, ctx, cs.full, SEED + P + 4, sc.slot_layout, "scatter, NULL lengths", with_lens=False)


@pytest.mark.parametrize("k,r,P", [(16, 16, 1200), (12, 12, 45), (32, 32, 16)])
def test_table_recovers_without_optional_outputs(quicfec_mod, oracle_mod, torch_cuda, k, r, P):
    """d_masks_out NULL (the masks build_records reads are then the workspace's), the var gather's
    and the scatter's d_symbol_len_out NULL too (the scatter's own symbol lengths behind them),
    d_status NULL: the rebuilt bytes are the same, the outputs not given are not missed."""
    torch = torch_cuda
    cs = table_cases(oracle_mod, k, r, P)
    with device_plan(quicfec_mod, product_ctx(quicfec_mod)) as ctx:
        b = fx.make_recover(torch, cs.fixed, SEED + 1)
        ctx.recover_gather_dev(b.table, G_MAIN, k, r, P, b.out, b.st, None)
        v = var.make_recover(torch, cs.lens, SEED + 2)
        ctx.recover_gather_var_dev(v.table, v.lens, G_MAIN, k, r, P, v.out, None, None, None)
        s = sc.make_scatter(torch, cs.lens, SEED + 3, sc.padded_layout(SEED + 4), want_sym=False)
        ctx.recover_scatter_dev(s.table, s.lens, s.dtab, G_MAIN, k, r, P, s.st, None, None)
        ctx.synchronize()
    for x, c in ((b, cs.fixed), (v, cs.lens)):
        whole = x.whole.cpu().numpy()
        assert (whole[:fx.GUARD] == 0x5A).all() and (whole[-fx.GUARD:] == 0x5A).all()
        assert np.array_equal(whole[fx.GUARD:-fx.GUARD].reshape(G_MAIN, r, P), c.slots)
        assert (x.mo.cpu().numpy() == 0x3C3C3C3C3C3C3C3C).all()              # not given: not written
        for d, a in zip(x.dev, x.arenas):
            assert np.array_equal(d.cpu().numpy(), a)
    assert np.array_equal(b.st.cpu().numpy(), cs.fixed.status)
    assert (v.st.cpu().numpy() == 7).all() and (v.sym.cpu().numpy() == 0x77777777).all()
    for d, image in s.images:
        assert np.array_equal(d.cpu().numpy(), image)
    assert np.array_equal(s.st.cpu().numpy(), cs.lens.status) and (s.mo.cpu().numpy() == 0x3C3C3C3C3C3C3C3C).all()


def test_default_mode_still_refuses_the_table_recovers(quicfec_mod, oracle_mod, torch_cuda):
    """The same calls on a context left in FEC_PLAN_CODEBOOK: FEC_ERR_RANGE, nothing launched, nothing
    written -- beside the same call served in FEC_PLAN_DEVICE."""
    torch = torch_cuda
    k, r, P = 16, 16, 32
    cs = table_cases(oracle_mod, k, r, P)
    lib = quicfec_mod.load_test_library()
    with hooks_ctx(quicfec_mod) as ctx:
        b = fx.make_recover(torch, cs.fixed, SEED + 1)
        v = var.make_recover(torch, cs.lens, SEED + 2)
        s = sc.make_scatter(torch, cs.lens, SEED + 3, sc.padded_layout(SEED + 4))
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(lib)
        _refused(quicfec_mod, ctx, fx.launch_recover, b)
        _refused(quicfec_mod, ctx, var.launch_recover, v)
        _refused(quicfec_mod, ctx, sc.launch_scatter, s)
        ctx.synchronize()
        assert quicfec_mod.launch_trace(lib) == []
        assert (b.whole == 0x5A).all().item() and (b.st == 7).all().item() and (v.whole == 0x5A).all().item()
        assert (s.dest == 0x5A).all().item() and (s.st == 7).all().item()
        device_plan(quicfec_mod, ctx)
        fx.launch_recover(ctx, b)
        var.launch_recover(ctx, v)
        sc.launch_scatter(ctx, s)
        ctx.synchronize()
        forms = [t["form"] for t in quicfec_mod.launch_trace(lib)]
    per_call = lambda name: ["classify_" + name, "build_records", "recover_" + name, "recover_" + name]   # r = 16: two passes
    assert forms == per_call("gather") + per_call("gather_var") + per_call("scatter")
    fx.check_recover(b)
    var.check_recover(v)
    sc.check_scatter(s)


# ------------------------------------------------------------------------------------------
# 6. Chunking
# ------------------------------------------------------------------------------------------
def _slot(k, r):
    return 128 + min(k, r) * k * 32                                          # gf256.hpp record_bytes(k, min(k, r))


@pytest.mark.parametrize("k,r,P", [(16, 16, 1200), (20, 7, 48)])
def test_chunked_walk_equals_the_single_chunk(quicfec_mod, oracle_mod, torch_cuda, monkeypatch, k, r, P):
    """The test library with the arena lowered to five slots, G = 67: 14 build_records launches of
    5, ..., 5, 2 groups, each followed by its chunk's passes; the bytes of the slot recover and of
    the scatter recover equal the single-chunk run's (and the oracle's)."""
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    c = contiguous_case(oracle_mod, k, r, P)
    cs = table_cases(oracle_mod, k, r, P)
    passes = -(-r // 8)
    outs = []
    with device_plan(quicfec_mod, hooks_ctx(quicfec_mod)) as ctx:
        for arena in (None, 5 * _slot(k, r)):
            if arena:
                monkeypatch.setenv("QUICFEC_PLAN_ARENA_BYTES", str(arena))
            b = make_call(torch, c, "slots")
            s = sc.make_scatter(torch, cs.lens, SEED + 3, sc.padded_layout(SEED + 4))
            torch.cuda.synchronize()
            quicfec_mod.launch_trace(lib)
            ctx.recover_dev(b.dd, b.dp, b.dm, c.G, k, r, P, b.out, b.st)
            sc.launch_scatter(ctx, s)
            ctx.synchronize()
            trace = quicfec_mod.launch_trace(lib)
            st.check(b, ("slots", arena))
            sc.check_scatter(s, ("scatter", arena))
            outs.append((b.out.cpu().numpy(), s.dest.cpu().numpy()))
            chunks = [(g0, min(5, 67 - g0)) for g0 in range(0, 67, 5)] if arena else [(0, 67)]
            assert len(chunks) == (14 if arena else 1)
            for call, (first, kernel) in zip((trace[:len(trace) // 2], trace[len(trace) // 2:]),
                                             (("classify", "decode_wave"), ("classify_scatter", "recover_scatter"))):
                want = [(first, 0, 67)]
                for g0, gn in chunks:
                    # build_records carries the chunk's place in the call; the consumer is launched on the
                    # chunk as a call of its own (pointers advanced), so its first group reads 0
                    want += [("build_records", g0, gn)] + [(kernel, 0, gn)] * passes
                assert [(t["form"], t["first_item"], t["items"]) for t in call] == want, (arena, kernel)
                assert [t["aux"] for t in call if t["form"] == kernel] == [8 * p for p in range(passes)] * len(chunks)
                assert all(t["k"] == 0 and t["r"] == 8 for t in call if t["form"] == kernel)     # the runtime-k forms
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------
# 7. No host synchronise
# ------------------------------------------------------------------------------------------
def test_queued_pipeline_on_side_stream(quicfec_mod, oracle_mod, torch_cuda):
    """test_gpu_streams.py's pipeline for k=16 r=16 P = 32 G = 131 in FEC_PLAN_DEVICE: fill -> encode
    -> every shard the rule does not read overwritten with the case's junk -> masks copied in -> recover
    into slots -> decode in place, all
    queued on one non-blocking side stream behind 32 fills of 1 GiB, one synchronise at the end.
    When the calls are made the masks say "every shard lost" (a host read would find every group
    unrecoverable), and when they have returned the stream is still busy with the work queued ahead
    of them, which a synchronise inside a call would have waited for."""
    torch = torch_cuda
    k, r, P, G = 16, 16, 32, 131
    c = st._case(oracle_mod, k, r, P, G)
    ro = us.roles(c.masks, k, r)
    d_junk_d, d_junk_p = st._dev(torch, ro.lost_d), st._dev(torch, ro.unread_p)
    d_broken, d_par_in = st._dev(torch, c.broken).view(G, k, P), st._dev(torch, c.par_in).view(G, r, P)
    d_masks_src = st._dev(torch, c.masks_in.view(np.int64))        # junk in the bits at and above k + r = 32
    dd = torch.full((G * k * P,), 0x11, dtype=torch.uint8, device="cuda")
    par = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
    dm = torch.full((G,), -1, dtype=torch.int64, device="cuda")
    slots = st.make_call(torch, c, "slots", inputs=(dd, par, dm))
    slots.st.fill_(0xAA)
    status = torch.full((G,), 0xAA, dtype=torch.uint8, device="cuda")
    ahead = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with device_plan(quicfec_mod, product_ctx(quicfec_mod)) as ctx:
        assert ctx.decode_prepare(k, r) == 0                                 # the parity matrix is uploaded here
        warm = make_call(torch, c, "slots")                                  # the stream's workspace, allocated ahead
        torch.cuda.synchronize()
        st.launch(ctx, warm, stream)
        torch.cuda.synchronize()
        for i in range(32):                                                  # several milliseconds of work ahead of the chain
            ctx.fill_random_dev(ahead, 1 << 30, 1 + i, 0, stream=s)
        ctx.fill_random_dev(dd, G * k * P, c.seed, 0, stream=s)
        ctx.encode_dev(dd, G, k, r, P, par, stream=s)
        with torch.cuda.stream(stream):
            dd.view(G, k, P).copy_(torch.where(d_junk_d[:, :, None], d_broken, dd.view(G, k, P)))
            par.view(G, r, P).copy_(torch.where(d_junk_p[:, :, None], d_par_in, par.view(G, r, P)))
            dm.copy_(d_masks_src, non_blocking=True)
        st.launch(ctx, slots, stream)
        with torch.cuda.stream(stream):
            broken_seen = dd.clone()
        ctx.decode_dev(dd, par, dm, G, k, r, P, status, stream=s)
        still_busy = not stream.query()
        torch.cuda.synchronize()
    assert still_busy
    st.check(warm)
    assert np.array_equal(dm.cpu().numpy().view(np.uint64), c.masks_in)
    assert np.array_equal(broken_seen.cpu().numpy(), c.broken)
    st.check(slots)
    assert np.array_equal(status.cpu().numpy(), c.status)
    assert np.array_equal(dd.cpu().numpy(), c.ref)
    assert np.array_equal(par.cpu().numpy(), c.par_in)


def test_two_threads_on_two_streams(quicfec_mod, oracle_mod, torch_cuda):
    """Two host threads, each with its own side stream, buffers and a different batch, make eight
    k=16 r=16 calls each on one context from a barrier: each stream's records are its own
    workspace's, so no result depends on the other stream's."""
    torch = torch_cuda
    k, r, G = 16, 16, 67
    cases = [contiguous_case(oracle_mod, k, r, 32), contiguous_case(oracle_mod, k, r, 1200)]
    assert not np.array_equal(cases[0].data[:64], cases[1].data[:64])
    work = [[make_call(torch, cases[t], ("in_place", "slots")[j % 2]) for j in range(8)] for t in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    barrier = threading.Barrier(2)
    errors = []

    def run(t, ctx):
        try:
            barrier.wait(timeout=60)
            for b in work[t]:
                st.launch(ctx, b, streams[t])
        except BaseException as e:                                           # re-raised in the test
            errors.append((t, e))

    with device_plan(quicfec_mod, product_ctx(quicfec_mod)) as ctx:
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
            st.check(b, (t, j, b.api))


# ------------------------------------------------------------------------------------------
# 8. Mode handling
# ------------------------------------------------------------------------------------------
def test_mode_values(quicfec_mod, torch_cuda):
    lib = quicfec_mod.load_library()
    with product_ctx(quicfec_mod) as ctx:
        for bad in (2, -1, 7):
            assert lib.fec_decode_plan_mode(ctx.handle, bad) == quicfec_mod.FEC_ERR_RANGE
            assert "unknown mode" in ctx.last_error()
        assert lib.fec_decode_plan_mode(None, quicfec_mod.FEC_PLAN_DEVICE) == quicfec_mod.FEC_ERR_NULL
        assert lib.fec_decode_plan_mode(ctx.handle, quicfec_mod.FEC_PLAN_DEVICE) == quicfec_mod.FEC_OK
        assert lib.fec_decode_plan_mode(ctx.handle, quicfec_mod.FEC_PLAN_CODEBOOK) == quicfec_mod.FEC_OK


def test_switching_back_restores_the_codebook_mode(quicfec_mod, oracle_mod, torch_cuda):
    """DEVICE -> CODEBOOK on one context (an unknown mode in between changes nothing): the table
    recover is refused again and the contiguous call takes the host-built records -- no classify, no
    build_records, the form's passes alone -- with the same bytes as in device mode."""
    torch = torch_cuda
    k, r, P = 16, 16, 32
    lib = quicfec_mod.load_test_library()
    c = contiguous_case(oracle_mod, k, r, P)
    cs = table_cases(oracle_mod, k, r, P)
    with hooks_ctx(quicfec_mod) as ctx:
        device_plan(quicfec_mod, ctx)
        a = make_call(torch, c, "slots")
        torch.cuda.synchronize()
        quicfec_mod.launch_trace(lib)
        ctx.recover_dev(a.dd, a.dp, a.dm, c.G, k, r, P, a.out, a.st)
        ctx.synchronize()
        assert [t["form"] for t in quicfec_mod.launch_trace(lib)] == ["classify", "build_records", "decode_wave", "decode_wave"]
        ctx.decode_plan_mode(quicfec_mod.FEC_PLAN_CODEBOOK)
        assert lib.fec_decode_plan_mode(ctx.handle, 5) == quicfec_mod.FEC_ERR_RANGE      # the mode stays
        b = make_call(torch, c, "slots")
        g = fx.make_recover(torch, cs.fixed, SEED + 1)
        torch.cuda.synchronize()
        ctx.recover_dev(b.dd, b.dp, b.dm, c.G, k, r, P, b.out, b.st)
        ctx.synchronize()
        assert [t["form"] for t in quicfec_mod.launch_trace(lib)] == ["decode_wave", "decode_wave"]
        _refused(quicfec_mod, ctx, fx.launch_recover, g)
        assert quicfec_mod.launch_trace(lib) == []
    st.check(a)
    st.check(b)
    assert np.array_equal(a.out.cpu().numpy(), b.out.cpu().numpy())
    assert (g.whole.cpu().numpy() == 0x5A).all()


def test_dense_shape_launches_what_it_launches_today(quicfec_mod, oracle_mod, torch_cuda):
    """k=10 r=3 in FEC_PLAN_DEVICE keeps its codebook: the traces of the slot recover, the in-place
    decode at 48 B and the gather recover equal those of a context in the default mode, field by
    field, and no build_records is among them."""
    torch = torch_cuda
    lib = quicfec_mod.load_test_library()
    traces = []
    for mode in (quicfec_mod.FEC_PLAN_CODEBOOK, quicfec_mod.FEC_PLAN_DEVICE):
        with hooks_ctx(quicfec_mod) as ctx:
            ctx.decode_plan_mode(mode)
            assert ctx.decode_prepare(10, 3) > 0
            calls = [st.make_call(torch, st._case(oracle_mod, 10, 3, 1200, 1031), "slots"),
                     st.make_call(torch, st._case(oracle_mod, 10, 3, 64, 1031), "in_place")]
            g = fx.make_recover(torch, fx.main_case(oracle_mod, 10, 3, 1200), SEED + 9)
            torch.cuda.synchronize()
            quicfec_mod.launch_trace(lib)
            ctx.recover_dev(calls[0].dd, calls[0].dp, calls[0].dm, 1031, 10, 3, 1200, calls[0].out, calls[0].st)
            ctx.decode_dev(calls[1].dd, calls[1].dp, calls[1].dm, 1031, 10, 3, 64, calls[1].st)
            fx.launch_recover(ctx, g)
            ctx.synchronize()
            traces.append(quicfec_mod.launch_trace(lib))
        for b in calls:
            st.check(b, mode)
        fx.check_recover(g, mode)
    assert traces[0] == traces[1] and len(traces[0]) >= 4
    assert "build_records" not in {t["form"] for t in traces[0]}
