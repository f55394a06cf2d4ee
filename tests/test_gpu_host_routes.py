"""The routes of the host-memory calls (csrc/fec_routes.hpp) that the larger GPU tests do not reach,
at the smallest shape that still exercises them: k=4 r=2, 17-byte packets, 7 groups, pipeline chunks
of two groups (four chunks over three slots).  Bit-exact against the oracle, statuses and the
unrecoverable count included.

Which test reaches which route:
  encode   zero_copy   test_gpu_parity.py::test_small_calls_zero_copy_and_dma[*-None]
           pipelined   test_gpu_parity.py::test_host_pipeline_multi_chunk; test_tiny_pipeline here
           staged      device buffers: test_gpu_parity.py::test_rs_encode_matches_oracle; host offsets:
                       test_rs_encode_gather_offsets; a device table of offsets over host data and the
                       reverse: test_encode_offsets_and_data_on_different_sides here
  decode   nothing     test_decode_nothing_to_rebuild here
           zero_copy   test_gpu_parity.py::test_small_calls_zero_copy_and_dma[*-None]
           compacted   test_gpu_parity.py::test_host_decode_compacted_sparse_loss; test_tiny_pipeline here
           pipelined   test_gpu_parity.py::test_host_pipeline_multi_chunk; test_tiny_pipeline here
           staged      all on the device: test_gpu_parity.py::test_rs_decode_matches_oracle; one buffer
                       on the device: test_decode_one_buffer_on_the_device here
  legacy   (calls the coalescer leaves alone)
           zero_copy, window staged   test_gpu_coalesce.py::test_coalesce_switch_same_bytes[0]
           zero_copy in place, staged with a rebased window   test_legacy_alone_on_its_context here
           staged, device slab        test_gpu_parity.py::test_legacy_batch_golden_host_pinned_device
"""
import numpy as np
import pytest

import unread_shards as us

pytestmark = pytest.mark.gpu

K, R, P, G = 4, 2, 17, 7
CHUNK_BYTES = 2 * K * P                    # two groups per pipeline chunk
# per group: nothing lost; one data shard; two; parity only; three data shards (unrecoverable);
# one data shard and a parity row; two data shards and a parity row (unrecoverable)
SPARSE = np.array([0, 0b000001, 0b001010, 0b010000, 0b000111, 0b010100, 0b100011], dtype=np.uint64)   # 3 of 7 to rebuild
DENSE = np.array([0b001000, 0b000001, 0b001010, 0b010000, 0b000111, 0b010100, 0b100011], dtype=np.uint64)  # 4 of 7
NOTHING = np.array([0, 0, 0b110000, 0b010000, 0b000111, 0, 0b100011], dtype=np.uint64)


@pytest.fixture(scope="module")
def case(oracle_mod):
    """The data, its parity and, per mask set, the decode's inputs (junk in every lost data shard,
    every parity row and every mask bit the erasure rule does not read, tests/unread_shards.py) and
    what the oracle makes of them."""
    data = oracle_mod.splitmix_bytes(G * K * P, 0x5EED0909)
    par = oracle_mod.rs_encode(data, G, K, R, P)
    out = {"data": data, "par": par}
    for name, masks in (("sparse", SPARSE), ("dense", DENSE), ("nothing", NOTHING)):
        # "nothing" rebuilds no group on purpose, so none has a chosen row to have a lost row below
        broken, par_in = us.inputs(data, par, masks, K, R, P, 0x5EED0909, need_lost_below=name != "nothing")
        # seven groups written out by hand: of the six planted groups those that exist get their pattern
        # (the two one row short and an untouched one in every set, two that use every row in two)
        masks_in = us.high_bits(masks, K, R, 0x5EED0909, need_full=False, need_short=False, need_untouched=False)
        assert len(us.planted(masks, K, R, 0x5EED0909, False, False, False)) >= 3
        ref, clean = broken.copy(), broken.copy()
        bad, st = oracle_mod.rs_decode(ref, par_in, masks_in, G, K, R, P)
        bad_clean, st_clean = oracle_mod.rs_decode(clean, par_in, masks, G, K, R, P)
        assert bad == bad_clean and np.array_equal(st, st_clean) and np.array_equal(ref, clean)
        ok = st == 0
        assert np.array_equal(ref.reshape(G, -1)[ok], data.reshape(G, -1)[ok])
        for a in (broken, par_in, ref, masks_in):
            a.setflags(write=False)
        out[name] = (masks, broken, ref, bad, st, par_in, masks_in)
    assert out["sparse"][3] == out["dense"][3] == out["nothing"][3] == 2
    return out


def _pinned(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).pin_memory()


@pytest.mark.parametrize("on_device", ["data", "parity", "masks"])
def test_decode_one_buffer_on_the_device(gpu_ctx, torch_cuda, case, on_device):
    """One input on the device, the others and the statuses in pageable host memory: the staged route."""
    torch = torch_cuda
    masks, broken, ref, bad_exp, st_exp, par_in, masks_in = case["sparse"]
    bufs = {"data": broken.copy(), "parity": par_in.copy(), "masks": masks_in.copy(),
            "status": np.full(G, 0xAA, dtype=np.uint8)}
    host = bufs[on_device]
    bufs[on_device] = torch.from_numpy(host.view(np.int64) if on_device == "masks" else host).cuda()
    bad = gpu_ctx.decode(bufs["data"], bufs["parity"], bufs["masks"], K, R, P, status_out=bufs["status"], num_groups=G)
    got = {n: (b.cpu().numpy() if n == on_device else b) for n, b in bufs.items()}
    assert bad == bad_exp
    assert np.array_equal(got["status"], st_exp)
    assert np.array_equal(got["data"], ref), us.mismatch(masks, K, R, got["data"], ref)
    assert np.array_equal(got["parity"], par_in)
    assert np.array_equal(got["masks"].view(np.uint64), masks_in)


@pytest.mark.parametrize("device", ["offsets", "data"])
def test_encode_offsets_and_data_on_different_sides(gpu_ctx, torch_cuda, case, device):
    """Packets at u64 offsets into a slab, the table of offsets on one side and the slab on the other:
    host data is staged as its window with the offsets brought back and rebased; device data takes the
    host's table up."""
    torch = torch_cuda
    rng = np.random.default_rng(9)
    stride, first = P + 5, 11
    offs = (np.uint64(first) + rng.permutation(G * K).astype(np.uint64) * np.uint64(stride)).astype(np.uint64)
    slab = np.full(first + G * K * stride + 3, 0x77, dtype=np.uint8)
    for i, o in enumerate(offs):
        slab[int(o):int(o) + P] = case["data"][i * P:(i + 1) * P]
    d_offs, d_slab = torch.from_numpy(offs.view(np.int64)).cuda(), torch.from_numpy(slab).cuda()
    par = np.zeros(G * R * P, dtype=np.uint8)
    if device == "offsets":
        gpu_ctx.encode(slab, K, R, P, par, num_groups=G, offsets=d_offs)
    else:
        gpu_ctx.encode(d_slab, K, R, P, par, num_groups=G, offsets=offs)
    assert np.array_equal(par, case["par"])


@pytest.mark.parametrize("pinned", [False, True])
def test_decode_nothing_to_rebuild(gpu_ctx, torch_cuda, case, pinned):
    """No group has lost data it can rebuild (parity-only losses, unrecoverable groups): the host's
    scan of the masks is the whole answer, the data stays as it is."""
    masks, broken, ref, bad_exp, st_exp, par_in, masks_in = case["nothing"]
    assert np.array_equal(ref, broken)
    data = _pinned(torch_cuda, broken) if pinned else broken.copy()
    par = _pinned(torch_cuda, par_in) if pinned else par_in.copy()
    st = np.full(G, 0xAA, dtype=np.uint8)
    hm = masks_in.copy()
    assert gpu_ctx.decode(data, par, hm, K, R, P, status_out=st, num_groups=G) == bad_exp
    assert np.array_equal(st, st_exp)
    assert np.array_equal(data.numpy() if pinned else data, ref)
    assert gpu_ctx.decode(data, par, hm, K, R, P, num_groups=G) == bad_exp     # without statuses
    assert np.array_equal(hm, masks_in)


@pytest.mark.parametrize("pinned", [False, True])
def test_tiny_pipeline(gpu_ctx, torch_cuda, case, monkeypatch, pinned):
    """Zero-copy switched off and chunks of two groups: the encode and the dense decode stream all 7
    groups through the three slots in four chunks; the sparse decode moves only its 3 groups."""
    monkeypatch.setenv("QUICFEC_SMALL_CALL_BYTES", "0")
    monkeypatch.setenv("QUICFEC_PIPE_CHUNK_BYTES", str(CHUNK_BYTES))

    def host(a):
        return _pinned(torch_cuda, a) if pinned else np.ascontiguousarray(a).copy()

    def npy(a):
        return a.numpy() if pinned else a

    par = host(np.zeros(G * R * P, dtype=np.uint8))
    gpu_ctx.encode(host(case["data"]), K, R, P, par, num_groups=G)
    assert np.array_equal(npy(par), case["par"])
    for name in ("dense", "sparse"):
        masks, broken, ref, bad_exp, st_exp, par_in, masks_in = case[name]
        data, hp, st, hm = host(broken), host(par_in), np.full(G, 0xAA, dtype=np.uint8), masks_in.copy()
        assert gpu_ctx.decode(data, hp, hm, K, R, P, status_out=st, num_groups=G) == bad_exp, name
        assert np.array_equal(hm, masks_in), name
        assert np.array_equal(st, st_exp), name
        assert np.array_equal(npy(data), ref), (name, us.mismatch(masks, K, R, npy(data), ref))
        assert np.array_equal(npy(hp), par_in), name


@pytest.mark.parametrize("small", ["0", None])
@pytest.mark.parametrize("pinned", [False, True])
def test_legacy_alone_on_its_context(gpu_ctx, oracle_mod, torch_cuda, case, monkeypatch, pinned, small):
    """fec_encode_batch with the coalescer off, packets scattered in a slab whose window starts past
    its first byte: zero-copy (a page-locked slab in place, a pageable one through its staged window)
    and, with zero-copy off, the window copied to the device with the offsets rebased."""
    monkeypatch.setenv("QUICFEC_COALESCE", "0")
    if small is None:
        monkeypatch.delenv("QUICFEC_SMALL_CALL_BYTES", raising=False)
    else:
        monkeypatch.setenv("QUICFEC_SMALL_CALL_BYTES", small)
    rng = np.random.default_rng(10)
    stride, first = P + 3, 29
    offs = (first + rng.permutation(G * 10) * stride).astype(np.uint32)
    slab = oracle_mod.splitmix_bytes(first + G * 10 * stride + 1, 0x5EED090A)
    rc, exp = oracle_mod.encode_batch_legacy(slab, offs, G, P)
    assert rc == 0
    h_slab = _pinned(torch_cuda, slab) if pinned else slab.copy()
    rep = _pinned(torch_cuda, np.zeros(G * P, dtype=np.uint8)) if pinned else np.zeros(G * P, dtype=np.uint8)
    assert gpu_ctx.encode_batch_legacy(h_slab, offs, G, P, rep) == 0
    assert np.array_equal(rep.numpy() if pinned else rep, exp)
