"""bench.py --dump-outputs: the sample of groups is fixed and within the size budget, and the
arrays written are what the timed path's calls left in the caller's buffers (parity against the
oracle's encode, rebuilt packets against the original lost shards), for every decode API."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
SEED = 0x5EED0D00


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_dump_mod", REPO / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_sorted_and_within_budget(bench):
    G, arrays, row = 1_000_000, 2, 3 * 1200
    s = bench.dump_sample(G, arrays, row)
    assert np.array_equal(s, bench.dump_sample(G, arrays, row))          # same groups every run
    assert len(s) * arrays * row * 4 <= bench.DUMP_BUDGET_BYTES < 64_000_000
    assert len(s) >= 1000 and np.all(np.diff(s) > 0) and 0 <= s[0] and s[-1] < G
    assert s[-1] > G // 2                                                # spread over the batch, not a prefix
    assert np.array_equal(bench.dump_sample(100, arrays, row), np.arange(100))   # a small batch whole


def test_bench_args_full_and_dump(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.steps == 7
    a = bench.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"
    assert not bench.legs_enabled(bench.parse_args(["--legs", "on"]), 8)     # legs only with --full
    assert bench.legs_enabled(bench.parse_args(["--full"]), 8)
    assert not bench.legs_enabled(bench.parse_args(["--full"]), 1)
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


@pytest.mark.gpu
@pytest.mark.parametrize("api,loss", [("recover", None), ("packed", None), ("in-place", None),
                                      ("recover", 0.15), ("packed", 0.15)])
def test_dump_outputs_match_oracle(bench, gpu_ctx, oracle_mod, torch_cuda, tmp_path, monkeypatch, api, loss):
    """An encode + decode as bench.py's step makes them, on 301 groups, dumped with a budget that
    keeps a sample: parity rows are the oracle's, rebuilt slots the original lost shards (0 where
    the call writes nothing: beyond the group's lost data shards, or a group past recovery), the
    in-place data the original."""
    torch = torch_cuda
    k, r, P, G = 10, 3, 1200, 301
    cfg = dict(k=k, r=r, P=P, erasures=2, decode=True)
    if loss:
        cfg["loss"] = loss
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 2 * r * P * 97)     # 97 of the 301 groups
    host = oracle_mod.splitmix_bytes(G * k * P, SEED)
    exp_par = oracle_mod.rs_encode(host, G, k, r, P).reshape(G, r, P)
    masks_h = bench.make_masks(cfg, G, SEED + 1)
    data = torch.from_numpy(host).cuda()
    parity = torch.empty(G * r * P, dtype=torch.uint8, device="cuda")
    masks = torch.from_numpy(masks_h.view(np.int64)).cuda()
    rebuilt = torch.full((G * r * P,), 0xAB, dtype=torch.uint8, device="cuda") if api != "in-place" else None
    row_start = torch.empty(G, dtype=torch.int32, device="cuda") if api == "packed" else None
    gpu_ctx.decode_prepare(k, r)
    gpu_ctx.encode_dev(data, G, k, r, P, parity)
    if api == "packed":
        gpu_ctx.recover_packed_dev(data, parity, masks, G, k, r, P, rebuilt, row_start, None, None)
    elif api == "recover":
        gpu_ctx.recover_dev(data, parity, masks, G, k, r, P, rebuilt, None)
    else:
        gpu_ctx.decode_dev(data, parity, masks, G, k, r, P, None)
    gpu_ctx.synchronize()
    shapes = bench.dump_outputs(tmp_path / "d", cfg, G, api, data, parity, rebuilt, row_start, masks_h)

    sample = bench.dump_sample(G, 2, (k if api == "in-place" else r) * P)
    n = len(sample)
    assert 1 < n < G
    got_par = np.load(tmp_path / "d" / "parity.npy")
    assert got_par.dtype == np.float32 and shapes["parity"] == [n, r, P]
    assert np.array_equal(got_par, exp_par[sample].astype(np.float32))
    if api == "in-place":
        got = np.load(tmp_path / "d" / "data.npy")
        assert got.dtype == np.float32 and np.array_equal(got, host.reshape(G, k, P)[sample].astype(np.float32))
        return
    got = np.load(tmp_path / "d" / "rebuilt.npy")
    assert got.dtype == np.float32 and got.shape == (n, r, P)
    want = np.zeros((n, r, P), dtype=np.float32)
    seen = set()
    for i, g in enumerate(sample):
        m = int(masks_h[g])
        lost = [j for j in range(k) if (m >> j) & 1]
        alive = r - bin(m >> k).count("1")
        seen.add(len(lost) if len(lost) <= alive else -1)
        if len(lost) <= alive:
            for s, j in enumerate(lost):
                want[i, s] = host.reshape(G, k, P)[g, j]
    assert {0, 1, 2} <= seen and (not loss or -1 in seen), seen    # the sample holds every kind of group
    assert np.array_equal(got, want)
