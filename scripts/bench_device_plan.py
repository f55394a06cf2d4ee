"""Device-built recovery records (FEC_PLAN_DEVICE) against the host-built sparse plan
(FEC_PLAN_CODEBOOK), in one process (recorded, not gated).

fec_recover_batch_rs_dev at shapes past the codebook cap -- k=20 r=8, k=16 r=16, k=32 r=8 --
1200 B packets, 65,536 groups, under two loss patterns:

  iid      every shard lost with probability 1 %: few distinct patterns, the regime where the
           host plan builds one record per pattern and the device plan one per group
  uniform  every group loses e data shards, e uniform in 1..r: nearly every group its own pattern

Two contexts, one per mode, called in turn on one side stream.  A call is timed by the host's
wall clock around the call and a stream synchronise (the codebook mode synchronises inside the
call, so events on the stream would not see its host work); after a warm-up, `calls` calls each,
alternating.  The outputs and statuses of the two modes are compared byte for byte.  The three
address-table recovers, which the codebook mode refuses for these shapes, are timed the same way in
device mode on the identity table (addresses into the contiguous buffers) and reported unratioed.
Prints one JSON line per (shape, pattern).

The split between build_records and the kernels that read the records is not visible from here;
it is taken from a kernel trace of this script (rocprofv3 --kernel-trace --stats).

  python scripts/bench_device_plan.py [--groups 65536] [--calls 20] [--shapes 20x8,16x16,32x8]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "quic-test_amd"))
import quicfec  # noqa: E402

P = 1200
SEED = 0x5EEDD71A


def loss(pattern: str, G: int, k: int, r: int, dev: str) -> torch.Tensor:
    """(G, k + r) bool: the lost shards."""
    if pattern == "iid":
        return torch.rand((G, k + r), device=dev) < 0.01
    e = torch.randint(1, min(k, r) + 1, (G, 1), device=dev)
    lost = torch.zeros((G, k + r), dtype=torch.bool, device=dev)
    lost[:, :k] = torch.rand((G, k), device=dev).argsort(dim=1).argsort(dim=1) < e
    return lost


def spread(ms: list) -> dict:
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def run(k: int, r: int, pattern: str, G: int, calls: int) -> dict:
    dev, n = "cuda", k + r
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.manual_seed(SEED + k * 100 + r)
    with quicfec.Context(device=0) as host_ctx, quicfec.Context(device=0) as dev_ctx, torch.cuda.stream(stream):
        dev_ctx.decode_plan_mode(quicfec.FEC_PLAN_DEVICE)
        assert host_ctx.decode_prepare(k, r) == 0 and dev_ctx.decode_prepare(k, r) == 0     # past the cap
        data = torch.empty(G * k * P, dtype=torch.uint8, device=dev)
        par = torch.empty(G * r * P, dtype=torch.uint8, device=dev)
        dev_ctx.fill_random_dev(data, data.numel(), SEED, stream=s)
        dev_ctx.encode_dev(data, G, k, r, P, par, stream=s)
        lost = loss(pattern, G, k, r, dev)
        masks = (lost.to(torch.int64) << torch.arange(n, device=dev)).sum(dim=1)
        patterns = int(torch.unique(masks).numel())
        lost_d = lost[:, :k]
        out = {m: torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device=dev) for m in ("codebook", "device")}
        st = {m: torch.full((G,), 7, dtype=torch.uint8, device=dev) for m in ("codebook", "device")}
        # the identity table, the full length table and the slot layout as a destination table
        sh = torch.arange(n, device=dev)
        g = torch.arange(G, device=dev)[:, None]
        ident = torch.where(sh < k, data.data_ptr() + (g * k + sh) * P, par.data_ptr() + (g * r + (sh - k)) * P)
        ident[lost] = 0
        ident = ident.contiguous()
        lens = torch.full((G * n,), P, dtype=torch.int32, device=dev)
        tout = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device=dev)
        m = (torch.cumsum(lost_d.to(torch.int64), dim=1) - 1).clamp(min=0, max=r - 1)
        dests = (tout.data_ptr() + (g * r + m) * P).contiguous()
        tst = torch.full((G,), 7, dtype=torch.uint8, device=dev)

        def contiguous(mode):
            ctx = host_ctx if mode == "codebook" else dev_ctx
            ctx.recover_dev(data, par, masks, G, k, r, P, out[mode], st[mode], stream=s)

        arms = {
            "codebook": lambda: contiguous("codebook"),
            "device": lambda: contiguous("device"),
            "gather": lambda: dev_ctx.recover_gather_dev(ident, G, k, r, P, tout, tst, None, stream=s),
            "gather_var": lambda: dev_ctx.recover_gather_var_dev(ident, lens, G, k, r, P, tout, tst, None, None, stream=s),
            "scatter": lambda: dev_ctx.recover_scatter_dev(ident, None, dests, G, k, r, P, tst, None, None, stream=s),
        }
        for arm in arms.values():                                       # plans, workspaces, code objects
            for _ in range(2):
                arm()
        stream.synchronize()
        same = bool(torch.equal(out["codebook"], out["device"]) and torch.equal(st["codebook"], st["device"]))
        table_same = {}
        for name in ("gather", "gather_var", "scatter"):
            tout.fill_(0x5A)
            tst.fill_(7)
            stream.synchronize()
            arms[name]()
            stream.synchronize()
            table_same[name] = bool(torch.equal(tout, out["codebook"]) and torch.equal(tst, st["codebook"]))
        ms = {a: [] for a in arms}
        for _ in range(calls):
            for a, arm in arms.items():                                 # the modes alternate call by call
                stream.synchronize()
                t0 = time.perf_counter()
                arm()
                stream.synchronize()
                ms[a].append((time.perf_counter() - t0) * 1e3)
        need = int(lost_d.any(dim=1).sum().item())
        rows = int(((lost_d.sum(dim=1) <= (r - lost[:, k:].sum(dim=1))) * lost_d.sum(dim=1)).sum().item())
        med = {a: statistics.median(v) for a, v in ms.items()}
        return {
            "bench": "device_plan", "k": k, "r": r, "P": P, "groups": G, "pattern": pattern, "calls": calls,
            "distinct_masks": patterns, "groups_to_rebuild": need, "rebuilt_rows": rows,
            "device_identical_to_codebook": same, "table_identical_to_codebook": table_same,
            "wall_ms": {a: spread(v) for a, v in ms.items()},
            "device_vs_codebook": round(med["device"] / med["codebook"], 4),
        }


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="20x8,16x16,32x8")
    ap.add_argument("--patterns", default="iid,uniform")
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        k, r = (int(x) for x in shape.split("x"))
        for pattern in args.patterns.split(","):
            print(json.dumps(run(k, r, pattern, args.groups, args.calls)), flush=True)


if __name__ == "__main__":
    main()
