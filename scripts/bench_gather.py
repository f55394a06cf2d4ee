"""The address-table recover against the contiguous one, in one process (recorded, not gated).

C3's shape -- k=10 r=3, 1200 B packets, 1M groups, 2 erasures per group (uniform over the 13 shards)
-- recovered four ways, alternating over rounds on one stream, each round `reps` back-to-back calls
timed by HIP events on that stream:

  a  fec_recover_batch_rs_dev on contiguous data / parity buffers and masks
  b  fec_recover_gather_rs_dev with the identity table (addresses into a's buffers, 0 where lost)
  c  fec_recover_gather_rs_dev from a shuffled arena: the survivors of all groups, data and parity
     mixed, in random order on a 1216-B stride; lost shards are nowhere
  d  what a caller without the gather call does: the survivors copied out of that arena into the
     contiguous form (one torch.index_select per buffer, 8-B elements), then a
  d_ideal  a with fec_copy_dev of the survivors' bytes before it: the copy at the box's HBM copy
     rate, the least any caller's gather copy could cost (an in-order copy, so a lower bound)

b, c and d must rebuild the same bytes and status as a.  Prints one JSON line.

  python scripts/bench_gather.py [--groups 1000000] [--rounds 7] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "quic-test_amd"))
import quicfec  # noqa: E402

K, R, P, ERASURES, STRIDE = 10, 3, 1200, 2, 1216
N = K + R
SEED = 0x5EED6A7E
CHUNK = 1 << 16  # groups per step while the arena is filled


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    G = args.groups
    dev = "cuda"
    stream = torch.cuda.Stream()
    torch.manual_seed(SEED)
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        s = stream.cuda_stream
        data = torch.empty(G * K * P, dtype=torch.uint8, device=dev)
        par = torch.empty(G * R * P, dtype=torch.uint8, device=dev)
        ctx.fill_random_dev(data, data.numel(), SEED, stream=s)
        ctx.encode_dev(data, G, K, R, P, par, stream=s)
        # exactly ERASURES distinct shards lost per group, uniform over the k + r shards
        lost = torch.zeros((G, N), dtype=torch.bool, device=dev)
        lost.scatter_(1, torch.rand((G, N), device=dev).argsort(dim=1)[:, :ERASURES], True)
        masks = (lost.to(torch.int64) << torch.arange(N, device=dev)).sum(dim=1)
        # identity table: addresses into data / par
        sh = torch.arange(N, device=dev)
        g = torch.arange(G, device=dev)[:, None]
        ident = torch.where(sh < K, data.data_ptr() + (g * K + sh) * P, par.data_ptr() + (g * R + (sh - K)) * P)
        ident[lost] = 0
        ident = ident.contiguous()
        # the shuffled arena: survivor i of (g, s) order lives in row slot[g, s]
        n_surv = int((~lost).sum().item())
        arena = torch.empty(n_surv * STRIDE, dtype=torch.uint8, device=dev)
        rows = arena.view(n_surv, STRIDE)
        slot = torch.full((G, N), -1, dtype=torch.int64, device=dev)
        slot[~lost] = torch.randperm(n_surv, device=dev)
        for g0 in range(0, G, CHUNK):
            g1 = min(G, g0 + CHUNK)
            both = torch.cat([data.view(G, K, P)[g0:g1], par.view(G, R, P)[g0:g1]], dim=1)
            keep = ~lost[g0:g1]
            rows[slot[g0:g1][keep], :P] = both[keep]
            del both
        table = torch.where(slot >= 0, arena.data_ptr() + slot * STRIDE, torch.zeros_like(slot)).contiguous()
        # d: the caller's copy.  Rows as 8-B elements.
        rows8 = arena.view(torch.int64).view(n_surv, STRIDE // 8)[:, :P // 8]
        data_d = torch.zeros(G * K * P, dtype=torch.uint8, device=dev)
        par_d = torch.zeros(G * R * P, dtype=torch.uint8, device=dev)
        dst_d = data_d.view(torch.int64).view(G * K, P // 8)
        dst_p = par_d.view(torch.int64).view(G * R, P // 8)
        # one source row per destination slot; a lost shard's slot takes row 0 (the masks say: ignore it)
        from_d, from_p = slot[:, :K].reshape(-1).clamp(min=0), slot[:, K:].reshape(-1).clamp(min=0)
        copy_bytes = n_surv * P // 16 * 16

        out = {a: torch.full((G * R * P,), 0x5A, dtype=torch.uint8, device=dev) for a in "abcd"}
        st = {a: torch.full((G,), 7, dtype=torch.uint8, device=dev) for a in "abcd"}
        scratch = torch.empty(copy_bytes, dtype=torch.uint8, device=dev)

        def caller_copy():
            torch.index_select(rows8, 0, from_d, out=dst_d)
            torch.index_select(rows8, 0, from_p, out=dst_p)

        def arm(a):
            if a == "a":
                ctx.recover_dev(data, par, masks, G, K, R, P, out["a"], st["a"], stream=s)
            elif a == "b":
                ctx.recover_gather_dev(ident, G, K, R, P, out["b"], st["b"], stream=s)
            elif a == "c":
                ctx.recover_gather_dev(table, G, K, R, P, out["c"], st["c"], stream=s)
            elif a == "d":
                caller_copy()
                ctx.recover_dev(data_d, par_d, masks, G, K, R, P, out["d"], st["d"], stream=s)
            elif a == "d_copy":
                caller_copy()
            else:  # d_ideal
                ctx.copy_dev(arena, scratch, copy_bytes, stream=s)
                ctx.recover_dev(data, par, masks, G, K, R, P, out["a"], st["a"], stream=s)

        arms = ["a", "b", "c", "d", "d_copy", "d_ideal"]
        for a in arms:  # warm up every arm (code objects, the decode plan, torch's kernels)
            for _ in range(2):
                arm(a)
        stream.synchronize()
        same = {a: bool(torch.equal(out[a], out["a"]) and torch.equal(st[a], st["a"])) for a in "bcd"}
        rebuilt_rows = int((lost[:, :K].sum(dim=1)).sum().item())
        ms = {a: [] for a in arms}
        for rd in range(args.rounds):
            order = arms[rd % len(arms):] + arms[:rd % len(arms)]
            for a in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(args.reps):
                    arm(a)
                e1.record(stream)
                e1.synchronize()
                ms[a].append(e0.elapsed_time(e1) / args.reps)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        # bytes the recover itself needs: k survivors read and the rebuilt rows written, per group to rebuild
        need = int((lost[:, :K].any(dim=1)).sum().item()) * K * P + rebuilt_rows * P
        print(json.dumps({
            "bench": "gather_recover", "k": K, "r": R, "P": P, "groups": G, "erasures": ERASURES, "stride": STRIDE,
            "rounds": args.rounds, "reps": args.reps, "survivors": n_surv, "rebuilt_rows": rebuilt_rows,
            "identical_to_a": same, "ms": {a: [round(x, 4) for x in v] for a, v in ms.items()},
            "median_ms": {a: round(v, 4) for a, v in med.items()},
            "TBps": {a: round(need / med[a] / 1e9, 3) for a in "abc"},
            "b_vs_a": round(med["b"] / med["a"], 4), "c_vs_a": round(med["c"] / med["a"], 4),
            "c_vs_d": round(med["c"] / med["d"], 4), "c_vs_d_ideal": round(med["c"] / med["d_ideal"], 4),
            "copy_TBps": {"d_copy": round(2 * n_surv * P / med["d_copy"] / 1e9, 3)},
        }), flush=True)


if __name__ == "__main__":
    main()
