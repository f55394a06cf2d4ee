"""The wide address-table recover, measured once (recorded, not gated): one process, warm-up, device
events, ten repeats, the two calls of a measurement alternating.

For 100+20 and 224+32 at 1200 B, 2,000 groups, with e = 2 and e = min(k, r) lost data shards per group:
fec_recover_scatter_wide_rs_dev on tables that point into the contiguous layout (no length table, slot
destinations) against fec_recover_wide_rs_dev on the same groups -- the call a receiver had to copy
its shards together for, and the yardstick.  Outputs and statuses are compared byte for byte.  Each
arm's time is the median of its repeats, and the bytes per second it achieves are over the
algorithmic bytes of its call (csrc/fec_wide_table.hip, csrc/fec_wide.hip): survivor reads
k * P * ceil(e / 8), e * k * 32 of record per walk pass, writes e * P; the table call also reads its
table rows ((k + r) * 8 per group in the classify, k * 8 + 8 * min(8, rows left) per row pass) and
writes and reads back 32 B of mask.

Prints one JSON line per measurement and writes all to --out.

  python scripts/measure_wide_table.py [--out profiles/wide_table/measure.json] [--repeats 10]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "quic-test_amd"))
sys.path.insert(0, str(REPO / "scripts"))
import quicfec  # noqa: E402
from measure_wide import lost_data_masks, setup, spread, timed  # noqa: E402

SEED = 0x5EED7AB1


def algorithmic_bytes(G, k, r, P, e, table):
    row_passes = -(-e // 8)
    walk_passes = P // 1024 + -(-(P % 1024) // 256)
    b = {"read": G * k * P * row_passes, "record": G * e * k * 32 * walk_passes, "written": G * e * P}
    if table:
        b["tables"] = G * ((k + r) * 8 + row_passes * k * 8 + e * 8 + 2 * 32)
    else:
        b["masks"] = G * 2 * 32                                             # the classify's and the builder's read
    return b


def one(k, r, P, G, e, repeats):
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.manual_seed(SEED + k * 100 + e)
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        data, par, masks = setup(ctx, G, k, r, P, e, s)
        lost = ((masks[:, :, None] >> torch.arange(64, device="cuda")) & 1).bool().view(G, 256)[:, :k + r]
        at = torch.cat([data.data_ptr() + torch.arange(G * k, device="cuda").view(G, k) * P,
                        par.data_ptr() + torch.arange(G * r, device="cuda").view(G, r) * P], dim=1)
        addrs = torch.where(lost, torch.zeros_like(at), at).contiguous()
        out = {a: torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda") for a in ("table", "wide")}
        st = {a: torch.full((G,), 7, dtype=torch.uint8, device="cuda") for a in ("table", "wide")}
        # slot destinations: the m-th lost data shard of group g at (g * r + m) * P
        m = torch.cumsum(lost[:, :k].to(torch.int64), dim=1) - 1
        slot = out["table"].data_ptr() + (torch.arange(G, device="cuda").view(G, 1) * r + m) * P
        dests = torch.where(lost[:, :k], slot, torch.zeros_like(slot)).contiguous()
        arms = {"table": lambda: ctx.recover_scatter_wide_dev(addrs, None, dests, G, k, r, P, st["table"], stream=s),
                "wide": lambda: ctx.recover_wide_dev(data, par, masks, G, k, r, P, out["wide"], st["wide"], stream=s)}
        for arm in arms.values():                                           # code objects, the matrix, workspaces
            for _ in range(3):
                arm()
        stream.synchronize()
        same = bool(torch.equal(out["table"], out["wide"]) and torch.equal(st["table"], st["wide"]))
        want = data.view(G, k, P)[lost[:, :k]].view(G, e, P)
        right = bool(torch.equal(out["table"].view(G, r, P)[:, :e], want) and int(st["table"].sum().item()) == 0)
        ms = timed(arms, repeats, stream)
    med = {a: statistics.median(v) for a, v in ms.items()}
    bytes_ = {"table": algorithmic_bytes(G, k, r, P, e, True), "wide": algorithmic_bytes(G, k, r, P, e, False)}
    return {"measure": "wide_table_vs_wide", "k": k, "r": r, "P": P, "groups": G, "lost_per_group": e, "repeats": repeats,
            "table_identical_to_wide": same, "rebuilt_rows_equal_the_data": right,
            "event_ms": {a: spread(v) for a, v in ms.items()}, "algorithmic_bytes": bytes_,
            "achieved_TB_per_s": {a: round(sum(bytes_[a].values()) / (med[a] * 1e-3) / 1e12, 4) for a in ms},
            "table_over_wide_time": round(med["table"] / med["wide"], 4),
            "wide_min_max_spread_ms": round(max(ms["wide"]) - min(ms["wide"]), 4)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "wide_table" / "measure.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--groups", type=int, default=2000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    results = []
    for k, r in ((100, 20), (224, 32)):
        for e in (2, min(k, r)):
            results.append(one(k, r, 1200, args.groups, e, args.repeats))
            print(json.dumps(results[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
