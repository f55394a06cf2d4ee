"""The packed recovers for every shape, measured once (recorded, not gated): one process, warm-up,
device events, the two calls of a measurement alternating repeat by repeat on the same inputs.

  1. k=20 r=5, 1200 B, 200,000 groups, 2 lost data shards per group: fec_recover_packed_rs_dev
     (rows prefix, classify, recover_packed over the dense codebook) against fec_recover_batch_rs_dev,
     the slot recover of the same mask width.
  2. 100+20, 1200 B, 20,000 groups, 4 lost data shards per group: fec_recover_packed_wide_rs_dev
     against fec_recover_wide_rs_dev; both build their records on the device, chunk after chunk.

The packed consumer reads the same bytes and writes the same number of rows as the slot form; it adds
the row prefix's launches and a u32 of row start per group.  Each arm's own run-to-run spread (min and
max over the repeats) is reported next to the medians, and the packed rows are compared byte for byte
with the slot rows compacted.

Prints one JSON line per measurement and writes both to --out.

  python scripts/measure_packed_any.py [--out profiles/packed_any/measure.json] [--repeats 20]
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
import quicfec  # noqa: E402

SEED = 0x5EED9AC4


def lost_data_masks(G: int, k: int, e: int, dev: str) -> torch.Tensor:
    """(G, 4) int64: exactly e lost data shards per group, no lost parity row."""
    lost = torch.zeros((G, 256), dtype=torch.bool, device=dev)
    lost[:, :k] = torch.rand((G, k), device=dev).argsort(dim=1).argsort(dim=1) < e
    words = lost.view(G, 4, 64).to(torch.int64) << torch.arange(64, device=dev)
    return words.sum(dim=2).contiguous()


def spread(ms: list) -> dict:
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def timed(arms: dict, repeats: int, stream) -> dict:
    """Device-event milliseconds of each arm, the arms alternating repeat by repeat."""
    ms = {a: [] for a in arms}
    for _ in range(repeats):
        for a, arm in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            t0.record(stream)
            arm()
            t1.record(stream)
            t1.synchronize()
            ms[a].append(t0.elapsed_time(t1))
    return ms


def packed_vs_slots(wide: bool, k: int, r: int, P: int, G: int, e: int, repeats: int) -> dict:
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.manual_seed(SEED + k)
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        data = torch.empty(G * k * P, dtype=torch.uint8, device="cuda")
        par = torch.empty(G * r * P, dtype=torch.uint8, device="cuda")
        ctx.fill_random_dev(data, data.numel(), SEED, stream=s)
        ctx.encode_dev(data, G, k, r, P, par, stream=s)
        masks = lost_data_masks(G, k, e, "cuda")
        if not wide:
            masks = masks[:, 0].contiguous()
        slots = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
        packed = torch.full((G * e * P,), 0x5A, dtype=torch.uint8, device="cuda")
        rs = torch.full((G,), -1, dtype=torch.int32, device="cuda")
        tot = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        st = {a: torch.full((G,), 7, dtype=torch.uint8, device="cuda") for a in ("slots", "packed")}
        if wide:
            arms = {"slots": lambda: ctx.recover_wide_dev(data, par, masks, G, k, r, P, slots, st["slots"], stream=s),
                    "packed": lambda: ctx.recover_packed_wide_dev(data, par, masks, G, k, r, P, packed, rs, tot, st["packed"], stream=s)}
        else:
            arms = {"slots": lambda: ctx.recover_dev(data, par, masks, G, k, r, P, slots, st["slots"], stream=s),
                    "packed": lambda: ctx.recover_packed_any_dev(data, par, masks, G, k, r, P, packed, rs, tot, st["packed"], stream=s)}
        for arm in arms.values():                                           # code objects, codebook or matrix, workspaces
            for _ in range(3):
                arm()
        stream.synchronize()
        same = bool(torch.equal(packed.view(G, e, P), slots.view(G, r, P)[:, :e]) and torch.equal(st["slots"], st["packed"])
                    and int(tot.item()) == G * e
                    and torch.equal(rs, torch.arange(G, device="cuda", dtype=torch.int32) * e))
        ms = timed(arms, repeats, stream)
    med = {a: statistics.median(v) for a, v in ms.items()}
    slot_spread = max(ms["slots"]) - min(ms["slots"])
    return {"measure": "packed_wide_vs_slots" if wide else "packed_vs_slots", "k": k, "r": r, "P": P, "groups": G,
            "lost_per_group": e, "repeats": repeats, "packed_rows_equal_the_slot_rows": same,
            "event_ms": {a: spread(v) for a, v in ms.items()},
            "packed_over_slots": round(med["packed"] / med["slots"], 4),
            "packed_minus_slots_ms": round(med["packed"] - med["slots"], 4),
            "slots_min_max_spread_ms": round(slot_spread, 4),
            "packed_min_max_spread_ms": round(max(ms["packed"]) - min(ms["packed"]), 4),
            "packed_slower_by_more_than_the_slots_spread": bool(med["packed"] - med["slots"] > slot_spread)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "packed_any" / "measure.json"))
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    results = [packed_vs_slots(False, 20, 5, 1200, 200_000, 2, args.repeats),
               packed_vs_slots(True, 100, 20, 1200, 20_000, 4, args.repeats)]
    for row in results:
        print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
