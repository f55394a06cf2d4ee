"""The wide calls, measured once (recorded, not gated): one process, warm-up, device events, ten
repeats, the two calls of a measurement alternating.

  1. 32+32, 1200 B, 20,000 groups, 4 lost data shards per group: fec_recover_wide_rs_dev against
     fec_recover_batch_rs_dev in FEC_PLAN_DEVICE, the only other code that serves the shape (and the
     same before the wide calls existed).  Outputs and statuses are compared byte for byte.
  2. 223+32, 1200 B, 2,000 groups, 16 lost per group: fec_recover_wide_rs_dev alone, its time and the
     bytes per second it achieves over the algorithmic bytes of a call (csrc/fec_wide.hip): reads
     k * P * ceil(e / 8) of survivors and e * k * 32 of record per walk pass, writes e * P, per group.

Prints one JSON line per measurement and writes both to --out.

  python scripts/measure_wide.py [--out profiles/wide/measure.json] [--repeats 10]
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

SEED = 0x5EED71DE


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


def setup(ctx, G, k, r, P, e, s, dev="cuda"):
    data = torch.empty(G * k * P, dtype=torch.uint8, device=dev)
    par = torch.empty(G * r * P, dtype=torch.uint8, device=dev)
    ctx.fill_random_dev(data, data.numel(), SEED, stream=s)
    ctx.encode_dev(data, G, k, r, P, par, stream=s)
    return data, par, lost_data_masks(G, k, e, dev)


def algorithmic_bytes(G, k, P, e):
    row_passes = -(-e // 8)
    walk_passes = P // 1024 + -(-(P % 1024) // 256)
    return {"read": G * k * P * row_passes, "record": G * e * k * 32 * walk_passes, "written": G * e * P}


def narrow_vs_wide(repeats: int) -> dict:
    k, r, P, G, e = 32, 32, 1200, 20000, 4
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.manual_seed(SEED)
    with quicfec.Context(device=0) as narrow_ctx, quicfec.Context(device=0) as wide_ctx, torch.cuda.stream(stream):
        narrow_ctx.decode_plan_mode(quicfec.FEC_PLAN_DEVICE)
        data, par, masks = setup(wide_ctx, G, k, r, P, e, s)
        word0 = masks[:, 0].contiguous()
        out = {a: torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda") for a in ("narrow", "wide")}
        st = {a: torch.full((G,), 7, dtype=torch.uint8, device="cuda") for a in ("narrow", "wide")}
        arms = {"narrow": lambda: narrow_ctx.recover_dev(data, par, word0, G, k, r, P, out["narrow"], st["narrow"], stream=s),
                "wide": lambda: wide_ctx.recover_wide_dev(data, par, masks, G, k, r, P, out["wide"], st["wide"], stream=s)}
        for arm in arms.values():                                           # code objects, matrices, workspaces
            for _ in range(3):
                arm()
        stream.synchronize()
        same = bool(torch.equal(out["narrow"], out["wide"]) and torch.equal(st["narrow"], st["wide"]))
        ms = timed(arms, repeats, stream)
    med = {a: statistics.median(v) for a, v in ms.items()}
    narrow_spread = max(ms["narrow"]) - min(ms["narrow"])
    return {"measure": "wide_vs_narrow", "k": k, "r": r, "P": P, "groups": G, "lost_per_group": e, "repeats": repeats,
            "wide_identical_to_narrow": same, "event_ms": {a: spread(v) for a, v in ms.items()},
            "wide_minus_narrow_ms": round(med["wide"] - med["narrow"], 4), "narrow_min_max_spread_ms": round(narrow_spread, 4),
            "wide_slower_by_more_than_the_spread": bool(med["wide"] - med["narrow"] > narrow_spread)}


def wide_alone(repeats: int) -> dict:
    k, r, P, G, e = 223, 32, 1200, 2000, 16
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    torch.manual_seed(SEED + 1)
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        data, par, masks = setup(ctx, G, k, r, P, e, s)
        out = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
        arms = {"wide": lambda: ctx.recover_wide_dev(data, par, masks, G, k, r, P, out, st, stream=s)}
        for _ in range(3):
            arms["wide"]()
        stream.synchronize()
        # the rebuilt rows are the original data (the e lost shards, ascending)
        lost = ((masks[:, :, None] >> torch.arange(64, device="cuda")) & 1).bool().view(G, 256)[:, :k]
        want = data.view(G, k, P)[lost].view(G, e, P)
        right = bool(torch.equal(out.view(G, r, P)[:, :e], want) and int(st.sum().item()) == 0)
        ms = timed(arms, repeats, stream)["wide"]
    b = algorithmic_bytes(G, k, P, e)
    total = sum(b.values())
    stride = 512 + min(k, r) * k * 32
    return {"measure": "wide_alone", "k": k, "r": r, "P": P, "groups": G, "lost_per_group": e, "repeats": repeats,
            "rebuilt_rows_equal_the_data": right, "event_ms": spread(ms), "algorithmic_bytes": b,
            "achieved_TB_per_s": round(total / (statistics.median(ms) * 1e-3) / 1e12, 4),
            "plan_chunks": -(-G // max(1, (64 << 20) // stride))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "wide" / "measure.json"))
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    results = [narrow_vs_wide(args.repeats), wide_alone(args.repeats)]
    for row in results:
        print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
