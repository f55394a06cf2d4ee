"""The wide scatter encode, measured once (recorded, not gated): one process, warm-up, device events
around each call on a side stream, ten repeats, the two calls of a pair alternating.

Packets are 1200 B, every length P (no length table), the tables point into the contiguous layout and
the destinations are the slots d_parity + (g*r + i)*P, so both calls of a pair move the same bytes.
Both yardsticks are calls that existed before this one:
  (a) 32+32 and 56+8, 20,000 groups: fec_encode_scatter_wide_rs_dev against fec_encode_scatter_rs_dev on
      the same tables;
  (b) 224+32 and 128+128, 2,000 groups: fec_encode_scatter_wide_rs_dev against fec_encode_batch_rs_dev on
      the same packets laid contiguously.
Outputs are compared byte for byte.  Each arm's time is the median (min-max) of its repeats; the margin
that counts as "no slower" is the yardstick's own min-max spread in this process.

Prints one JSON line per pair and writes all to --out.

  python scripts/measure_wide_encode.py [--out profiles/wide_encode/measure.json] [--repeats 10]
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
from measure_wide import SEED, spread, timed  # noqa: E402


def algorithmic_bytes(G, k, r, P, table):
    """The wide kernel's own account (csrc/fec_wide_encode.hip); the yardsticks read each packet once per
    pass of theirs, which is not restated here: the bytes a caller moves are packets + rows."""
    row_passes = -(-r // 8)
    walk_passes = P // 1024 + -(-(P % 1024) // 256)
    b = {"read": G * k * P * row_passes, "coefficients": G * r * k * 32 * walk_passes, "written": G * r * P}
    if table:
        b["tables"] = G * row_passes * (k * 8 + 8 * 8)
    return b


def one(k, r, P, G, yardstick, repeats):
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        data = torch.empty(G * k * P, dtype=torch.uint8, device="cuda")
        ctx.fill_random_dev(data, data.numel(), SEED + k * 1000 + r, stream=s)
        out = {a: torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda") for a in ("wide", yardstick)}
        sym = {a: torch.full((G,), -1, dtype=torch.int32, device="cuda") for a in ("wide", yardstick)}
        addrs = (data.data_ptr() + torch.arange(G * k, device="cuda", dtype=torch.int64) * P).contiguous()
        dests = {a: (out[a].data_ptr() + torch.arange(G * r, device="cuda", dtype=torch.int64) * P).contiguous() for a in out}
        arms = {"wide": lambda: ctx.encode_scatter_wide_dev(addrs, None, dests["wide"], G, k, r, P, sym["wide"], stream=s)}
        if yardstick == "scatter":
            arms["scatter"] = lambda: ctx.encode_scatter_dev(addrs, None, dests["scatter"], G, k, r, P, sym["scatter"], stream=s)
        else:
            arms["batch"] = lambda: ctx.encode_dev(data, G, k, r, P, out["batch"], stream=s)
        for arm in arms.values():                                           # code objects, coefficient tables
            for _ in range(3):
                arm()
        stream.synchronize()
        same = bool(torch.equal(out["wide"], out[yardstick]))
        lengths = bool((sym["wide"] == P).all().item())
        ms = timed(arms, repeats, stream)
    med = {a: statistics.median(v) for a, v in ms.items()}
    margin = max(ms[yardstick]) - min(ms[yardstick])
    bytes_ = algorithmic_bytes(G, k, r, P, True)
    return {"measure": f"wide_encode_vs_{yardstick}", "k": k, "r": r, "P": P, "groups": G, "repeats": repeats,
            "outputs_identical": same, "symbol_lengths_are_P": lengths,
            "event_ms": {a: spread(v) for a, v in ms.items()},
            "wide_algorithmic_bytes": bytes_,
            "wide_achieved_TB_per_s": round(sum(bytes_.values()) / (med["wide"] * 1e-3) / 1e12, 4),
            "caller_bytes_TB_per_s": {a: round(G * (k + r) * P / (med[a] * 1e-3) / 1e12, 4) for a in ms},
            "wide_over_yardstick_time": round(med["wide"] / med[yardstick], 4),
            "yardstick_min_max_spread_ms": round(margin, 4),
            "wide_slower_by_more_than_the_spread": bool(med["wide"] - med[yardstick] > margin)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "wide_encode" / "measure.json"))
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    results = []
    for k, r, G, yardstick in ((32, 32, 20000, "scatter"), (56, 8, 20000, "scatter"), (224, 32, 2000, "batch"),
                               (128, 128, 2000, "batch")):
        results.append(one(k, r, 1200, G, yardstick, args.repeats))
        print(json.dumps(results[-1]), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
