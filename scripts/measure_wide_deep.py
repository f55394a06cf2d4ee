"""The wide calls past min(k, r) <= 32 (FEC_WIDE_ROWS_ALL), measured once (recorded, not gated):
fec_recover_wide_rs_dev at 33+33, 100+100 and 128+128 and, for scale, at 32+32 on the wide path;
1200 B, every data shard of every group lost (e = min(k, r) = k), a G that fills four plan chunks.

  1. Whole calls: one process, warm-up, device events, ten repeats; the rebuilt rows are compared
     with the data.  One JSON line per shape, all of them to --out.
  2. The split between the record build and the consumer passes is not visible from a call's events;
     it is taken from a kernel trace of this script, one shape per run:
         rocprofv3 --kernel-trace --stats -d DIR/KxR -o run --output-format csv -- \\
             python scripts/measure_wide_deep.py --shape KxR --calls 5 --note DIR/KxR/run.json
     and then  python scripts/measure_wide_deep.py --summarise DIR --out ...  which divides the
     kernels' total time by the calls and the groups: microseconds per group of the build and of the
     consumer passes, and the bytes per second the consumers achieve over their algorithmic bytes
     (csrc/fec_wide.hip: reads k * P * ceil(e / 8) of survivors and e * k * 32 of record per walk pass,
     writes e * P, per group).
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "quic-test_amd"))

SEED = 0x5EEDDEE9
P = 1200
SHAPES = [(33, 33), (100, 100), (128, 128), (32, 32)]
ARENA = 64 << 20


def plan(k: int, r: int) -> dict:
    stride = 512 + min(k, r) * k * 32
    per_chunk = ARENA // stride
    return {"stride": stride, "per_chunk": per_chunk, "groups": 4 * per_chunk, "plan_chunks": 4, "passes": -(-min(k, r) // 8)}


def algorithmic_bytes(G: int, k: int, e: int) -> dict:
    row_passes = -(-e // 8)
    walk_passes = P // 1024 + -(-(P % 1024) // 256)
    return {"read": G * k * P * row_passes, "record": G * e * k * 32 * walk_passes, "written": G * e * P}


def run_shape(k: int, r: int, calls: int, repeats: int) -> dict:
    import torch
    import quicfec
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    pl = plan(k, r)
    G, e = pl["groups"], min(k, r)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        if min(k, r) > 32:
            ctx.wide_rows_mode(quicfec.FEC_WIDE_ROWS_ALL)
        data = torch.empty(G * k * P, dtype=torch.uint8, device="cuda")
        par = torch.empty(G * r * P, dtype=torch.uint8, device="cuda")
        ctx.fill_random_dev(data, data.numel(), SEED, stream=s)
        ctx.encode_dev(data, G, k, r, P, par, stream=s)
        lost = torch.zeros((G, 256), dtype=torch.bool, device="cuda")
        lost[:, :e] = True                                                  # e = k: every data shard
        masks = (lost.view(G, 4, 64).to(torch.int64) << torch.arange(64, device="cuda")).sum(dim=2).contiguous()
        out = torch.full((G * r * P,), 0x5A, dtype=torch.uint8, device="cuda")
        st = torch.full((G,), 7, dtype=torch.uint8, device="cuda")
        call = lambda: ctx.recover_wide_dev(data, par, masks, G, k, r, P, out, st, stream=s)
        call()                                                              # code objects, the matrix, the workspace
        stream.synchronize()
        right = bool(torch.equal(out.view(G, r, P)[:, :e], data.view(G, k, P)[:, :e]) and int(st.sum().item()) == 0)
        ms = []
        for _ in range(calls):
            call()
        for _ in range(repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            stream.synchronize()
            t0.record(stream)
            call()
            t1.record(stream)
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
        stream.synchronize()
    row = {"measure": "recover_wide_all_data_lost", "k": k, "r": r, "P": P, "lost_per_group": e, **pl,
           "path": "deep" if min(k, r) > 32 else "wide", "rebuilt_rows_equal_the_data": right, "calls_made": 1 + calls + repeats}
    if ms:
        med = statistics.median(ms)
        row["event_ms"] = {"median": round(med, 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
        row["whole_call_us_per_group"] = round(med * 1e3 / G, 3)
    return row


def summarise(root: Path) -> list:
    rows = []
    for k, r in SHAPES:
        d = root / f"{k}x{r}"
        stats = sorted(d.rglob("*kernel_stats.csv"))
        note = d / "run.json"
        if not stats or not note.exists():
            rows.append({"measure": "split", "k": k, "r": r, "build_us_per_group": "unmeasured", "consumer_us_per_group": "unmeasured"})
            continue
        run = json.loads(note.read_text())
        G, calls, e = run["groups"], run["calls_made"], run["lost_per_group"]
        ns = {"build": 0, "consumer": 0, "classify": 0}
        for line in csv.DictReader(stats[0].open()):
            name = line["Name"]
            kind = "build" if "build_records" in name else "consumer" if "decode_wide" in name else "classify" if "classify_wide" in name else None
            if kind:
                ns[kind] += int(line["TotalDurationNs"])
        b = algorithmic_bytes(G, k, e)
        consumer_s = ns["consumer"] / calls * 1e-9
        rows.append({"measure": "split", "k": k, "r": r, "P": P, "groups": G, "lost_per_group": e, "calls": calls, "path": run["path"],
                     "build_us_per_group": round(ns["build"] / calls / G * 1e-3, 3),
                     "consumer_us_per_group": round(ns["consumer"] / calls / G * 1e-3, 3),
                     "classify_us_per_call": round(ns["classify"] / calls * 1e-3, 3), "consumer_algorithmic_bytes": b,
                     "consumer_TB_per_s": round(sum(b.values()) / consumer_s / 1e12, 4) if consumer_s else "unmeasured"})
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "wide_deep" / "measure.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--shape", help="KxR: this shape alone, --calls calls and no events (the run a kernel trace is taken of)")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--note", help="with --shape: where to write what the run did")
    ap.add_argument("--summarise", help="directory of the kernel traces, one KxR subdirectory per shape")
    args = ap.parse_args()
    if args.summarise:
        results = summarise(Path(args.summarise))
    elif args.shape:
        k, r = (int(x) for x in args.shape.split("x"))
        results = [run_shape(k, r, args.calls, 0)]
        if args.note:
            Path(args.note).parent.mkdir(parents=True, exist_ok=True)
            Path(args.note).write_text(json.dumps(results[0]) + "\n")
    else:
        results = [run_shape(k, r, 2, args.repeats) for k, r in SHAPES]
    for row in results:
        print(json.dumps(row), flush=True)
    if not args.shape:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
