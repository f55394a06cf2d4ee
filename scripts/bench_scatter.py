"""The scatter recover against the gather recovers and against a caller's own second pass, in one
process (recorded, not gated).

C3's shape -- k=10 r=3, P=1200, 1M groups, 2 erasures per group (uniform over the 13 shards) -- on
the shuffled 1216-B-stride arena of scripts/bench_gather.py, which here also reserves a row (a
hole, 0xEE) for every lost data packet.  Arms alternate over rounds on one stream, each round
`reps` back-to-back calls timed by HIP events on that stream, medians reported:

  a  fec_recover_gather_rs_dev into the slot layout
  b  fec_recover_scatter_rs_dev without a length table, destinations on the slot layout: b / a is
     the price of the destination table alone
  b_same  b with the destinations on a's own buffer: the same bytes at the same addresses, so
     b_same / a leaves out where the driver placed the second output buffer
  c  the scatter recover into the holes of the arena (in-place gathered decode)
  d  what a caller without the scatter call does: a, then its own pass that moves the rebuilt rows
     from the slots into the holes, with torch indexing
  d_move   that pass alone
  d_ideal  a, then fec_copy_dev of as many bytes in order: a copy at the box's HBM copy rate, the
     least any caller's pass could cost (a lower bound: it scatters nothing)
  e_var      the §7 length mix (half the packets 1200 B, half uniform in 40..1199, parity cut at the
     symbol length): fec_recover_gather_var_rs_dev into full 1200-B slots
  e_scatter  the scatter recover with the length table, destinations on the slot layout
  e_same     e_scatter with the destinations on e_var's own buffer (as b_same)
  e_holes    the same into the holes of the arena

b must write a's bytes, c and d must leave the same packets in the holes, e_scatter the first L_g
bytes of e_var's rows and 0x5A after them, e_holes the original packets.  Prints one JSON line.

  python scripts/bench_scatter.py [--groups 1000000] [--rounds 7] [--reps 20]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "quic-test_amd"))
sys.path.insert(0, str(REPO / "scripts"))
import quicfec  # noqa: E402
from bench_gather_var import CHUNK, fill_arena, timed  # noqa: E402

K, R, P, ERASURES, STRIDE = 10, 3, 1200, 2, 1216
N = K + R
SEED = 0x5EED5CA7


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
    res = {"bench": "scatter", "k": K, "r": R, "P": P, "groups": G, "erasures": ERASURES, "stride": STRIDE,
           "rounds": args.rounds, "reps": args.reps}
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        s = stream.cuda_stream
        col = torch.arange(P, device=dev)
        data = torch.empty(G * K * P, dtype=torch.uint8, device=dev)
        par = torch.empty(G * R * P, dtype=torch.uint8, device=dev)
        ctx.fill_random_dev(data, data.numel(), SEED, stream=s)
        ctx.encode_dev(data, G, K, R, P, par, stream=s)
        lost = torch.zeros((G, N), dtype=torch.bool, device=dev)
        lost.scatter_(1, torch.rand((G, N), device=dev).argsort(dim=1)[:, :ERASURES], True)
        lost_d = lost[:, :K]
        hole = torch.cat([lost_d, torch.zeros((G, R), dtype=torch.bool, device=dev)], dim=1)   # every lost data packet is rebuilt
        placed = ~lost | hole
        n_rows = int(placed.sum().item())
        n_holes = int(hole.sum().item())
        slot = torch.full((G, N), -1, dtype=torch.int64, device=dev)
        slot[placed] = torch.randperm(n_rows, device=dev)
        src_slot = torch.where(lost, torch.full_like(slot, -1), slot)
        m = (lost_d.cumsum(dim=1) - 1)[lost_d]                                # the m-th lost of its group
        gi = lost_d.nonzero()[:, 0]
        slot_rows = gi * R + m                                                # row of the slot layout
        hole_rows = slot[:, :K][lost_d]                                       # row of the arena

        def arena_of(parts, lens):
            arena = torch.full((n_rows * STRIDE,), 0xEE, dtype=torch.uint8, device=dev)
            fill_arena(arena, src_slot, parts, lens, G)
            table = torch.where(src_slot >= 0, arena.data_ptr() + src_slot * STRIDE, torch.zeros_like(slot)).contiguous()
            dests = torch.where(lost_d, arena.data_ptr() + slot[:, :K] * STRIDE, torch.zeros_like(slot[:, :K])).contiguous()
            return arena, table, dests

        def slot_dests(out):
            d = torch.zeros((G, K), dtype=torch.int64, device=dev)
            d[lost_d] = out.data_ptr() + slot_rows * P
            return d.contiguous()

        full = torch.full((G, N), P, dtype=torch.int32, device=dev)
        arena, table, holes = arena_of([data.view(G, K, P), par.view(G, R, P)], full)
        lost_packets = data.view(G, K, P)[lost_d].clone()
        # e: the length mix.  The packets are cut in place, the parity is theirs.
        dl = torch.where(torch.rand((G, K), device=dev) < 0.5, torch.full((G, K), P, device=dev),
                         torch.randint(40, P, (G, K), device=dev)).to(torch.int32)
        dv = data.view(G, K, P)
        for g0 in range(0, G, CHUNK):
            g1 = min(G, g0 + CHUNK)
            dv[g0:g1] *= (col[None, None, :] < dl[g0:g1, :, None])
        ctx.encode_dev(data, G, K, R, P, par, stream=s)
        sym = dl.max(dim=1).values                                            # the symbol length the sender's repair packets carry
        lens = torch.cat([dl, sym[:, None].expand(G, R)], dim=1).contiguous()
        arena_v, table_v, holes_v = arena_of([dv, par.view(G, R, P)], lens)
        lost_packets_v = dv[lost_d].clone()
        # L_g as the receiver sees it: over the present entries
        seen = torch.where(lost, torch.zeros_like(lens), lens).max(dim=1).values
        del par

        out = {a: torch.full((G * R * P,), 0x5A, dtype=torch.uint8, device=dev) for a in ("a", "b", "e_var", "e_scatter")}
        st = {a: torch.full((G,), 7, dtype=torch.uint8, device=dev) for a in ("a", "b", "c", "e_var", "e_scatter", "e_holes")}
        dests_a, dests_b, dests_e = slot_dests(out["a"]), slot_dests(out["b"]), slot_dests(out["e_scatter"])
        dests_ev = slot_dests(out["e_var"])
        symo = torch.zeros(G, dtype=torch.int32, device=dev)
        copy_bytes = n_holes * P // 16 * 16
        scratch = torch.empty(copy_bytes, dtype=torch.uint8, device=dev)
        arena_rows = arena.view(-1, STRIDE)

        def move():
            arena_rows[hole_rows, :P] = out["a"].view(-1, P)[slot_rows]

        def arm(a):
            if a == "a":
                ctx.recover_gather_dev(table, G, K, R, P, out["a"], st["a"], stream=s)
            elif a == "b":
                ctx.recover_scatter_dev(table, None, dests_b, G, K, R, P, st["b"], stream=s)
            elif a == "b_same":
                ctx.recover_scatter_dev(table, None, dests_a, G, K, R, P, st["b"], stream=s)
            elif a == "c":
                ctx.recover_scatter_dev(table, None, holes, G, K, R, P, st["c"], stream=s)
            elif a == "d":
                ctx.recover_gather_dev(table, G, K, R, P, out["a"], st["a"], stream=s)
                move()
            elif a == "d_move":
                move()
            elif a == "d_ideal":
                ctx.recover_gather_dev(table, G, K, R, P, out["a"], st["a"], stream=s)
                ctx.copy_dev(out["a"], scratch, copy_bytes, stream=s)
            elif a == "e_var":
                ctx.recover_gather_var_dev(table_v, lens, G, K, R, P, out["e_var"], st["e_var"], None, symo, stream=s)
            elif a == "e_scatter":
                ctx.recover_scatter_dev(table_v, lens, dests_e, G, K, R, P, st["e_scatter"], None, symo, stream=s)
            elif a == "e_same":
                ctx.recover_scatter_dev(table_v, lens, dests_ev, G, K, R, P, st["e_scatter"], None, symo, stream=s)
            else:  # e_holes
                ctx.recover_scatter_dev(table_v, lens, holes_v, G, K, R, P, st["e_holes"], None, symo, stream=s)

        # the holes after c alone, then after d alone
        arm("c")
        stream.synchronize()
        holes_c = arena_rows[hole_rows].clone()
        arena_rows[hole_rows] = 0xEE
        arm("d")
        stream.synchronize()
        holes_d = arena_rows[hole_rows].clone()
        arms = ["a", "b", "b_same", "c", "d", "d_move", "d_ideal", "e_var", "e_scatter", "e_same", "e_holes"]
        for a in arms:
            for _ in range(2):
                arm(a)
        stream.synchronize()
        cut = col[None, :] < seen[gi][:, None]                                # the first L_g bytes of a rebuilt row
        rows_var = out["e_var"].view(-1, P)[slot_rows]
        rows_sc = out["e_scatter"].view(-1, P)[slot_rows]
        rows_holes = arena_v.view(-1, STRIDE)[hole_rows]
        same = {
            "b_a": bool(torch.equal(out["b"], out["a"]) and torch.equal(st["b"], st["a"])),
            "a_packets": bool(torch.equal(out["a"].view(-1, P)[slot_rows], lost_packets)),
            "c_holes": bool(torch.equal(holes_c[:, :P], lost_packets) and bool((holes_c[:, P:] == 0xEE).all())),
            "d_holes": bool(torch.equal(holes_d, holes_c)),
            "status": bool(all(int(v.sum().item()) == 0 for v in st.values())),
            "e_var_packets": bool(torch.equal(rows_var, lost_packets_v)),
            "e_scatter_cut": bool(torch.equal(torch.where(cut, rows_var, torch.full_like(rows_var, 0x5A)), rows_sc)),
            "e_holes_cut": bool(torch.equal(torch.where(cut, lost_packets_v, torch.full_like(rows_var, 0xEE)), rows_holes[:, :P])
                                and bool((rows_holes[:, P:] == 0xEE).all())),
            "symbol_len": bool(torch.equal(symo, seen)),
        }
        del holes_c, holes_d, rows_var, rows_sc, rows_holes, cut
        ms = timed(stream, arms, arm, args.rounds, args.reps)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        res["recover"] = {
            "arena_rows": n_rows, "rebuilt_rows": n_holes, "identical": same,
            "ms": {a: [round(x, 4) for x in v] for a, v in ms.items()}, "median_ms": {a: round(v, 4) for a, v in med.items()},
            "a_spread": round((max(ms["a"]) - min(ms["a"])) / med["a"], 4),
            "b_vs_a": round(med["b"] / med["a"], 4), "b_same_vs_a": round(med["b_same"] / med["a"], 4), "c_vs_a": round(med["c"] / med["a"], 4),
            "c_vs_d": round(med["c"] / med["d"], 4), "c_vs_d_ideal": round(med["c"] / med["d_ideal"], 4),
            "e_scatter_vs_e_var": round(med["e_scatter"] / med["e_var"], 4),
            "e_same_vs_e_var": round(med["e_same"] / med["e_var"], 4),
            "e_holes_vs_e_var": round(med["e_holes"] / med["e_var"], 4),
            "bytes_written_full_rows": n_holes * P, "bytes_written_cut": int(seen[gi].sum().item()),
        }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
