"""The scatter encode against the gather encodes and against a sender's own second pass, in one
process (recorded, not gated).

C2's shape -- k=10 r=3, P=1200, 1M groups -- on the shuffled 1216-B-stride arena of
scripts/bench_gather_var.py (fill_arena), which here also reserves a row (0xEE) for every repair
payload: the hole behind its header in the send ring.  Arms alternate over rounds on one stream,
each round `reps` back-to-back calls timed by HIP events on that stream, medians reported:

  a  fec_encode_gather_rs_dev into the slot layout
  b  fec_encode_scatter_rs_dev without a length table, destinations on a second buffer in the slot
     layout: b / a is the price of the destination table and of the runtime-k kernel
  b_same  b with the destinations on a's own buffer: the same bytes at the same addresses, so
     b_same / a leaves out where the driver placed the second output buffer
  c  the scatter encode into the reserved rows of the arena
  d  what a sender without the scatter call does: a, then its own pass that moves the rows from the
     slots to those places, with torch indexing
  d_move   that pass alone
  d_ideal  a, then fec_copy_dev of as many bytes in order: a copy at the box's HBM copy rate, the
     least any sender's pass could cost (a lower bound: it scatters nothing)
  e_var      the §7 length mix (half the packets 1200 B, half uniform in 40..1199):
     fec_encode_gather_var_rs_dev into full 1200-B slots
  e_scatter  the scatter encode with the length table, destinations on the slot layout
  e_holes    the same into the reserved rows of the arena
  s_var      a short mix, every length uniform in 40..300, through fec_encode_gather_var_rs_dev
  s_scatter  the same short mix through the scatter encode, destinations on the slot layout

a must write the contiguous encode's parity, b a's bytes, c and d must leave the same rows in the
reserved places, e_scatter / s_scatter the first L_g bytes of e_var's / s_var's rows and 0x5A after
them, e_holes the same bytes in the arena and 0xEE after them.  Prints one JSON line.

  python scripts/bench_scatter_encode.py [--groups 1000000] [--rounds 7] [--reps 20]
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

K, R, P, STRIDE = 10, 3, 1200, 1216
N = K + R
SEED = 0x5EED5CE7
ROWS = 1 << 19   # rows per step of a check


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
    res = {"bench": "scatter_encode", "k": K, "r": R, "P": P, "groups": G, "stride": STRIDE, "rounds": args.rounds,
           "reps": args.reps}
    with quicfec.Context(device=0) as ctx, torch.cuda.stream(stream):
        s = stream.cuda_stream
        col = torch.arange(P, device=dev)
        data = torch.empty(G * K * P, dtype=torch.uint8, device=dev)
        ctx.fill_random_dev(data, data.numel(), SEED, stream=s)
        dv = data.view(G, K, P)
        par = torch.empty(G * R * P, dtype=torch.uint8, device=dev)          # the contiguous encode's parity
        ctx.encode_dev(data, G, K, R, P, par, stream=s)
        slot = torch.randperm(G * N, device=dev).view(G, N)                  # packets, then the group's repair rows
        hole_rows = slot[:, K:].reshape(-1)

        def arena_of(lens):
            arena = torch.full((G * N * STRIDE,), 0xEE, dtype=torch.uint8, device=dev)
            fill_arena(arena, slot[:, :K], [dv], lens, G)
            table = (arena.data_ptr() + slot[:, :K] * STRIDE).contiguous()
            holes = (arena.data_ptr() + slot[:, K:] * STRIDE).contiguous()
            return arena, table, holes

        def slot_dests(out):
            return (out.data_ptr() + torch.arange(G * R, device=dev) * P).contiguous()

        def cut_data(lens):                                                  # the packets cut in place
            for g0 in range(0, G, CHUNK):
                g1 = min(G, g0 + CHUNK)
                dv[g0:g1] *= (col[None, None, :] < lens[g0:g1, :, None])

        full = torch.full((G, K), P, dtype=torch.int32, device=dev)
        arena, table, holes = arena_of(full)
        # e: the length mix
        dl = torch.where(torch.rand((G, K), device=dev) < 0.5, torch.full((G, K), P, device=dev),
                         torch.randint(40, P, (G, K), device=dev)).to(torch.int32)
        cut_data(dl)
        arena_v, table_v, holes_v = arena_of(dl)
        sym_v = dl.max(dim=1).values
        # s: the short mix
        ds = torch.randint(40, 301, (G, K), device=dev).to(torch.int32)
        cut_data(ds)
        arena_s, table_s, _ = arena_of(ds)
        sym_s = ds.max(dim=1).values
        del data, dv

        names = ("a", "b", "e_var", "e_scatter", "s_var", "s_scatter")
        out = {a: torch.full((G * R * P,), 0x5A, dtype=torch.uint8, device=dev) for a in names}
        dests = {a: slot_dests(out[a]) for a in ("a", "b", "e_scatter", "s_scatter")}
        symo = {a: torch.zeros(G, dtype=torch.int32, device=dev) for a in ("e_var", "e_scatter", "e_holes", "s_var", "s_scatter")}
        scratch = torch.empty(G * R * P, dtype=torch.uint8, device=dev)
        arena_rows = arena.view(-1, STRIDE)

        def move():
            arena_rows[hole_rows, :P] = out["a"].view(-1, P)

        def arm(a):
            if a == "a":
                ctx.encode_gather_dev(table, G, K, R, P, out["a"], stream=s)
            elif a == "b":
                ctx.encode_scatter_dev(table, None, dests["b"], G, K, R, P, stream=s)
            elif a == "b_same":
                ctx.encode_scatter_dev(table, None, dests["a"], G, K, R, P, stream=s)
            elif a == "c":
                ctx.encode_scatter_dev(table, None, holes, G, K, R, P, stream=s)
            elif a == "d":
                ctx.encode_gather_dev(table, G, K, R, P, out["a"], stream=s)
                move()
            elif a == "d_move":
                move()
            elif a == "d_ideal":
                ctx.encode_gather_dev(table, G, K, R, P, out["a"], stream=s)
                ctx.copy_dev(out["a"], scratch, G * R * P, stream=s)
            elif a == "e_var":
                ctx.encode_gather_var_dev(table_v, dl, G, K, R, P, out["e_var"], symo["e_var"], stream=s)
            elif a == "e_scatter":
                ctx.encode_scatter_dev(table_v, dl, dests["e_scatter"], G, K, R, P, symo["e_scatter"], stream=s)
            elif a == "e_holes":
                ctx.encode_scatter_dev(table_v, dl, holes_v, G, K, R, P, symo["e_holes"], stream=s)
            elif a == "s_var":
                ctx.encode_gather_var_dev(table_s, ds, G, K, R, P, out["s_var"], symo["s_var"], stream=s)
            else:  # s_scatter
                ctx.encode_scatter_dev(table_s, ds, dests["s_scatter"], G, K, R, P, symo["s_scatter"], stream=s)

        def rows_equal(got_rows, want_rows, L, after, width):
            """got_rows[:, :P] is want_rows cut at L per row with `after` behind it, up to `width` bytes per row."""
            for r0 in range(0, got_rows.shape[0], ROWS):
                r1 = min(got_rows.shape[0], r0 + ROWS)
                want = torch.full((r1 - r0, width), after, dtype=torch.uint8, device=dev)
                want[:, :P] = torch.where(col[None, :] < L[r0:r1, None], want_rows[r0:r1], want[:, :P])
                if not torch.equal(got_rows[r0:r1], want):
                    return False
            return True

        # the reserved rows after c alone, then after d alone
        arm("c")
        stream.synchronize()
        holes_c = arena_rows[hole_rows].clone()
        arena_rows[hole_rows] = 0xEE
        arm("d")
        stream.synchronize()
        holes_d = arena_rows[hole_rows].clone()
        arms = ["a", "b", "b_same", "c", "d", "d_move", "d_ideal", "e_var", "e_scatter", "e_holes", "s_var", "s_scatter"]
        for a in arms:
            for _ in range(2):
                arm(a)
        stream.synchronize()
        Pfull = torch.full((G * R,), P, dtype=torch.int32, device=dev)
        Lv, Ls = sym_v.repeat_interleave(R), sym_s.repeat_interleave(R)
        same = {
            "a_parity": bool(torch.equal(out["a"], par)),
            "b_a": bool(torch.equal(out["b"], out["a"])),
            "c_holes": rows_equal(holes_c, out["a"].view(-1, P), Pfull, 0xEE, STRIDE),
            "d_holes": bool(torch.equal(holes_d, holes_c)),
            "e_scatter_cut": rows_equal(out["e_scatter"].view(-1, P), out["e_var"].view(-1, P), Lv, 0x5A, P),
            "e_holes_cut": rows_equal(arena_v.view(-1, STRIDE)[hole_rows], out["e_var"].view(-1, P), Lv, 0xEE, STRIDE),
            "s_scatter_cut": rows_equal(out["s_scatter"].view(-1, P), out["s_var"].view(-1, P), Ls, 0x5A, P),
            "symbol_len": bool(all(torch.equal(symo[a], sym_v) for a in ("e_var", "e_scatter", "e_holes")) and
                               all(torch.equal(symo[a], sym_s) for a in ("s_var", "s_scatter"))),
        }
        del holes_c, holes_d, par
        ms = timed(stream, arms, arm, args.rounds, args.reps)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        ratio = lambda x, y: round(med[x] / med[y], 4)   # noqa: E731
        res["encode"] = {
            "arena_rows": G * N, "parity_rows": G * R, "identical": same,
            "ms": {a: [round(x, 4) for x in v] for a, v in ms.items()}, "median_ms": {a: round(v, 4) for a, v in med.items()},
            "a_spread": round((max(ms["a"]) - min(ms["a"])) / med["a"], 4),
            "b_vs_a": ratio("b", "a"), "b_same_vs_a": ratio("b_same", "a"), "c_vs_a": ratio("c", "a"),
            "c_vs_d": ratio("c", "d"), "c_vs_d_ideal": ratio("c", "d_ideal"),
            "e_var_vs_a": ratio("e_var", "a"), "e_scatter_vs_e_var": ratio("e_scatter", "e_var"),
            "e_holes_vs_e_var": ratio("e_holes", "e_var"),
            "s_var_vs_a": ratio("s_var", "a"), "s_scatter_vs_s_var": ratio("s_scatter", "s_var"),
            "bytes_written_full_rows": G * R * P, "bytes_written_cut_e": int(sym_v.sum().item()) * R,
            "bytes_written_cut_s": int(sym_s.sum().item()) * R,
            "bytes_read_full": G * K * P, "bytes_read_e": int(dl.sum().item()), "bytes_read_s": int(ds.sum().item()),
        }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
