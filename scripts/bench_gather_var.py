"""The variable-length address-table calls against the fixed-length ones, in one process
(recorded, not gated).

C3's shape -- k=10 r=3, P=1200, 1M groups, 2 erasures per group (uniform over the 13 shards) -- on
the shuffled 1216-B-stride arena of scripts/bench_gather.py, arms alternating over rounds on one
stream, each round `reps` back-to-back calls timed by HIP events on that stream, medians reported:

  a  fec_recover_gather_rs_dev, every shard 1200 B
  b  fec_recover_gather_var_rs_dev on a's table with every length = 1200: b / a is what the length
     handling costs
  c  the var call on a seeded length mix (half the packets 1200 B, half uniform in 40..1199): the
     packets sit at their true length in their arena slots (0xEE after them), the parity shards
     are cut at their group's symbol length
  d  what a caller without the var call does: c's shards copied into zero-filled 1200-B slots
     (a masked copy in arena order, the cheapest such copy), then a on the copies
  d_copy  that copy alone
  d_ideal a after fec_copy_dev of as many bytes in order: a copy at the box's HBM copy rate, the
     least any caller's copy could cost (a lower bound: it masks nothing)

and the same for the encode (all k packets of every group in an arena of their own):
  ea fec_encode_gather_rs_dev, eb the var encode with every length 1200, ec the var encode on the
  length mix, ed the masked copy then ea, ed_copy the copy alone, ed_ideal the in-order copy then ea.

b must write a's bytes, c must write d's, eb ea's, ec ed's; c's rows are also the original
zero-padded packets.  Prints one JSON line.

  python scripts/bench_gather_var.py [--groups 1000000] [--rounds 7] [--reps 20]
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
SEED = 0x5EED7A4E
CHUNK = 1 << 16   # groups per step while an arena is filled
ROWS = 1 << 20    # arena rows per step of the caller's masked copy


def timed(stream, arms, arm, rounds, reps):
    ms = {a: [] for a in arms}
    for rd in range(rounds):
        for a in arms[rd % len(arms):] + arms[:rd % len(arms)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                arm(a)
            e1.record(stream)
            e1.synchronize()
            ms[a].append(e0.elapsed_time(e1) / reps)
    return ms


def fill_arena(arena, slot, parts, lens, G):
    """Shard (g, s) of `parts` (tensors (G, n_i, P), concatenated along s) to row slot[g, s], its first
    lens[g, s] bytes; what follows in the row keeps the arena's fill."""
    rows = arena.view(-1, STRIDE)
    col = torch.arange(P, device=arena.device)
    for g0 in range(0, G, CHUNK):
        g1 = min(G, g0 + CHUNK)
        both = torch.cat([p[g0:g1] for p in parts], dim=1)
        keep = slot[g0:g1] >= 0
        idx = slot[g0:g1][keep]
        old = rows[idx, :P]
        rows[idx, :P] = torch.where(col[None, :] < lens[g0:g1][keep][:, None], both[keep], old)
        del both, old


def masked_copy(src_arena, lens_rows, dst):
    """The caller's copy: every arena row's first len bytes into its zero-filled P-byte slot."""
    rows = src_arena.view(-1, STRIDE)
    col = torch.arange(P, device=dst.device)
    zero = torch.zeros((), dtype=torch.uint8, device=dst.device)
    out = dst.view(-1, P)
    for r0 in range(0, rows.shape[0], ROWS):
        r1 = min(rows.shape[0], r0 + ROWS)
        out[r0:r1] = torch.where(col[None, :] < lens_rows[r0:r1, None], rows[r0:r1, :P], zero)


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
    res = {"bench": "gather_var", "k": K, "r": R, "P": P, "groups": G, "erasures": ERASURES, "stride": STRIDE,
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
        n_surv = int((~lost).sum().item())
        slot = torch.full((G, N), -1, dtype=torch.int64, device=dev)
        slot[~lost] = torch.randperm(n_surv, device=dev)
        full = torch.full((G, N), P, dtype=torch.int32, device=dev)
        # a, b: every shard 1200 B
        arena = torch.full((n_surv * STRIDE,), 0xEE, dtype=torch.uint8, device=dev)
        fill_arena(arena, slot, [data.view(G, K, P), par.view(G, R, P)], full, G)
        table = torch.where(slot >= 0, arena.data_ptr() + slot * STRIDE, torch.zeros_like(slot)).contiguous()
        # c, d: the length mix.  The packets are cut in place, the parity is theirs.
        dl = torch.where(torch.rand((G, K), device=dev) < 0.5, torch.full((G, K), P, device=dev),
                         torch.randint(40, P, (G, K), device=dev)).to(torch.int32)
        dv = data.view(G, K, P)
        for g0 in range(0, G, CHUNK):
            g1 = min(G, g0 + CHUNK)
            dv[g0:g1] *= (col[None, None, :] < dl[g0:g1, :, None])
        par_v = torch.empty_like(par)
        ctx.encode_dev(data, G, K, R, P, par_v, stream=s)
        sym = dl.max(dim=1).values
        lens = torch.cat([dl, sym[:, None].expand(G, R)], dim=1).contiguous()
        arena_v = torch.full((n_surv * STRIDE,), 0xEE, dtype=torch.uint8, device=dev)
        fill_arena(arena_v, slot, [dv, par_v.view(G, R, P)], lens, G)
        table_v = torch.where(slot >= 0, arena_v.data_ptr() + slot * STRIDE, torch.zeros_like(slot)).contiguous()
        lens_rows = torch.zeros(n_surv, dtype=torch.int32, device=dev)
        lens_rows[slot[~lost]] = lens[~lost]
        slots_d = torch.zeros(n_surv * P, dtype=torch.uint8, device=dev)
        table_d = torch.where(slot >= 0, slots_d.data_ptr() + slot * P, torch.zeros_like(slot)).contiguous()

        out = {a: torch.full((G * R * P,), 0x5A, dtype=torch.uint8, device=dev) for a in "abcd"}
        st = {a: torch.full((G,), 7, dtype=torch.uint8, device=dev) for a in "abcd"}
        symo = torch.zeros(G, dtype=torch.int32, device=dev)
        copy_bytes = n_surv * P // 16 * 16
        scratch = torch.empty(max(copy_bytes, G * K * P), dtype=torch.uint8, device=dev)   # the encode's copy too

        def arm(a):
            if a == "a":
                ctx.recover_gather_dev(table, G, K, R, P, out["a"], st["a"], stream=s)
            elif a == "b":
                ctx.recover_gather_var_dev(table, full, G, K, R, P, out["b"], st["b"], None, symo, stream=s)
            elif a == "c":
                ctx.recover_gather_var_dev(table_v, lens, G, K, R, P, out["c"], st["c"], None, symo, stream=s)
            elif a == "d":
                masked_copy(arena_v, lens_rows, slots_d)
                ctx.recover_gather_dev(table_d, G, K, R, P, out["d"], st["d"], stream=s)
            elif a == "d_copy":
                masked_copy(arena_v, lens_rows, slots_d)
            else:  # d_ideal
                ctx.copy_dev(arena_v, scratch, copy_bytes, stream=s)
                ctx.recover_gather_dev(table, G, K, R, P, out["a"], st["a"], stream=s)

        arms = ["a", "b", "c", "d", "d_copy", "d_ideal"]
        for a in arms:
            for _ in range(2):
                arm(a)
        stream.synchronize()
        same = {"b_a": bool(torch.equal(out["b"], out["a"]) and torch.equal(st["b"], st["a"])),
                "c_d": bool(torch.equal(out["c"], out["d"]) and torch.equal(st["c"], st["d"]))}
        # c's rows are the original zero-padded packets
        lost_d = lost[:, :K]
        m = (lost_d.cumsum(dim=1) - 1)[lost_d]
        gi = lost_d.nonzero()[:, 0]
        same["c_packets"] = bool(torch.equal(out["c"].view(G, R, P)[gi, m], dv[lost_d]))
        rebuilt_rows = int(lost_d.sum().item())
        # the survivors a rebuilding group reads: its surviving data and its e lowest surviving parity rows
        e = lost_d.sum(dim=1)
        alive_p = ~lost[:, K:]
        used = torch.cat([~lost_d & (e > 0)[:, None], alive_p & (alive_p.cumsum(dim=1) <= e[:, None])], dim=1)
        read_fixed = int(used.sum().item()) * P
        read_var = int(lens[used].sum().item())
        ms = timed(stream, arms, arm, args.rounds, args.reps)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        res["recover"] = {
            "survivors": n_surv, "rebuilt_rows": rebuilt_rows, "identical": same,
            "ms": {a: [round(x, 4) for x in v] for a, v in ms.items()}, "median_ms": {a: round(v, 4) for a, v in med.items()},
            "a_spread": round((max(ms["a"]) - min(ms["a"])) / med["a"], 4),
            "b_vs_a": round(med["b"] / med["a"], 4), "c_vs_d": round(med["c"] / med["d"], 4), "c_vs_d_ideal": round(med["c"] / med["d_ideal"], 4),
            "c_vs_a": round(med["c"] / med["a"], 4),
            "extra_table_bytes_share": round(N * 4 / (K * P + ERASURES * P), 5),
            "bytes_read_fixed": read_fixed, "bytes_read_var": read_var, "bytes_not_read": read_fixed - read_var,
        }
        del arena, arena_v, slots_d, out, par, table, table_v, table_d

        # ---- encode: all k packets of every group in an arena of their own, in random order ----
        eslot = torch.randperm(G * K, device=dev).view(G, K)
        efull = torch.full((G, K), P, dtype=torch.int32, device=dev)
        ectx_data = torch.empty(G * K * P, dtype=torch.uint8, device=dev)          # full-length packets again
        ctx.fill_random_dev(ectx_data, ectx_data.numel(), SEED, stream=s)
        earena = torch.full((G * K * STRIDE,), 0xEE, dtype=torch.uint8, device=dev)
        fill_arena(earena, eslot, [ectx_data.view(G, K, P)], efull, G)
        del ectx_data
        earena_v = torch.full((G * K * STRIDE,), 0xEE, dtype=torch.uint8, device=dev)
        fill_arena(earena_v, eslot, [dv], dl, G)
        etable = (earena.data_ptr() + eslot * STRIDE).contiguous()
        etable_v = (earena_v.data_ptr() + eslot * STRIDE).contiguous()
        elens_rows = torch.zeros(G * K, dtype=torch.int32, device=dev)
        elens_rows[eslot.reshape(-1)] = dl.reshape(-1)
        eslots_d = torch.zeros(G * K * P, dtype=torch.uint8, device=dev)
        etable_d = (eslots_d.data_ptr() + eslot * P).contiguous()
        eout = {a: torch.full((G * R * P,), 0x5A, dtype=torch.uint8, device=dev) for a in ("ea", "eb", "ec", "ed")}

        def earm(a):
            if a == "ea":
                ctx.encode_gather_dev(etable, G, K, R, P, eout["ea"], stream=s)
            elif a == "eb":
                ctx.encode_gather_var_dev(etable, efull, G, K, R, P, eout["eb"], symo, stream=s)
            elif a == "ec":
                ctx.encode_gather_var_dev(etable_v, dl, G, K, R, P, eout["ec"], symo, stream=s)
            elif a == "ed":
                masked_copy(earena_v, elens_rows, eslots_d)
                ctx.encode_gather_dev(etable_d, G, K, R, P, eout["ed"], stream=s)
            elif a == "ed_copy":
                masked_copy(earena_v, elens_rows, eslots_d)
            else:  # ed_ideal
                ctx.copy_dev(earena_v, scratch, G * K * P, stream=s)
                ctx.encode_gather_dev(etable, G, K, R, P, eout["ea"], stream=s)

        earms = ["ea", "eb", "ec", "ed", "ed_copy", "ed_ideal"]
        for a in earms:
            for _ in range(2):
                earm(a)
        stream.synchronize()
        esame = {"eb_ea": bool(torch.equal(eout["eb"], eout["ea"])), "ec_ed": bool(torch.equal(eout["ec"], eout["ed"])),
                 "ec_parity": bool(torch.equal(eout["ec"], par_v)), "symbol_len": bool(torch.equal(symo, sym))}
        ms = timed(stream, earms, earm, args.rounds, args.reps)
        med = {a: sorted(v)[len(v) // 2] for a, v in ms.items()}
        res["encode"] = {
            "identical": esame, "ms": {a: [round(x, 4) for x in v] for a, v in ms.items()},
            "median_ms": {a: round(v, 4) for a, v in med.items()},
            "ea_spread": round((max(ms["ea"]) - min(ms["ea"])) / med["ea"], 4),
            "eb_vs_ea": round(med["eb"] / med["ea"], 4), "ec_vs_ed": round(med["ec"] / med["ed"], 4),
            "ec_vs_ed_ideal": round(med["ec"] / med["ed_ideal"], 4),
            "ec_vs_ea": round(med["ec"] / med["ea"], 4),
            "bytes_read_fixed": G * K * P, "bytes_read_var": int(dl.sum().item()),
            "bytes_not_read": G * K * P - int(dl.sum().item()),
        }
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
