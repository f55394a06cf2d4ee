"""CPU tests of tests/big_buffers.py: the arithmetic the 4 GiB offset tests stand on."""
import numpy as np
import pytest

import big_buffers as bb

# the shapes of tests/test_gpu_offsets_4gib.py: (G, rows, P) of every buffer a case claims to cross
CASE_BUFFERS = [(1_200_000, 10, 1200), (1_200_000, 3, 1200), (720_000, 20, 1200), (720_000, 5, 1200),
                (224_000, 16, 1201), (44_800_000, 8, 12), (360_000, 10, 1200), (112_000, 40, 1200),
                (112_000, 32, 1200), (54_400, 66, 1200), (8_600_000, 63, 8), (8_600_000, 64, 8),
                (2_200_000, 255, 8), (2_200_000, 256, 8)]


def _drawn_shapes(n=300):
    rng = np.random.default_rng(0xB16B0FF)
    out = list(CASE_BUFFERS)
    for _ in range(n):
        rows, P = int(rng.integers(1, 257)), int(rng.integers(1, 4097))
        per = rows * P
        # from less than one group past nothing to a few lines: G * per in (0, 5 * 2^32)
        total = int(rng.integers(1, 5 * bb.LINE))
        out.append((max(1, total // per), rows, P))
    # buffers that end exactly at, one byte before and one group past a line
    out += [(bb.LINE // 4096, 1, 4096), (bb.LINE // 4096 + 1, 1, 4096), (bb.LINE // 4096 - 1, 1, 4096), (1, 1, 1),
            (3, 7, 5), (2 * bb.LINE // 65536 + 1, 16, 4096)]
    return out


@pytest.mark.parametrize("halo", [0, 1, 2, 5])
def test_boundary_groups_hold_every_line(halo):
    for G, rows, P in _drawn_shapes():
        per = rows * P
        got = bb.boundary_groups(G, rows, P, halo)
        assert got, (G, rows, P)
        assert got == sorted(set(got)) and got[0] == 0 and (got[-1] == G - 1 or halo == 0)
        assert all(0 <= g < G for g in got)
        held = set(got)
        assert set(range(min(G, halo + 1))) <= held and set(range(max(0, G - halo), G)) <= held
        lines = list(range(bb.LINE, G * per, bb.LINE))
        assert len(lines) == (G * per - 1) // bb.LINE
        for line in lines:
            for byte in (line - 1, line):
                g = byte // per
                assert g * per <= byte < (g + 1) * per and g in held, (G, rows, P, line)
                assert set(range(max(0, g - halo), min(G, g + halo + 1))) <= held
        # no more than the ends and a window per line
        assert len(got) <= 2 * halo + 1 + len(lines) * (2 * halo + 2)


def test_boundary_groups_of_the_cases_cross():
    for G, rows, P in CASE_BUFFERS:
        assert bb.crosses(G * rows * P), (G, rows, P)
        # at least 150 groups past the first line
        assert G - bb.LINE // (rows * P) - 1 >= 150, (G, rows, P)
        assert len(bb.boundary_groups(G, rows, P)) > 5


def test_boundary_groups_small_buffer_is_its_ends():
    assert bb.boundary_groups(100, 3, 1200) == [0, 1, 2, 98, 99]
    assert bb.boundary_groups(1, 3, 1200) == [0]
    assert bb.boundary_groups(4, 3, 1200, halo=2) == [0, 1, 2, 3]


@pytest.mark.parametrize("limit", [2**31 - 2**20, 2**20, 4097])
def test_pieces_cover_once_below_the_limit(limit):
    for G, rows, P in _drawn_shapes(100):
        per = rows * P
        if per >= limit:
            with pytest.raises(ValueError):
                bb.pieces(G, per, limit)
            continue
        if G // max(1, (limit - 1) // per) > 200_000:
            continue
        got = bb.pieces(G, per, limit)
        assert got[0][0] == 0 and got[-1][1] == G
        for (a0, a1), (b0, b1) in zip(got, got[1:]):
            assert a1 == b0                                    # no gap, no overlap
        for g0, g1 in got:
            assert g0 < g1 and (g1 - g0) * per < limit
        assert sum(g1 - g0 for g0, g1 in got) == G


def test_pieces_default_limit_keeps_offsets_below_2_31():
    for G, rows, P in CASE_BUFFERS:
        for g0, g1 in bb.pieces(G, rows * P):
            assert (g1 - g0) * rows * P < 2**31 - 2**20


def test_special_every_is_the_smallest_prime_that_still_crosses():
    for G, rows, P in [(1_200_000, 3, 1200), (720_000, 5, 1200), (224_000, 16, 1201), (112_000, 32, 1200),
                       (3_590_000, 1, 1200), (bb.LINE // 64 + 20_000, 1, 64)]:
        S = bb.special_every(G, rows, P)
        special = bb.special_groups(G, S)
        assert bb._is_prime(S) and len(special) == G // S and len(special) >= 1
        assert 0 not in special and (np.diff(special) == S).all()
        assert (G - len(special)) * rows * P > bb.LINE + bb.MARGIN
        for T in range(2, S):
            if bb._is_prime(T):
                assert (G - G // T) * rows * P <= bb.LINE + bb.MARGIN, (G, rows, P, T)
    assert [n for n in range(30) if bb._is_prime(n)] == [2, 3, 5, 7, 11, 13, 17, 19, 23, 29]


def test_special_every_raises_when_nothing_crosses():
    with pytest.raises(ValueError):
        bb.special_every(1000, 3, 1200)
    # G groups cross, G - 1 do not: no room for a special group
    per = 3 * 1200
    G = (bb.LINE + bb.MARGIN) // per + 1
    assert bb.crosses(G * per) and not bb.crosses((G - 1) * per)
    with pytest.raises(ValueError):
        bb.special_every(G, 3, 1200)
    assert bb.special_every(G + 1, 3, 1200) > G // 2            # one special group at the most


class _HostFill:
    """fill_random_dev of a context, on host tensors, from the oracle's generator."""

    def __init__(self, oracle):
        self.oracle, self.calls = oracle, []

    def fill_random_dev(self, dst, nbytes, seed, byte_offset=0, stream=None):
        self.calls.append((nbytes, byte_offset))
        dst.numpy()[:nbytes] = self.oracle.splitmix_bytes(nbytes, seed, byte_offset)

    def synchronize(self):
        pass


def test_same_as_stream_finds_the_first_difference(oracle_mod, monkeypatch):
    import torch
    monkeypatch.setattr(bb, "SLAB", 1000)
    n, seed = 3517, 0xF00D
    ctx = _HostFill(oracle_mod)
    buf = torch.from_numpy(oracle_mod.splitmix_bytes(n, seed))
    assert bb.same_as_stream(ctx, torch, buf, seed) is None
    assert ctx.calls == [(1000, 0), (1000, 1000), (1000, 2000), (517, 3000)]
    for at in (0, 999, 1000, 2500, n - 1):
        bad = buf.clone()
        bad[at] ^= 0x40
        bad[n - 1] ^= 0x01 if at != n - 1 else 0
        assert bb.same_as_stream(ctx, torch, bad, seed) == at
