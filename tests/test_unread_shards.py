"""The helper the decode cases take their inputs from (tests/unread_shards.py), and the oracle under
those inputs.  No GPU.

fec_mask.hpp: "the survivors a rebuild reads are the surviving data shards ascending, then the e
lowest surviving parity rows"; include/fec_hip.h: "a lost shard's entry, and a parity row the rule
does not use, is never read".  The GPU tests hold the library to the oracle on inputs with junk in
every such shard; here the oracle itself is held to the original data on them, `roles` to a plain
loop, and a deliberately wrong decoder shows what true bytes in lost rows let through.
"""
import numpy as np
import pytest

import unread_shards as us
from test_code_definition import cauchy_parity, gf_mul, solve

EXHAUSTIVE = [(4, 2), (10, 1), (10, 2), (10, 3), (5, 5)]
DRAWN = [(20, 5), (7, 4), (12, 12), (16, 16), (32, 32), (60, 4)]


def all_masks(k, r):
    return np.arange(1 << (k + r), dtype=np.uint64)


def drawn_masks(k, r, n, seed):
    """n masks: 0..r+1 lost shards anywhere (unrecoverable and lost-parity groups included), plus
    loss by a coin per shard for a third of them, and junk in the bits at and above k + r."""
    rng = np.random.default_rng(seed)
    masks = np.zeros(n, dtype=np.uint64)
    for g in range(n):
        if g % 3 == 2:
            lost = np.flatnonzero(rng.random(k + r) < rng.choice([0.05, 0.2, 0.5]))
        else:
            lost = rng.permutation(k + r)[: rng.integers(0, r + 2)]
        m = sum(1 << int(s) for s in lost)
        if k + r < 64:
            m |= int(rng.integers(0, 1 << (64 - k - r), dtype=np.uint64)) << (k + r)
        masks[g] = m
    return masks


# ---- roles against a plain loop -------------------------------------------------------------------
@pytest.mark.parametrize("k,r", [(4, 2), (10, 3), (5, 5)])
def test_roles_equal_the_restated_rule(k, r):
    """Every mask, with junk above k + r on a second pass: lost shards from the bits, the chosen rows
    the first e surviving ones (the parity part of alive[:k], as test_code_definition.py walks it)."""
    base = all_masks(k, r)
    for masks in (base, base | (np.uint64(0xA5A5A5A5A5A5A5A5) << np.uint64(k + r))):
        ro = us.roles(masks, k, r)
        assert ro.lost_d.shape == (len(masks), k) and ro.chosen.shape == ro.lost_p.shape == ro.unread_p.shape == (len(masks), r)
        for g, m in enumerate(int(x) for x in masks):
            lost = [s for s in range(k + r) if m >> s & 1]
            alive = [s for s in range(k + r) if s not in lost]
            e = sum(1 for s in lost if s < k)
            alive_rows = [s - k for s in alive if s >= k]
            ok = e <= len(alive_rows)
            chosen = alive_rows[:e] if ok else []
            if ok:
                assert [s - k for s in alive[:k] if s >= k] == chosen           # "any k survivors", lowest first
            assert np.flatnonzero(ro.lost_d[g]).tolist() == [s for s in lost if s < k]
            assert np.flatnonzero(ro.lost_p[g]).tolist() == [s - k for s in lost if s >= k]
            assert bool(ro.ok[g]) == ok
            assert np.flatnonzero(ro.chosen[g]).tolist() == chosen, (hex(m), chosen)
            assert np.flatnonzero(ro.unread_p[g]).tolist() == [i for i in range(r) if i not in chosen]


def test_inputs_junk_exactly_the_unread_shards(oracle_mod):
    k, r, P = 10, 3, 48
    masks = all_masks(k, r)
    G = len(masks)
    data = oracle_mod.splitmix_bytes(G * k * P, 11)
    par = oracle_mod.rs_encode(data, G, k, r, P, nthreads=8)
    d_in, p_in = us.inputs(data, par, masks, k, r, P, seed=5)
    ro = us.roles(masks, k, r)
    assert np.array_equal((d_in != data).reshape(G, k, P).any(axis=2), ro.lost_d)
    assert np.array_equal((p_in != par).reshape(G, r, P).any(axis=2), ro.unread_p)
    again = us.inputs(data, par, masks, k, r, P, seed=5)
    assert np.array_equal(again[0], d_in) and np.array_equal(again[1], p_in)      # seeded
    assert not np.array_equal(us.inputs(data, par, masks, k, r, P, seed=6)[1], p_in)
    # per-byte junk, not a constant fill
    assert len(np.unique(p_in.reshape(G, r, P)[ro.unread_p][0])) > P // 2
    # a case without the groups that make it say something is refused
    with pytest.raises(AssertionError):
        us.inputs(data[:k * P], par[:r * P], np.array([0b11], dtype=np.uint64), k, r, P, seed=1)
    with pytest.raises(AssertionError):     # two lost, rows 0 and 2 chosen, row 1 lost: no unchosen surviving row
        us.inputs(data[:k * P], par[:r * P], np.array([0b11 | 2 << k], dtype=np.uint64), k, r, P, seed=1)
    us.inputs(data[:k * P], par[:r * P], np.array([0b11 | 2 << k], dtype=np.uint64), k, r, P, seed=1, need_unchosen_alive=False)


# ---- the oracle under the helper's inputs ---------------------------------------------------------
def check_oracle(oracle, k, r, P, masks, seed):
    G = len(masks)
    data = oracle.splitmix_bytes(G * k * P, 0x5EED9000 + seed)
    par = oracle.rs_encode(data, G, k, r, P, nthreads=8)
    d_in, p_in = us.inputs(data, par, masks, k, r, P, seed, need_lost_below=r > 1, need_unchosen_alive=True)
    ro = us.roles(masks, k, r)
    for decode in (oracle.rs_decode, oracle.rs_decode_fast):
        out, p = d_in.copy(), p_in.copy()
        bad, st = decode(out, p, masks, G, k, r, P, nthreads=8)
        assert np.array_equal(p, p_in)
        assert np.array_equal(st != 0, ~ro.ok) and np.array_equal(st[~ro.ok], np.ones(int((~ro.ok).sum()), dtype=st.dtype))
        assert bad == int((~ro.ok).sum())
        got, want = out.reshape(G, k, P), np.where(ro.ok[:, None, None], data.reshape(G, k, P), d_in.reshape(G, k, P))
        wrong = (got != want).any(axis=(1, 2))
        assert not wrong.any(), (decode.__name__, us.describe(ro, masks, k, r, wrong))


@pytest.mark.parametrize("k,r", EXHAUSTIVE)
def test_oracle_reads_no_unread_shard_every_mask(oracle_mod, k, r):
    """Every mask at 48 B: rs_decode and rs_decode_fast give the original data where the group is
    recoverable, leave every other group as it came (junk included), and report status 1 exactly
    for the unrecoverable ones."""
    check_oracle(oracle_mod, k, r, 48, all_masks(k, r), k * 10 + r)


@pytest.mark.parametrize("k,r", DRAWN)
def test_oracle_reads_no_unread_shard_drawn_masks(oracle_mod, k, r):
    """3000 drawn masks at 32 B with junk in the bits at and above k + r."""
    check_oracle(oracle_mod, k, r, 32, drawn_masks(k, r, 3000, k * 100 + r), k * 10 + r)


# ---- the definition's own decode, and a wrong one -------------------------------------------------
def gauss_decode(C, k, shards_d, shards_p, lost_d, rows):
    """The data rebuilt by Gauss-Jordan over the generator rows of the surviving data shards and of
    parity rows `rows`."""
    gen = [[int(i == j) for j in range(k)] for i in range(k)] + C
    take = [j for j in range(k) if j not in lost_d] + [k + i for i in rows]
    shards = shards_d + shards_p
    return solve([gen[s] for s in take], [shards[s] for s in take])


def _small_case(oracle, k, r, P, seed):
    data = oracle.splitmix_bytes(k * P, 0x5EED7100 + seed)
    C = cauchy_parity(k, r)
    d = data.reshape(k, P).tolist()
    par = [[0] * P for _ in range(r)]
    for i in range(r):
        for j in range(k):
            for b in range(P):
                par[i][b] ^= gf_mul(C[i][j], d[j][b])
    return C, data, d, par


def _small_masks(k, r, seed):
    if k + r <= 6:
        return all_masks(k, r)
    return drawn_masks(k, r, 24, seed) & np.uint64((1 << (k + r)) - 1)


@pytest.mark.parametrize("k,r,P,seed", [(10, 3, 24, 1), (4, 2, 16, 2), (20, 5, 8, 3), (6, 4, 5, 4)])
def test_definition_decode_on_junked_shards(oracle_mod, k, r, P, seed):
    """Gauss-Jordan over the rows the rule names rebuilds the data from the junked shards, and the
    oracle returns the same bytes."""
    C, data, d, par = _small_case(oracle_mod, k, r, P, seed)
    masks = _small_masks(k, r, seed)
    G = len(masks)
    par_flat = np.array(par, dtype=np.uint8).reshape(-1)
    d_in, p_in = us.inputs(np.tile(data, G), np.tile(par_flat, G), masks, k, r, P, seed)
    ro = us.roles(masks, k, r)
    out = d_in.copy()
    _, st = oracle_mod.rs_decode(out, p_in, masks, G, k, r, P)
    assert ro.ok.any() and ro.lost_p[ro.ok].any()
    for g in np.flatnonzero(ro.ok):
        lost_d, rows = np.flatnonzero(ro.lost_d[g]).tolist(), np.flatnonzero(ro.chosen[g]).tolist()
        X = gauss_decode(C, k, d_in.reshape(G, k, P)[g].tolist(), p_in.reshape(G, r, P)[g].tolist(), lost_d, rows)
        assert X == d, hex(int(masks[g]))
        assert st[g] == 0 and np.array_equal(out.reshape(G, k, P)[g], data.reshape(k, P))


def test_control_wrong_pick_passes_true_parity_and_fails_junk(oracle_mod):
    """A decoder that takes the lowest e rows whether lost or not, with the matching matrix: exact
    on every recoverable mask while lost rows hold true parity (what the decode cases used to
    hand over), wrong on the helper's inputs exactly where one of its rows is lost."""
    k, r, P, seed = 4, 2, 16, 2
    C, data, d, par = _small_case(oracle_mod, k, r, P, seed)
    masks = all_masks(k, r)
    G = len(masks)
    par_flat = np.array(par, dtype=np.uint8).reshape(-1)
    ro = us.roles(masks, k, r)
    # the old inputs: a constant in lost data shards, true parity everywhere
    old_d = np.tile(data, G).reshape(G, k, P)
    old_d[ro.lost_d] = 0xEE
    d_in, p_in = us.inputs(np.tile(data, G), np.tile(par_flat, G), masks, k, r, P, seed)
    caught = 0
    for g in np.flatnonzero(ro.ok & ro.lost_d.any(axis=1)):
        lost_d = np.flatnonzero(ro.lost_d[g]).tolist()
        wrong_rows = list(range(len(lost_d)))
        assert gauss_decode(C, k, old_d[g].tolist(), par, lost_d, wrong_rows) == d            # passes the old case
        X = gauss_decode(C, k, d_in.reshape(G, k, P)[g].tolist(), p_in.reshape(G, r, P)[g].tolist(), lost_d, wrong_rows)
        reads_lost_row = bool(ro.lost_p[g][wrong_rows].any())
        assert (X != d) == reads_lost_row, hex(int(masks[g]))
        caught += X != d
    assert caught == 4          # one lost data shard (4 ways) with row 0 lost and row 1 alive
