"""The helper the decode cases take their inputs from (tests/unread_shards.py), and the oracle under
those inputs.  No GPU.

fec_mask.hpp: "the survivors a rebuild reads are the surviving data shards ascending, then the e
lowest surviving parity rows"; include/fec_hip.h: "a lost shard's entry, and a parity row the rule
does not use, is never read".  The GPU tests hold the library to the oracle on inputs with junk in
every such shard; here the oracle itself is held to the original data on them, `roles` to a plain
loop, and a deliberately wrong decoder shows what true bytes in lost rows let through.

fec_mask.hpp again: "Bits at and above k + r are ignored."  The GPU tests hand over masks with junk
up there (`high_bits`); here the helper's promises are checked, the oracle is held to say the same
with and without the junk, and four deliberately wrong readers of the rule show that clean masks
let each of them through and the helper's masks do not.
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


# ---- junk in the mask bits at and above k + r ------------------------------------------------------
def _every_high(k, r):
    return np.uint64(((1 << (64 - k - r)) - 1) << (k + r))


def test_high_bits_keeps_the_rule_and_plants_its_groups():
    k, r = 10, 3
    masks = all_masks(k, r)
    np.random.default_rng(3).shuffle(masks)
    out = us.high_bits(masks, k, r, seed=5)
    low = np.uint64((1 << (k + r)) - 1)
    assert out.dtype == np.uint64 and out is not masks and np.array_equal(out & low, masks)
    assert np.array_equal(us.high_bits(masks, k, r, seed=5), out)                  # seeded
    assert not np.array_equal(us.high_bits(masks, k, r, seed=6), out)
    assert np.array_equal(us.high_bits(out, k, r, seed=5), out)                    # junk that comes in is replaced
    high = out & ~low
    every = _every_high(k, r)
    share = lambda sel: float(sel.mean())
    assert 0.2 < share(high == 0) < 0.3 and 0.2 < share(high == every) < 0.3       # a quarter clean, a quarter all set
    assert len(np.unique(high)) > len(masks) // 3                                  # the rest drawn per group
    ro, pl = us.roles(masks, k, r), us.planted(masks, k, r, seed=5)
    assert tuple(pl) == us.PLANTED and len({g for g, _ in pl.values()}) == len(us.PLANTED)     # six distinct groups
    want = {"full_first": 1 << (k + r), "full_all": int(every), "full_top": 1 << 63,
            "short_all_but_first": int(every) & ~(1 << (k + r)), "short_clean": 0, "untouched_all": int(every)}
    for name, (g, pat) in pl.items():
        assert pat == want[name] and int(high[g]) == pat, name
        kind = us.full_groups if name.startswith("full") else us.short_groups if name.startswith("short") else us.untouched_groups
        assert kind(ro)[g], name
    e, alive = ro.lost_d.sum(axis=1), (~ro.lost_p).sum(axis=1)
    for name in us.PLANTED[:3]:
        g = pl[name][0]
        assert ro.ok[g] and e[g] >= 1 and e[g] == alive[g]
    for name in us.PLANTED[3:5]:
        g = pl[name][0]
        assert not ro.ok[g] and e[g] == alive[g] + 1
    assert masks[pl["untouched_all"][0]] == 0
    # k + r = 64: no such bit, a copy, and no condition is checked
    one = np.array([1], dtype=np.uint64)
    same = us.high_bits(one, 60, 4, seed=1)
    assert np.array_equal(same, one) and same is not one
    # a case without the groups is refused unless the caller says it has none
    lost_two = np.array([0b11] * 8, dtype=np.uint64)                               # e = 2, three rows alive
    for need in ({}, dict(need_full=False), dict(need_full=False, need_short=False)):
        with pytest.raises(AssertionError):
            us.high_bits(lost_two, k, r, seed=1, **need)
    got = us.high_bits(lost_two, k, r, seed=1, need_full=False, need_short=False, need_untouched=False)
    assert np.array_equal(got & low, lost_two)
    two_full = np.array([0b111, 0b111, 0], dtype=np.uint64)                        # three are planted, not two
    with pytest.raises(AssertionError):
        us.high_bits(two_full, k, r, seed=1, need_short=False)
    us.high_bits(two_full, k, r, seed=1, need_full=False, need_short=False)


def check_oracle_ignores(oracle, k, r, P, masks, masks_in, seed):
    """rs_decode and rs_decode_fast: byte-identical data, statuses and counts for masks_in and masks."""
    G = len(masks)
    low = np.uint64((1 << (k + r)) - 1)
    assert np.array_equal(masks_in & low, masks) and (masks_in != masks).any()
    data = oracle.splitmix_bytes(G * k * P, 0x5EED9100 + seed)
    par = oracle.rs_encode(data, G, k, r, P, nthreads=8)
    d_in, p_in = us.inputs(data, par, masks, k, r, P, seed, need_lost_below=r > 1)
    for decode in (oracle.rs_decode, oracle.rs_decode_fast):
        got = []
        for m in (masks, masks_in):
            out, p, m = d_in.copy(), p_in.copy(), m.copy()
            bad, st = decode(out, p, m, G, k, r, P, nthreads=8)
            got.append((out, st, bad, p))
        (o0, s0, b0, p0), (o1, s1, b1, p1) = got
        assert b0 == b1 and np.array_equal(s0, s1), (decode.__name__, us.mismatch(masks, k, r, s1, s0))
        assert np.array_equal(o0, o1), (decode.__name__, us.mismatch(masks, k, r, o1, o0))
        assert np.array_equal(p0, p_in) and np.array_equal(p1, p_in)


def junk_patterns(masks, k, r, seed):
    """The three patterns of the GPU every-mask passes: only bit k + r, every high bit, the helper's draw."""
    return {"first": masks | np.uint64(1 << (k + r)), "every": masks | _every_high(k, r),
            "drawn": us.high_bits(masks, k, r, seed)}


@pytest.mark.parametrize("pattern", ["first", "every", "drawn"])
@pytest.mark.parametrize("k,r", EXHAUSTIVE)
def test_oracle_ignores_high_bits_every_mask(oracle_mod, k, r, pattern):
    """Every mask at 48 B with junk at and above k + r: the oracle says what it says without it."""
    masks = all_masks(k, r)
    check_oracle_ignores(oracle_mod, k, r, 48, masks, junk_patterns(masks, k, r, k * 10 + r)[pattern], k * 10 + r)


@pytest.mark.parametrize("pattern", ["first", "every", "drawn"])
@pytest.mark.parametrize("k,r", [s for s in DRAWN if sum(s) < 64])
def test_oracle_ignores_high_bits_drawn_masks(oracle_mod, k, r, pattern):
    """3000 drawn masks at 32 B, the shapes with a bit to spare."""
    masks = drawn_masks(k, r, 3000, k * 100 + r) & np.uint64((1 << (k + r)) - 1)
    check_oracle_ignores(oracle_mod, k, r, 32, masks, junk_patterns(masks, k, r, k * 10 + r)[pattern], k * 10 + r)


# ---- four wrong readers of "bits at and above k + r are ignored" ----------------------------------
def _pop(x):
    return bin(x).count("1")


def wrong_reader(kind, m, k, r):
    """(ok, chosen rows, untouched) of mask m as one wrong restatement of the rule reads it, written
    like the kernels' hand-written copy (fec_decode_fused.hip fused_group): e = popc(m & kmask),
    pm = (m >> k) & rmask, bad = e > r - popc(pm), rows = the e lowest bits of ~pm & rmask.
      lost_unmasked  pm without `& rmask` in the count: junk bits count as lost rows
      wide           rmask one bit too wide in the count: bit k + r counts as a lost row
      alive_unmasked both `& rmask` gone and the kernel's own uint32 arithmetic: enough junk wraps
                     r - popc(pm), the group is accepted, and a clear bit k + r is 'surviving row r'
      zero           'nothing lost' judged from m == 0"""
    kmask, rmask, u64 = (1 << k) - 1, (1 << r) - 1, (1 << 64) - 1
    e = _pop(m & kmask)
    pm, alive = (m >> k) & rmask, ~(m >> k) & rmask
    if kind == "lost_unmasked":
        ok = e <= r - _pop(m >> k)
    elif kind == "wide":
        ok = e <= r - _pop((m >> k) & ((1 << (r + 1)) - 1))
    elif kind == "alive_unmasked":
        ok = e <= (r - _pop(m >> k)) % (1 << 32)
        alive = ~(m >> k) & u64
    else:
        ok = e <= r - _pop(pm)
    rows = []
    if ok and e >= 1:
        for _ in range(e):
            rows.append((alive & -alive).bit_length() - 1)
            alive &= alive - 1
    untouched = m == 0 if kind == "zero" else (m & ((1 << (k + r)) - 1)) == 0
    return ok, tuple(rows), untouched


# the planted group each wrong reader trips on
TRIPS_ON = {"lost_unmasked": "full_top", "wide": "full_first", "alive_unmasked": "short_all_but_first", "zero": "untouched_all"}


def disagreements(kind, masks, k, r):
    """Groups where the reader and `roles` differ in status, chosen rows or 'nothing lost'."""
    ro = us.roles(masks, k, r)
    untouched = us.untouched_groups(ro)
    out = []
    for g, m in enumerate(int(x) for x in masks):
        truth = (bool(ro.ok[g]), tuple(np.flatnonzero(ro.chosen[g]).tolist()), bool(untouched[g]))
        if wrong_reader(kind, m, k, r) != truth:
            out.append(g)
    return out


def check_readers_trip(masks, k, r, seed):
    masks_in = us.high_bits(masks, k, r, seed)
    pl = us.planted(masks, k, r, seed)
    for kind, name in TRIPS_ON.items():
        wrong = disagreements(kind, masks_in, k, r)
        assert pl[name][0] in wrong, (kind, name, k, r)
    # what each planted pattern does to its reader
    g = pl["full_top"][0]
    assert wrong_reader("lost_unmasked", int(masks_in[g]), k, r)[0] is False          # a good group refused
    assert wrong_reader("wide", int(masks_in[g]), k, r)[0] is True                    # bit 63 is outside the wide mask
    assert wrong_reader("wide", int(masks_in[pl["full_first"][0]]), k, r)[0] is False
    assert wrong_reader("lost_unmasked", int(masks_in[pl["full_all"][0]]), k, r)[0] is False
    g = pl["short_all_but_first"][0]
    ok, rows, _ = wrong_reader("alive_unmasked", int(masks_in[g]), k, r)
    assert ok and rows[-1] == r                                                       # rebuilt from past the parity rows
    for kind in TRIPS_ON:                                                             # the clean short group: refused by all
        assert wrong_reader(kind, int(masks_in[pl["short_clean"][0]]), k, r)[0] is False
    assert wrong_reader("zero", int(masks_in[pl["untouched_all"][0]]), k, r)[2] is False
    return masks_in


@pytest.mark.parametrize("k,r", [(4, 2), (10, 3)])
def test_control_wrong_readers_pass_clean_masks_and_fail_junk(k, r):
    """Each wrong reader agrees with `roles` on every clean mask -- what the GPU every-mask pass used
    to hand over -- and disagrees on the helper's masks, on the group planted for it.  (With only the
    guard of the row pick gone and the status right, a reader is the rule: the pick of a recoverable
    group never leaves the r rows.  That guard shows only together with a wrong status.)"""
    masks = all_masks(k, r)
    for kind in TRIPS_ON:
        assert disagreements(kind, masks, k, r) == [], kind
    masks_in = check_readers_trip(masks, k, r, seed=k * 10 + r)
    ro, rmask = us.roles(masks_in, k, r), (1 << r) - 1
    for g in np.flatnonzero(ro.ok & ro.lost_d.any(axis=1)):                           # the pick alone, unmasked: the same rows
        alive, rows = ~(int(masks_in[g]) >> k) & ((1 << 64) - 1), []
        for _ in range(int(ro.lost_d[g].sum())):
            rows.append((alive & -alive).bit_length() - 1)
            alive &= alive - 1
        assert rows == np.flatnonzero(ro.chosen[g]).tolist() and max(rows) < r and (1 << max(rows)) & rmask


def test_control_wrong_readers_fail_the_gpu_cases_masks():
    """The same on the masks the GPU decode matrix hands over: perm_masks of the five shapes at their
    real group counts and seeds (both ends of the size list and 1024 B), through the helper as Case
    applies it."""
    import test_gpu_forms as forms
    for k, r in forms.DECODE_SHAPES:
        G = 261 if (k, r) == (20, 5) else 1031
        for P in (forms.DECODE_P[0], 1024, forms.DECODE_P[-1]):
            masks = forms.perm_masks(k, r, G, k * 1000 + r * 100 + P)
            for kind in TRIPS_ON:
                assert disagreements(kind, masks, k, r) == [], (kind, k, r, P)
            masks_in = check_readers_trip(masks, k, r, forms.SEED + k * 31 + r * 7 + P)
            # many groups, not only the planted ones
            assert len(disagreements("lost_unmasked", masks_in, k, r)) > G // 20


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
