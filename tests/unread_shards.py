"""Decode inputs with junk in every shard the erasure rule does not read.

The rule (quic-test_amd/csrc/fec_mask.hpp, include/fec_hip.h): a rebuild reads the surviving data
shards and the e lowest surviving parity rows; a lost shard's entry, and a parity row the rule
does not use, is never read.  A case that leaves true bytes in those shards cannot see a decoder
that picks its rows wrongly but consistently, so the decode cases of the suite take their inputs
from here: seeded per-byte random junk in every lost data shard and in every parity row that is
not chosen (lost rows, surviving rows past the e-th, every row of a group that rebuilds nothing).

`roles` is written in numpy from the sentences of fec_mask.hpp; it calls neither the library nor
the oracle.  A plain module like forms_support.py: no fixtures, no tests.
"""
import numpy as np

_SALT = 0x0BADF00D5EED


class Roles:
    """Boolean arrays per group: lost_d (G,k), lost_p (G,r), chosen (G,r), unread_p (G,r), ok (G,)."""

    def __init__(self, lost_d, lost_p, chosen, unread_p, ok):
        self.lost_d, self.lost_p, self.chosen, self.unread_p, self.ok = lost_d, lost_p, chosen, unread_p, ok


def roles(masks, k, r):
    """Who is lost, chosen and unread in each group.  Bit j < k: data shard j is lost; bit k + i:
    parity row i is lost; bits at and above k + r are ignored.  ok: the e lost data shards find e
    surviving rows.  chosen: the e lowest surviving rows of an ok group with e >= 1, else none.
    unread_p: every parity row that is not chosen."""
    m = np.asarray(masks, dtype=np.uint64).reshape(-1)
    bits = ((m[:, None] >> np.arange(k + r, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    lost_d, lost_p = bits[:, :k], bits[:, k:k + r]
    e = lost_d.sum(axis=1)
    alive = ~lost_p
    ok = e <= alive.sum(axis=1)
    nth_alive = np.cumsum(alive, axis=1)                     # 1-based rank of a surviving row
    chosen = alive & (nth_alive <= e[:, None]) & ok[:, None]
    return Roles(lost_d, lost_p, chosen, ~chosen, ok)


def junk(nbytes, seed):
    """nbytes per-byte random bytes, a stream of its own (never the case's data stream)."""
    return np.random.default_rng([_SALT, int(seed) & 0xFFFFFFFFFFFFFFFF]).integers(0, 256, size=int(nbytes), dtype=np.uint8)


def has_lost_row_below_chosen(ro):
    """Groups with a lost parity row below their highest chosen row: the pick is not 'the lowest e
    rows'."""
    r = ro.chosen.shape[1]
    top = np.where(ro.chosen.any(axis=1), r - 1 - np.argmax(ro.chosen[:, ::-1], axis=1), -1)
    return (ro.lost_p & (np.arange(r)[None, :] < top[:, None])).any(axis=1)


def has_unchosen_alive_row(ro):
    """Groups with a surviving parity row the rule does not use."""
    return (~ro.lost_p & ~ro.chosen).any(axis=1)


def inputs(data, par, masks, k, r, P, seed, need_lost_below=True, need_unchosen_alive=True):
    """(data_in, par_in) of a decode case: flat copies of the true data and parity with junk in
    every lost data shard and every row of unread_p; everything else is true.  Every junked shard
    differs from the true one.  The case must hold a group with a lost parity row below its
    highest chosen row, and one with an unchosen surviving row, unless the caller says it has none
    (need_* = False: r = 1 for the first, or a case built without one)."""
    G = len(masks)
    ro = roles(masks, k, r)
    d_true = np.asarray(data, dtype=np.uint8).reshape(G, k, P)
    p_true = np.asarray(par, dtype=np.uint8).reshape(G, r, P)
    d_in, p_in = d_true.copy(), p_true.copy()
    for true, out, where, s in ((d_true, d_in, ro.lost_d, int(seed)), (p_true, p_in, ro.unread_p, int(seed) ^ 0x9E3779B97F4A7C15)):
        j = junk(int(where.sum()) * P, s).reshape(-1, P)
        j[(j == true[where]).all(axis=1)] ^= 0xFF             # P is tiny and the draw hit the truth
        out[where] = j
    assert (d_in != d_true).any(axis=2)[ro.lost_d].all() and (p_in != p_true).any(axis=2)[ro.unread_p].all()
    assert np.array_equal(d_in[~ro.lost_d], d_true[~ro.lost_d]) and np.array_equal(p_in[ro.chosen], p_true[ro.chosen])
    if need_lost_below:
        assert has_lost_row_below_chosen(ro).any(), "no group with a lost parity row below its highest chosen row"
    if need_unchosen_alive:
        assert has_unchosen_alive_row(ro).any(), "no group with a surviving parity row the rule does not use"
    return d_in.reshape(-1), p_in.reshape(-1)


def describe(ro, masks, k, r, wrong):
    """For an assertion message: the first group in `wrong` (bool per group), its mask and roles."""
    g = int(np.flatnonzero(wrong)[0])
    return (f"group {g} mask {int(masks[g]):#x} lost data {np.flatnonzero(ro.lost_d[g]).tolist()} "
            f"lost rows {np.flatnonzero(ro.lost_p[g]).tolist()} chosen {np.flatnonzero(ro.chosen[g]).tolist()} "
            f"ok {bool(ro.ok[g])} ({int(wrong.sum())} groups differ)")


def mismatch(masks, k, r, got, want):
    """For an assertion message: where two per-group arrays (anything that reshapes to (G, ...))
    differ, by the roles of the first such group."""
    G = len(masks)
    wrong = (np.asarray(got).reshape(G, -1) != np.asarray(want).reshape(G, -1)).any(axis=1)
    return describe(roles(masks, k, r), masks, k, r, wrong) if wrong.any() else "equal"
