"""The erasure rule for four-word masks (k + r <= 256), restated in numpy for the tests of the wide
calls, as unread_shards.py restates it for one word.

The rule (include/fec_hip.h, quic-test_amd/csrc/fec_mask_wide.hpp): a group's mask is four u64, shard
s at bit s & 63 of word s >> 6; bit j < k: data shard j is lost; bit k + i: parity row i is lost;
bits at and above k + r are ignored, in the partial word and in the whole words above it; e lost
data shards need e surviving parity rows; the survivors are the surviving data shards and the e
lowest surviving rows.

`roles` calls neither the library nor the oracle and returns unread_shards.Roles.  A plain module:
no fixtures, no tests.
"""
import numpy as np

import unread_shards as us

WORDS = 4


def to_bits(masks):
    """(G, 4) u64 -> (G, 256) bool, shard s in column s."""
    m = np.ascontiguousarray(masks, dtype=np.uint64).reshape(-1, WORDS)
    return ((m[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool).reshape(len(m), 256)


def from_bits(bits):
    """(G, 256) bool -> (G, 4) u64."""
    b = np.asarray(bits, dtype=bool).reshape(-1, WORDS, 64)
    return (b.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, None, :]).sum(axis=2, dtype=np.uint64)


def roles(masks, k, r):
    """unread_shards.roles for (G, 4) masks: lost_d (G,k), lost_p (G,r), chosen (G,r), unread_p (G,r),
    ok (G,)."""
    bits = to_bits(masks)
    lost_d, lost_p = bits[:, :k], bits[:, k:k + r]
    e = lost_d.sum(axis=1)
    alive = ~lost_p
    ok = e <= alive.sum(axis=1)
    chosen = alive & (np.cumsum(alive, axis=1) <= e[:, None]) & ok[:, None]
    return us.Roles(lost_d, lost_p, chosen, ~chosen, ok)


def status(ro):
    return (~ro.ok).astype(np.uint8)


def with_high_junk(masks, k, r, seed):
    """The masks with junk in what the rule ignores: seeded random bits in the partial word above
    k + r (a quarter of the groups every such bit, a quarter none), all ones in every whole word
    above it.  Bits below k + r as given."""
    bits = to_bits(masks)
    G = len(bits)
    top = min(256, -(-(k + r) // 64) * 64)                   # end of the partial word
    rng = np.random.default_rng([0x41B176, int(seed) & 0xFFFFFFFFFFFFFFFF])
    if top > k + r:
        junk = rng.random((G, top - k - r)) < 0.5
        coin = rng.random(G)
        junk[coin < 0.25] = False
        junk[(coin >= 0.25) & (coin < 0.5)] = True
        bits[:, k + r:top] = junk
    bits[:, top:] = True
    out = from_bits(bits)
    a, b = roles(masks, k, r), roles(out, k, r)
    assert all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("lost_d", "lost_p", "chosen", "ok"))
    return out


def inputs(data, par, ro, P, seed):
    """unread_shards.inputs for given roles: flat copies of the true data and parity with seeded junk
    in every lost data shard and every parity row the rule does not read."""
    G, k = ro.lost_d.shape
    r = ro.lost_p.shape[1]
    d_true = np.asarray(data, dtype=np.uint8).reshape(G, k, P)
    p_true = np.asarray(par, dtype=np.uint8).reshape(G, r, P)
    d_in, p_in = d_true.copy(), p_true.copy()
    for true, out, where, s in ((d_true, d_in, ro.lost_d, int(seed)), (p_true, p_in, ro.unread_p, int(seed) ^ 0x9E3779B97F4A7C15)):
        j = us.junk(int(where.sum()) * P, s).reshape(-1, P)
        j[(j == true[where]).all(axis=1)] ^= 0xFF
        out[where] = j
    assert (d_in != d_true).any(axis=2)[ro.lost_d].all() and (p_in != p_true).any(axis=2)[ro.unread_p].all()
    return d_in.reshape(-1), p_in.reshape(-1)
