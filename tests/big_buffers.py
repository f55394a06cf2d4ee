"""Arithmetic for the tests that put a call's buffers across byte offset 2^32
(tests/test_gpu_offsets_4gib.py): which groups to copy to the host, how to cut a call into pieces
whose offsets stay below 2^31, how thinly the special groups must be sown for the packed output to
cross the line all the same, and the comparison of a device buffer with the generator's stream.

Every kernel finds its bytes as base + (g * rows + row) * P + column; a product that is formed in 32
bits wraps at a multiple of 2^32, so the groups worth the CPU oracle's time are the ones around
each such multiple and at the two ends of the buffer.

tests/test_big_buffers.py checks this arithmetic on the CPU.  A plain module like
unread_shards.py: numpy (and the torch module a caller hands in), no fixtures, no tests.
"""
import numpy as np

LINE = 1 << 32                       # the offset a 32-bit product wraps at
MARGIN = 1 << 20                     # a buffer "crosses" when it exceeds LINE + MARGIN bytes
SLAB = 1 << 30                       # most bytes same_as_stream compares at a time


def crosses(nbytes):
    """The condition every case asserts of a buffer it claims to cross, before it launches."""
    return int(nbytes) > LINE + MARGIN


def boundary_groups(G, rows, P, halo=2):
    """For a buffer of G groups of rows * P bytes: the sorted group indices to check on the host.
    Groups 0..halo, the last halo groups, and for every multiple m * 2^32 inside the buffer the
    groups holding bytes m * 2^32 - 1 and m * 2^32 with halo neighbours on each side."""
    G, per, halo = int(G), int(rows) * int(P), int(halo)
    assert G > 0 and per > 0 and halo >= 0
    out = set(range(0, min(G, halo + 1))) | set(range(max(0, G - halo), G))
    total = G * per
    for line in range(LINE, total, LINE):                    # line < total: the byte at `line` exists
        lo, hi = (line - 1) // per, line // per
        out |= set(range(max(0, lo - halo), min(G, hi + halo + 1)))
    return sorted(out)


def pieces(G, bytes_per_group, limit=2**31 - 2**20):
    """Group ranges [(g0, g1), ...] that cover [0, G) exactly once, each spanning fewer than
    `limit` bytes of the widest buffer of the call (bytes_per_group is that buffer's)."""
    G, per, limit = int(G), int(bytes_per_group), int(limit)
    assert G > 0 and per > 0
    n = (limit - 1) // per                                   # n * per < limit
    if n < 1:
        raise ValueError(f"one group of {per} bytes does not stay below {limit}")
    return [(g0, min(G, g0 + n)) for g0 in range(0, G, n)]


def _is_prime(n):
    if n < 2:
        return False
    if n % 2 == 0:
        return n == 2
    f = 3
    while f * f <= n:
        if n % f == 0:
            return False
        f += 2
    return True


def special_groups(G, S):
    """Groups S - 1, 2S - 1, ...: every S-th group, group 0 staying an ordinary one."""
    return np.arange(int(S) - 1, int(G), int(S))


def special_every(G, rows_per_group, P):
    """The smallest prime S such that, if every S-th group (special_groups) rebuilt nothing, the
    rows of the others would still exceed 2^32 + 2^20 bytes.  Raises when there is none: the shape
    does not cross the line even with a single special group."""
    G, per = int(G), int(rows_per_group) * int(P)
    need = (LINE + MARGIN) // per + 1                        # ordinary groups needed: need * per > LINE + MARGIN
    if G - 1 < need:
        raise ValueError(f"{G} groups of {per} bytes: no room for a special group above {LINE + MARGIN} bytes")
    for S in range(2, G + 1):
        if _is_prime(S) and G - G // S >= need:              # G // S groups are special
            return S
    raise ValueError(f"no prime up to {G} leaves {need} ordinary groups")


def first_true(torch, flags):
    """Index of the first True of a flat bool tensor that holds one (no index list is built)."""
    return int(flags.view(torch.uint8).argmax().item())


def same_as_stream(ctx, torch, buf, seed):
    """Compare a device buffer of bytes with the generator's stream (fec_fill_random_dev, byte i of
    the buffer against byte i of the stream of `seed`) in slabs of at most 1 GiB: a scratch tensor is
    refilled with fill_random_dev(..., byte_offset=slab_start) and compared.  Returns the first
    differing byte offset, or None."""
    n = int(buf.numel())
    scratch = torch.empty(min(n, SLAB), dtype=torch.uint8, device=buf.device)
    try:
        for start in range(0, n, SLAB):
            size = min(SLAB, n - start)
            if buf.is_cuda:
                torch.cuda.synchronize()                     # the fill runs on the context's stream
            ctx.fill_random_dev(scratch, size, seed, start)
            ctx.synchronize()
            got = buf[start:start + size]
            if not torch.equal(got, scratch[:size]):
                return start + first_true(torch, got != scratch[:size])
        return None
    finally:
        del scratch
