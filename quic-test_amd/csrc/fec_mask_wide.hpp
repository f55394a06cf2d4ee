// fec_mask_wide.hpp — the erasure-mask rule of fec_mask.hpp for groups of up to 256 shards: a mask
// of four u64 words (fec_hip.h FEC_WIDE_MASK_WORDS), shard s at bit s & 63 of word s >> 6.
//
// The rule is fec_mask.hpp's, word for word, with k + r <= 256:
//  * Bit j < k: data shard j is lost.  Bit k + i: parity row i is lost.  Bits at and above k + r
//    are ignored, in the partial word and in the whole words above it.
//  * e lost data shards need e surviving parity rows; with fewer the group is unrecoverable.
//  * The survivors are the surviving data shards ascending, then the e lowest surviving rows.
// Each function here is the counterpart of the one-word function it is named after and gives the
// same answer for k + r <= 64 whatever words 1..3 hold (tests/csrc/mask_wide_test.cpp checks both,
// and every function against a per-bit loop).  There are no ranks and no codebook record: a wide
// shape's record is always built per group (fec_plan_build_wide.hpp).
//
// Who calls it: classify_wide and build_records_wide (fec_wide.hip), the wide record builder, and
// the host test programs.  Plain C++ with no HIP include.  No path shifts a 64-bit value by 64 or
// more, whatever k and r; no word is taken by a computed index (a lane's own index into w[] would
// put the mask into scratch memory on the device), wide_word selects instead.
#pragma once

#include <cstdint>

#include "fec_mask.hpp"  // QFEC_HD, bit_count, low_bits, lowest_bit, MaskLosses

namespace qfec {

constexpr uint32_t kWideMaskWords = 4;
constexpr uint32_t kWideMaskBits = 64 * kWideMaskWords;  // k + r <= 256

struct WideMask {
  uint64_t w[kWideMaskWords];
};

// Word i of m, i < 4.
QFEC_HD uint64_t wide_word(const WideMask& m, uint32_t i) { return i == 0 ? m.w[0] : i == 1 ? m.w[1] : i == 2 ? m.w[2] : m.w[3]; }
// Bit s of m, s < 256.
QFEC_HD bool wide_bit(const WideMask& m, uint32_t s) { return ((wide_word(m, s >> 6) >> (s & 63u)) & 1u) != 0; }

// Word i of the n lowest bits set, n <= 256: low_bits of what is left of n above 64 * i.
QFEC_HD uint64_t wide_low_word(uint32_t n, uint32_t i) { return n <= 64u * i ? 0ull : low_bits(n - 64u * i); }
QFEC_HD WideMask wide_low_bits(uint32_t n) {
  return {{wide_low_word(n, 0), wide_low_word(n, 1), wide_low_word(n, 2), wide_low_word(n, 3)}};
}
QFEC_HD WideMask wide_and(const WideMask& a, const WideMask& b) {
  return {{a.w[0] & b.w[0], a.w[1] & b.w[1], a.w[2] & b.w[2], a.w[3] & b.w[3]}};
}
QFEC_HD WideMask wide_not(const WideMask& a) { return {{~a.w[0], ~a.w[1], ~a.w[2], ~a.w[3]}}; }
QFEC_HD bool wide_any(const WideMask& a) { return (a.w[0] | a.w[1] | a.w[2] | a.w[3]) != 0; }
QFEC_HD uint32_t wide_bit_count(const WideMask& a) {
  return bit_count(a.w[0]) + bit_count(a.w[1]) + bit_count(a.w[2]) + bit_count(a.w[3]);
}
// Set bits of m below bit n, n <= 256.
QFEC_HD uint32_t wide_count_below(const WideMask& m, uint32_t n) { return wide_bit_count(wide_and(m, wide_low_bits(n))); }

// m >> s, s < 256: whole words first (by the two bits of s >> 6), then the s & 63 bits left, the
// word above coming in as (x << 1) << (63 - bits) -- 0 when bits == 0, and never a shift by 64.
QFEC_HD WideMask wide_shift_right(const WideMask& m, uint32_t s) {
  uint64_t t0 = m.w[0], t1 = m.w[1], t2 = m.w[2], t3 = m.w[3];
  const uint32_t words = s >> 6, bits = s & 63u;
  if (words & 1u) t0 = t1, t1 = t2, t2 = t3, t3 = 0;
  if (words & 2u) t0 = t2, t1 = t3, t2 = 0, t3 = 0;
  const uint32_t up = 63u - bits;
  return {{(t0 >> bits) | ((t1 << 1) << up), (t1 >> bits) | ((t2 << 1) << up), (t2 >> bits) | ((t3 << 1) << up), t3 >> bits}};
}

// ---- the sets (fec_mask.hpp lost_data, lost_parity, alive_rows) ----
QFEC_HD WideMask wide_lost_data(const WideMask& m, uint32_t k) { return wide_and(m, wide_low_bits(k)); }
QFEC_HD WideMask wide_lost_parity(const WideMask& m, uint32_t k, uint32_t r) {
  return wide_and(wide_shift_right(m, k), wide_low_bits(r));
}
QFEC_HD WideMask wide_alive_rows(const WideMask& m, uint32_t k, uint32_t r) {
  return wide_and(wide_not(wide_shift_right(m, k)), wide_low_bits(r));
}

// ---- losses (fec_mask.hpp mask_losses, mask_rows) ----
QFEC_HD MaskLosses wide_mask_losses(const WideMask& m, uint32_t k, uint32_t r) {
  const uint32_t e = wide_bit_count(wide_lost_data(m, k));
  const uint32_t alive = r - wide_bit_count(wide_lost_parity(m, k, r));
  return {e, e > alive};
}
QFEC_HD uint32_t wide_mask_rows(const WideMask& m, uint32_t k, uint32_t r) {
  const MaskLosses l = wide_mask_losses(m, k, r);
  return l.lost > 0 && !l.unrecoverable ? l.lost : 0u;
}

// f(s) for every set bit s of `set`, ascending.
template <class F>
QFEC_HD void wide_for_each_bit(const WideMask& set, F&& f) {
  for (uint32_t i = 0; i < kWideMaskWords; ++i)
    for (uint64_t w = wide_word(set, i); w; w &= w - 1) f(64u * i + lowest_bit(w));
}
// f(j) for every lost data shard j of mask m, ascending (fec_mask.hpp for_each_lost).
template <class F>
QFEC_HD void wide_for_each_lost(const WideMask& m, uint32_t k, F&& f) {
  wide_for_each_bit(wide_lost_data(m, k), f);
}
// The chosen-row walk (fec_mask.hpp for_each_chosen): row(i, t) for the chosen rows ascending,
// parity row i the t-th, t = 0..e-1, of the e lowest in `alive` (which has at least e bits).
template <class ROW>
QFEC_HD void wide_for_each_chosen(const WideMask& alive, uint32_t e, ROW&& row) {
  uint32_t t = 0;
  for (uint32_t i = 0; i < kWideMaskWords && t < e; ++i)
    for (uint64_t w = wide_word(alive, i); w && t < e; w &= w - 1, ++t) row(64u * i + lowest_bit(w), t);
}

// The pick of a recoverable mask (fec_mask.hpp mask_pick, without the survivor set: a wide group's
// survivors do not fit one mask shifted by k, the builder lists them).
struct WidePick {
  WideMask erased;  // the lost data shards (bit j)
  WideMask rows;    // the chosen parity rows (bit i)
  uint32_t e;
  bool xor_only;    // e == 1 with parity row 0 alive
};
QFEC_HD WidePick wide_mask_pick(const WideMask& m, uint32_t k, uint32_t r) {
  WidePick p{wide_lost_data(m, k), {{0, 0, 0, 0}}, 0, false};
  p.e = wide_bit_count(p.erased);
  const WideMask alive = wide_alive_rows(m, k, r);
  wide_for_each_chosen(alive, p.e, [&](uint32_t i, uint32_t) {
    const uint64_t bit = 1ull << (i & 63u);
    p.rows.w[0] |= (i >> 6) == 0 ? bit : 0, p.rows.w[1] |= (i >> 6) == 1 ? bit : 0;
    p.rows.w[2] |= (i >> 6) == 2 ? bit : 0, p.rows.w[3] |= (i >> 6) == 3 ? bit : 0;
  });
  p.xor_only = p.e == 1 && (alive.w[0] & 1u);
  return p;
}

}  // namespace qfec
