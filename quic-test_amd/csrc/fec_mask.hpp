// fec_mask.hpp — what a group's erasure mask means, stated for the host and for the cold kernels.
//
// The rule.  A group has k data shards and r parity rows, k + r <= 64.
//  * Bit j < k of the mask: data shard j is lost.  Bit k + i: parity row i is lost.  Bits at and
//    above k + r are ignored.
//  * e lost data shards need e surviving parity rows; with fewer the group is unrecoverable
//    (status 1, nothing rebuilt).  A recoverable group rebuilds e rows, any other group none.
//  * The survivors a rebuild reads are the surviving data shards ascending, then the e lowest
//    surviving parity rows (the chosen rows).
//  * xor_only: e == 1 with parity row 0 among the chosen rows (every coefficient is 1).
//  * The codebook record of a pattern is base[e] + (rank_e * count_r[e] + rank_r) * stride[e], with
//    rank_e / rank_r the colex ranks of the erased set and of the chosen rows (gf256.hpp
//    codebook_layout, build_codebook).
//
// Who calls it: the host (fec_routes.hpp, gf256.hpp, the shim, the batcher), classify_mask
// (classify and the address-table classify kernels), the rows_* prefix kernels, the record builder
// (fec_plan_build.hpp, build_records) and the probes.  Plain C++ with no HIP include, so a host
// program checks these very functions (tests/csrc/mask_rule_test.cpp); no path shifts a 64-bit
// value by 64, whatever k and r.
// Who does NOT: the mask-addressed hot kernels (fec_decode_fused.hip decode_fused's DIRECT / INLINE
// forms, fec_runs.hip recover_runs) keep their own hand-written statement of this rule, with compile-time K and
// their own guards, because calling these functions changes their instructions
// (profiles/mask_rule/VERDICT.md); they take only low_bits(K) and ChooseSmall from here.  A change
// to the rule has to be made there too, and only the GPU tests check their copy: the every-mask
// test (tests/test_gpu_forms.py test_every_mask: every mask with the bits at and above k + r clean,
// all set, only bit k + r set, and drawn) and the decode cases, whose masks all carry junk in those
// bits (tests/unread_shards.py high_bits; its wrong readers on the CPU show what that junk catches).
#pragma once

#include <cstdint>

// host + device + inline: one definition, the same in fec_varlen.hpp and coef_tables.hpp
#if defined(__HIPCC__)
#define QFEC_HD __host__ __device__ __forceinline__
#else
#define QFEC_HD inline
#endif

namespace qfec {

QFEC_HD constexpr uint64_t low_bits(uint32_t n) { return (n >= 64 ? 0ull : 1ull << n) - 1; }
QFEC_HD constexpr uint64_t lost_data(uint64_t m, uint32_t k) { return m & low_bits(k); }
QFEC_HD constexpr uint64_t lost_parity(uint64_t m, uint32_t k, uint32_t r) {
  return k >= 64 ? 0 : (m >> k) & low_bits(r);
}
QFEC_HD uint32_t bit_count(uint64_t x) { return static_cast<uint32_t>(__builtin_popcountll(x)); }
QFEC_HD uint32_t lowest_bit(uint64_t x) { return static_cast<uint32_t>(__builtin_ctzll(x)); }  // x != 0

// ---- losses ----
struct MaskLosses {
  uint32_t lost;       // e: data shards to rebuild
  bool unrecoverable;  // fewer than e parity rows survive (so e > 0): status 1, data untouched
};
QFEC_HD MaskLosses mask_losses(uint64_t m, uint32_t k, uint32_t r) {
  const uint32_t e = bit_count(lost_data(m, k));
  const uint32_t alive = r - bit_count(lost_parity(m, k, r));
  return {e, e > alive};
}
// Rows the group rebuilds: e when recoverable, else 0.
QFEC_HD uint32_t mask_rows(uint64_t m, uint32_t k, uint32_t r) {
  const MaskLosses l = mask_losses(m, k, r);
  return l.lost > 0 && !l.unrecoverable ? l.lost : 0u;
}
// f(j) for every lost data shard j of mask m, ascending.
template <class F>
QFEC_HD void for_each_lost(uint64_t m, uint32_t k, F&& f) {
  for (uint64_t lost = lost_data(m, k); lost; lost &= lost - 1) f(lowest_bit(lost));
}

// ---- the pick (of a recoverable mask: mask_losses says e rows survive) ----
QFEC_HD uint64_t alive_rows(uint64_t m, uint32_t k, uint32_t r) { return ~(k >= 64 ? 0 : m >> k) & low_bits(r); }
// row(i, t) for the chosen rows ascending: parity row i is the t-th, t = 0..e-1, of the e lowest
// in `alive`.
template <class ROW>
QFEC_HD void for_each_chosen(uint64_t alive, uint32_t e, ROW&& row) {
  for (uint32_t t = 0; t < e; ++t) {
    row(lowest_bit(alive), t);
    alive &= alive - 1;
  }
}
struct MaskPick {
  uint64_t erased;     // the lost data shards (bit j)
  uint64_t rows;       // the chosen parity rows (bit i)
  uint64_t survivors;  // surviving data shards | rows << k: k bits, ascending = survivor order
  uint32_t e;
  bool xor_only;
};
QFEC_HD MaskPick mask_pick(uint64_t m, uint32_t k, uint32_t r) {
  const uint64_t erased = lost_data(m, k);
  const uint32_t e = bit_count(erased);
  const uint64_t alive = alive_rows(m, k, r);
  uint64_t rows = 0;
  for_each_chosen(alive, e, [&](uint32_t i, uint32_t) { rows |= 1ull << i; });
  return {erased, rows, (~erased & low_bits(k)) | (k >= 64 ? 0 : rows << k), e, e == 1 && (alive & 1u)};
}

// ---- ranks and the record ----
// C(n, t) for t = 1..3 without a table (the mask-addressed decode ranks inline; its shapes have
// r <= 3, so e <= 3).  n < t gives 0 like the table.
struct ChooseSmall {
  QFEC_HD uint64_t operator()(uint32_t n, uint32_t t) const {
    const uint64_t a = n, b = n - 1u, c = n - 2u;
    return t == 1u ? a : t == 2u ? (a * b) >> 1 : (a * b * c) / 6u;
  }
};
// C(n, t) from a table of rows of 65 (gf256.hpp Binom, the device's copy of it).
struct ChooseTable {
  const uint64_t* binom;
  QFEC_HD uint64_t operator()(uint32_t n, uint32_t t) const { return binom[n * 65 + t]; }
};
// Colex rank of a bit set {c_0 < c_1 < ...}: sum_t C(c_t, t + 1).
template <class CHOOSE>
QFEC_HD uint64_t colex_rank(uint64_t set, CHOOSE choose) {
  uint64_t rank = 0;
  for (uint32_t t = 0; set; ++t) {
    rank += choose(lowest_bit(set), t + 1u);
    set &= set - 1;
  }
  return rank;
}
// The same sum over the chosen rows, as for_each_chosen visits them.
template <class CHOOSE>
QFEC_HD uint64_t chosen_rank(uint64_t alive, uint32_t e, CHOOSE choose) {
  uint64_t rank = 0;
  for_each_chosen(alive, e, [&](uint32_t i, uint32_t t) { rank += choose(i, t + 1u); });
  return rank;
}
// Byte offset of the record of level e with ranks rank_e (erased set) and rank_r (chosen rows);
// META has base[], stride[], count_r[] by level (LevelMeta, RankMeta).
template <class META>
QFEC_HD uint64_t record_offset(const META& meta, uint32_t e, uint64_t rank_e, uint64_t rank_r) {
  return meta.base[e] + (rank_e * meta.count_r[e] + rank_r) * meta.stride[e];
}
// The record of a recoverable mask with e >= 1 lost data shards (mask_losses' count).
template <class META, class CHOOSE>
QFEC_HD uint64_t mask_record(uint64_t m, uint32_t k, uint32_t r, uint32_t e, const META& meta, CHOOSE choose) {
  return record_offset(meta, e, colex_rank(lost_data(m, k), choose), chosen_rank(alive_rows(m, k, r), e, choose));
}

}  // namespace qfec
