// fec_plan_build.hpp — one group's recovery record, built from its erasure mask and the r x k parity
// matrix: the bytes gf256.hpp's build_record writes for the pattern (E, R), E = the lost data
// shards, R = the e lowest surviving parity rows (the rule of fec_mask.hpp).
// For the shapes whose codebook of every pattern is past its cap, where a record cannot be looked
// up and is built per group instead (fec_plan.hip build_records, FEC_PLAN_DEVICE).
//
// The build is a sequence of steps, each a loop over independent cells that the lanes of a wave
// share: cell t belongs to lane t % lanes.  A step reads only what earlier steps wrote and no two
// cells of a step touch the same byte, so the lanes of a step may run in any order, or one after
// the other.  `each` runs a step: each(f) calls f(lane, lanes) for every lane and returns when all
// have finished -- on the device a wave's 64 lanes at once and a wave barrier (fec_plan.hip), on
// the host a loop over the lanes.  Plain C++ with no HIP dependency: a host program builds every
// record into a heap block of exactly record_bytes(k, e) bytes under AddressSanitizer and compares
// it with build_record's (tests/csrc/plan_build_test.cpp).
//
// Arithmetic: GF(2^8), polynomial 0x11D, by shift and xor (no table).  The inverse of M[R][E] is
// Gauss-Jordan without a row search: the leading principal minors of M[R][E] are minors of a
// row- and column-scaled Cauchy matrix, none of them zero, so the pivot at [c][c] is never zero.
// A zero pivot is still met with a guard: plan_build_record returns false, having divided by
// nothing, and the caller marks the group unrecoverable.
#pragma once

#include <cstdint>

#include "fec_mask.hpp"  // QFEC_HD; lost_data, alive_rows, low_bits, bit_count

namespace qfec {

constexpr uint32_t kPlanMaxE = 32;        // e <= min(k, r), k + r <= 64
constexpr uint32_t kPlanHeaderBytes = 128;  // gf256.hpp kRecordHeader
constexpr uint32_t kPlanEntryBytes = 32;    // sizeof(CoefEntry)

// The bytes of a record with e rows: gf256.hpp record_bytes(k, e) of the CoefEntry layout.
QFEC_HD uint64_t plan_record_bytes(uint32_t k, uint32_t e) {
  return kPlanHeaderBytes + static_cast<uint64_t>(e) * k * kPlanEntryBytes;
}

// What a wave keeps while it builds one record (the device: a per-wave LDS slice).
struct PlanScratch {
  uint8_t erased[kPlanMaxE];          // E ascending
  uint8_t rows[kPlanMaxE];            // R ascending
  uint8_t surv[64];                   // survivor shard ids, k of them
  uint8_t sub[kPlanMaxE * kPlanMaxE];  // M[R][E], reduced in place (e x e, row-major)
  uint8_t inv[kPlanMaxE * kPlanMaxE];  // its inverse
  uint8_t coef[kPlanMaxE * kPlanMaxE];  // the record's e x k coefficients: e * k <= 1024 as e <= min(k, 64 - k)
};

QFEC_HD uint32_t plan_gf_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 8; ++i) {
    p ^= (b & 1u) ? a : 0u;
    b >>= 1;
    a = (a << 1) ^ ((a & 0x80u) ? 0x11Du : 0u);
  }
  return p & 0xFFu;
}

// a^254 = 1 / a; 0 for a = 0 (GF256::inv).
QFEC_HD uint32_t plan_gf_inv(uint32_t a) {
  const uint32_t a2 = plan_gf_mul(a, a), a4 = plan_gf_mul(a2, a2), a8 = plan_gf_mul(a4, a4);
  const uint32_t a16 = plan_gf_mul(a8, a8), a32 = plan_gf_mul(a16, a16), a64 = plan_gf_mul(a32, a32);
  const uint32_t a128 = plan_gf_mul(a64, a64);
  return plan_gf_mul(plan_gf_mul(plan_gf_mul(a128, a64), plan_gf_mul(a32, a16)),
                     plan_gf_mul(plan_gf_mul(a8, a4), a2));
}

// One 16-B half of coefficient c's table entry (gf256.hpp make_entry): half 0 = t0lo, t0hi, t1lo,
// t1hi (c * v and c * (v << 3), v = 0..7), half 1 = t2 (c * (v << 6), v = 0..3), c, 0, 0.  A
// product with v is the xor of c * 2^i over the bits i of v.
struct alignas(16) PlanHalf {
  uint32_t w[4];
};
QFEC_HD PlanHalf plan_entry_half(uint32_t c, uint32_t half) {
  uint32_t p[8];  // c * 2^i
  p[0] = c & 0xFFu;
  for (int i = 1; i < 8; ++i) p[i] = ((p[i - 1] << 1) ^ ((p[i - 1] & 0x80u) ? 0x11Du : 0u)) & 0xFFu;
  // bytes v = 0..3 of the table over (x0, x1) = c * (1, 2) << shift: bits 0 and 1 of v select them
  const auto word = [](uint32_t x0, uint32_t x1) { return (x0 << 8) | (x1 << 16) | ((x0 ^ x1) << 24); };
  PlanHalf h;
  if (half == 0) {
    h.w[0] = word(p[0], p[1]), h.w[1] = h.w[0] ^ p[2] * 0x01010101u;
    h.w[2] = word(p[3], p[4]), h.w[3] = h.w[2] ^ p[5] * 0x01010101u;
  } else {
    h.w[0] = word(p[6], p[7]), h.w[1] = c & 0xFFu, h.w[2] = 0, h.w[3] = 0;
  }
  return h;
}

// Builds the record of `mask` at rec: plan_record_bytes(k, e) bytes, 16-B aligned, every one of
// them written.  Needs mask_losses(mask, k, r) = {e >= 1, recoverable} and k + r <= 64; M is the
// r x k parity matrix, row-major.  Returns false on a zero pivot (the record is then not valid).
// Every lane gets the same answer.
template <typename EACH>
QFEC_HD bool plan_build_record(uint32_t k, uint32_t r, const uint8_t* M, uint64_t mask, PlanScratch& sc, uint8_t* rec,
                               EACH each) {
  // the pick of fec_mask.hpp, one cell per shard: the erased set and the alive rows are its sets;
  // row i is chosen when it is alive and fewer than e alive rows lie below it (mask_pick's rows,
  // without its walk over them)
  const uint64_t dm = lost_data(mask, k);
  const uint64_t alive = alive_rows(mask, k, r);
  const uint32_t e = bit_count(dm);
  // survivors: the data shards not lost, ascending, then k + R_t; E and R
  each([&](uint32_t lane, uint32_t lanes) {
    for (uint32_t j = lane; j < k; j += lanes) {
      const uint32_t before = bit_count(dm & low_bits(j));
      if ((dm >> j) & 1u) sc.erased[before] = static_cast<uint8_t>(j);
      else sc.surv[j - before] = static_cast<uint8_t>(j);
    }
    for (uint32_t i = lane; i < r; i += lanes) {
      const uint32_t rank = bit_count(alive & low_bits(i));
      if (((alive >> i) & 1u) && rank < e) {
        sc.rows[rank] = static_cast<uint8_t>(i);
        sc.surv[k - e + rank] = static_cast<uint8_t>(k + i);
      }
    }
  });
  each([&](uint32_t lane, uint32_t lanes) {
    for (uint32_t t = lane; t < e * e; t += lanes) {
      const uint32_t a = t / e, b = t - a * e;
      sc.sub[t] = M[sc.rows[a] * k + sc.erased[b]];
      sc.inv[t] = a == b ? 1 : 0;
    }
  });
  // Gauss-Jordan on [sub | inv], pivot [c][c].  Column c of sub is read by step c and written by
  // none; the columns of sub at and left of c are those of the identity when the step ends and are
  // neither written nor read again.
  bool ok = true;
  for (uint32_t c = 0; c < e; ++c) {
    const uint32_t pivot = sc.sub[c * e + c];
    ok = ok && pivot != 0;
    const uint32_t pinv = plan_gf_inv(pivot);  // 0 for a zero pivot: nothing is divided by it
    each([&](uint32_t lane, uint32_t lanes) {  // row c scaled to a pivot of 1
      for (uint32_t j = lane; j < 2 * e; j += lanes) {
        if (j < e) {
          if (j > c) sc.sub[c * e + j] = static_cast<uint8_t>(plan_gf_mul(sc.sub[c * e + j], pinv));
        } else {
          sc.inv[c * e + j - e] = static_cast<uint8_t>(plan_gf_mul(sc.inv[c * e + j - e], pinv));
        }
      }
    });
    each([&](uint32_t lane, uint32_t lanes) {  // column c cleared from the other rows
      for (uint32_t t = lane; t < e * 2 * e; t += lanes) {
        const uint32_t i = t / (2 * e), j = t - i * 2 * e;
        if (i == c) continue;
        const uint32_t f = sc.sub[i * e + c];
        if (j < e) {
          if (j > c) sc.sub[i * e + j] ^= static_cast<uint8_t>(plan_gf_mul(f, sc.sub[c * e + j]));
        } else {
          sc.inv[i * e + j - e] ^= static_cast<uint8_t>(plan_gf_mul(f, sc.inv[c * e + j - e]));
        }
      }
    });
  }
  // coefficient of output row m at survivor slot s: a data survivor's sum_t inv[m][t] * M[R_t][j],
  // parity survivor R_t's inv[m][t]
  each([&](uint32_t lane, uint32_t lanes) {
    for (uint32_t t = lane; t < e * k; t += lanes) {
      const uint32_t m = t / k, s = t - m * k;
      uint32_t c = 0;
      if (s < k - e) {
        const uint32_t j = sc.surv[s];
        for (uint32_t u = 0; u < e; ++u) c ^= plan_gf_mul(sc.inv[m * e + u], M[sc.rows[u] * k + j]);
      } else {
        c = sc.inv[m * e + s - (k - e)];
      }
      sc.coef[t] = static_cast<uint8_t>(c);
    }
  });
  // Every coefficient 1 (the plain XOR)?  With e >= 2 never: the parity slots of each row would
  // make inv the all-ones matrix, which has no inverse.
  bool all_one = e == 1;
  if (all_one)
    for (uint32_t s = 0; s < k; ++s) all_one = all_one && sc.coef[s] == 1;
  each([&](uint32_t lane, uint32_t lanes) {
    // the header, 8 halves of 16 B: survivor ids at [0, k), erased ids at [64, 64 + e), e at 96,
    // the XOR flag at 97, zeros elsewhere
    for (uint32_t t = lane; t < kPlanHeaderBytes / 16u; t += lanes) {
      PlanHalf h{};
      for (uint32_t b = 0; b < 16; ++b) {
        const uint32_t at = t * 16u + b;
        const uint32_t v = at < k ? sc.surv[at] : at >= 64 && at < 64 + e ? sc.erased[at - 64] : at == 96 ? e : at == 97 ? (all_one ? 1u : 0u) : 0u;
        h.w[b >> 2] |= v << (8u * (b & 3u));
      }
      *reinterpret_cast<PlanHalf*>(rec + t * 16u) = h;
    }
    // the e x k table entries, two halves each; consecutive lanes store consecutive 16 B
    for (uint32_t t = lane; t < e * k * 2u; t += lanes)
      *reinterpret_cast<PlanHalf*>(rec + kPlanHeaderBytes + t * 16u) = plan_entry_half(sc.coef[t >> 1], t & 1u);
  });
  return ok;
}

}  // namespace qfec
