// fec_plan_build_wide.hpp — one group's recovery record for a shape of up to 256 shards, built from
// its four-word erasure mask (fec_mask_wide.hpp) and the r x k parity matrix: plan_build_record's
// steps (fec_plan_build.hpp) over a WideMask, for k + r <= 256 and min(k, r) <= 32.
//
// The wide record.  A header of kWideHeaderBytes = 512 bytes, then the e x k CoefEntry tables
// exactly as gf256.hpp make_entry writes them, row m, survivor s at tabs[m * k + s]:
//     [  0, 256)  survivor shard ids, k of them (k <= 255): the surviving data shards ascending,
//                 then k + R_t for the chosen rows R_t ascending
//     [256, 288)  erased data shard ids ascending, e of them (e <= 32)
//      288        e
//      289        the XOR flag: 1 when every coefficient is 1 (e == 1 with parity row 0 chosen)
//     [290, 512)  zero
//     [512, 512 + e * k * 32)  the tables
// 512 is a multiple of 32 (record offsets are counted in 32-B units, fec_wide.hip) and keeps every
// table entry on its own 32-B line.  The one-word record (gf256.hpp build_record) has the same
// fields at 0, 64, 96, 97 of a 128-B header; its table region is byte for byte this one's
// (tests/csrc/plan_build_wide_test.cpp compares them for k + r <= 64).
//
// The build is the sequence of steps fec_plan_build.hpp describes: each a loop over independent
// cells shared by the lanes of a wave through `each`, which returns when every lane has finished
// the step.  Plain C++ with no HIP dependency; the arithmetic (plan_gf_mul, plan_gf_inv,
// plan_entry_half) is fec_plan_build.hpp's.  The inverse is Gauss-Jordan without a row search, for
// the reason given there: M is a row- and column-scaled Cauchy matrix for every k + r <= 256, so no
// leading principal minor of M[R][E] is zero.  A zero pivot is still met with a guard.
#pragma once

#include <cstdint>

#include "fec_mask_wide.hpp"
#include "fec_plan_build.hpp"  // plan_gf_mul, plan_gf_inv, PlanHalf, plan_entry_half, kPlanEntryBytes

namespace qfec {

constexpr uint32_t kWideMaxE = 32;          // e <= min(k, r) <= 32
constexpr uint32_t kWideMaxK = 255;         // r >= 1
constexpr uint32_t kWideHeaderBytes = 512;  // the layout above
constexpr uint32_t kWideErasedAt = 256, kWideCountAt = 288, kWideXorAt = 289;
// e * k <= 32 * 224: e <= min(k, 256 - k, 32), largest at k = 224
constexpr uint32_t kWideMaxCoefs = 32 * 224;
// r * k <= 32 * 224 as well: min(k, r) <= 32 and k + r <= 256
constexpr uint32_t kWideMaxMatrix = 32 * 224;

QFEC_HD constexpr uint64_t wide_record_bytes(uint32_t k, uint32_t e) {
  return kWideHeaderBytes + static_cast<uint64_t>(e) * k * kPlanEntryBytes;
}

// What a wave keeps while it builds one record (the device: a per-wave LDS slice, 9,536 B).
struct WidePlanScratch {
  uint8_t erased[kWideMaxE];           // E ascending
  uint8_t rows[kWideMaxE];             // R ascending
  uint8_t surv[256];                   // survivor shard ids, k of them
  uint8_t sub[kWideMaxE * kWideMaxE];  // M[R][E], reduced in place (e x e, row-major)
  uint8_t inv[kWideMaxE * kWideMaxE];  // its inverse
  uint8_t coef[kWideMaxCoefs];         // the record's e x k coefficients
};

// Builds the record of `mask` at rec: wide_record_bytes(k, e) bytes, 16-B aligned, every one of
// them written.  Needs wide_mask_losses(mask, k, r) = {e >= 1, recoverable}, k + r <= 256 and
// e <= 32; M is the r x k parity matrix, row-major.  Returns false on a zero pivot (the record is
// then not valid).  Every lane gets the same answer.
template <typename EACH>
QFEC_HD bool wide_plan_build_record(uint32_t k, uint32_t r, const uint8_t* M, const WideMask& mask, WidePlanScratch& sc,
                                    uint8_t* rec, EACH each) {
  // the pick, one cell per shard: row i is chosen when it is alive and fewer than e alive rows lie
  // below it
  const WideMask dm = wide_lost_data(mask, k);
  const WideMask alive = wide_alive_rows(mask, k, r);
  const uint32_t e = wide_bit_count(dm);
  // survivors: the data shards not lost, ascending, then k + R_t; E and R
  each([&](uint32_t lane, uint32_t lanes) {
    for (uint32_t j = lane; j < k; j += lanes) {
      const uint32_t before = wide_count_below(dm, j);
      if (wide_bit(dm, j)) sc.erased[before] = static_cast<uint8_t>(j);
      else sc.surv[j - before] = static_cast<uint8_t>(j);
    }
    for (uint32_t i = lane; i < r; i += lanes) {
      const uint32_t rank = wide_count_below(alive, i);
      if (wide_bit(alive, i) && rank < e) {
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
  // Gauss-Jordan on [sub | inv], pivot [c][c] (fec_plan_build.hpp: which cells a step reads and writes)
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
  // Every coefficient 1 (the plain XOR)?  With e >= 2 never (fec_plan_build.hpp).
  bool all_one = e == 1;
  if (all_one)
    for (uint32_t s = 0; s < k; ++s) all_one = all_one && sc.coef[s] == 1;
  each([&](uint32_t lane, uint32_t lanes) {
    // the header, 32 halves of 16 B
    for (uint32_t t = lane; t < kWideHeaderBytes / 16u; t += lanes) {
      PlanHalf h{};
      for (uint32_t b = 0; b < 16; ++b) {
        const uint32_t at = t * 16u + b;
        const uint32_t v = at < k                                          ? sc.surv[at]
                           : at >= kWideErasedAt && at < kWideErasedAt + e ? sc.erased[at - kWideErasedAt]
                           : at == kWideCountAt                            ? e
                           : at == kWideXorAt                              ? (all_one ? 1u : 0u)
                                                                           : 0u;
        h.w[b >> 2] |= v << (8u * (b & 3u));
      }
      *reinterpret_cast<PlanHalf*>(rec + t * 16u) = h;
    }
    // the e x k table entries, two halves each; consecutive lanes store consecutive 16 B
    for (uint32_t t = lane; t < e * k * 2u; t += lanes)
      *reinterpret_cast<PlanHalf*>(rec + kWideHeaderBytes + t * 16u) = plan_entry_half(sc.coef[t >> 1], t & 1u);
  });
  return ok;
}

}  // namespace qfec
