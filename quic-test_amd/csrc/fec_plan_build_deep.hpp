// fec_plan_build_deep.hpp — one group's recovery record for a shape of up to 256 shards whose
// min(k, r) is past the wide builder's 32 rows: wide_plan_build_record's steps
// (fec_plan_build_wide.hpp) for k + r <= 256 and e <= min(k, r) <= 128, in a scratch of 48.5 KiB
// that the 256 lanes of one workgroup share (fec_wide_deep.hip build_records_deep) instead of the
// 64 lanes of a wave.
//
// The deep record.  The wide record with one field moved: 128 erased ids do not fit the wide
// record's [256, 288), so they follow the count instead.
//     [  0, 256)  survivor shard ids, k of them (k <= 255): the surviving data shards ascending,
//                 then k + R_t for the chosen rows R_t ascending
//     [256, 288)  zero
//      288        e (one byte: 128 fits)
//      289        the XOR flag: 1 when every coefficient is 1
//     [290, 320)  zero
//     [320, 448)  erased data shard ids ascending, e of them (e <= 128)
//     [448, 512)  zero
//     [512, 512 + e * k * 32)  the tables, exactly the wide record's
// The count, the flag and the tables lie where the wide record has them, so WideHead
// (fec_wide_head.hpp) reads a deep record unchanged; the one thing a consumer sees differently is
// where the erased ids start (kDeepErasedAt for kWideErasedAt).
//
// Every step is a loop over independent cells shared by the lanes through `each`, which returns
// when every lane has finished the step; the Gauss-Jordan steps never write column c or the pivot
// row's cells that the same step reads from other lanes (fec_plan_build.hpp), so they are race-free
// at any lane count.  Plain C++ with no HIP dependency: tests/csrc/plan_build_deep_test.cpp runs it
// on the host with one lane and with 256.  M is read where it lies (the device: global memory, the
// r x k <= 16 KiB matrix served by L2), not staged: with a staged copy a workgroup would take 64.5 KiB
// of the CU's 160 KiB of LDS and two would be resident where three fit.
#pragma once

#include <cstdint>

#include "fec_mask_wide.hpp"
#include "fec_plan_build_wide.hpp"  // kWideHeaderBytes, kWideCountAt, kWideXorAt, wide_record_bytes; the arithmetic

namespace qfec {

constexpr uint32_t kDeepMaxE = 128;  // e <= min(k, r) <= 128 as k + r <= 256
constexpr uint32_t kDeepErasedAt = 320;
// e * k <= min(k, 256 - k) * k: largest at k = 128
constexpr uint32_t kDeepMaxCoefs = 128 * 128;
static_assert(kWideMaxK <= kWideErasedAt && kWideErasedAt <= kWideCountAt, "the survivor ids end before the count");
static_assert(kWideXorAt + 1u <= kDeepErasedAt && kDeepErasedAt + kDeepMaxE <= kWideHeaderBytes,
              "the erased ids lie between the flag and the tables");
static_assert(kDeepErasedAt % 4u == 0, "rec_byte reads the ids from whole words");

// What a workgroup keeps while it builds one record (the device: 49,664 B of LDS).
struct DeepPlanScratch {
  uint8_t erased[kDeepMaxE];           // E ascending
  uint8_t rows[kDeepMaxE];             // R ascending
  uint8_t surv[256];                   // survivor shard ids, k of them
  uint8_t sub[kDeepMaxE * kDeepMaxE];  // M[R][E], reduced in place (e x e, row-major)
  uint8_t inv[kDeepMaxE * kDeepMaxE];  // its inverse
  uint8_t coef[kDeepMaxCoefs];         // the record's e x k coefficients
};
static_assert(sizeof(DeepPlanScratch) == 49664, "three workgroups' scratch fit the CU's 160 KiB of LDS");

// Builds the record of `mask` at rec: wide_record_bytes(k, e) bytes, 16-B aligned, every one of
// them written.  Needs wide_mask_losses(mask, k, r) = {e >= 1, recoverable} and k + r <= 256; M is
// the r x k parity matrix, row-major.  Returns false on a zero pivot (the record is then not
// valid).  Every lane gets the same answer.
template <typename EACH>
QFEC_HD bool deep_plan_build_record(uint32_t k, uint32_t r, const uint8_t* M, const WideMask& mask, DeepPlanScratch& sc,
                                    uint8_t* rec, EACH each) {
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
                           : at >= kDeepErasedAt && at < kDeepErasedAt + e ? sc.erased[at - kDeepErasedAt]
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
