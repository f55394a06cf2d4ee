// plan_build_wide_test.cpp — the wide record builder (csrc/fec_plan_build_wide.hpp) with no GPU: 64
// lanes on the host, each step lane after lane, every record in a heap block of exactly
// wide_record_bytes(k, e) bytes filled 0xEE before.  Built plain and with
// -fsanitize=address,undefined (tests/test_wide_masks.py): a store before the block or past its
// end, or past a field of the scratch, is a report.
//
// Against the host's build_record (csrc/gf256.hpp), for k + r <= 64 -- every pattern of 4+2 and
// 10+3, 2,000 drawn masks each of 16+16 and 32+32, junk in words 1..3 of every mask: the survivor
// ids, the erased ids, e, the XOR flag and, by memcmp, the whole table region equal build_record's;
// the rest of the wide header is zero.
//
// Against the definition, for 60+5, 64+2, 65+3, 127+3, 190+5, 224+32, 32+224, 255+1, 1+255 and
// 100+20 -- 500 drawn plus the planted masks each, junk at and above k + r: the header lists the
// survivors and the erased shards the rule names (a per-bit loop), and the coefficient matrix C,
// read from the entries' coefficient bytes, satisfies  sum_s C[m][s] * G[surv_s] = unit row of
// erased[m]  with G = [I; M] and a shift-and-xor multiply; every entry equals make_entry of its
// coefficient.
// Prints "<shape> <records>" per shape, then "ok".
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/plan_build_wide_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fec_plan_build_wide.hpp"
#include "gf256.hpp"

using namespace qfec;

namespace {

uint64_t g_rng = 0x5EED00D1CE03ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

uint32_t slow_mul(uint32_t a, uint32_t b) {  // shift and xor, polynomial 0x11D
  uint32_t p = 0;
  for (int i = 0; i < 8; ++i) {
    if (b & 1u) p ^= a;
    b >>= 1;
    a <<= 1;
    if (a & 0x100u) a ^= 0x11Du;
  }
  return p & 0xFFu;
}

void set_bit(WideMask& m, uint32_t s) { m.w[s / 64] |= 1ull << (s % 64); }
bool get_bit(const WideMask& m, uint32_t s) { return (m.w[s / 64] >> (s % 64)) & 1u; }

// Junk in every bit at and above k + r.
void junk_high(WideMask& m, uint32_t k, uint32_t r, uint32_t turn) {
  for (uint32_t s = k + r; s < 256; ++s)
    if (turn % 3 == 0 || (turn % 3 == 1 && (rnd() & 1u))) set_bit(m, s);
}

// A mask with e lost data shards and `lostp` lost parity rows, drawn.
WideMask draw(uint32_t k, uint32_t r, uint32_t e, uint32_t lostp) {
  WideMask m{{0, 0, 0, 0}};
  for (uint32_t n = 0; n < e;) {
    const uint32_t j = static_cast<uint32_t>(rnd() % k);
    if (!get_bit(m, j)) set_bit(m, j), ++n;
  }
  for (uint32_t n = 0; n < lostp;) {
    const uint32_t i = static_cast<uint32_t>(rnd() % r);
    if (!get_bit(m, k + i)) set_bit(m, k + i), ++n;
  }
  return m;
}

struct Built {
  std::vector<uint32_t> E, R;
  uint8_t* rec = nullptr;
  uint64_t bytes = 0;
};

// Builds the record of a recoverable mask with e >= 1 into a block of exactly its bytes and checks
// the header against the per-bit rule.  The caller frees b.rec.
bool build(uint32_t k, uint32_t r, const std::vector<uint8_t>& M, const WideMask& m, Built& b) {
  for (uint32_t j = 0; j < k; ++j)
    if (get_bit(m, j)) b.E.push_back(j);
  const uint32_t e = static_cast<uint32_t>(b.E.size());
  for (uint32_t i = 0; i < r && b.R.size() < e; ++i)
    if (!get_bit(m, k + i)) b.R.push_back(i);
  if (e == 0 || b.R.size() != e || e > kWideMaxE) return false;
  b.bytes = wide_record_bytes(k, e);
  b.rec = static_cast<uint8_t*>(std::malloc(b.bytes));
  std::memset(b.rec, 0xEE, b.bytes);
  WidePlanScratch* sc = static_cast<WidePlanScratch*>(std::malloc(sizeof(WidePlanScratch)));
  std::memset(sc, 0xDD, sizeof(WidePlanScratch));
  const bool ok = wide_plan_build_record(k, r, M.data(), m, *sc, b.rec, [](auto step) {
    for (uint32_t lane = 0; lane < 64; ++lane) step(lane, 64u);
  });
  std::free(sc);
  if (!ok) return std::fprintf(stderr, "zero pivot\n"), false;
  // the header: survivors, erased ids, e, the flag, zeros elsewhere
  std::vector<uint8_t> want(kWideHeaderBytes, 0);
  uint32_t ns = 0;
  for (uint32_t j = 0; j < k; ++j)
    if (!get_bit(m, j)) want[ns++] = static_cast<uint8_t>(j);
  for (uint32_t t = 0; t < e; ++t) want[ns++] = static_cast<uint8_t>(k + b.R[t]);
  if (ns != k) return false;
  for (uint32_t t = 0; t < e; ++t) want[kWideErasedAt + t] = static_cast<uint8_t>(b.E[t]);
  want[kWideCountAt] = static_cast<uint8_t>(e);
  // the flag: every coefficient is 1 -- e == 1 from parity row 0 (the XOR row), and, with k == 1,
  // from any row (column 0 of M is all ones)
  bool all_one = e == 1;
  for (uint32_t s = 0; s < k && all_one; ++s) all_one = reinterpret_cast<const CoefEntry*>(b.rec + kWideHeaderBytes)[s].coef == 1;
  if (all_one != (e == 1 && (b.R[0] == 0 || k == 1))) return std::fprintf(stderr, "XOR flag\n"), false;
  want[kWideXorAt] = all_one ? 1 : 0;
  if (std::memcmp(b.rec, want.data(), kWideHeaderBytes) != 0) return std::fprintf(stderr, "header differs\n"), false;
  return true;
}

bool fail(uint32_t k, uint32_t r, const WideMask& m, const char* what) {
  std::fprintf(stderr, "k=%u r=%u mask=%016llx %016llx %016llx %016llx: %s\n", k, r, (unsigned long long)m.w[3],
               (unsigned long long)m.w[2], (unsigned long long)m.w[1], (unsigned long long)m.w[0], what);
  return false;
}

// k + r <= 64: against build_record.
bool check_narrow(uint32_t k, uint32_t r, const std::vector<uint8_t>& M, const WideMask& m, uint64_t& built) {
  const MaskLosses l = mask_losses(m.w[0], k, r);
  const MaskLosses w = wide_mask_losses(m, k, r);
  if (l.lost != w.lost || l.unrecoverable != w.unrecoverable) return fail(k, r, m, "losses differ from fec_mask.hpp's");
  if (l.lost == 0 || l.unrecoverable) return true;
  Built b;
  if (!build(k, r, M, m, b)) return fail(k, r, m, "build");
  const uint32_t e = l.lost;
  std::vector<uint8_t> ref(record_bytes(k, e), 0);
  if (!build_record(k, M, b.E.data(), b.R.data(), e, ref.data())) return fail(k, r, m, "build_record");
  bool ok = std::memcmp(b.rec, ref.data(), k) == 0 && std::memcmp(b.rec + kWideErasedAt, ref.data() + 64, e) == 0 &&
            b.rec[kWideCountAt] == ref[96] && b.rec[kWideXorAt] == ref[97];
  ok = ok && b.bytes - kWideHeaderBytes == ref.size() - kRecordHeader &&
       std::memcmp(b.rec + kWideHeaderBytes, ref.data() + kRecordHeader, ref.size() - kRecordHeader) == 0;
  std::free(b.rec);
  ++built;
  return ok ? true : fail(k, r, m, "record differs from build_record's");
}

// Any shape: against the definition.
bool check_wide(uint32_t k, uint32_t r, const std::vector<uint8_t>& M, const WideMask& m, uint64_t& built) {
  const MaskLosses w = wide_mask_losses(m, k, r);
  if (w.lost == 0 || w.unrecoverable) return true;
  Built b;
  if (!build(k, r, M, m, b)) return fail(k, r, m, "build");
  const uint32_t e = w.lost;
  const CoefEntry* ent = reinterpret_cast<const CoefEntry*>(b.rec + kWideHeaderBytes);
  bool ok = true;
  std::vector<uint8_t> row(k);
  for (uint32_t mm = 0; mm < e && ok; ++mm) {
    std::fill(row.begin(), row.end(), 0);
    for (uint32_t s = 0; s < k; ++s) {
      const CoefEntry& en = ent[mm * k + s];
      const CoefEntry want = make_entry(static_cast<uint8_t>(en.coef));
      ok = ok && en.coef < 256 && std::memcmp(&en, &want, sizeof(CoefEntry)) == 0;
      const uint32_t c = en.coef & 0xFFu, sid = b.rec[s];
      if (sid < k) row[sid] ^= static_cast<uint8_t>(c);  // G[sid] = unit row sid
      else
        for (uint32_t j = 0; j < k; ++j) row[j] ^= static_cast<uint8_t>(slow_mul(c, M[(sid - k) * k + j]));
    }
    for (uint32_t j = 0; j < k; ++j) ok = ok && row[j] == (j == b.E[mm] ? 1 : 0);
  }
  std::free(b.rec);
  ++built;
  return ok ? true : fail(k, r, m, "the coefficients do not rebuild the erased shards");
}

}  // namespace

int main() {
  const uint16_t probe = 1;
  if (*reinterpret_cast<const uint8_t*>(&probe) != 1) {
    std::fprintf(stderr, "little-endian hosts only\n");
    return 2;
  }
  std::vector<uint8_t> M;
  const uint32_t all[][2] = {{4, 2}, {10, 3}};
  for (const auto& kr : all) {
    const uint32_t k = kr[0], r = kr[1];
    uint64_t built = 0;
    if (!parity_matrix(k, r, M)) return 1;
    for (uint64_t mask = 0; mask < (1ull << (k + r)); ++mask) {
      WideMask m{{mask | rnd() << (k + r), rnd(), rnd(), rnd()}};
      if (!check_narrow(k, r, M, m, built) || !check_wide(k, r, M, m, built)) return 1;
    }
    std::printf("%u+%u %llu\n", k, r, static_cast<unsigned long long>(built / 2));
  }
  const uint32_t drawn[][2] = {{16, 16}, {32, 32}};
  for (const auto& kr : drawn) {
    const uint32_t k = kr[0], r = kr[1], emax = k < r ? k : r;
    uint64_t built = 0;
    if (!parity_matrix(k, r, M)) return 1;
    for (uint32_t turn = 0; turn < 2000; ++turn) {
      const uint32_t e = turn % 8 == 0 ? emax : turn % 8 == 1 ? 1 : 1 + static_cast<uint32_t>(rnd() % emax);
      WideMask m = draw(k, r, e, turn % 8 == 7 ? r - e + 1 : static_cast<uint32_t>(rnd() % (r - e + 1)));
      if (k + r < 64) m.w[0] |= rnd() << (k + r);
      m.w[1] = rnd(), m.w[2] = rnd(), m.w[3] = rnd();
      if (!check_narrow(k, r, M, m, built)) return 1;
    }
    std::printf("%u+%u %llu\n", k, r, static_cast<unsigned long long>(built));
  }
  const uint32_t wide[][2] = {{60, 5}, {64, 2}, {65, 3}, {127, 3}, {190, 5}, {224, 32}, {32, 224}, {255, 1}, {1, 255}, {100, 20}};
  for (const auto& kr : wide) {
    const uint32_t k = kr[0], r = kr[1], emax = (k < r ? k : r) < kWideMaxE ? (k < r ? k : r) : kWideMaxE;
    uint64_t built = 0;
    if (!parity_matrix(k, r, M)) return 1;
    std::vector<WideMask> masks;
    for (uint32_t turn = 0; turn < 500; ++turn) {
      const uint32_t e = turn % 8 == 0 ? emax : turn % 8 == 1 ? 1 : 1 + static_cast<uint32_t>(rnd() % emax);
      masks.push_back(draw(k, r, e, static_cast<uint32_t>(rnd() % (r - e + 1))));
    }
    // planted: shards 0 and k - 1; the lowest and the highest e = emax shards with the top rows (every
    // lower row lost); a lost shard at each word boundary the shape has, rebuilt from the top row alone
    WideMask m{{0, 0, 0, 0}};
    set_bit(m, 0), set_bit(m, k - 1);
    if (k >= 2 && r >= 2) masks.push_back(m);
    for (int high = 0; high < 2; ++high) {
      m = WideMask{{0, 0, 0, 0}};
      for (uint32_t t = 0; t < emax; ++t) set_bit(m, high ? k - 1 - t : t);
      for (uint32_t i = 0; i + emax < r; ++i) set_bit(m, k + i);
      masks.push_back(m);
    }
    for (uint32_t s : {63u, 64u, 127u, 128u, 191u, 192u}) {
      if (s >= k) continue;
      m = WideMask{{0, 0, 0, 0}};
      set_bit(m, s);
      for (uint32_t i = 0; i + 1 < r; ++i) set_bit(m, k + i);
      masks.push_back(m);
    }
    uint32_t turn = 0;
    for (WideMask& mk : masks) {
      junk_high(mk, k, r, turn++);
      if (!check_wide(k, r, M, mk, built)) return 1;
    }
    if (built != masks.size()) return std::fprintf(stderr, "%u+%u: %llu of %zu masks built\n", k, r, (unsigned long long)built, masks.size()), 1;
    std::printf("%u+%u %llu\n", k, r, static_cast<unsigned long long>(built));
  }
  std::printf("ok\n");
  return 0;
}
