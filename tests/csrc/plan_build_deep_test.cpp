// plan_build_deep_test.cpp — the deep record builder (csrc/fec_plan_build_deep.hpp) with no GPU.
// Every record is built twice, with a single lane (each step one loop) and with 256 emulated lanes
// (each step lane after lane, as a workgroup shares it), both into heap blocks of exactly
// wide_record_bytes(k, e) bytes filled 0xEE before, the scratch a heap block filled 0xDD; the two
// must be equal byte for byte.  Built plain and with -fsanitize=address,undefined
// (tests/test_wide_deep_forms.py): a store before a block or past its end is a report.
//
//  (a) By the definition, for 33+33, 65+65, 100+100, 128+128, 40+216, 216+40, 96+160: with G = [I; M]
//      and S the k rows of G the header's survivor ids name, the coefficient row m, read from the
//      entries' coefficient bytes, times S is the unit row of erased id m; every entry equals
//      make_entry of its coefficient.  A shift-and-xor multiply, not the builder's.
//  (b) For 32+32 and 224+32, shapes the wide builder serves too: the table region is byte for byte
//      wide_plan_build_record's, and so are the survivor ids, e and the flag.
//  (c) The header, all 512 bytes: the survivors and the erased shards a per-bit loop names, e at
//      288, the flag at 289, the erased ids from 320, zero everywhere else.
// Patterns per shape: e in {1, 2, 32, 33, 64, 65, min(k, r)} (those the shape holds) with the lost
// shards and the chosen rows lowest, highest and spread; then 200 drawn masks; junk at and above
// k + r.  Prints "<shape> <records>" per shape, then "ok".
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/plan_build_deep_test.cpp
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fec_plan_build_deep.hpp"
#include "fec_plan_build_wide.hpp"
#include "gf256.hpp"

using namespace qfec;

namespace {

uint64_t g_rng = 0xDEE9C0DE5EEDull;
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

void junk_high(WideMask& m, uint32_t k, uint32_t r, uint32_t turn) {
  for (uint32_t s = k + r; s < 256; ++s)
    if (turn % 3 == 0 || (turn % 3 == 1 && (rnd() & 1u))) set_bit(m, s);
}

// e lost data shards and the rows to choose, each placed 0 = lowest, 1 = highest, 2 = spread; every
// row that is not to be chosen and lies below the highest chosen one is lost.
WideMask planted(uint32_t k, uint32_t r, uint32_t e, int where) {
  WideMask m{{0, 0, 0, 0}};
  std::vector<bool> chosen(r, false);
  for (uint32_t t = 0; t < e; ++t) {
    set_bit(m, where == 0 ? t : where == 1 ? k - 1 - t : static_cast<uint32_t>(uint64_t{t} * k / e));
    chosen[where == 0 ? t : where == 1 ? r - 1 - t : static_cast<uint32_t>(uint64_t{t} * r / e)] = true;
  }
  uint32_t top = 0;
  for (uint32_t i = 0; i < r; ++i)
    if (chosen[i]) top = i;
  for (uint32_t i = 0; i < top; ++i)
    if (!chosen[i]) set_bit(m, k + i);
  return m;
}

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

bool fail(uint32_t k, uint32_t r, const WideMask& m, const char* what) {
  std::fprintf(stderr, "k=%u r=%u mask=%016llx %016llx %016llx %016llx: %s\n", k, r, (unsigned long long)m.w[3],
               (unsigned long long)m.w[2], (unsigned long long)m.w[1], (unsigned long long)m.w[0], what);
  return false;
}

// One build with `lanes` lanes into a block of exactly `bytes`.
uint8_t* build_with(uint32_t lanes, uint32_t k, uint32_t r, const std::vector<uint8_t>& M, const WideMask& m, uint64_t bytes, bool* ok) {
  uint8_t* rec = static_cast<uint8_t*>(std::malloc(bytes));
  std::memset(rec, 0xEE, bytes);
  DeepPlanScratch* sc = static_cast<DeepPlanScratch*>(std::malloc(sizeof(DeepPlanScratch)));
  std::memset(sc, 0xDD, sizeof(DeepPlanScratch));
  *ok = deep_plan_build_record(k, r, M.data(), m, *sc, rec, [lanes](auto step) {
    for (uint32_t lane = 0; lane < lanes; ++lane) step(lane, lanes);
  });
  std::free(sc);
  return rec;
}

struct Built {
  std::vector<uint32_t> E, R;
  uint8_t* rec = nullptr;
  uint64_t bytes = 0;
};

// Builds the record of a recoverable mask with e >= 1 both ways and checks (c).  The caller frees b.rec.
bool build(uint32_t k, uint32_t r, const std::vector<uint8_t>& M, const WideMask& m, Built& b) {
  for (uint32_t j = 0; j < k; ++j)
    if (get_bit(m, j)) b.E.push_back(j);
  const uint32_t e = static_cast<uint32_t>(b.E.size());
  for (uint32_t i = 0; i < r && b.R.size() < e; ++i)
    if (!get_bit(m, k + i)) b.R.push_back(i);
  if (e == 0 || b.R.size() != e || e > kDeepMaxE) return false;
  b.bytes = wide_record_bytes(k, e);
  bool ok1 = false, ok256 = false;
  b.rec = build_with(1, k, r, M, m, b.bytes, &ok1);
  uint8_t* shared = build_with(256, k, r, M, m, b.bytes, &ok256);
  const bool same = std::memcmp(b.rec, shared, b.bytes) == 0;
  std::free(shared);
  if (!ok1 || !ok256) return std::fprintf(stderr, "zero pivot\n"), false;
  if (!same) return std::fprintf(stderr, "1 lane and 256 lanes differ\n"), false;
  std::vector<uint8_t> want(kWideHeaderBytes, 0);
  uint32_t ns = 0;
  for (uint32_t j = 0; j < k; ++j)
    if (!get_bit(m, j)) want[ns++] = static_cast<uint8_t>(j);
  for (uint32_t t = 0; t < e; ++t) want[ns++] = static_cast<uint8_t>(k + b.R[t]);
  if (ns != k) return false;
  for (uint32_t t = 0; t < e; ++t) want[kDeepErasedAt + t] = static_cast<uint8_t>(b.E[t]);
  want[kWideCountAt] = static_cast<uint8_t>(e);
  bool all_one = e == 1;
  for (uint32_t s = 0; s < k && all_one; ++s) all_one = reinterpret_cast<const CoefEntry*>(b.rec + kWideHeaderBytes)[s].coef == 1;
  if (all_one != (e == 1 && (b.R[0] == 0 || k == 1))) return std::fprintf(stderr, "XOR flag\n"), false;
  want[kWideXorAt] = all_one ? 1 : 0;
  if (std::memcmp(b.rec, want.data(), kWideHeaderBytes) != 0) return std::fprintf(stderr, "header differs\n"), false;
  return true;
}

// (a): against the definition.
bool check_definition(uint32_t k, uint32_t r, const std::vector<uint8_t>& M, const WideMask& m, uint64_t& built) {
  const MaskLosses w = wide_mask_losses(m, k, r);
  if (w.lost == 0 || w.unrecoverable) return fail(k, r, m, "the test's mask is not recoverable");
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

// (b): against the wide builder, e <= 32.
bool check_against_wide(uint32_t k, uint32_t r, const std::vector<uint8_t>& M, const WideMask& m, uint64_t& built) {
  const MaskLosses w = wide_mask_losses(m, k, r);
  if (w.lost == 0 || w.unrecoverable || w.lost > kWideMaxE) return fail(k, r, m, "the test's mask is not the wide builder's");
  Built b;
  if (!build(k, r, M, m, b)) return fail(k, r, m, "build");
  std::vector<uint8_t> ref(b.bytes, 0xEE);
  WidePlanScratch* sc = static_cast<WidePlanScratch*>(std::malloc(sizeof(WidePlanScratch)));
  const bool wok = wide_plan_build_record(k, r, M.data(), m, *sc, ref.data(), [](auto step) {
    for (uint32_t lane = 0; lane < 64; ++lane) step(lane, 64u);
  });
  std::free(sc);
  bool ok = wok && std::memcmp(b.rec + kWideHeaderBytes, ref.data() + kWideHeaderBytes, b.bytes - kWideHeaderBytes) == 0;
  ok = ok && std::memcmp(b.rec, ref.data(), 256) == 0 && b.rec[kWideCountAt] == ref[kWideCountAt] && b.rec[kWideXorAt] == ref[kWideXorAt];
  ok = ok && std::memcmp(b.rec + kDeepErasedAt, ref.data() + kWideErasedAt, w.lost) == 0;
  std::free(b.rec);
  ++built;
  return ok ? true : fail(k, r, m, "record differs from wide_plan_build_record's");
}

std::vector<WideMask> patterns(uint32_t k, uint32_t r, uint32_t emax) {
  std::vector<WideMask> masks;
  std::vector<uint32_t> es = {1u, 2u, 32u, 33u, 64u, 65u, emax};
  std::sort(es.begin(), es.end());
  es.erase(std::unique(es.begin(), es.end()), es.end());
  for (uint32_t e : es) {
    if (e > emax) continue;
    for (int where = 0; where < 3; ++where) masks.push_back(planted(k, r, e, where));
  }
  for (uint32_t turn = 0; turn < 200; ++turn) {
    // every e is drawn; odd turns lean to small e (a record costs about e^3)
    const uint32_t u = static_cast<uint32_t>(rnd() % emax), v = static_cast<uint32_t>(rnd() % emax);
    const uint32_t e = turn % 32 == 0 ? emax : 1 + (turn % 2 ? u * v / emax : u);
    masks.push_back(draw(k, r, e, turn % 8 == 7 ? r - e : static_cast<uint32_t>(rnd() % (r - e + 1))));
  }
  uint32_t turn = 0;
  for (WideMask& m : masks) junk_high(m, k, r, turn++);
  return masks;
}

}  // namespace

int main() {
  const uint16_t probe = 1;
  if (*reinterpret_cast<const uint8_t*>(&probe) != 1) {
    std::fprintf(stderr, "little-endian hosts only\n");
    return 2;
  }
  std::vector<uint8_t> M;
  const uint32_t deep[][2] = {{33, 33}, {65, 65}, {100, 100}, {128, 128}, {40, 216}, {216, 40}, {96, 160}};
  for (const auto& kr : deep) {
    const uint32_t k = kr[0], r = kr[1];
    uint64_t built = 0;
    if (!parity_matrix(k, r, M)) return 1;
    const std::vector<WideMask> masks = patterns(k, r, k < r ? k : r);
    for (const WideMask& m : masks)
      if (!check_definition(k, r, M, m, built)) return 1;
    if (built != masks.size()) return 1;
    std::printf("%u+%u %llu\n", k, r, static_cast<unsigned long long>(built));
  }
  const uint32_t both[][2] = {{32, 32}, {224, 32}};
  for (const auto& kr : both) {
    const uint32_t k = kr[0], r = kr[1];
    uint64_t built = 0;
    if (!parity_matrix(k, r, M)) return 1;
    const std::vector<WideMask> masks = patterns(k, r, 32);
    for (const WideMask& m : masks)
      if (!check_against_wide(k, r, M, m, built)) return 1;
    if (built != masks.size()) return 1;
    std::printf("%u+%u %llu\n", k, r, static_cast<unsigned long long>(built));
  }
  std::printf("ok\n");
  return 0;
}
