// plan_build_test.cpp — the device-plan record builder (csrc/fec_plan_build.hpp) against the host's
// build_record (csrc/gf256.hpp), with no GPU.
//
// For every mask tried, the shared mask_losses (fec_mask.hpp: what build_records asks before it
// builds) is compared with a count of the mask's bits, one by one; for a
// recoverable mask with e >= 1 lost data shards, plan_build_record runs with all 64 lanes (each
// step lane after lane) into a heap block of exactly record_bytes(k, e) bytes, filled 0xEE before,
// and the block is compared by memcmp with the record build_record writes for E = the lost data
// shards, R = the e lowest surviving parity rows.  Built plain and with
// -fsanitize=address,undefined (tests/test_device_plan.py): a store before the block or past its
// end is a report.
//   shapes (4,2), (5,5), (10,3): every mask of k + r bits, so every pattern (E, R);
//   shapes (12,12), (20,7), (24,6), (16,16), (32,8), (60,4), (30,20), (32,32): 2,000 seeded masks
//   each, drawn in turn from the kinds below.
// Prints "<kind> <count>" for every kind of mask met, then "ok":
//   none        nothing lost among the data shards
//   bad         unrecoverable
//   xor         e = 1, parity row 0 alive (flag byte 1)
//   single      e = 1, parity row 0 lost (flag byte 0)
//   full        e = min(k, r)
//   skip_rows   a lost parity row below one the record uses
//   first_last  data shards 0 and k - 1 both lost
//   built       records compared
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/plan_build_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fec_plan_build.hpp"
#include "gf256.hpp"

using namespace qfec;

namespace {

enum Kind { kNone, kBad, kXor, kSingle, kFull, kSkipRows, kFirstLast, kBuilt, kKinds };
uint64_t g_count[kKinds];

uint64_t g_rng = 0x5EED00D1CEull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// `n` distinct bits below `width`, at random.
uint64_t random_bits(uint32_t n, uint32_t width) {
  uint64_t m = 0;
  while (static_cast<uint32_t>(__builtin_popcountll(m)) < n) m |= 1ull << (rnd() % width);
  return m;
}

bool check(uint32_t k, uint32_t r, const std::vector<uint8_t>& M, uint64_t mask) {
  MaskLosses want{0, false};  // bit by bit
  uint32_t rows_alive = 0;
  for (uint32_t j = 0; j < k; ++j) want.lost += static_cast<uint32_t>((mask >> j) & 1u);
  for (uint32_t i = 0; i < r; ++i) rows_alive += static_cast<uint32_t>(~(mask >> (k + i)) & 1u);
  want.unrecoverable = want.lost > rows_alive;
  const MaskLosses got = mask_losses(mask, k, r);
  if (got.lost != want.lost || got.unrecoverable != want.unrecoverable) {
    std::fprintf(stderr, "k=%u r=%u mask=%llx: mask_losses {%u, %d}, bit by bit {%u, %d}\n", k, r,
                 static_cast<unsigned long long>(mask), got.lost, got.unrecoverable, want.lost, want.unrecoverable);
    return false;
  }
  if (want.lost == 0) return ++g_count[kNone], true;
  if (want.unrecoverable) return ++g_count[kBad], true;
  const uint32_t e = want.lost;
  uint32_t E[kMaxDecodeShards], R[kMaxDecodeShards], ne = 0, nr = 0;
  for_each_lost(mask, k, [&](uint32_t j) { E[ne++] = j; });
  const uint64_t pm = lost_parity(mask, k, r);
  for (uint32_t i = 0; i < r && nr < e; ++i)
    if (!((pm >> i) & 1u)) R[nr++] = i;
  const uint64_t bytes = record_bytes(k, e);
  std::vector<uint8_t> ref(bytes, 0);
  if (!build_record(k, M, E, R, e, ref.data())) return false;
  if (plan_record_bytes(k, e) != bytes) return false;
  uint8_t* rec = static_cast<uint8_t*>(std::malloc(bytes));  // exactly the record
  std::memset(rec, 0xEE, bytes);
  PlanScratch* sc = static_cast<PlanScratch*>(std::malloc(sizeof(PlanScratch)));
  std::memset(sc, 0xDD, sizeof(PlanScratch));
  const bool built = plan_build_record(k, r, M.data(), mask, *sc, rec, [](auto step) {
    for (uint32_t lane = 0; lane < 64; ++lane) step(lane, 64u);
  });
  const bool same = built && std::memcmp(rec, ref.data(), bytes) == 0;
  if (!same) {
    uint64_t at = 0;
    while (at < bytes && rec[at] == ref[at]) ++at;
    std::fprintf(stderr, "k=%u r=%u mask=%llx e=%u: %s, first difference at byte %llu of %llu\n", k, r,
                 static_cast<unsigned long long>(mask), e, built ? "built" : "zero pivot", static_cast<unsigned long long>(at),
                 static_cast<unsigned long long>(bytes));
  }
  ++g_count[kBuilt];
  if (e == 1) ++g_count[(pm & 1u) ? kSingle : kXor];
  if (e == 1 && ref[97] != ((pm & 1u) ? 0 : 1)) return false;  // the flag byte as the kinds above name it
  if (e == (k < r ? k : r)) ++g_count[kFull];
  if (pm & low_bits(R[e - 1])) ++g_count[kSkipRows];
  if ((mask & 1u) && ((mask >> (k - 1)) & 1u)) ++g_count[kFirstLast];
  std::free(sc);
  std::free(rec);
  return same;
}

// One mask of the kind `turn` asks for (turn % 8), else any.
uint64_t random_mask(uint32_t k, uint32_t r, uint64_t turn) {
  const uint32_t emax = k < r ? k : r;
  // the data part (dm) drawn first, then the parity part (pm): one statement each, so the
  // sequence of draws is the same under every compiler
  uint64_t dm = 0, pm = 0;
  // up to `most` parity rows lost, at random
  const auto lose_rows = [r](uint32_t most) { return random_bits(static_cast<uint32_t>(rnd() % (most + 1)), r); };
  switch (turn % 8) {
    case 0:  // e = 1, parity row 0 alive
      dm = random_bits(1, k);
      pm = lose_rows(r - 1) & ~1ull;
      break;
    case 1:  // e = 1, parity row 0 lost
      dm = random_bits(1, k);
      pm = lose_rows(r - 2) | 1ull;
      break;
    case 2:  // e = min(k, r), as many parity rows lost as that leaves
      dm = random_bits(emax, k);
      pm = lose_rows(r - emax);
      break;
    case 3: {  // lost parity rows below the ones used
      const uint32_t lostp = 1 + static_cast<uint32_t>(rnd() % (r - 1));
      const uint32_t e = 1 + static_cast<uint32_t>(rnd() % (r - lostp < k ? r - lostp : k));
      dm = random_bits(e, k);
      pm = random_bits(lostp - 1, r) | 1ull;
      break;
    }
    case 4: {  // shards 0 and k - 1 among the lost
      const uint32_t e = 2 + static_cast<uint32_t>(rnd() % (emax - 1));
      dm = 1ull | 1ull << (k - 1);
      while (static_cast<uint32_t>(__builtin_popcountll(dm)) < e) dm |= 1ull << (rnd() % k);
      pm = lose_rows(r - e);
      break;
    }
    case 5:  // anything, unrecoverable ones and untouched groups included
      dm = rnd();
      dm &= rnd();
      return dm & low_bits(k + r);
    default: {  // e uniform in 1..min(k, r), recoverable
      const uint32_t e = 1 + static_cast<uint32_t>(rnd() % emax);
      dm = random_bits(e, k);
      pm = lose_rows(r - e);
      break;
    }
  }
  return dm | pm << k;
}

}  // namespace

int main() {
  const uint16_t probe = 1;
  if (*reinterpret_cast<const uint8_t*>(&probe) != 1) {
    std::fprintf(stderr, "little-endian hosts only\n");
    return 2;
  }
  std::vector<uint8_t> M;
  const uint32_t all[][2] = {{4, 2}, {5, 5}, {10, 3}};
  for (const auto& kr : all) {
    if (!parity_matrix(kr[0], kr[1], M)) return 1;
    for (uint64_t mask = 0; mask < (1ull << (kr[0] + kr[1])); ++mask)
      if (!check(kr[0], kr[1], M, mask)) return 1;
  }
  const uint32_t drawn[][2] = {{12, 12}, {20, 7}, {24, 6}, {16, 16}, {32, 8}, {60, 4}, {30, 20}, {32, 32}};
  for (const auto& kr : drawn) {
    if (!parity_matrix(kr[0], kr[1], M)) return 1;
    for (uint64_t turn = 0; turn < 2000; ++turn)
      if (!check(kr[0], kr[1], M, random_mask(kr[0], kr[1], turn))) return 1;
  }
  const char* names[kKinds] = {"none", "bad", "xor", "single", "full", "skip_rows", "first_last", "built"};
  for (int c = 0; c < kKinds; ++c) std::printf("%s %llu\n", names[c], static_cast<unsigned long long>(g_count[c]));
  std::printf("ok\n");
  return 0;
}
