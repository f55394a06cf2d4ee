// mask_rule_test.cpp — the rule of an erasure mask (csrc/fec_mask.hpp), the code the kernels and
// the host both call, against independent statements of it, with no GPU.
//
// For every mask tried:
//   * mask_losses / mask_rows against the oracle's shard walk (oracle/fec_oracle.c: erased data
//     shards in order, then parity rows taken in order until k survivors; status 1 when they run
//     out), restated here bit by bit;
//   * for a recoverable mask with e >= 1, mask_pick against the record gf256.hpp's build_record
//     writes for the walk's (E, R): survivor ids at bytes 0..k-1, erased ids from byte 64, e and
//     the XOR flag in word 24; the chosen rows against R;
//   * colex_rank and chosen_rank against sum_t C(c_t, t + 1) over this file's own Pascal triangle,
//     with the binom table functor always and with ChooseSmall where e <= 3;
//   * where codebook_layout has a book for the shape, mask_record (both functors) against
//     level_base[e] + (rank(E) * C(r, e) + rank(R)) * level_stride[e]; for the exhaustive shapes
//     the record at that place of build_codebook's book is build_record's, byte for byte.
// Shapes: every mask of (4,2), (10,1), (10,2), (10,3) (the mask-addressed shapes) and (5,5); 2,000
// seeded masks each of (20,5), (60,4), (32,32), (63,1), with random junk in the bits at and above
// k + r (ignoring it is part of the rule).  A set of planted masks is added to every shape.
// Built plain and with -fsanitize=address,undefined (tests/test_mask_rule.py): a shift by 64 is a
// report.  Prints "<kind> <count>" for every kind of mask met, then "ok":
//   empty        nothing lost at all
//   all_data     every data shard lost
//   no_parity    every parity row lost and data lost (unrecoverable)
//   xor          e = 1, parity row 0 alive (xor_only)
//   single       e = 1, parity row 0 lost, recoverable (not xor_only)
//   exact_rows   recoverable with exactly e parity rows alive
//   skip_rows    the e lowest parity rows lost, recoverable: every chosen row is past a lost one
//   first_last   data shards 0 and k - 1 both lost
//   bad          unrecoverable
//   picked       recoverable masks with e >= 1, compared with build_record
//   placed       record offsets compared with codebook_layout
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/mask_rule_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fec_mask.hpp"
#include "gf256.hpp"

using namespace qfec;

namespace {

enum Kind { kEmpty, kAllData, kNoParity, kXor, kSingle, kExactRows, kSkipRows, kFirstLast, kBad, kPicked, kPlaced, kKinds };
uint64_t g_count[kKinds];

uint64_t g_rng = 0x5EED0A5C0DEull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

uint64_t g_pascal[65][65];  // this file's own C(n, t)
void fill_pascal() {
  for (int n = 0; n <= 64; ++n) {
    g_pascal[n][0] = 1;
    for (int t = 1; t <= n; ++t) g_pascal[n][t] = g_pascal[n - 1][t - 1] + (t <= n - 1 ? g_pascal[n - 1][t] : 0);
  }
}
uint64_t pascal_rank(const uint32_t* c, uint32_t n) {
  uint64_t rank = 0;
  for (uint32_t t = 0; t < n; ++t) rank += g_pascal[c[t]][t + 1];
  return rank;
}

struct Meta {  // the levels as the kernels get them (LevelMeta, RankMeta)
  uint64_t base[65], stride[65], count_r[65];
};

struct Shape {
  uint32_t k, r;
  std::vector<uint8_t> M;
  bool has_book = false;  // codebook_layout serves the shape
  CodebookLayout L;
  Meta meta;
  std::vector<uint8_t> book;  // exhaustive shapes only
};

#define FAIL(...)                                                                                       \
  do {                                                                                                  \
    std::fprintf(stderr, "k=%u r=%u mask=%llx: ", k, r, static_cast<unsigned long long>(mask));         \
    std::fprintf(stderr, __VA_ARGS__);                                                                  \
    std::fprintf(stderr, "\n");                                                                         \
    return false;                                                                                       \
  } while (0)

bool check(const Shape& sh, uint64_t mask) {
  const uint32_t k = sh.k, r = sh.r;
  // the oracle's walk; a bit is tested only below 64
  uint32_t E[64], S[64], R[64], ne = 0, ns = 0, nr = 0, rows_alive = 0;
  for (uint32_t j = 0; j < k; ++j) {
    if ((mask >> j) & 1u) E[ne++] = j;
    else S[ns++] = j;
  }
  for (uint32_t i = 0; i < r; ++i) {
    if ((mask >> (k + i)) & 1u) continue;
    ++rows_alive;
    if (ns < k) S[ns++] = k + i, R[nr++] = i;
  }
  const bool bad = ne > 0 && ns < k;
  const uint8_t status = bad ? 1 : 0;

  const MaskLosses l = mask_losses(mask, k, r);
  if (l.lost != ne || l.unrecoverable != bad) FAIL("mask_losses {%u, %d}, the walk {%u, %d}", l.lost, l.unrecoverable, ne, bad);
  if ((l.unrecoverable ? 1 : 0) != status) FAIL("status");
  const uint32_t rows = mask_rows(mask, k, r);
  if (rows != (bad ? 0u : ne)) FAIL("mask_rows %u, e %u, unrecoverable %d", rows, ne, bad);
  uint32_t seen = 0;
  bool in_order = true;
  for_each_lost(mask, k, [&](uint32_t j) { in_order = in_order && seen < ne && E[seen] == j, ++seen; });
  if (!in_order || seen != ne) FAIL("for_each_lost");

  const uint64_t below = mask & (k + r >= 64 ? ~0ull : (1ull << (k + r)) - 1);
  if (below == 0) ++g_count[kEmpty];
  if (ne == k) ++g_count[kAllData];
  if (ne > 0 && rows_alive == 0) ++g_count[kNoParity];
  if (ne >= 2 && (mask & 1u) && ((mask >> (k - 1)) & 1u)) ++g_count[kFirstLast];
  if (bad) ++g_count[kBad];
  if (ne == 0 || bad) return true;

  const uint32_t e = ne;
  const MaskPick p = mask_pick(mask, k, r);
  std::vector<uint8_t> rec(record_bytes(k, e), 0);
  if (!build_record(k, sh.M, E, R, e, rec.data())) FAIL("build_record");
  uint32_t word24;
  std::memcpy(&word24, rec.data() + 96, 4);
  if (p.e != (word24 & 0xFFu) || p.e != e) FAIL("pick.e %u, record %u", p.e, word24 & 0xFFu);
  if (p.xor_only != (((word24 >> 8) & 0xFFu) != 0)) FAIL("pick.xor_only %d, record flag %u", p.xor_only, (word24 >> 8) & 0xFFu);
  if (bit_count(p.survivors) != k) FAIL("%u survivors", bit_count(p.survivors));
  uint64_t x = p.survivors;
  for (uint32_t s = 0; s < k; ++s, x &= x - 1)
    if (lowest_bit(x) != rec[s] || rec[s] != S[s]) FAIL("survivor %u: pick %u, record %u, walk %u", s, lowest_bit(x), rec[s], S[s]);
  x = p.erased;
  if (bit_count(x) != e) FAIL("%u erased", bit_count(x));
  for (uint32_t t = 0; t < e; ++t, x &= x - 1)
    if (lowest_bit(x) != rec[64 + t]) FAIL("erased %u: pick %u, record %u", t, lowest_bit(x), rec[64 + t]);
  x = p.rows;
  if (bit_count(x) != e) FAIL("%u rows", bit_count(x));
  for (uint32_t t = 0; t < e; ++t, x &= x - 1)
    if (lowest_bit(x) != R[t]) FAIL("row %u: pick %u, walk %u", t, lowest_bit(x), R[t]);
  ++g_count[kPicked];
  if (e == 1) ++g_count[p.xor_only ? kXor : kSingle];
  if (e == 1 && p.xor_only != (R[0] == 0)) FAIL("xor_only %d with row %u", p.xor_only, R[0]);
  if (rows_alive == e) ++g_count[kExactRows];
  if (R[0] >= e) ++g_count[kSkipRows];  // rows 0..e-1 hold none of the chosen: all lost

  // ranks and the record's place
  const uint64_t rank_e = pascal_rank(E, e), rank_r = pascal_rank(R, e);
  const uint64_t alive = alive_rows(mask, k, r);
  if (colex_rank(p.erased, choose_binom()) != rank_e || colex_rank(p.rows, choose_binom()) != rank_r ||
      chosen_rank(alive, e, choose_binom()) != rank_r)
    FAIL("colex_rank, table");
  if (e <= 3 && (colex_rank(p.erased, ChooseSmall{}) != rank_e || colex_rank(p.rows, ChooseSmall{}) != rank_r ||
                 chosen_rank(alive, e, ChooseSmall{}) != rank_r))
    FAIL("colex_rank, ChooseSmall");
  // the walk over the chosen rows sees them in order
  uint32_t walked = 0;
  bool rows_in_order = true;
  for_each_chosen(alive, e, [&](uint32_t i, uint32_t t) { rows_in_order = rows_in_order && t == walked && t < e && R[t] == i, ++walked; });
  if (!rows_in_order || walked != e) FAIL("for_each_chosen");
  if (sh.has_book) {
    const uint64_t want = sh.L.level_base[e] + (rank_e * g_pascal[r][e] + rank_r) * sh.L.level_stride[e];
    const uint64_t table = mask_record(mask, k, r, e, sh.meta, choose_binom());
    if (table != want) FAIL("mask_record (table) %llu, layout %llu", static_cast<unsigned long long>(table), static_cast<unsigned long long>(want));
    if (e <= 3 && mask_record(mask, k, r, e, sh.meta, ChooseSmall{}) != table) FAIL("mask_record (ChooseSmall)");
    if (record_offset(sh.meta, e, rank_e, rank_r) != want) FAIL("record_offset");
    if (!sh.book.empty() && (want + rec.size() > sh.book.size() || std::memcmp(sh.book.data() + want, rec.data(), rec.size()) != 0))
      FAIL("the book's record at %llu is not build_record's", static_cast<unsigned long long>(want));
    ++g_count[kPlaced];
  }
  return true;
}

// `n` distinct bits below `width`, at random.
uint64_t random_bits(uint32_t n, uint32_t width) {
  uint64_t m = 0;
  while (bit_count(m) < n) m |= 1ull << (rnd() % width);
  return m;
}

// Random bits at and above k + r (none when k + r = 64).
uint64_t junk(uint32_t k, uint32_t r) { return k + r >= 64 ? 0 : rnd() & ~((1ull << (k + r)) - 1); }

bool planted(const Shape& sh, bool with_junk) {
  const uint32_t k = sh.k, r = sh.r, emax = k < r ? k : r;
  const uint64_t data = k >= 64 ? ~0ull : (1ull << k) - 1, par = (1ull << r) - 1;  // r < 64 in every shape here
  std::vector<uint64_t> ms;
  ms.push_back(0);                                 // empty
  ms.push_back(data);                              // all data lost
  ms.push_back(1ull | par << k);                   // all parity lost, one data shard lost
  ms.push_back(1ull << (k / 2));                   // one data shard, row 0 alive
  ms.push_back(1ull << (k / 2) | 1ull << k);       // one data shard, row 0 lost
  for (uint32_t e = 1; e <= emax; e += (emax > 4 ? emax / 4 : 1)) {
    const uint64_t dm = random_bits(e, k);
    ms.push_back(dm | ((par >> e) << e) << k);     // exactly e rows alive: the e lowest
    ms.push_back(dm | (par >> e) << k);            // exactly e rows alive: the e highest
    if (2 * e <= r) ms.push_back(dm | ((1ull << e) - 1) << k);  // the e lowest rows lost
  }
  ms.push_back(1ull | 1ull << (k - 1));            // first and last data shard
  ms.push_back(1ull | 1ull << (k - 1) | (r > 2 ? 1ull << k : 0));
  for (uint64_t m : ms)
    if (!check(sh, with_junk ? m | junk(k, r) : m)) return false;
  return true;
}

uint64_t drawn(uint32_t k, uint32_t r, uint64_t turn) {
  const uint32_t emax = k < r ? k : r;
  uint64_t dm = 0, pm = 0;  // one statement per draw: the same sequence under every compiler
  switch (turn % 4) {
    case 0:  // a few losses anywhere
      dm = random_bits(1 + static_cast<uint32_t>(rnd() % (r + 1)), k + r);
      return dm | junk(k, r);
    case 1: {  // recoverable, e uniform in 1..min(k, r)
      const uint32_t e = 1 + static_cast<uint32_t>(rnd() % emax);
      dm = random_bits(e, k);
      pm = random_bits(static_cast<uint32_t>(rnd() % (r - e + 1)), r);
      break;
    }
    case 2:  // an eighth of the bits
      dm = rnd();
      dm &= rnd();
      dm &= rnd();
      return dm;  // its high bits are the junk
    default:  // a quarter of the bits
      dm = rnd();
      dm &= rnd();
      return dm;
  }
  return dm | pm << k | junk(k, r);
}

bool prepare(Shape& sh, uint32_t k, uint32_t r, bool exhaustive) {
  sh.k = k, sh.r = r;
  if (!parity_matrix(k, r, sh.M)) return false;
  sh.has_book = codebook_layout(k, r, 2ull << 30, sh.L);
  std::memset(&sh.meta, 0, sizeof(sh.meta));
  if (sh.has_book)
    for (uint32_t e = 1; e <= r && e <= k; ++e)
      sh.meta.base[e] = sh.L.level_base[e], sh.meta.stride[e] = sh.L.level_stride[e], sh.meta.count_r[e] = g_pascal[r][e];
  if (exhaustive && (!sh.has_book || !build_codebook(sh.L, sh.M, sh.book))) return false;
  return true;
}

}  // namespace

int main() {
  fill_pascal();
  const uint32_t all[][2] = {{4, 2}, {10, 1}, {10, 2}, {10, 3}, {5, 5}};
  for (const auto& kr : all) {
    Shape sh;
    if (!prepare(sh, kr[0], kr[1], true)) return 1;
    for (uint64_t mask = 0; mask < (1ull << (kr[0] + kr[1])); ++mask)
      if (!check(sh, mask)) return 1;
    if (!planted(sh, false) || !planted(sh, true)) return 1;
  }
  const uint32_t some[][2] = {{20, 5}, {60, 4}, {32, 32}, {63, 1}};
  for (const auto& kr : some) {
    Shape sh;
    if (!prepare(sh, kr[0], kr[1], false)) return 1;
    for (uint64_t turn = 0; turn < 2000; ++turn)
      if (!check(sh, drawn(kr[0], kr[1], turn))) return 1;
    if (!planted(sh, false) || !planted(sh, true)) return 1;
  }
  const char* names[kKinds] = {"empty", "all_data", "no_parity", "xor", "single", "exact_rows", "skip_rows", "first_last", "bad", "picked", "placed"};
  for (int c = 0; c < kKinds; ++c) std::printf("%s %llu\n", names[c], static_cast<unsigned long long>(g_count[c]));
  std::printf("ok\n");
  return 0;
}
