// mask_wide_test.cpp — the four-word erasure-mask rule (csrc/fec_mask_wide.hpp) against a plain
// per-bit loop, with no GPU.
//
// For every mask tried, every function of fec_mask_wide.hpp -- wide_bit, wide_lost_data,
// wide_lost_parity, wide_alive_rows, wide_mask_losses, wide_mask_rows, wide_for_each_lost,
// wide_for_each_chosen, wide_mask_pick -- is compared with what a loop over the mask's bits, one by
// one, says; for the planted and the first 30 drawn masks of a shape also the helpers under them:
// wide_low_bits and wide_count_below for every n in 0..256, wide_shift_right for every shift 0..255.
// Masks:
// drawn ones and planted ones (nothing, everything, single bits at the word boundaries, every bit
// at and above k + r set) of 60+5, 64+2, 65+3, 127+3, 190+5, 224+32, 32+224, 255+1, 1+255; and of
// 10+3 and 32+32, where every answer must also equal fec_mask.hpp's on word 0, whatever words
// 1..3 hold.  Built plain and with -fsanitize=address,undefined (tests/test_wide_masks.py): a shift
// by 64 or more is a report.
// Prints "<shape> <masks checked>" per shape, then "ok".
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/mask_wide_test.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fec_mask_wide.hpp"

using namespace qfec;

namespace {

uint64_t g_rng = 0x5EED00D1CE02ull;
uint64_t rnd() {  // splitmix64
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

using Bits = std::vector<bool>;  // 256 of them

Bits bits_of(const WideMask& m) {
  Bits b(256);
  for (uint32_t s = 0; s < 256; ++s) b[s] = (m.w[s / 64] >> (s % 64)) & 1u;
  return b;
}
bool same(const WideMask& m, const Bits& b) { return bits_of(m) == b; }

#define CHECK(cond)                                                                                   \
  do {                                                                                                \
    if (!(cond)) {                                                                                    \
      std::fprintf(stderr, "k=%u r=%u mask=%016llx %016llx %016llx %016llx: %s (line %d)\n", k, r,     \
                   (unsigned long long)m.w[3], (unsigned long long)m.w[2], (unsigned long long)m.w[1], \
                   (unsigned long long)m.w[0], #cond, __LINE__);                                      \
      return false;                                                                                   \
    }                                                                                                 \
  } while (0)

// helpers: also wide_low_bits and wide_count_below for every n, wide_shift_right for every shift.
bool check(uint32_t k, uint32_t r, const WideMask& m, bool narrow, bool helpers) {
  const Bits b = bits_of(m);
  for (uint32_t s = 0; s < 256; ++s) CHECK(wide_bit(m, s) == b[s]);
  // the sets, bit by bit
  Bits lost_d(256), lost_p(256), alive(256);
  uint32_t e = 0, n_alive = 0;
  for (uint32_t j = 0; j < k; ++j) lost_d[j] = b[j], e += b[j];
  for (uint32_t i = 0; i < r; ++i) lost_p[i] = b[k + i], alive[i] = !b[k + i], n_alive += !b[k + i];
  CHECK(same(wide_lost_data(m, k), lost_d));
  CHECK(same(wide_lost_parity(m, k, r), lost_p));
  const WideMask al = wide_alive_rows(m, k, r);
  CHECK(same(al, alive));
  CHECK(wide_bit_count(al) == n_alive && wide_any(al) == (n_alive != 0));
  const MaskLosses l = wide_mask_losses(m, k, r);
  CHECK(l.lost == e && l.unrecoverable == (e > n_alive));
  CHECK(wide_mask_rows(m, k, r) == (e > 0 && e <= n_alive ? e : 0u));
  // the walks
  std::vector<uint32_t> want_lost, got_lost;
  for (uint32_t j = 0; j < k; ++j)
    if (b[j]) want_lost.push_back(j);
  wide_for_each_lost(m, k, [&](uint32_t j) { got_lost.push_back(j); });
  CHECK(want_lost == got_lost);
  if (e <= n_alive) {
    std::vector<uint32_t> want_rows, got_rows;
    for (uint32_t i = 0; i < r && want_rows.size() < e; ++i)
      if (alive[i]) want_rows.push_back(i);
    bool in_order = true;
    wide_for_each_chosen(al, e, [&](uint32_t i, uint32_t t) {
      in_order = in_order && t == got_rows.size();
      got_rows.push_back(i);
    });
    CHECK(in_order && want_rows == got_rows);
    const WidePick p = wide_mask_pick(m, k, r);
    Bits rows(256);
    for (uint32_t i : want_rows) rows[i] = true;
    CHECK(p.e == e && same(p.erased, lost_d) && same(p.rows, rows) && p.xor_only == (e == 1 && alive[0]));
    if (narrow) {
      const MaskPick q = mask_pick(m.w[0], k, r);
      CHECK(q.e == p.e && q.erased == p.erased.w[0] && q.rows == p.rows.w[0] && q.xor_only == p.xor_only);
      CHECK((p.erased.w[1] | p.erased.w[2] | p.erased.w[3] | p.rows.w[1] | p.rows.w[2] | p.rows.w[3]) == 0);
    }
  }
  if (narrow) {  // fec_mask.hpp on word 0, whatever the words above hold
    const uint64_t w = m.w[0];
    const MaskLosses n = mask_losses(w, k, r);
    CHECK(n.lost == l.lost && n.unrecoverable == l.unrecoverable);
    CHECK(mask_rows(w, k, r) == wide_mask_rows(m, k, r));
    CHECK(lost_data(w, k) == wide_lost_data(m, k).w[0] && lost_parity(w, k, r) == wide_lost_parity(m, k, r).w[0]);
    CHECK(alive_rows(w, k, r) == al.w[0] && (al.w[1] | al.w[2] | al.w[3]) == 0);
  }
  if (!helpers) return true;
  // the helpers under them
  for (uint32_t n = 0; n <= 256; ++n) {
    Bits low(256);
    uint32_t below = 0;
    for (uint32_t s = 0; s < n; ++s) low[s] = true, below += b[s];
    CHECK(same(wide_low_bits(n), low));
    CHECK(wide_count_below(m, n) == below);
  }
  for (uint32_t s = 0; s < 256; ++s) {
    Bits sh(256);
    for (uint32_t t = 0; t + s < 256; ++t) sh[t] = b[t + s];
    CHECK(same(wide_shift_right(m, s), sh));
  }
  return true;
}

WideMask drawn(uint32_t turn) {
  WideMask m{{rnd(), rnd(), rnd(), rnd()}};
  if (turn % 3 == 1)  // sparse
    for (auto& w : m.w) w &= rnd() & rnd();
  if (turn % 3 == 2)  // dense
    for (auto& w : m.w) w |= rnd() | rnd();
  return m;
}

WideMask with_bit(WideMask m, uint32_t s, bool on) {
  if (on) m.w[s / 64] |= 1ull << (s % 64);
  else m.w[s / 64] &= ~(1ull << (s % 64));
  return m;
}

}  // namespace

int main() {
  const uint32_t shapes[][2] = {{60, 5}, {64, 2}, {65, 3}, {127, 3}, {190, 5}, {224, 32}, {32, 224}, {255, 1}, {1, 255}, {10, 3}, {32, 32}};
  for (const auto& kr : shapes) {
    const uint32_t k = kr[0], r = kr[1];
    const bool narrow = k + r <= 64;
    uint64_t n = 0;
    std::vector<WideMask> planted;
    const WideMask none{{0, 0, 0, 0}}, all{{~0ull, ~0ull, ~0ull, ~0ull}};
    planted.push_back(none);
    planted.push_back(all);
    planted.push_back(wide_not(wide_low_bits(k + r)));  // only the ignored bits
    planted.push_back(wide_low_bits(k + r));            // only the read ones
    for (uint32_t s : {0u, 63u, 64u, 127u, 128u, 191u, 192u, 255u, k - 1, k, k + r - 1, k + r == 256 ? 255u : k + r}) {
      planted.push_back(with_bit(none, s, true));
      planted.push_back(with_bit(all, s, false));
    }
    for (const WideMask& m : planted) {
      if (!check(k, r, m, narrow, true)) return 1;
      ++n;
    }
    for (uint32_t turn = 0; turn < 300; ++turn) {
      if (!check(k, r, drawn(turn), narrow, turn < 30)) return 1;
      ++n;
    }
    std::printf("%u+%u %llu\n", k, r, static_cast<unsigned long long>(n));
  }
  std::printf("ok\n");
  return 0;
}
