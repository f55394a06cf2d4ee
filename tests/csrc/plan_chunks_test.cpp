// plan_chunks_test.cpp — the sizes and the walk of a device-plan call (csrc/fec_forms.hpp
// plan_slot_stride, plan_arena, plan_slot_rec, plan_chunks, plan_workspace), with no GPU.
//
// For each shape, each arena budget (64 MiB; one slot; one slot and a byte; five slots) and each G
// in {1, 4, 5, 67, 2^32 - 1} it checks and prints one line
//   "k=<k> r=<r> budget=<bytes> G=<G> | stride=<..> per_chunk=<..> arena=<..> chunks=<..> last=<..>
//    ws=rec_off:<off>,masks:<off>,symlen:<off>,arena:<off>,bytes:<..>"
// (the workspace with both optional regions present), then "ok".  Checked:
//   * the slot stride is record_bytes(k, min(k, r)) (gf256.hpp), a multiple of 32;
//   * the chunks plan_chunks hands out tile [0, G): in order, each of 1..per_chunk groups, ending at
//     G (walked in full up to 2^20 chunks; beyond that the first 2^20 are walked and the count and
//     the last chunk come from ceil(G / per_chunk));
//   * the largest record of the last slot of a chunk ends inside the arena, and the arena takes no
//     more than max(budget, one slot);
//   * every slot's rec_off, in 32-B units, is below kRecBad and names the slot's byte offset;
//   * the workspace regions -- with and without the masks, with and without the symbol lengths --
//     follow each other without overlap, the masks 8-B and the arena 256-B aligned, inside `bytes`.
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/plan_chunks_test.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdint>
#include <cstdio>

#include "fec_forms.hpp"
#include "gf256.hpp"

using namespace qfec;

namespace {

#define REQUIRE(cond)                                                                                       \
  do {                                                                                                      \
    if (!(cond)) {                                                                                          \
      std::fprintf(stderr, "k=%u r=%u budget=%llu G=%llu: %s\n", k, r, static_cast<unsigned long long>(budget), \
                   static_cast<unsigned long long>(G), #cond);                                              \
      return false;                                                                                         \
    }                                                                                                       \
  } while (0)

bool check(uint32_t k, uint32_t r, uint64_t budget, uint64_t G) {
  const uint32_t emax = k < r ? k : r;
  const PlanArena a = plan_arena(k, r, G, budget);
  REQUIRE(a.stride == record_bytes(k, emax) && a.stride == plan_slot_stride(k, r) && a.stride % 32 == 0);
  REQUIRE(a.per_chunk >= 1 && a.per_chunk <= G);
  REQUIRE(a.bytes == a.per_chunk * a.stride && a.bytes <= (budget > a.stride ? budget : a.stride));
  REQUIRE(a.per_chunk == G || (a.per_chunk + 1) * a.stride > budget);  // as many slots as the budget holds
  // the walk
  const uint64_t chunks = (G + a.per_chunk - 1) / a.per_chunk, last = G - (chunks - 1) * a.per_chunk;
  REQUIRE(last >= 1 && last <= a.per_chunk);
  const uint64_t kWalk = 1ull << 20;
  uint64_t next = 0, seen = 0;
  bool tiles = true;
  plan_chunks(G, a.per_chunk, [&](uint64_t g0, uint64_t gn) {
    tiles = tiles && g0 == next && gn >= 1 && gn <= a.per_chunk && g0 + gn <= G && (gn == a.per_chunk || g0 + gn == G);
    next = g0 + gn;
    return tiles && ++seen < kWalk;
  });
  REQUIRE(tiles);
  REQUIRE(chunks > kWalk ? seen == kWalk && next == kWalk * a.per_chunk : seen == chunks && next == G);
  // the slots: the first, the last, and a stride of them in between
  const uint64_t step = a.per_chunk > 4096 ? a.per_chunk / 4096 : 1;
  for (uint64_t i = 0; i < a.per_chunk; i = (i + step < a.per_chunk || i == a.per_chunk - 1) ? i + step : a.per_chunk - 1) {
    REQUIRE(i * a.stride + record_bytes(k, emax) <= a.bytes);
    REQUIRE(i * (a.stride / 32) < kPlanRecLimit);
    REQUIRE(uint64_t{plan_slot_rec(a, i)} * 32 == i * a.stride);
  }
  // the workspace
  for (int own = 0; own < 4; ++own) {
    const bool masks = own & 1, symlen = own & 2;
    const PlanWorkspace w = plan_workspace(G, masks, symlen, a);
    REQUIRE(w.rec_off == 0 && w.masks >= w.rec_off + G * 4 && w.masks % 8 == 0);
    REQUIRE(w.symlen >= w.masks + (masks ? G * 8 : 0) && w.symlen % 4 == 0);
    REQUIRE(w.arena >= w.symlen + (symlen ? G * 4 : 0) && w.arena % 256 == 0);
    REQUIRE(w.bytes == w.arena + a.bytes);
  }
  const PlanWorkspace w = plan_workspace(G, true, true, a);
  std::printf("k=%u r=%u budget=%llu G=%llu | stride=%llu per_chunk=%llu arena=%llu chunks=%llu last=%llu "
              "ws=rec_off:%llu,masks:%llu,symlen:%llu,arena:%llu,bytes:%llu\n",
              k, r, static_cast<unsigned long long>(budget), static_cast<unsigned long long>(G),
              static_cast<unsigned long long>(a.stride), static_cast<unsigned long long>(a.per_chunk),
              static_cast<unsigned long long>(a.bytes), static_cast<unsigned long long>(chunks),
              static_cast<unsigned long long>(last), static_cast<unsigned long long>(w.rec_off),
              static_cast<unsigned long long>(w.masks), static_cast<unsigned long long>(w.symlen),
              static_cast<unsigned long long>(w.arena), static_cast<unsigned long long>(w.bytes));
  return true;
}

}  // namespace

int main() {
  if (plan_arena_budget() != kPlanArenaBytes || kPlanArenaBytes != (64ull << 20)) {
    std::fprintf(stderr, "the default budget is not 64 MiB\n");
    return 1;
  }
  const uint32_t shapes[][2] = {{4, 2},  {5, 5},  {10, 3}, {12, 12}, {20, 7}, {24, 6},
                                {16, 16}, {32, 8}, {60, 4}, {30, 20}, {32, 32}};
  for (const auto& kr : shapes) {
    const uint64_t slot = plan_slot_stride(kr[0], kr[1]);
    for (uint64_t budget : {kPlanArenaBytes, slot, slot + 1, 5 * slot})
      for (uint64_t G : {1ull, 4ull, 5ull, 67ull, (1ull << 32) - 1})
        if (!check(kr[0], kr[1], budget, G)) return 1;
  }
  std::printf("ok\n");
  return 0;
}
