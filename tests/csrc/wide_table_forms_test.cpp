// wide_table_forms_test.cpp — the workspace and the chunk walk of the wide address-table recover
// (csrc/fec_forms.hpp wide_table_workspace over wide_arena; plan_chunks), with no GPU.  Arguments:
//   "G k r P" quadruples: prints  served=<WideRefusal as int>
//   "--workspace budget G k r own_masks own_symlen ..." sextuples (budget 0: plan_arena_budget()):
//     per_chunk=<n> stride=<bytes> rec_off=<at> masks=<at> symlen=<at> arena=<at> bytes=<n> chunks=<n> passes=<n>
// The program itself checks, for every sextuple, what does not depend on the numbers' values: the
// regions in order and disjoint, each aligned as plan_workspace aligns (masks 8, arena 256), the
// totals, every record offset below the markers, and that plan_chunks covers [0, G) once, in order,
// in pieces of at most per_chunk (counted arithmetically past 1M chunks).
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/wide_table_forms_test.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fec_forms.hpp"

using namespace qfec;

static int fail(const char* what) {
  std::printf("FAIL %s\n", what);
  return 1;
}

int main(int argc, char** argv) {
  int i = 1;
  for (; i + 3 < argc && std::strcmp(argv[i], "--workspace") != 0; i += 4) {
    const uint64_t G = std::strtoull(argv[i], nullptr, 10);
    const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i + 1])), r = static_cast<uint32_t>(std::atoi(argv[i + 2]));
    const uint32_t P = static_cast<uint32_t>(std::atoi(argv[i + 3]));
    std::printf("served=%d\n", static_cast<int>(wide_served(G, k, r, P)));
  }
  if (i < argc && std::strcmp(argv[i], "--workspace") == 0) {
    for (++i; i + 5 < argc; i += 6) {
      uint64_t budget = std::strtoull(argv[i], nullptr, 10);
      if (budget == 0) budget = plan_arena_budget();
      const uint64_t G = std::strtoull(argv[i + 1], nullptr, 10);
      const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i + 2])), r = static_cast<uint32_t>(std::atoi(argv[i + 3]));
      const bool own_masks = std::atoi(argv[i + 4]) != 0, own_symlen = std::atoi(argv[i + 5]) != 0;
      if (wide_served(G, k, r, 16) != WideRefusal::kServed) return fail("a workspace is asked for a served call only");
      const PlanArena a = wide_arena(k, r, G, budget);
      const PlanWorkspace w = wide_table_workspace(G, own_masks, own_symlen, a);
      if (a.stride != wide_slot_stride(k, r) || a.bytes != a.per_chunk * a.stride) return fail("arena");
      if (a.per_chunk == 0 || a.per_chunk > G) return fail("per_chunk");
      // in order, disjoint, aligned
      if (w.rec_off != 0 || w.masks < G * 4 || w.masks % 8 != 0) return fail("record offsets");
      if (w.symlen != w.masks + (own_masks ? G * 32 : 0)) return fail("masks");
      if (w.arena < w.symlen + (own_symlen ? G * 4 : 0) || w.arena % 256 != 0 || w.arena - w.symlen - (own_symlen ? G * 4 : 0) >= 256)
        return fail("symbol lengths");
      if (w.bytes != w.arena + a.bytes) return fail("total");
      // the workspace with both regions empty is the wide calls'
      const PlanWorkspace plain = wide_workspace(G, a), none = wide_table_workspace(G, false, false, a);
      if (plain.arena != none.arena || plain.bytes != none.bytes || plain.masks != none.masks) return fail("wide_workspace");
      // the last slot's record offset is below the markers
      if ((a.per_chunk - 1) * (a.stride / 32u) >= kPlanRecLimit || a.stride % 32 != 0) return fail("record offset");
      // the walk
      uint64_t chunks = 0;
      if (G / a.per_chunk > (1u << 20)) {
        chunks = (G + a.per_chunk - 1) / a.per_chunk;
      } else {
        uint64_t next = 0;
        const bool done = plan_chunks(G, a.per_chunk, [&](uint64_t g0, uint64_t gn) {
          if (g0 != next || gn == 0 || gn > a.per_chunk) return false;
          next += gn, ++chunks;
          return true;
        });
        if (!done || next != G) return fail("plan_chunks");
      }
      std::printf("per_chunk=%llu stride=%llu rec_off=%llu masks=%llu symlen=%llu arena=%llu bytes=%llu chunks=%llu passes=%u\n",
                  (unsigned long long)a.per_chunk, (unsigned long long)a.stride, (unsigned long long)w.rec_off,
                  (unsigned long long)w.masks, (unsigned long long)w.symlen, (unsigned long long)w.arena,
                  (unsigned long long)w.bytes, (unsigned long long)chunks, wide_passes(k, r));
    }
  }
  std::printf("ok\n");
  return 0;
}
