// wide_forms_test.cpp — the served-shape rule and the arena arithmetic of the wide calls
// (csrc/fec_forms.hpp wide_served, wide_slot_stride, wide_arena, wide_workspace, wide_passes), with
// no GPU.  Arguments: quadruples "G k r P"; prints per quadruple
//   served=<WideRefusal as int> stride=<bytes> passes=<n>
// then per triple of the second list ("--arena budget G k r ..."):
//   per_chunk=<n> arena=<bytes> rec_off=<at> arena_at=<at> bytes=<n>
// The test library's budget switch is read through plan_arena_budget when budget is 0.
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/wide_forms_test.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fec_forms.hpp"

using namespace qfec;

int main(int argc, char** argv) {
  int i = 1;
  for (; i + 3 < argc && std::strcmp(argv[i], "--arena") != 0; i += 4) {
    const uint64_t G = std::strtoull(argv[i], nullptr, 10);
    const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i + 1])), r = static_cast<uint32_t>(std::atoi(argv[i + 2]));
    const uint32_t P = static_cast<uint32_t>(std::atoi(argv[i + 3]));
    std::printf("served=%d stride=%llu passes=%u\n", static_cast<int>(wide_served(G, k, r, P)),
                static_cast<unsigned long long>(wide_slot_stride(k, r)), wide_passes(k, r));
  }
  if (i < argc && std::strcmp(argv[i], "--arena") == 0) {
    for (++i; i + 3 < argc; i += 4) {
      uint64_t budget = std::strtoull(argv[i], nullptr, 10);
      if (budget == 0) budget = plan_arena_budget();
      const uint64_t G = std::strtoull(argv[i + 1], nullptr, 10);
      const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i + 2])), r = static_cast<uint32_t>(std::atoi(argv[i + 3]));
      const PlanArena a = wide_arena(k, r, G, budget);
      const PlanWorkspace w = wide_workspace(G, a);
      if (a.stride != wide_slot_stride(k, r) || a.bytes != a.per_chunk * a.stride || w.bytes != w.arena + a.bytes) return 1;
      std::printf("per_chunk=%llu arena=%llu rec_off=%llu arena_at=%llu bytes=%llu\n", (unsigned long long)a.per_chunk,
                  (unsigned long long)a.bytes, (unsigned long long)w.rec_off, (unsigned long long)w.arena,
                  (unsigned long long)w.bytes);
    }
  }
  std::printf("ok\n");
  return 0;
}
