// wide_deep_forms_test.cpp — what csrc/fec_forms.hpp decides for a wide call on a context in either
// rows mode (wide_route over wide_served and wide_rows_all_served; wide_deep_slot_stride,
// wide_deep_arena), with no GPU.  Arguments: quintuples "mode G k r P"; prints per quintuple
//   path=<WidePath as int> why=<WideRefusal as int> passes=<n> capped=<wide_served as int> all=<wide_rows_all_served as int>
// then per quadruple of the second list ("--arena budget G k r ..."):
//   per_chunk=<n> stride=<bytes> arena=<bytes> chunks=<n> arena_at=<at> bytes=<n>
// and "--ids": the numbers of WideDeepLaunchForm and the form bit.
// The test library's budget switch is read through plan_arena_budget when budget is 0.
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/wide_deep_forms_test.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fec_forms.hpp"
#include "fec_knobs.hpp"

using namespace qfec;

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--ids") == 0) {
    std::printf("build_records_deep %lld\n", static_cast<long long>(WideDeepLaunchForm::kBuildRecordsDeep));
    std::printf("decode_wide_deep %lld\n", static_cast<long long>(WideDeepLaunchForm::kDecodeWideDeep));
    std::printf("recover_scatter_wide_deep %lld\n", static_cast<long long>(WideDeepLaunchForm::kRecoverScatterWideDeep));
    std::printf("deep_record_bit %d\n", kDeepRecord);
    std::printf("pol_in_place %d\npol_slots %d\npol_table %d\n", kWideDeepPolInPlace, kWidePolSlots, kWideDeepTablePol);
    std::printf("ok\n");
    return 0;
  }
  int i = 1;
  for (; i + 4 < argc && std::strcmp(argv[i], "--arena") != 0; i += 5) {
    const int mode = std::atoi(argv[i]);
    const uint64_t G = std::strtoull(argv[i + 1], nullptr, 10);
    const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i + 2])), r = static_cast<uint32_t>(std::atoi(argv[i + 3]));
    const uint32_t P = static_cast<uint32_t>(std::atoi(argv[i + 4]));
    const WideRoute rt = wide_route(mode, G, k, r, P);
    std::printf("path=%d why=%d passes=%u capped=%d all=%d\n", static_cast<int>(rt.path), static_cast<int>(rt.why), rt.passes,
                static_cast<int>(wide_served(G, k, r, P)), static_cast<int>(wide_rows_all_served(G, k, r, P)));
  }
  if (i < argc && std::strcmp(argv[i], "--arena") == 0) {
    for (++i; i + 3 < argc; i += 4) {
      uint64_t budget = std::strtoull(argv[i], nullptr, 10);
      if (budget == 0) budget = plan_arena_budget();
      const uint64_t G = std::strtoull(argv[i + 1], nullptr, 10);
      const uint32_t k = static_cast<uint32_t>(std::atoi(argv[i + 2])), r = static_cast<uint32_t>(std::atoi(argv[i + 3]));
      const PlanArena a = wide_deep_arena(k, r, G, budget);
      const PlanWorkspace w = wide_workspace(G, a);
      if (a.stride != wide_deep_slot_stride(k, r) || a.bytes != a.per_chunk * a.stride || w.bytes != w.arena + a.bytes) return 1;
      uint64_t chunks = 0, seen = 0;
      plan_chunks(G, a.per_chunk, [&](uint64_t g0, uint64_t gn) {
        if (g0 != seen || gn == 0 || gn > a.per_chunk) return false;
        seen += gn, ++chunks;
        return chunks < 1000;  // 2^32 - 1 groups: the count is the division's
      });
      if (seen == G && chunks != (G + a.per_chunk - 1) / a.per_chunk) return 1;
      std::printf("per_chunk=%llu stride=%llu arena=%llu chunks=%llu arena_at=%llu bytes=%llu\n", (unsigned long long)a.per_chunk,
                  (unsigned long long)a.stride, (unsigned long long)a.bytes,
                  (unsigned long long)((G + a.per_chunk - 1) / a.per_chunk), (unsigned long long)w.arena,
                  (unsigned long long)w.bytes);
    }
  }
  std::printf("ok\n");
  return 0;
}
