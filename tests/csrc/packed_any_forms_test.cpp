// packed_any_forms_test.cpp — the route and the workspace of the packed recovers for every shape
// (csrc/fec_forms.hpp packed_route, packed_wide_route, packed_arena, packed_workspace), with no GPU.
// Arguments, any number of commands:
//   route <wide 0|1> <bits> <G> <k> <r> <P>
//       prints  path=<PackedPath as int> why=<PackedRefusal as int> passes=<n> dense=<0|1>
//       bits: kPackedPlanDevice 1, kPackedRowsAll 4; the one-word call's kPackedDense (2) is added
//       here, from gf256.hpp's codebook_layout under the library's 2 GiB cap, as the shim adds it
//   delegates <k> <r> <Pmax>
//       prints  delegates=<a>-<b>,...  the packet sizes in [1, Pmax] whose one-word route at G = 1031
//       is kDelegate, as closed ranges
//   workspace <PackedPath as int> <G> <k> <r> <budget>      (budget 0: plan_arena_budget())
//       prints  block_sums=<at> rec_off=<at> arena=<at> bytes=<n> per_chunk=<n> stride=<n>
// The program itself checks, for every workspace, what does not depend on the numbers' values: the
// regions in order and disjoint, the u32 arrays 8-B and the arena 256-B aligned, the total the sum,
// and for every route that a served path is one of the enum's and a refusal has path kRefused.
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/packed_any_forms_test.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fec_forms.hpp"
#include "gf256.hpp"

using namespace qfec;

static int fail(const char* what) {
  std::printf("FAIL %s\n", what);
  return 1;
}

static bool dense(uint32_t k, uint32_t r) {
  CodebookLayout layout;
  return codebook_layout(k, r, 2ull << 30, layout);
}

int main(int argc, char** argv) {
  const auto u64 = [&](int i) { return std::strtoull(argv[i], nullptr, 10); };
  const auto u32 = [&](int i) { return static_cast<uint32_t>(std::strtoul(argv[i], nullptr, 10)); };
  for (int i = 1; i < argc;) {
    if (std::strcmp(argv[i], "route") == 0 && i + 6 < argc) {
      const bool wide = u32(i + 1) != 0;
      int bits = static_cast<int>(u32(i + 2));
      const uint64_t G = u64(i + 3);
      const uint32_t k = u32(i + 4), r = u32(i + 5), P = u32(i + 6);
      const bool d = !wide && dense(k, r);
      if (d) bits |= kPackedDense;
      const PackedRoute rt = wide ? packed_wide_route(bits, G, k, r, P) : packed_route(bits, G, k, r, P);
      if ((rt.path == PackedPath::kRefused) != (rt.why != PackedRefusal::kServed)) return fail("refusal without a reason");
      if (static_cast<int>(rt.path) < 0 || static_cast<int>(rt.path) > static_cast<int>(PackedPath::kDeep)) return fail("path");
      const bool consumer = rt.path == PackedPath::kCodebook || rt.path == PackedPath::kDevicePlan ||
                            rt.path == PackedPath::kWide || rt.path == PackedPath::kDeep;
      if (consumer != (rt.passes != 0) || (consumer && rt.passes != packed_passes(k, r))) return fail("passes");
      if (wide && (rt.path == PackedPath::kEmpty || rt.path == PackedPath::kDelegate || rt.path == PackedPath::kCodebook ||
                   rt.path == PackedPath::kDevicePlan))
        return fail("a one-word path for the wide call");
      if (!wide && (rt.path == PackedPath::kWide || rt.path == PackedPath::kDeep)) return fail("a wide path for the one-word call");
      std::printf("path=%d why=%d passes=%u dense=%d\n", static_cast<int>(rt.path), static_cast<int>(rt.why), rt.passes, d ? 1 : 0);
      i += 7;
    } else if (std::strcmp(argv[i], "delegates") == 0 && i + 3 < argc) {
      const uint32_t k = u32(i + 1), r = u32(i + 2), pmax = u32(i + 3);
      const int bits = dense(k, r) ? kPackedDense : 0;
      std::printf("delegates=");
      bool open = false, any = false;
      uint32_t from = 0;
      for (uint32_t P = 1; P <= pmax + 1; ++P) {
        const bool del = P <= pmax && packed_route(bits, 1031, k, r, P).path == PackedPath::kDelegate;
        if (del != (P <= pmax && packed_old_serves(1031, k, r, P) && P >= kVecMinP)) return fail("delegate is not the old call's rule");
        if (del && !open) from = P, open = true;
        if (!del && open) {
          std::printf("%s%u-%u", any ? "," : "", from, P - 1);
          open = false, any = true;
        }
      }
      std::printf("\n");
      i += 4;
    } else if (std::strcmp(argv[i], "workspace") == 0 && i + 5 < argc) {
      const PackedPath path = static_cast<PackedPath>(u32(i + 1));
      const uint64_t G = u64(i + 2);
      const uint32_t k = u32(i + 3), r = u32(i + 4);
      uint64_t budget = u64(i + 5);
      if (budget == 0) budget = plan_arena_budget();
      const PlanArena a = packed_arena(path, k, r, G, budget);
      const PackedWorkspace w = packed_workspace(G, a);
      const uint64_t blocks = (G + kPackedRowsPerBlock - 1) / kPackedRowsPerBlock;
      if (path == PackedPath::kCodebook) {
        if (a.bytes != 0 || a.per_chunk != 0 || a.stride != 0) return fail("the codebook path has no arena");
      } else {
        if (a.per_chunk == 0 || a.per_chunk > G || a.bytes != a.per_chunk * a.stride || a.stride % 32 != 0) return fail("arena");
        if ((a.per_chunk - 1) * (a.stride / 32u) >= kPlanRecLimit) return fail("record offset");
      }
      // in order, disjoint, aligned, the total the sum
      if (w.block_sums != 0 || w.block_sums % 8 != 0) return fail("block sums");
      if (w.rec_off < w.block_sums + blocks * 4 || w.rec_off % 8 != 0 || w.rec_off - blocks * 4 >= 8) return fail("record offsets");
      if (w.arena < w.rec_off + G * 4 || w.arena % 256 != 0 || w.arena - (w.rec_off + G * 4) >= 256) return fail("arena offset");
      if (w.bytes != w.arena + a.bytes) return fail("total");
      std::printf("block_sums=%llu rec_off=%llu arena=%llu bytes=%llu per_chunk=%llu stride=%llu\n",
                  (unsigned long long)w.block_sums, (unsigned long long)w.rec_off, (unsigned long long)w.arena,
                  (unsigned long long)w.bytes, (unsigned long long)a.per_chunk, (unsigned long long)a.stride);
      i += 6;
    } else {
      return fail("arguments");
    }
  }
  std::printf("ok\n");
  return 0;
}
