// workspace_dump.cpp — prints how a call carves the caller stream's workspace (csrc/fec_shim.cpp
// stream_workspace), with no GPU: one line per query,
//   "<id> G=<G> rec_off=<off> masks=<off> symlen=<off> arena=<off> bytes=<n> stride=<n> per_chunk=<n>"
// byte offsets from the start of the buffer.  A region the layout does not have is empty: its offset
// is the next region's (so masks = symlen, symlen = arena, arena = bytes); a layout without a record
// arena has stride = per_chunk = 0.  tests/test_cross_family_layout.py asserts, from these lines, that
// the sequences of tests/test_gpu_cross_family.py put one family's regions under another's.
//
//   workspace_dump  <id> <layout> <k> <r> <G> <own_masks> <own_symlen> <budget>  ...   (eight per query)
//
// <budget>: the record arena's budget in bytes, 0 = kPlanArenaBytes (what the product library has).
// <layout> and where its sizes come from:
//   prefix      fec_recover_batch_rs_dev_packed's block sums, restated from fec_runs.hip
//               rows_prefix_workspace_bytes (a .hip file: not for a host program to include):
//               ceil(G / kRowsPerBlock) u32 with kRowsPerBlock = 256 * kRowsPerThread = 1024.  Printed
//               in the rec_off column: the block sums are the first and only region.
//   offsets     G u32 record offsets, restated from fec_shim.cpp decode_dev_locked and
//               table_recover_locked with ws_words = 1: "stream_workspace(ctx, s, G * sizeof(uint32_t), &ws)".
//   offsets2    the scatter recover that keeps its own symbol lengths, restated from fec_shim.cpp
//               table_recover_locked with ws_words = 2: "ws_words * G * sizeof(uint32_t)" bytes and
//               "a.symlen = a.rec_off + G".
//   plan        plan_arena, plan_workspace(G, own_masks, own_symlen)
//   wide        wide_arena, wide_workspace
//   wide_table  wide_arena, wide_table_workspace(G, own_masks, own_symlen)
//   deep        wide_deep_arena, wide_workspace
//   deep_table  wide_deep_arena, wide_table_workspace(G, own_masks, own_symlen)
// tests/test_cross_family_layout.py checks that the restated lines are still in those files.
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/workspace_dump.cpp quic-test_amd/csrc/fec_knobs.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fec_forms.hpp"

using namespace qfec;

namespace {

constexpr uint64_t kRowsPerBlock = 256 * 4;  // fec_runs.hip kRowsPerBlock = 256 * kRowsPerThread

struct Line {
  PlanWorkspace w;
  PlanArena a;
};

Line flat(uint64_t rec_off_bytes, uint64_t symlen_bytes) {
  Line l{};
  l.w.rec_off = 0;
  l.w.masks = l.w.symlen = rec_off_bytes;
  l.w.arena = l.w.bytes = rec_off_bytes + symlen_bytes;
  return l;
}

bool layout(const char* kind, uint32_t k, uint32_t r, uint64_t G, bool own_masks, bool own_symlen, uint64_t budget,
            Line* out) {
  if (!std::strcmp(kind, "prefix")) {
    *out = flat(((G + kRowsPerBlock - 1) / kRowsPerBlock) * sizeof(uint32_t), 0);
  } else if (!std::strcmp(kind, "offsets")) {
    *out = flat(G * sizeof(uint32_t), 0);
  } else if (!std::strcmp(kind, "offsets2")) {
    *out = flat(G * sizeof(uint32_t), G * sizeof(uint32_t));
  } else if (!std::strcmp(kind, "plan")) {
    out->a = plan_arena(k, r, G, budget);
    out->w = plan_workspace(G, own_masks, own_symlen, out->a);
  } else if (!std::strcmp(kind, "wide") || !std::strcmp(kind, "deep")) {
    out->a = kind[0] == 'w' ? wide_arena(k, r, G, budget) : wide_deep_arena(k, r, G, budget);
    out->w = wide_workspace(G, out->a);
  } else if (!std::strcmp(kind, "wide_table") || !std::strcmp(kind, "deep_table")) {
    out->a = kind[0] == 'w' ? wide_arena(k, r, G, budget) : wide_deep_arena(k, r, G, budget);
    out->w = wide_table_workspace(G, own_masks, own_symlen, out->a);
  } else {
    return false;
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 9 || (argc - 1) % 8 != 0) {
    std::fprintf(stderr, "usage: workspace_dump <id> <layout> <k> <r> <G> <own_masks> <own_symlen> <budget> ...\n");
    return 2;
  }
  for (int i = 1; i < argc; i += 8) {
    const uint32_t k = static_cast<uint32_t>(std::strtoul(argv[i + 2], nullptr, 10));
    const uint32_t r = static_cast<uint32_t>(std::strtoul(argv[i + 3], nullptr, 10));
    const uint64_t G = std::strtoull(argv[i + 4], nullptr, 10);
    const bool own_masks = std::atoi(argv[i + 5]) != 0, own_symlen = std::atoi(argv[i + 6]) != 0;
    uint64_t budget = std::strtoull(argv[i + 7], nullptr, 10);
    if (budget == 0) budget = kPlanArenaBytes;
    Line l{};
    if (G == 0 || !layout(argv[i + 1], k, r, G, own_masks, own_symlen, budget, &l)) {
      std::fprintf(stderr, "%s: unknown layout %s or no groups\n", argv[i], argv[i + 1]);
      return 1;
    }
    std::printf("%s G=%llu rec_off=%llu masks=%llu symlen=%llu arena=%llu bytes=%llu stride=%llu per_chunk=%llu\n", argv[i],
                static_cast<unsigned long long>(G), static_cast<unsigned long long>(l.w.rec_off),
                static_cast<unsigned long long>(l.w.masks), static_cast<unsigned long long>(l.w.symlen),
                static_cast<unsigned long long>(l.w.arena), static_cast<unsigned long long>(l.w.bytes),
                static_cast<unsigned long long>(l.a.stride), static_cast<unsigned long long>(l.a.per_chunk));
  }
  return 0;
}
