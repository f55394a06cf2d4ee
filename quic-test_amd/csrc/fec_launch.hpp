// fec_launch.hpp — what the host launchers of the kernel translation units (fec_encode.hip,
// fec_decode.hip, fec_decode_fused.hip, fec_runs.hip, fec_server.hip, fec_util.hip, fec_gather.hip,
// fec_gather_var.hip, fec_scatter.hip, fec_scatter_encode.hip, fec_plan.hip, fec_wide.hip,
// fec_wide_table.hip, fec_wide_encode.hip, fec_wide_deep.hip, fec_packed.hip) share: the per-launch
// limits with their test switches, the chunk walk, the pass-and-chunk walk of the wave-per-group
// kernels, the row passes of the runtime-k encodes, the launch trace's record, and the small
// launch arguments more than one unit computes (knob, decode_swizzle, rank_meta).  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"  // RankMeta
#include "fec_forms.hpp"
#include "fec_knobs.hpp"

namespace qfec {

// A test-library switch (fec_knobs.hpp) as an int; `def` in the product library.
inline int knob(TestKnob k, int def) { return static_cast<int>(test_knob(k, def)); }

// XCD-aware group order for a decode kernel: at k=10 r=3 measured +10% for decode_fused and
// -1%..+5% for decode_wave over two boxes (tools/probe_decode.hip; tunable per kernel).
inline uint32_t decode_swizzle(const DecodeLaunch& a, int tuned) {
  return static_cast<uint32_t>(a.xcd_swizzle >= 0 ? a.xcd_swizzle : tuned);
}

namespace {
// Levels 1..3 of the codebook, all the mask-addressed kernels rank (RankMeta is internal to its
// translation unit, as all of fec_device.hpp).
inline RankMeta rank_meta(const LevelMeta& m) {
  RankMeta rm{};
  for (int e = 1; e <= 3; ++e) rm.base[e] = m.base[e], rm.stride[e] = m.stride[e], rm.count_r[e] = m.count_r[e];
  return rm;
}
}  // namespace

constexpr uint32_t kMaxThreadsPerLaunch = 1u << 30;
// Wave-per-group decode launches: 256-thread workgroups, so at most 2^22 of them keep the
// grid's work-item count (blocks * 256) inside 32 bits with room to spare.
constexpr uint64_t kMaxWaveBlocks = kMaxThreadsPerLaunch / 256u;
// Blocks per wave-per-group decode launch: kMaxWaveBlocks (the test library's
// TestKnob::kMaxWaveBlocks forces the chunked launches, which otherwise start only past 16.7M
// groups).
inline uint64_t max_wave_blocks() {
  const long n = test_knob(TestKnob::kMaxWaveBlocks, 0);
  return n > 0 && static_cast<uint64_t>(n) < kMaxWaveBlocks ? static_cast<uint64_t>(n) : kMaxWaveBlocks;
}
// Work items per launch of the kernels that map one item to a lane: kMaxThreadsPerLaunch (the
// test library's TestKnob::kMaxLaunchThreads lowers it, so the chunk loops, which otherwise
// start only past 2^30 items, run at a few thousand).
inline uint32_t max_launch_threads() {
  const long n = test_knob(TestKnob::kMaxLaunchThreads, 0);
  return n > 0 && static_cast<uint64_t>(n) < kMaxThreadsPerLaunch ? static_cast<uint32_t>(n) : kMaxThreadsPerLaunch;
}
// Groups per launch when each takes `per_group` work items (at least one group).
inline uint64_t groups_per_launch(uint32_t per_group) {
  const uint64_t n = max_launch_threads() / (per_group ? per_group : 1u);
  return n ? n : 1;
}

inline uint32_t blocks_for(uint64_t n) { return static_cast<uint32_t>((n + 255) / 256); }

// The launch trace's record (fec_knobs.hpp; trace_launch() is empty in the product library).
inline LaunchRecord launch_record(int64_t form, uint64_t grid, uint32_t block, uint64_t first_item, uint64_t items) {
  LaunchRecord t{};
  t.form = form;
  t.grid = static_cast<int64_t>(grid);
  t.block = block;
  t.first_item = static_cast<int64_t>(first_item);
  t.items = static_cast<int64_t>(items);
  return t;
}
inline LaunchRecord launch_record(LaunchForm form, uint64_t grid, uint32_t block, uint64_t first_item, uint64_t items) {
  return launch_record(static_cast<int64_t>(form), grid, block, first_item, items);
}

// Walks `n` items in pieces of at most `per`: launch(first, count) traces and launches one
// piece; stops at the first launch error.
template <typename F>
hipError_t for_chunks(uint64_t n, uint64_t per, F launch) {
  for (uint64_t i0 = 0; i0 < n; i0 += per) {
    launch(i0, n - i0 < per ? n - i0 : per);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The launches of a wave-per-group kernel (4 groups per 256-lane workgroup) that rebuilds `maxe`
// rows per pass: for every pass of rows [m0, m0 + maxe) below r (e <= r), all groups in chunks of
// whole workgroups, at most max_wave_blocks() per launch; every chunk of a pass before the next
// pass.  launch(first group, groups, workgroups, m0) traces and launches one chunk.
template <typename F>
hipError_t for_wave_passes(uint64_t groups, uint32_t r, uint32_t maxe, F launch) {
  for (uint32_t m0 = 0; m0 < r; m0 += maxe) {
    const hipError_t e = for_chunks(groups, max_wave_blocks() * 4, [&](uint64_t g0, uint64_t gn) {
      launch(g0, gn, (gn + 3) / 4, m0);
    });
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// The walk of a call whose records are built on the device (fec_forms.hpp PlanLaunch): every group
// classified once, then chunk after chunk of the arena's per_chunk groups: build(first group,
// groups) launches build_records for the chunk, consume(first group, groups) every row pass of the
// call's kernel on it -- in stream order, so the arena is free again when the next chunk's records
// are written.  Each returns its error; stops at the first.
template <typename C, typename B, typename F>
hipError_t for_plan_chunks(uint64_t groups, uint64_t per_chunk, C classify, B build, F consume) {
  hipError_t e = classify();
  if (e != hipSuccess) return e;
  plan_chunks(groups, per_chunk, [&](uint64_t g0, uint64_t gn) {
    e = build(g0, gn);
    if (e == hipSuccess) e = consume(g0, gn);
    return e == hipSuccess;
  });
  return e;
}

// The passes of a runtime-k encode over its r parity rows (fec_forms.hpp encode_pass_rows), in row
// order: launch(row0, rows, first) launches pass [row0, row0 + rows), every chunk of it, and
// returns its error; `first`: the pass that owns the XOR row.  Stops at the first error.
template <typename F>
hipError_t for_row_passes(uint32_t r, F launch) {
  for (uint32_t row0 = 0; row0 < r; row0 += kEncodePassRows) {
    const hipError_t e = launch(row0, encode_pass_rows(r, row0 / kEncodePassRows), row0 == 0);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace qfec
