// fec_kernels.hpp — launch interface between the C-ABI shim (fec_shim.cpp) and the
// gfx950 kernels, one translation unit per kernel family: fec_encode.hip, fec_decode.hip,
// fec_decode_fused.hip, fec_runs.hip, fec_server.hip, fec_util.hip; the address-table units
// fec_gather.hip, fec_gather_var.hip, fec_scatter.hip, fec_scatter_encode.hip with their shared
// fec_table.hpp; fec_plan.hip; fec_wide.hip; fec_wide_table.hip; fec_wide_encode.hip; fec_wide_deep.hip;
// fec_packed.hip.  Internal to libfec_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_forms.hpp"   // launch descriptions and the choice of kernel form
#include "fec_server.hpp"  // the resident encoder's ring protocol

namespace qfec {

// Tuned occupancy caps (waves per CU) of the streaming kernels: fewer concurrent waves
// than the hardware allows keep the HBM request stream more local and measured faster
// (tools/probe_encode.hip, tools/probe_decode.hip).
// Encode: 2 workgroups per CU (k=10/1200 B: 2 x 5 waves, 5.70 vs 5.26 TB/s uncapped;
// 1024 B: 2 x 4 waves 6.12 vs 5.92 at 3; 1216 B: 2 x 6 waves 5.92 vs 5.25 at 1); one more
// for r >= 4 (k=20 r=5: 5.47 at 3 vs 4.99 at 2); none for the runtime-k kernel
// (k=10 r=2: 5.61 uncapped vs 3.66 at 2).  profiles/r01_encode_blocks_sweep.txt.
constexpr int kEncodeBlocksPerCU = 2;
constexpr int kEncodeXorWavesPerCU = 15;  // r = 1 (XOR row only), rounded to whole workgroups
constexpr int kDecodeWavesPerCU = 0;   // measured: any cap below ~20 waves/CU is slower

// Dynamic LDS bytes that cap a workgroup of `waves_per_block` waves at about
// `waves_per_cu` waves per CU (160 KiB LDS per CU); 0 = no cap.
inline uint32_t occupancy_cap_lds(int waves_per_cu, uint32_t waves_per_block) {
  if (waves_per_cu <= 0 || waves_per_block == 0) return 0;
  // nearest whole number of workgroups (a 6-wave workgroup under a 10-wave cap gets 2, not 1)
  uint32_t blocks = (static_cast<uint32_t>(waves_per_cu) + waves_per_block / 2) / waves_per_block;
  if (blocks == 0) blocks = 1;
  if (blocks * waves_per_block >= 32) return 0;
  return 160u * 1024u / (blocks + 1) + 16u;
}

constexpr int kDecodeFusedXcdSwizzle = 1;  // tuned per kernel (fec_launch.hpp decode_swizzle)
constexpr int kDecodeWaveXcdSwizzle = 1;

// The contiguous encodes (fec_encode.hip).
hipError_t launch_encode(const EncodeLaunch& a, hipStream_t s);
// The record- and mask-addressed decodes (fec_decode.hip): the plan-chunk walk, the checks, the
// classify launch and the dispatch of decode_form's choice.  Its decode_fused forms are a unit of
// their own (fec_decode_fused.hip), entered through launch_decode_fused with the form launch_decode
// chose (f.kernel == DecodeKernel::kFused); nothing else calls it.
hipError_t launch_decode(const DecodeLaunch& a, hipStream_t s);
hipError_t launch_decode_fused(const DecodeLaunch& a, const DecodeForm& f, hipStream_t s);
// Recover from an address table (fec_gather.hip): the classify scan (fec_table.hpp classify_table,
// one kernel template for the three table recovers, traced under each call's own classify form),
// then table_recover_form's recover_gather.
hipError_t launch_recover_gather(const TableRecoverLaunch& a, hipStream_t s);
// The same with a length per table entry (fec_gather_var.hip): classify_table with the lengths, then
// table_recover_form's recover_gather_var; and the encode from addresses and lengths, 0 = absent:
// table_encode_form's passes of encode_gather_var.
hipError_t launch_recover_gather_var(const TableRecoverLaunch& a, hipStream_t s);
hipError_t launch_encode_gather_var(const TableEncodeLaunch& a, hipStream_t s);
// Recover from an address table into a table of destinations (fec_scatter.hip): classify_table
// with a nullable length table, then table_recover_form's recover_scatter.
hipError_t launch_recover_scatter(const TableRecoverLaunch& a, hipStream_t s);
// Encode from an address table (with a nullable length table) into a table of destinations
// (fec_scatter_encode.hip): table_encode_form's passes of encode_scatter.
hipError_t launch_encode_scatter(const TableEncodeLaunch& a, hipStream_t s);
// The records of one plan chunk built on the device (fec_plan.hip build_records): for each of the
// `groups` groups from masks / rec_off / status (the chunk's first entries) whose rec_off the
// classify left below kRecBad, the record of its mask into slot i of p.arena and rec_off[i] = its
// place there; a group whose build meets a zero pivot gets kRecBad and status 1.  first_group: the
// chunk's place in the call, for the launch trace.
hipError_t launch_build_records(const PlanLaunch& p, const uint64_t* masks, uint32_t* rec_off, uint8_t* status,
                                uint64_t first_group, uint64_t groups, uint32_t k, uint32_t r, hipStream_t s);
// The wide calls (fec_wide.hip; k + r <= 256, four mask words per group): classify_wide over every
// group, then per chunk of a.plan's arena build_records_wide and wide_passes(k, r) launches of
// decode_wide, in stream order.
hipError_t launch_decode_wide(const WideLaunch& a, hipStream_t s);
// The wide records of one plan chunk (fec_wide.hip build_records_wide), as launch_build_records for
// the one-word shapes: groups [first_group, first_group + groups) of the call whose masks (four words
// per group), rec_off and status start at group 0, group first_group + i into slot i of p.arena.
hipError_t launch_build_records_wide(const PlanLaunch& p, const uint64_t* masks, uint32_t* rec_off, uint8_t* status,
                                     uint64_t first_group, uint64_t groups, uint32_t k, uint32_t r, hipStream_t s);
// The wide recover from an address table into a table of destinations (fec_wide_table.hip):
// classify_table_wide over every group, then per chunk of a.plan's arena build_records_wide and
// wide_passes(k, r) launches of recover_scatter_wide, in stream order.
hipError_t launch_recover_scatter_wide(const WideTableLaunch& a, hipStream_t s);
// The wide encode from an address table into a table of destinations (fec_wide_encode.hip):
// wide_encode_form's passes of encode_scatter_wide; no classify, no record, no workspace.
hipError_t launch_encode_scatter_wide(const WideEncodeLaunch& a, hipStream_t s);
// The wide calls for a shape past the wide builder's rows, min(k, r) > 32 (fec_wide_deep.hip; a
// context in FEC_WIDE_ROWS_ALL, fec_forms.hpp wide_route): the same walk as launch_decode_wide and
// launch_recover_scatter_wide with a.plan sized by wide_deep_arena -- the unchanged classify, then
// per chunk build_records_deep (one workgroup per group) and wide_passes(k, r) launches of the
// consumer: decode_wide over the deep record in place, the wide path's own decode_wide into slots,
// recover_scatter_wide over the deep record to a table of destinations.
hipError_t launch_decode_wide_deep(const WideLaunch& a, hipStream_t s);
hipError_t launch_recover_scatter_wide_deep(const WideTableLaunch& a, hipStream_t s);
// What fec_wide_deep.hip calls in the units of the kernels it shares: classify_wide over every group
// of the call and the row passes of decode_wide over groups [first_group, first_group + groups) of a
// deep call (fec_wide.hip: in place the instantiation over the deep record, into slots the wide
// path's own); classify_table_wide and the row passes of recover_scatter_wide over the deep record
// (fec_wide_table.hip).
hipError_t launch_classify_wide(const WideLaunch& a, hipStream_t s);
hipError_t launch_decode_wide_deep_rows(const WideLaunch& a, uint64_t first_group, uint64_t groups, hipStream_t s);
hipError_t launch_classify_table_wide(const WideTableLaunch& a, hipStream_t s);
hipError_t launch_recover_scatter_wide_deep_rows(const WideTableLaunch& a, uint64_t first_group, uint64_t groups, hipStream_t s);
// Packed recover rows (fec_runs.hip): row_start[g] = exclusive prefix sum of the rows each group rebuilds
// (lost data shards when recoverable, else 0); *total (nullable) = all rows.  block_sums:
// rows_prefix_workspace_bytes(groups) of device workspace.
uint64_t rows_prefix_workspace_bytes(uint64_t groups);
hipError_t launch_rows_prefix(const uint64_t* masks, uint64_t groups, uint32_t k, uint32_t r, uint32_t* row_start,
                              uint32_t* block_sums, uint64_t* total, hipStream_t s);
// The packed recovers for every shape (fec_packed.hip; fec_forms.hpp PackedLaunch, a.path one of
// kCodebook, kDevicePlan, kWide, kDeep): the row prefix over the call's masks (launch_rows_prefix for
// one-word masks, the unit's own block sums and row-start write for four-word masks), the path's
// classify over every group, then per chunk of a.plan's arena (the codebook path: all groups at once)
// the path's record build and packed_passes(k, r) launches of recover_packed / recover_packed_wide,
// in stream order.
hipError_t launch_recover_packed(const PackedLaunch& a, hipStream_t s);
// What fec_packed.hip calls in the units of the kernels it shares: `classify` over every group of a
// one-word call (fec_decode.hip; an all-zero a.meta gives the device plans' classify), the one-block
// scan of `blocks` block sums (fec_runs.hip rows_scan_blocks, which reads no mask) and the deep
// records of one plan chunk (fec_wide_deep.hip build_records_deep, as launch_build_records_wide).
hipError_t launch_classify(const DecodeLaunch& a, hipStream_t s);
hipError_t launch_rows_scan_blocks(uint32_t* block_sums, uint64_t blocks, uint64_t groups, uint64_t* total, hipStream_t s);
hipError_t launch_build_records_deep(const PlanLaunch& p, const uint64_t* masks, uint32_t* rec_off, uint8_t* status,
                                     uint64_t first_group, uint64_t groups, uint32_t k, uint32_t r, hipStream_t s);
// LDS run image per workgroup of 512 groups (tools/probe_runs.hip; DESIGN_HISTORY.md §5 round 4): C5's
// ~59 rows per tile fit 48 KB (40 rows) mostly; two workgroups per CU.
// recover_runs' run image per workgroup.
constexpr int kRunsStageBytes = 48 * 1024;
uint32_t runs_launches(uint64_t groups);
uint64_t runs_workspace_bytes(uint64_t groups);
uint32_t runs_stage_bytes(const RunsLaunch& a);
hipError_t launch_recover_runs(const RunsLaunch& a, hipStream_t s);
// ---- resident legacy encoder (fec_server.hip; the ring's protocol -- slots, control and
// coordination words, tags and the epoch, serving classes -- is fec_server.hpp's) ----
// One resident instance serving the ring, each class from its progress mark, until every class
// has found nothing to do for idle_ticks, or it lived life_ticks (wall-clock ticks,
// hipDeviceAttributeWallClockRate), or the host sets ctl->stop; on leaving a workgroup stores its
// class's progress, and the last one to leave stores exited = gen.
// coord: nullptr when classes == 1.  slow_ticks: a workgroup other than class 0's without work
// for that long polls slowly (~5 us apart instead of ~1.5) until it finds some.
// stamps: nullptr, or 256 x 8 words of host memory for the diagnostic phase stamps of class 0
// (test library, fec_knobs.hpp kResidentStamps).
// inl: the inline data areas (kInlineSlotBytes per slot) when the ring is in VRAM, else nullptr;
// then the host's stop word (host memory) is read by every 16th poll only, not every poll.
// epoch: laps per tag epoch (server_tag), a power of two, 1 .. kServerEpoch.
hipError_t launch_legacy_server(ServerSlot* ring, uint8_t* inl, uint64_t* done, ServerControl* ctl,
                                ServerCoord* coord, uint32_t classes, uint64_t gen, uint64_t idle_ticks,
                                uint64_t slow_ticks, uint64_t life_ticks, uint64_t* stamps, uint32_t epoch,
                                hipStream_t s);

// Synthetic data and the box calibration copy (fec_util.hip).
hipError_t launch_fill_splitmix(uint8_t* dst, uint64_t nbytes, uint64_t seed, uint64_t byte_offset,
                                hipStream_t s);
// dst <- src, nbytes a multiple of 16, both 16-B aligned (box calibration).
hipError_t launch_copy_words(const uint8_t* src, uint8_t* dst, uint64_t nbytes, hipStream_t s);

// Each kernel translation unit is a code object of its own, and the HIP runtime loads a code object
// onto the current device at the first use of one of its functions.  load_*_unit asks for the
// attributes of one kernel of its unit -- no launch -- which is such a use; load_kernel_units loads
// the six units of the contiguous calls, so that no first call pays for it (fec_shim.cpp
// warm_device_once).  The address-table and plan units load at their first call.
hipError_t load_encode_unit();
hipError_t load_decode_unit();
hipError_t load_decode_fused_unit();
hipError_t load_runs_unit();
hipError_t load_server_unit();
hipError_t load_util_unit();
inline hipError_t load_kernel_units() {
  hipError_t (*const units[])() = {load_encode_unit, load_decode_unit, load_decode_fused_unit,
                                   load_runs_unit,   load_server_unit, load_util_unit};
  for (auto load : units) {
    const hipError_t e = load();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// Records marking "nothing to do" / "unrecoverable" in rec_off.
constexpr uint32_t kRecNone = 0xFFFFFFFFu;
constexpr uint32_t kRecBad = 0xFFFFFFFEu;

}  // namespace qfec
