// fec_wide_deep.hip — gfx950 kernels of the wide calls (fec_decode_wide_rs_dev, fec_recover_wide_rs_dev,
// fec_recover_scatter_wide_rs_dev) for the shapes past the wide record builder's rows: k + r <= 256
// with min(k, r) in 33..128, served by a context in FEC_WIDE_ROWS_ALL (fec_forms.hpp wide_route).
// The calls walk as the wide ones do (fec_launch.hpp for_plan_chunks): the unchanged classify of
// fec_wide.hip or fec_wide_table.hip over every group, then per chunk of the arena (fec_forms.hpp
// wide_deep_arena) the records and wide_passes(k, r) launches, up to 16, of the consumer.
//
//  * build_records_deep: one group per workgroup of 256 lanes, which share one DeepPlanScratch
//    (49,664 B of LDS; three workgroups per CU against its 160 KiB).  The build is
//    fec_plan_build_deep.hpp's (plain C++, run on the host under a sanitizer by
//    tests/csrc/plan_build_deep_test.cpp) with `each` = the step, then __syncthreads().  One group
//    per workgroup is what makes that barrier legal: every exit before the build -- past `groups`,
//    nothing lost, unrecoverable -- is taken by all 256 lanes, and so is the build, whose verdict
//    comes from the group's mask alone.  The parity matrix is read from global memory (r * k <=
//    16 KiB, every workgroup of the launch reads the same one: L2 serves it); staged in LDS it would
//    leave two workgroups per CU.  The slot's place goes to rec_off; a zero pivot gives kRecBad and
//    status 1.
//  * The consumers are not kernels of this unit but instantiations of the wide path's own templates
//    over the deep record (fec_forms.hpp kDeepRecord; fec_wide_head.hpp wide_erased_at), in the units
//    that hold them: decode_wide<kWideDeepPolInPlace> (fec_wide.hip) puts row m0 + m at the erased
//    shard of id byte kDeepErasedAt + m0 + m; recover_scatter_wide<kWideDeepTablePol, VAR>
//    (fec_wide_table.hip) takes the row's destination from the entry of that id.  The slots layout
//    needs no new instantiation: decode_wide<kWidePolSlots> reads no erased id.
// Not tuned: nothing about the build's speed has been measured against a variant.
//
// The build reads e * e + e * (k - e) bytes of the matrix, the second part e times over, from L2
// and writes 512 + e * k * 32 bytes of record.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"
#include "fec_forms.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_mask_wide.hpp"
#include "fec_plan_build_deep.hpp"
#include "fec_wide_head.hpp"  // load_wide_mask, uniform64

namespace qfec {
namespace {

static_assert(kWideDeepMaxRows == kDeepMaxE, "fec_forms.hpp states the limit for host-only code");
static_assert(wide_deep_slot_stride(128, 128) == wide_record_bytes(128, 128) && wide_deep_slot_stride(216, 40) == wide_record_bytes(216, 40) &&
                  wide_deep_slot_stride(40, 216) == wide_record_bytes(40, 40),
              "fec_forms.hpp's slot is the builder's largest record");
static_assert(wide_deep_slot_stride(128, 128) % 32u == 0 && kPlanArenaBytes / 32u < kRecBad, "record offsets are counted in 32-B units");
static_assert(sizeof(DeepPlanScratch) * 3 <= 160u * 1024u, "three workgroups per CU");

__global__ __launch_bounds__(256) void build_records_deep(const uint64_t* __restrict__ masks,
                                                          uint32_t* __restrict__ rec_off,
                                                          uint8_t* __restrict__ status,
                                                          const uint8_t* __restrict__ matrix,
                                                          uint8_t* __restrict__ arena, uint64_t stride,
                                                          uint64_t groups, uint32_t k, uint32_t r) {
  __shared__ DeepPlanScratch scratch;
  const uint64_t g = blockIdx.x;  // one group per workgroup, group g of the chunk into slot g: every branch below is the workgroup's
  if (g >= groups) return;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[g]);
  __syncthreads();  // every wave has the classify's verdict before lane 0 may overwrite it
  if (rec >= kRecBad) return;  // nothing lost, or unrecoverable
  const WideMask loaded = load_wide_mask(masks, g);
  const WideMask m = {{uniform64(loaded.w[0]), uniform64(loaded.w[1]), uniform64(loaded.w[2]), uniform64(loaded.w[3])}};
  // the classify's verdict again, from the mask the record is built from: 1 <= e <= min(k, r) <= 128
  // is what keeps the build inside its scratch and its slot
  const MaskLosses losses = wide_mask_losses(m, k, r);
  bool ok = losses.lost != 0 && !losses.unrecoverable && losses.lost <= kDeepMaxE;
  const uint32_t tid = threadIdx.x;
  if (ok) {
    ok = deep_plan_build_record(k, r, matrix, m, scratch, arena + g * stride, [tid](auto step) {
      step(tid, 256u);
      __syncthreads();
    });
  }
  if (tid == 0) {
    rec_off[g] = ok ? static_cast<uint32_t>(g * (stride / 32u)) : kRecBad;
    if (!ok && status) status[g] = 1;
  }
}

// The records of groups [c0, c0 + cn), one plan chunk: group c0 + i into slot i, a workgroup each, in
// one launch -- a chunk never has more groups than a grid may have workgroups.
static_assert(kPlanArenaBytes / wide_deep_slot_stride(33, 33) <= kMaxWaveBlocks, "the smallest deep slot bounds a chunk's groups");
hipError_t run_build_records_deep(const PlanLaunch& p, const uint64_t* masks, uint32_t* rec_off, uint8_t* status, uint64_t c0,
                                  uint64_t cn, uint32_t k, uint32_t r, hipStream_t s) {
  if (cn == 0 || cn > p.per_chunk || cn > kMaxWaveBlocks) return hipErrorInvalidValue;
  LaunchRecord t = launch_record(static_cast<int64_t>(WideDeepLaunchForm::kBuildRecordsDeep), cn, 256, c0, cn);
  t.k = 0, t.aux = 0;
  trace_launch(t);
  hipLaunchKernelGGL(build_records_deep, dim3(static_cast<uint32_t>(cn)), dim3(256), 0, s, masks + c0 * kWideMaskWords, rec_off + c0,
                     status ? status + c0 : nullptr, p.matrix, p.arena, p.stride, cn, k, r);
  return hipGetLastError();
}

// The deep path's launch: a shape past the cap that FEC_WIDE_ROWS_ALL serves, its plan sized by
// wide_deep_arena.  A slot holds the shape's largest record and a chunk has at most per_chunk
// groups (for_plan_chunks): every record lies inside the arena.
bool deep_plan_ok(const PlanLaunch& p, uint64_t groups, uint32_t k, uint32_t r, uint32_t P) {
  return wide_route(kWideRowsAll, groups, k, r, P).path == WidePath::kDeep && p.arena != nullptr && p.matrix != nullptr &&
         p.per_chunk != 0 && p.stride == wide_deep_slot_stride(k, r);
}

}  // namespace

hipError_t launch_decode_wide_deep(const WideLaunch& a, hipStream_t s) {
  if (!deep_plan_ok(a.plan, a.groups, a.k, a.r, a.P) || a.data == nullptr || a.parity == nullptr || a.out == nullptr ||
      a.masks == nullptr || a.rec_off == nullptr)
    return hipErrorInvalidValue;
  return for_plan_chunks(
      a.groups, a.plan.per_chunk, [&] { return launch_classify_wide(a, s); },
      [&](uint64_t c0, uint64_t cn) { return run_build_records_deep(a.plan, a.masks, a.rec_off, a.status, c0, cn, a.k, a.r, s); },
      [&](uint64_t c0, uint64_t cn) { return launch_decode_wide_deep_rows(a, c0, cn, s); });
}

// build_records_deep for another unit's call (fec_packed.hip), as launch_build_records_wide: groups
// [first_group, first_group + groups) of a call on the deep path, one plan chunk.
hipError_t launch_build_records_deep(const PlanLaunch& p, const uint64_t* masks, uint32_t* rec_off, uint8_t* status,
                                     uint64_t first_group, uint64_t groups, uint32_t k, uint32_t r, hipStream_t s) {
  if (masks == nullptr || rec_off == nullptr || p.arena == nullptr || p.matrix == nullptr ||
      p.stride != wide_deep_slot_stride(k, r) || uint64_t{k} + r > kWideMaxShards || (k < r ? k : r) > kWideDeepMaxRows)
    return hipErrorInvalidValue;
  return run_build_records_deep(p, masks, rec_off, status, first_group, groups, k, r, s);
}

hipError_t launch_recover_scatter_wide_deep(const WideTableLaunch& a, hipStream_t s) {
  if (!deep_plan_ok(a.plan, a.groups, a.k, a.r, a.P) || a.addrs == nullptr || a.dests == nullptr || a.masks == nullptr ||
      a.rec_off == nullptr)
    return hipErrorInvalidValue;
  if (a.lens != nullptr && a.symlen == nullptr) return hipErrorInvalidValue;  // the kernel reads the symbol lengths
  return for_plan_chunks(
      a.groups, a.plan.per_chunk, [&] { return launch_classify_table_wide(a, s); },
      [&](uint64_t c0, uint64_t cn) { return run_build_records_deep(a.plan, a.masks, a.rec_off, a.status, c0, cn, a.k, a.r, s); },
      [&](uint64_t c0, uint64_t cn) { return launch_recover_scatter_wide_deep_rows(a, c0, cn, s); });
}

}  // namespace qfec
