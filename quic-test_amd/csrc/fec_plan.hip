// fec_plan.hip — gfx950 kernel of the device plans (FEC_PLAN_DEVICE): recovery records built on the
// device, per call, for the shapes whose codebook of every pattern is past its cap.
//
//  * build_records: one wave per group, four per workgroup, like the kernels that read the
//    records.  A wave whose group the classify left recoverable (rec_off below kRecBad) builds the
//    record of the group's mask -- fec_plan_build.hpp's plan_build_record, the bytes of gf256.hpp's
//    build_record -- into the group's slot of the arena and stores the slot's place in rec_off.
//    Groups with nothing to rebuild are skipped: their slots stay unwritten and are never read.
// The build's steps, its arithmetic and its stores are fec_plan_build.hpp's (plain C++, run on the
// host under a sanitizer by tests/csrc/plan_build_test.cpp); this file holds the mapping of groups
// to waves, the LDS the build works in and the launcher.  Which calls build records, into how many
// slots and in which chunks is decided in fec_forms.hpp (plan_arena) and walked by fec_launch.hpp's
// for_plan_chunks.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_forms.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_plan_build.hpp"

namespace qfec {
namespace {

static_assert(kPlanRecLimit == kRecBad, "fec_forms.hpp states the record limit for host-only code");
static_assert(plan_slot_stride(32, 32) == kPlanHeaderBytes + uint64_t{32} * 32 * kPlanEntryBytes,
              "fec_forms.hpp's slot is the builder's largest record");
static_assert(kPlanMaxE * kPlanMaxE == 1024, "the parity matrix (r * k <= 1024 as k + r <= 64) fits the LDS copy");

// Per workgroup: the parity matrix once (at most 1 KiB) and a PlanScratch per wave (3.2 KiB each).
__global__ __launch_bounds__(256) void build_records(const uint64_t* __restrict__ masks,
                                                     uint32_t* __restrict__ rec_off,
                                                     uint8_t* __restrict__ status,
                                                     const uint8_t* __restrict__ matrix,
                                                     uint8_t* __restrict__ arena, uint64_t stride,
                                                     uint64_t groups, uint32_t slot0, uint32_t k, uint32_t r) {
  __shared__ __attribute__((aligned(16))) uint8_t M[kPlanMaxE * kPlanMaxE];
  __shared__ PlanScratch scratch[4];
  // every wave takes part in the copy and the barrier, then the idle ones leave
  for (uint32_t i = threadIdx.x; i < r * k; i += 256u) M[i] = matrix[i];
  __syncthreads();
  const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * 4u + wave;
  if (g >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[g]);
  if (rec >= kRecBad) return;  // nothing lost, or unrecoverable
  const uint64_t mask = masks[g];
  const uint32_t mask_lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(mask));
  const uint32_t mask_hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(mask >> 32));
  const uint64_t m = static_cast<uint64_t>(mask_hi) << 32 | mask_lo;
  // the classify's verdict again, from the mask the record is built from: 1 <= e <= min(k, r) is
  // what keeps the build inside its scratch and its slot
  const MaskLosses losses = mask_losses(m, k, r);
  bool ok = losses.lost != 0 && !losses.unrecoverable;
  const uint64_t slot = slot0 + g;
  if (ok) {
    ok = plan_build_record(k, r, M, m, scratch[wave], arena + slot * stride, [lane](auto step) {
      step(lane, 64u);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    });
  }
  if (lane == 0) {
    rec_off[g] = ok ? static_cast<uint32_t>(slot * (stride / 32u)) : kRecBad;
    if (!ok && status) status[g] = 1;
  }
}

}  // namespace

hipError_t launch_build_records(const PlanLaunch& p, const uint64_t* masks, uint32_t* rec_off, uint8_t* status,
                                uint64_t first_group, uint64_t groups, uint32_t k, uint32_t r, hipStream_t s) {
  if (groups == 0) return hipSuccess;
  if (p.arena == nullptr || p.matrix == nullptr || masks == nullptr || rec_off == nullptr || groups > p.per_chunk ||
      p.stride % 32u != 0 || p.stride < plan_slot_stride(k, r) || k + r > 64u)
    return hipErrorInvalidValue;
  return for_chunks(groups, max_wave_blocks() * 4, [&](uint64_t g0, uint64_t gn) {
    const uint64_t bn = (gn + 3) / 4;
    LaunchRecord t = launch_record(static_cast<int64_t>(PlanLaunchForm::kBuildRecords), bn, 256, first_group + g0, gn);
    t.k = 0, t.aux = static_cast<int64_t>(g0);
    trace_launch(t);
    hipLaunchKernelGGL(build_records, dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s, masks + g0, rec_off + g0,
                       status ? status + g0 : nullptr, p.matrix, p.arena, p.stride, gn, static_cast<uint32_t>(g0), k, r);
  });
}

}  // namespace qfec
