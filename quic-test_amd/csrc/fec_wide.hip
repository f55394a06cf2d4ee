// fec_wide.hip — gfx950 kernels of the wide calls (fec_decode_wide_rs_dev, fec_recover_wide_rs_dev):
// groups of up to 256 shards, k + r <= 256 and min(k, r) <= 32, their erasure masks four u64 words
// per group (fec_mask_wide.hpp).  A wide shape has no codebook; every call builds its records on
// the device, in the arena of the caller stream's workspace, chunk after chunk (fec_forms.hpp
// wide_arena, fec_launch.hpp for_plan_chunks).
//
//  * classify_wide: one lane per group.  The group's 32 B of mask as two 16-B loads, the rule of
//    fec_mask_wide.hpp, rec_off[g] = 0 where a record is needed, kRecNone where nothing is lost,
//    kRecBad where the group is unrecoverable, and every status byte.
//  * build_records_wide: one wave per group, four per workgroup, as build_records (fec_plan.hip).
//    The parity matrix is staged once per workgroup (r * k <= 7,168 B), each wave works in its own
//    WidePlanScratch (9,536 B): 45,312 B of LDS per workgroup.  The build is
//    fec_plan_build_wide.hpp's (plain C++, run on the host under a sanitizer by
//    tests/csrc/plan_build_wide_test.cpp) with the wave-barrier `each`.  The slot's place goes to
//    rec_off; a zero pivot gives kRecBad and status 1.
//  * decode_wide<POL>: one wave per group, four per workgroup, runtime k, groups in decode_block's
//    XCD-aware order, 8 rows per pass.  The rebuild is decode_piece<0, 8, POL, NW, SRC, DST>
//    (fec_device.hpp) in decode_wave's walk: survivor s comes from the wide header's id byte s (an
//    id below k is a data shard, else a parity row), row m0 + m goes to the erased shard (in place)
//    or to the slot row (recover).  The policy bits are those of the runtime-k decode_wave<0, 8>
//    forms (fec_forms.hpp kWidePolInPlace, kWidePolSlots).  Not tuned: nothing about its speed has
//    been measured against a variant.
//    With kDeepRecord among its bits it reads a deep record (fec_plan_build_deep.hpp), whose erased
//    ids start elsewhere (fec_wide_head.hpp wide_erased_at): the in-place consumer of the shapes with
//    min(k, r) > 32, which fec_wide_deep.hip builds the records of on a context in FEC_WIDE_ROWS_ALL.
//
// Algorithmic bytes per group with e rows to rebuild: reads k * P * ceil(e / 8) (the survivors are
// re-read per row pass, as in every runtime-k form), e * k * 32 of record per walk pass through the
// scalar cache, writes e * P.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"  // Tab, ldw / stw, rec_byte, decode_block, decode_piece
#include "fec_forms.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_mask_wide.hpp"
#include "fec_plan_build_wide.hpp"
#include "fec_wide_head.hpp"  // WideHead, the record's header as decode_wide reads it

namespace qfec {
namespace {

static_assert(kWideHeader == kWideHeaderBytes, "fec_forms.hpp states the header for host-only code");
static_assert(kWideMaxRows == kWideMaxE && kWideMaxShards == kWideMaskBits, "fec_forms.hpp states the limits for host-only code");
static_assert(wide_slot_stride(224, 32) == wide_record_bytes(224, 32) && wide_slot_stride(32, 224) == wide_record_bytes(32, 32),
              "fec_forms.hpp's slot is the builder's largest record");
static_assert(kWideHeaderBytes % 32u == 0, "record offsets are counted in 32-B units");
static_assert(kPlanRecLimit == kRecBad, "fec_forms.hpp states the record limit for host-only code");

__global__ __launch_bounds__(256) void classify_wide(const uint64_t* __restrict__ masks, uint64_t groups, uint32_t k,
                                                     uint32_t r, uint32_t* __restrict__ rec_off,
                                                     uint8_t* __restrict__ status) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * 256u + threadIdx.x;
  if (g >= groups) return;
  const MaskLosses l = wide_mask_losses(load_wide_mask(masks, g), k, r);
  rec_off[g] = l.lost == 0 ? kRecNone : l.unrecoverable ? kRecBad : 0u;
  if (status) status[g] = l.lost != 0 && l.unrecoverable ? 1 : 0;
}

__global__ __launch_bounds__(256) void build_records_wide(const uint64_t* __restrict__ masks,
                                                          uint32_t* __restrict__ rec_off,
                                                          uint8_t* __restrict__ status,
                                                          const uint8_t* __restrict__ matrix,
                                                          uint8_t* __restrict__ arena, uint64_t stride,
                                                          uint64_t groups, uint32_t slot0, uint32_t k, uint32_t r) {
  __shared__ __attribute__((aligned(16))) uint8_t M[kWideMaxMatrix];
  __shared__ WidePlanScratch scratch[4];
  // every wave takes part in the copy and the barrier, then the idle ones leave
  for (uint32_t i = threadIdx.x; i < r * k; i += 256u) M[i] = matrix[i];
  __syncthreads();
  const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * 4u + wave;
  if (g >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[g]);
  if (rec >= kRecBad) return;  // nothing lost, or unrecoverable
  const WideMask loaded = load_wide_mask(masks, g);
  const WideMask m = {{uniform64(loaded.w[0]), uniform64(loaded.w[1]), uniform64(loaded.w[2]), uniform64(loaded.w[3])}};
  // the classify's verdict again, from the mask the record is built from: 1 <= e <= min(k, r) <= 32
  // is what keeps the build inside its scratch and its slot
  const MaskLosses losses = wide_mask_losses(m, k, r);
  bool ok = losses.lost != 0 && !losses.unrecoverable && losses.lost <= kWideMaxE;
  const uint64_t slot = slot0 + g;
  if (ok) {
    ok = wide_plan_build_record(k, r, M, m, scratch[wave], arena + slot * stride, [lane](auto step) {
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

// (decode_piece's SRC, WideBases: fec_wide_head.hpp, shared with the packed consumer, fec_packed.hip)
// decode_piece's DST: row m0 + m at the erased shard (in place; its id at byte ERASED_AT + m0 + m of
// the record) or at the slot row (SLOTS, which reads no erased id).
template <bool SLOTS, uint32_t ERASED_AT>
struct WideRows {
  const uint32_t* rw;
  uint8_t* og;
  uint32_t P, m0;
  template <int NW, int POL>
  __device__ __forceinline__ void store(uint32_t m, uint32_t off, const uint32_t (&v)[NW]) const {
    const uint32_t row = SLOTS ? m0 + m : rec_byte(rw, ERASED_AT + m0 + m);
    stw<NW, POL>(og + row * static_cast<uint64_t>(P) + off, v);
  }
};

template <int POL>
__global__ __launch_bounds__(256) void decode_wide(const uint8_t* data, const uint8_t* __restrict__ parity,
                                                   const uint32_t* __restrict__ rec_off,
                                                   const uint8_t* __restrict__ arena, uint64_t groups, uint32_t P,
                                                   uint32_t k, uint32_t r, uint32_t m0, uint8_t* out, uint32_t swz) {
  constexpr bool kSlots = (POL & kCompactOut) != 0;
  const uint64_t gw = static_cast<uint64_t>(decode_block(swz)) * 4u +
                      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
  if (rec >= kRecBad) return;
  const WideHead h{reinterpret_cast<const uint32_t*>(arena + static_cast<uint64_t>(rec) * 32u)};
  const uint32_t e = h.e();
  const bool xor_only = h.xor_only();
  if (m0 >= e) return;
  const Tab* tabs = h.tabs();
  const WideBases src{h.rw, data + gw * k * static_cast<uint64_t>(P), parity + gw * r * static_cast<uint64_t>(P), k, P};
  const WideRows<kSlots, wide_erased_at<POL>> dst{h.rw, out + gw * (kSlots ? r : k) * static_cast<uint64_t>(P), P, m0};
  // decode_wave's walk: 16-B pieces per whole 1 KiB, then 4-B tail pieces shifted back to end at P
  const uint32_t main_end = P & ~1023u;
  for (uint32_t base = 0; base < main_end; base += 1024u)
    decode_piece<0, 8, POL, 4>(h.rw, tabs, nullptr, nullptr, nullptr, k, P, base + lane * 16u, e, m0, xor_only, src, dst);
  for (uint32_t base = main_end; base < P; base += 256u) {
    const uint32_t off = base + lane * 4u;
    decode_piece<0, 8, POL, 1>(h.rw, tabs, nullptr, nullptr, nullptr, k, P, off + 4u <= P ? off : P - 4u, e, m0, xor_only, src, dst);
  }
}

hipError_t run_classify_wide(const WideLaunch& a, hipStream_t s) {
  return for_chunks(a.groups, max_launch_threads(), [&](uint64_t g0, uint64_t gn) {
    trace_launch(launch_record(static_cast<int64_t>(WideLaunchForm::kClassifyWide), blocks_for(gn), 256, g0, gn));
    hipLaunchKernelGGL(classify_wide, dim3(blocks_for(gn)), dim3(256), 0, s, a.masks + g0 * kWideMaskWords, gn, a.k, a.r,
                       a.rec_off + g0, a.status ? a.status + g0 : nullptr);
  });
}

// The records of groups [c0, c0 + cn), one plan chunk: group c0 + i into slot i.
hipError_t run_build_records_wide(const WideLaunch& a, uint64_t c0, uint64_t cn, hipStream_t s) {
  return for_chunks(cn, max_wave_blocks() * 4, [&](uint64_t g0, uint64_t gn) {
    const uint64_t bn = (gn + 3) / 4;
    LaunchRecord t = launch_record(static_cast<int64_t>(WideLaunchForm::kBuildRecordsWide), bn, 256, c0 + g0, gn);
    t.k = 0, t.aux = static_cast<int64_t>(g0);
    trace_launch(t);
    hipLaunchKernelGGL(build_records_wide, dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                       a.masks + (c0 + g0) * kWideMaskWords, a.rec_off + c0 + g0, a.status ? a.status + c0 + g0 : nullptr,
                       a.plan.matrix, a.plan.arena, a.plan.stride, gn, static_cast<uint32_t>(g0), a.k, a.r);
  });
}

// The row passes over groups [c0, c0 + cn), their records in the arena.  The instantiation over
// the deep record (kDeepRecord) is traced under a form of its own.
template <int POL>
hipError_t run_decode_wide(const WideLaunch& a, uint64_t c0, uint64_t cn, hipStream_t s) {
  constexpr int64_t kForm = (POL & kDeepRecord) != 0 ? static_cast<int64_t>(WideDeepLaunchForm::kDecodeWideDeep)
                                                     : static_cast<int64_t>(WideLaunchForm::kDecodeWide);
  const uint64_t P = a.P;
  const uint32_t rows = a.k < a.r ? a.k : a.r;
  return for_wave_passes(cn, rows, kWidePassRows, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    const uint64_t first = c0 + g0;
    LaunchRecord t = launch_record(kForm, bn, 256, first, gn);
    t.k = 0, t.r = kWidePassRows, t.pol = POL, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((decode_wide<POL>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s, a.data + first * a.k * P,
                       a.parity + first * a.r * P, a.rec_off + first, a.plan.arena, gn, a.P, a.k, a.r, m0,
                       a.out + first * ((POL & kCompactOut) != 0 ? a.r : a.k) * P, static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
  });
}

}  // namespace

// build_records_wide for another unit's call (fec_wide_table.hip): run_build_records_wide on the
// fields it reads.
hipError_t launch_build_records_wide(const PlanLaunch& p, const uint64_t* masks, uint32_t* rec_off, uint8_t* status,
                                     uint64_t first_group, uint64_t groups, uint32_t k, uint32_t r, hipStream_t s) {
  if (masks == nullptr || rec_off == nullptr || p.arena == nullptr || p.matrix == nullptr || groups > p.per_chunk ||
      p.stride != wide_slot_stride(k, r))
    return hipErrorInvalidValue;
  WideLaunch a{};
  a.masks = masks, a.rec_off = rec_off, a.status = status;
  a.k = k, a.r = r;
  a.plan = p;
  return run_build_records_wide(a, first_group, groups, s);
}

// classify_wide and the row passes of one plan chunk for a call on the deep path (fec_wide_deep.hip,
// which has checked the launch and built the chunk's deep records).  In place: decode_wide over the
// deep record.  Slots: the very instantiation the wide path runs -- it reads the count, the flag,
// the survivor ids and the tables, which a deep record has where a wide one has them, and no
// erased id (WideRows<true>; decode_piece asks a DST functor for every store).
hipError_t launch_classify_wide(const WideLaunch& a, hipStream_t s) {
  if (a.masks == nullptr || a.rec_off == nullptr || a.groups == 0) return hipErrorInvalidValue;
  return run_classify_wide(a, s);
}
hipError_t launch_decode_wide_deep_rows(const WideLaunch& a, uint64_t first_group, uint64_t groups, hipStream_t s) {
  if (a.data == nullptr || a.parity == nullptr || a.out == nullptr || a.rec_off == nullptr || a.plan.arena == nullptr ||
      first_group + groups > a.groups)
    return hipErrorInvalidValue;
  return a.slots ? run_decode_wide<kWidePolSlots>(a, first_group, groups, s)
                 : run_decode_wide<kWideDeepPolInPlace>(a, first_group, groups, s);
}

hipError_t launch_decode_wide(const WideLaunch& a, hipStream_t s) {
  // a slot holds the shape's largest record and a chunk has at most per_chunk groups (for_plan_chunks):
  // every record lies inside the arena
  if (wide_served(a.groups, a.k, a.r, a.P) != WideRefusal::kServed || a.data == nullptr || a.parity == nullptr ||
      a.out == nullptr || a.masks == nullptr || a.rec_off == nullptr || a.plan.arena == nullptr || a.plan.matrix == nullptr ||
      a.plan.per_chunk == 0 || a.plan.stride != wide_slot_stride(a.k, a.r))
    return hipErrorInvalidValue;
  return for_plan_chunks(
      a.groups, a.plan.per_chunk, [&] { return run_classify_wide(a, s); },
      [&](uint64_t c0, uint64_t cn) { return run_build_records_wide(a, c0, cn, s); },
      [&](uint64_t c0, uint64_t cn) {
        return a.slots ? run_decode_wide<kWidePolSlots>(a, c0, cn, s) : run_decode_wide<kWidePolInPlace>(a, c0, cn, s);
      });
}

}  // namespace qfec
