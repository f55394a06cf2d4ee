// fec_packed.hip — gfx950 kernels of the packed recovers for every shape (fec_recover_packed_rs_dev,
// fec_recover_packed_wide_rs_dev): the rebuilt packets of a whole batch back to back, group g's rows
// from row row_start[g], for the shapes whose slot recover is record-addressed.  Which path a call
// takes is decided in fec_forms.hpp (packed_route, packed_wide_route); a call the old packed call
// serves never comes here.
//
//  * rows_block_sums_wide, rows_write_wide<DIRECT>: the row prefix of fec_runs.hip over four-word
//    masks.  row_start[g] = the rows groups 0..g-1 rebuild, a group's rows being fec_mask_wide.hpp's
//    wide_mask_rows (the losses classify_wide decides on).  Blocks of 1024 groups, four per thread,
//    each mask as two 16-B loads at the caller's 8-B alignment; the block scan and sum are
//    fec_scan.hpp's, the one-block scan of the block sums in between (past kRowsDirectBlocks blocks)
//    is fec_runs.hip's own rows_scan_blocks, which reads no mask.  The one-word prefix is
//    fec_runs.hip's launch_rows_prefix, unchanged.
//  * recover_packed<POL>: one wave per group, four per workgroup, runtime k, 8 rows per pass,
//    record-addressed: decode_walk<0, 8, POL> (fec_device.hpp; decode_wave's walk over decode_piece)
//    with the survivors at the contiguous shards the record's ids name and the group's compact run
//    starting at out + row_start[g] * P, so row m0 + m lands at out + (row_start[g] + m0 + m) * P.
//    The record comes from the dense codebook or from the arena build_records (fec_plan.hip) filled.
//  * recover_packed_wide<POL>: decode_wide's walk (fec_wide.hip) with a destination functor at the
//    same place.  It reads the count, the flag, the survivor ids and the tables of a wide or a deep
//    record, which both have in the same place, and no erased id: one instantiation serves the wide
//    and the deep path, as decode_wide<kWidePolSlots> does for the slots.
// A group whose record build met a zero pivot (the code's matrix is MDS: it cannot) has kRecBad in
// rec_off and status 1, as in the slot recovers; its rows stay reserved in row_start and unwritten.
// Not tuned: nothing about these kernels' speed has been measured against a variant.
//
// Algorithmic bytes per group with e rows to rebuild: those of the slot form of the same mask width
// (reads k * P * ceil(e / 8), writes e * P), plus 4 B of row_start per group and pass.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"  // Tab, rec_head, decode_block, decode_piece, decode_walk
#include "fec_forms.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_mask_wide.hpp"
#include "fec_scan.hpp"       // block_inclusive_scan, block_sum
#include "fec_wide_head.hpp"  // WideHead, WideBases, load_wide_mask

namespace qfec {
namespace {

// the prefix's block and its two-launch limit: fec_runs.hip's, stated in fec_forms.hpp
constexpr uint32_t kRowsPerThread = kPackedRowsPerThread, kRowsPerBlock = kPackedRowsPerBlock;
constexpr uint32_t kRowsDirectBlocks = kPackedRowsDirectBlocks;
static_assert(kPackedPassRows == kWidePassRows && kPackedPol == kWidePolSlots, "the packed consumers walk as the slot forms do");
static_assert((kPackedPol & kCompactOut) != 0, "decode_piece's compact rows are what places row m0 + m after the run's start");

// The rows of a thread's kRowsPerThread consecutive groups.
__device__ __forceinline__ void thread_rows_wide(const uint64_t* __restrict__ masks, uint64_t groups, uint64_t g0,
                                                 uint32_t k, uint32_t r, uint32_t (&rows)[kRowsPerThread]) {
#pragma unroll
  for (uint32_t i = 0; i < kRowsPerThread; ++i)
    rows[i] = g0 + i < groups ? wide_mask_rows(load_wide_mask(masks, g0 + i), k, r) : 0u;
}

__global__ __launch_bounds__(256) void rows_block_sums_wide(const uint64_t* __restrict__ masks, uint64_t groups,
                                                            uint32_t k, uint32_t r, uint32_t* __restrict__ block_sums) {
  __shared__ uint32_t lds[4];
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x * kRowsPerThread;
  uint32_t rows[kRowsPerThread];
  thread_rows_wide(masks, groups, g0, k, r, rows);
  const uint32_t total = block_sum(rows[0] + rows[1] + rows[2] + rows[3], lds);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// DIRECT: block_sums holds the blocks' own sums; each block adds up those before it (and the
// last block writes the total).  Else block_sums holds exclusive offsets (rows_scan_blocks).
template <bool DIRECT>
__global__ __launch_bounds__(256) void rows_write_wide(const uint64_t* __restrict__ masks, uint64_t groups, uint32_t k,
                                                       uint32_t r, const uint32_t* __restrict__ block_sums,
                                                       uint32_t* __restrict__ row_start, uint64_t* __restrict__ total) {
  __shared__ uint32_t lds[256];
  uint32_t base;
  if constexpr (DIRECT) {
    uint32_t part = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256) part += block_sums[b];
    base = block_sum(part, lds);
  } else {
    base = block_sums[blockIdx.x];
  }
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * kRowsPerBlock + threadIdx.x * kRowsPerThread;
  uint32_t rows[kRowsPerThread];
  thread_rows_wide(masks, groups, g0, k, r, rows);
  const uint32_t sum = rows[0] + rows[1] + rows[2] + rows[3];
  const uint32_t incl = block_inclusive_scan(sum, lds);
  uint32_t at = base + incl - sum;
#pragma unroll
  for (uint32_t i = 0; i < kRowsPerThread; ++i) {
    if (g0 + i < groups) row_start[g0 + i] = at;
    at += rows[i];
  }
  if constexpr (DIRECT) {
    if (total != nullptr && blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) *total = base + incl;
  }
}

// One wave per group (4 per workgroup), rows [m0, m0 + 8) per launch.  data / parity / rec_off /
// row_start are the launch's first group's; `out` is the call's: rows are placed by global row index.
template <int POL>
__global__ __launch_bounds__(256) void recover_packed(const uint8_t* __restrict__ data, const uint8_t* __restrict__ parity,
                                                      const uint32_t* __restrict__ rec_off,
                                                      const uint32_t* __restrict__ row_start,
                                                      const uint8_t* __restrict__ codebook, uint64_t groups, uint32_t P,
                                                      uint32_t k, uint32_t r, uint32_t m0, uint8_t* __restrict__ out,
                                                      uint32_t swz) {
  const uint64_t gw = static_cast<uint64_t>(decode_block(swz)) * 4u +
                      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
  if (rec >= kRecBad) return;
  const RecHead h = rec_head(codebook, rec);
  const uint32_t e = h.e();
  const bool xor_only = h.xor_only();
  if (m0 >= e) return;
  const uint32_t first = __builtin_amdgcn_readfirstlane(row_start[gw]);
  // the group's compact run starts at its first row: decode_piece puts row m0 + m at og + (m0 + m) * P
  decode_walk<0, 8, POL>(h.rw, h.tabs(), data + gw * k * static_cast<uint64_t>(P), parity + gw * r * static_cast<uint64_t>(P),
                         out + first * static_cast<uint64_t>(P), k, P, lane, e, m0, xor_only);
}

// decode_piece's DST: row m0 + m of the group at packed row first + m0 + m.
struct PackedRows {
  uint8_t* out;
  uint32_t P, first, m0;
  template <int NW, int POL>
  __device__ __forceinline__ void store(uint32_t m, uint32_t off, const uint32_t (&v)[NW]) const {
    stw<NW, POL>(out + (static_cast<uint64_t>(first) + m0 + m) * P + off, v);
  }
};

template <int POL>
__global__ __launch_bounds__(256) void recover_packed_wide(const uint8_t* __restrict__ data,
                                                           const uint8_t* __restrict__ parity,
                                                           const uint32_t* __restrict__ rec_off,
                                                           const uint32_t* __restrict__ row_start,
                                                           const uint8_t* __restrict__ arena, uint64_t groups, uint32_t P,
                                                           uint32_t k, uint32_t r, uint32_t m0, uint8_t* __restrict__ out,
                                                           uint32_t swz) {
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
  const uint32_t first = __builtin_amdgcn_readfirstlane(row_start[gw]);
  const WideBases src{h.rw, data + gw * k * static_cast<uint64_t>(P), parity + gw * r * static_cast<uint64_t>(P), k, P};
  const PackedRows dst{out, P, first, m0};
  // decode_wave's walk: 16-B pieces per whole 1 KiB, then 4-B tail pieces shifted back to end at P
  const uint32_t main_end = P & ~1023u;
  for (uint32_t base = 0; base < main_end; base += 1024u)
    decode_piece<0, 8, POL, 4>(h.rw, tabs, nullptr, nullptr, nullptr, k, P, base + lane * 16u, e, m0, xor_only, src, dst);
  for (uint32_t base = main_end; base < P; base += 256u) {
    const uint32_t off = base + lane * 4u;
    decode_piece<0, 8, POL, 1>(h.rw, tabs, nullptr, nullptr, nullptr, k, P, off + 4u <= P ? off : P - 4u, e, m0, xor_only, src, dst);
  }
}

// ---------------------------------------------------------------------------------
// Launchers: which path a call takes is decided in fec_forms.hpp; these only launch it.
// ---------------------------------------------------------------------------------
// launch_rows_prefix (fec_runs.hip) over four-word masks, both of its forms.
hipError_t run_rows_prefix_wide(const PackedLaunch& a, hipStream_t s) {
  const uint64_t nb = (a.groups + kRowsPerBlock - 1) / kRowsPerBlock;
  if (nb > 0xFFFFFFFFull) return hipErrorInvalidValue;
  // the two-launch form's block limit (the test library's TestKnob::kRowsDirectBlocks forces the other form)
  const uint64_t direct_max = static_cast<uint64_t>(knob(TestKnob::kRowsDirectBlocks, kRowsDirectBlocks));
  const dim3 grid(static_cast<uint32_t>(nb));
  const bool direct = nb <= direct_max;
  trace_launch(launch_record(static_cast<int64_t>(PackedLaunchForm::kRowsBlockSumsWide), nb, 256, 0, a.groups));
  hipLaunchKernelGGL(rows_block_sums_wide, grid, dim3(256), 0, s, a.masks, a.groups, a.k, a.r, a.block_sums);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (!direct && (e = launch_rows_scan_blocks(a.block_sums, nb, a.groups, a.total, s)) != hipSuccess) return e;
  LaunchRecord t = launch_record(static_cast<int64_t>(PackedLaunchForm::kRowsWriteWide), nb, 256, 0, a.groups);
  t.direct = direct;
  trace_launch(t);
  if (direct) {
    hipLaunchKernelGGL(rows_write_wide<true>, grid, dim3(256), 0, s, a.masks, a.groups, a.k, a.r, a.block_sums, a.row_start,
                       a.total);
  } else {
    hipLaunchKernelGGL(rows_write_wide<false>, grid, dim3(256), 0, s, a.masks, a.groups, a.k, a.r, a.block_sums, a.row_start,
                       nullptr);
  }
  return hipGetLastError();
}

// The row passes over groups [c0, c0 + cn) of the call, their records at `records` (the codebook, or
// the arena holding this plan chunk's).  WIDE: recover_packed_wide over a wide or a deep record.
template <bool WIDE>
hipError_t run_recover_packed(const PackedLaunch& a, const uint8_t* records, uint64_t c0, uint64_t cn, hipStream_t s) {
  constexpr int64_t kForm = static_cast<int64_t>(WIDE ? PackedLaunchForm::kRecoverPackedWide : PackedLaunchForm::kRecoverPacked);
  const uint64_t P = a.P;
  const uint32_t rows = a.k < a.r ? a.k : a.r;
  return for_wave_passes(cn, rows, kPackedPassRows, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    const uint64_t first = c0 + g0;
    LaunchRecord t = launch_record(kForm, bn, 256, first, gn);
    t.k = 0, t.r = kPackedPassRows, t.pol = kPackedPol, t.aux = m0;
    trace_launch(t);
    // `out` is not offset: rows are placed by global row index
    if constexpr (WIDE) {
      hipLaunchKernelGGL((recover_packed_wide<kPackedPol>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                         a.data + first * a.k * P, a.parity + first * a.r * P, a.rec_off + first, a.row_start + first, records, gn,
                         a.P, a.k, a.r, m0, a.out, static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
    } else {
      hipLaunchKernelGGL((recover_packed<kPackedPol>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                         a.data + first * a.k * P, a.parity + first * a.r * P, a.rec_off + first, a.row_start + first, records, gn,
                         a.P, a.k, a.r, m0, a.out, static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
    }
  });
}

// The one-word call's classify: over the dense codebook's levels, or (device plan) over an all-zero
// level table, which leaves 0 where a record is to be built.
hipError_t run_classify_packed(const PackedLaunch& a, hipStream_t s) {
  DecodeLaunch c{};
  c.masks = a.masks, c.rec_off = a.rec_off, c.status = a.status;
  c.groups = a.groups, c.k = a.k, c.r = a.r, c.P = a.P;
  c.binom = a.binom;
  if (a.path == PackedPath::kCodebook) c.meta = a.meta;
  return launch_classify(c, s);
}

WideLaunch wide_view(const PackedLaunch& a) {
  WideLaunch w{};
  w.masks = a.masks, w.rec_off = a.rec_off, w.status = a.status;
  w.groups = a.groups, w.k = a.k, w.r = a.r, w.P = a.P;
  w.plan = a.plan;
  return w;
}

}  // namespace

hipError_t launch_recover_packed(const PackedLaunch& a, hipStream_t s) {
  if (a.data == nullptr || a.parity == nullptr || a.masks == nullptr || a.out == nullptr || a.row_start == nullptr ||
      a.block_sums == nullptr || a.rec_off == nullptr || a.groups == 0 || a.groups >= (1ull << 32) || a.P < kVecMinP ||
      !packed_rows_fit(a.groups, a.k, a.r))
    return hipErrorInvalidValue;
  const bool one_word = a.path == PackedPath::kCodebook || a.path == PackedPath::kDevicePlan;
  // a slot holds the shape's largest record and a chunk has at most per_chunk groups (for_plan_chunks):
  // every record lies inside the arena
  if (a.path != PackedPath::kCodebook &&
      (a.plan.arena == nullptr || a.plan.matrix == nullptr || a.plan.per_chunk == 0 ||
       a.plan.stride != packed_arena(a.path, a.k, a.r, a.groups, kPlanArenaBytes).stride))
    return hipErrorInvalidValue;
  if (one_word) {
    if (a.k == 0 || a.r == 0 || a.k + a.r > kPackedMaxShards || a.binom == nullptr) return hipErrorInvalidValue;
    if (a.path == PackedPath::kCodebook && a.codebook == nullptr) return hipErrorInvalidValue;
    const hipError_t e = launch_rows_prefix(a.masks, a.groups, a.k, a.r, a.row_start, a.block_sums, a.total, s);
    if (e != hipSuccess) return e;
    if (a.path == PackedPath::kCodebook) {
      const hipError_t ce = run_classify_packed(a, s);
      return ce != hipSuccess ? ce : run_recover_packed<false>(a, a.codebook, 0, a.groups, s);
    }
    return for_plan_chunks(
        a.groups, a.plan.per_chunk, [&] { return run_classify_packed(a, s); },
        [&](uint64_t c0, uint64_t cn) {
          return launch_build_records(a.plan, a.masks + c0, a.rec_off + c0, a.status ? a.status + c0 : nullptr, c0, cn, a.k, a.r, s);
        },
        [&](uint64_t c0, uint64_t cn) { return run_recover_packed<false>(a, a.plan.arena, c0, cn, s); });
  }
  if (a.path != PackedPath::kWide && a.path != PackedPath::kDeep) return hipErrorInvalidValue;
  const WidePath want = a.path == PackedPath::kDeep ? WidePath::kDeep : WidePath::kWide;
  if (wide_route(kWideRowsAll, a.groups, a.k, a.r, a.P).path != want) return hipErrorInvalidValue;
  const hipError_t e = run_rows_prefix_wide(a, s);
  if (e != hipSuccess) return e;
  const WideLaunch w = wide_view(a);
  return for_plan_chunks(
      a.groups, a.plan.per_chunk, [&] { return launch_classify_wide(w, s); },
      [&](uint64_t c0, uint64_t cn) {
        return a.path == PackedPath::kDeep ? launch_build_records_deep(a.plan, a.masks, a.rec_off, a.status, c0, cn, a.k, a.r, s)
                                           : launch_build_records_wide(a.plan, a.masks, a.rec_off, a.status, c0, cn, a.k, a.r, s);
      },
      [&](uint64_t c0, uint64_t cn) { return run_recover_packed<true>(a, a.plan.arena, c0, cn, s); });
}

}  // namespace qfec
