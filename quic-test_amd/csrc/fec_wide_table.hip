// fec_wide_table.hip — gfx950 kernels of fec_recover_scatter_wide_rs_dev: the scatter recover
// (fec_scatter.hip) for groups of up to 256 shards, k + r <= 256 and min(k, r) <= 32.  Shards are
// taken where they lie, through a table of addresses (0 = lost) with a nullable table of lengths;
// every rebuilt packet goes where a table of destinations says, exactly the group's symbol length
// L of it.  A wide shape has no codebook: the records are built on the device per call, by
// fec_wide.hip's build_records_wide (launch_build_records_wide), from the masks the classify here
// derives, chunk after chunk of the arena (fec_forms.hpp wide_arena, fec_launch.hpp
// for_plan_chunks).
//
//  * classify_table_wide: classify_scan (fec_table.hpp) for rows of up to 256 entries.  256 lanes =
//    256 consecutive groups, their k + r address entries one contiguous run read once by
//    consecutive lanes; a zero entry sets bit s & 63 of the group's word s >> 6 in LDS, any other
//    raises the group's symbol length.  Lane t then applies the rule of fec_mask_wide.hpp to group
//    t: rec_off (0 where a record is needed, kRecNone, kRecBad), the status, the four mask words
//    (always written: the record builder reads them) and the symbol length.  9 KiB of LDS.
//  * recover_scatter_wide<POL, VAR>: one wave per group, four per workgroup, runtime k, groups in
//    decode_block's XCD-aware order, 8 rows per pass (kWidePassRows), record-addressed through
//    WideHead.  Survivor s is the table entry of the header's id byte s, with its length when VAR;
//    both are fetched once per group into per-wave LDS slices, the lanes striding over s < k, and so
//    are the destinations of the pass, row m0 + m from the entry of erased id byte
//    kWideErasedAt + m0 + m.  The slices of a workgroup: 4 x 256 u64 of addresses (8,192 B), 4 x 256
//    u32 of lengths when VAR (4,096 B), 4 x 8 u64 of destinations (256 B) and 4 u32 (16 B): 12,560 B,
//    about 12.3 KiB against the CU's 160 KiB, so LDS is not what bounds the waves per CU.  The walk
//    is scatter_decode's over [0, L) (fec_scatter_decode.hpp): passes below the shortest survivor
//    take plain loads, every other pass var_load; which bytes are stored is fec_scatter_cut.hpp's;
//    the rebuild is decode_piece<0, 8, POL, NW> unchanged.  Not tuned.
//    With kDeepRecord among its bits the record is a deep one (fec_plan_build_deep.hpp; the erased
//    ids at fec_wide_head.hpp wide_erased_at): the consumer of the shapes with min(k, r) > 32 on a
//    context in FEC_WIDE_ROWS_ALL, whose records fec_wide_deep.hip builds.
//
// A lost shard's source entry, a parity row the rule does not use, and the destination entry of any
// shard the call does not rebuild are never read.  A destination of 0 is not stored to.
//
// Algorithmic bytes per group with e rows to rebuild: survivor reads k * L * ceil(e / 8), the table
// rows ((k + r) * 8, with lengths * 12) once and k * 8 (* 12) + e * 8 per pass, e * k * 32 of record
// per walk pass, writes e * L.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"
#include "fec_forms.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_mask_wide.hpp"
#include "fec_scatter_cut.hpp"
#include "fec_scatter_decode.hpp"  // ScatterDst, scatter_decode
#include "fec_table.hpp"
#include "fec_varlen.hpp"
#include "fec_wide_head.hpp"

namespace qfec {
namespace {

static_assert(kWideMaxShards == kWideMaskBits && kWideMaskWords == 4, "a table row is at most 256 entries, four mask words");
static_assert(kWidePassRows == 8, "recover_scatter_wide rebuilds decode_piece<0, 8>'s rows per pass");

__global__ __launch_bounds__(256) void classify_table_wide(const uint64_t* __restrict__ addrs,
                                                           const uint32_t* __restrict__ lens, uint64_t groups,
                                                           uint32_t k, uint32_t r, uint32_t P,
                                                           uint32_t* __restrict__ rec_off,
                                                           uint8_t* __restrict__ status,
                                                           uint64_t* __restrict__ masks_out,
                                                           uint32_t* __restrict__ symlen_out) {
  // word w of group t at lost[w * 256 + t]: the LDS index is (s >> 6) * 256 + group, never a
  // register array's
  __shared__ unsigned long long lost[kWideMaskWords * 256];
  __shared__ uint32_t symlen[256];
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * 256u;
  const uint32_t gn = groups - g0 < 256u ? static_cast<uint32_t>(groups - g0) : 256u;
  const uint32_t n = k + r;
  for (uint32_t w = 0; w < kWideMaskWords; ++w) lost[w * 256u + threadIdx.x] = 0;
  symlen[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t* __restrict__ tab = addrs + g0 * n;
  const uint32_t* __restrict__ ltab = lens ? lens + g0 * n : nullptr;
  const uint32_t entries = gn * n;  // at most 256 * 256
  for (uint32_t i = threadIdx.x; i < entries; i += 256u) {
    const uint32_t grp = i / n, s = i - grp * n;
    if (tab[i] == 0) {
      atomicOr(&lost[(s >> 6) * 256u + grp], 1ull << (s & 63u));  // a lost entry's length is ignored
    } else if (symlen_out) {
      atomicMax(&symlen[grp], ltab ? min_u32(ltab[i], P) : P);
    }
  }
  __syncthreads();
  if (threadIdx.x >= gn) return;
  const uint64_t g = g0 + threadIdx.x;
  const WideMask m = {{lost[threadIdx.x], lost[256u + threadIdx.x], lost[512u + threadIdx.x], lost[768u + threadIdx.x]}};
  const MaskLosses l = wide_mask_losses(m, k, r);
  rec_off[g] = l.lost == 0 ? kRecNone : l.unrecoverable ? kRecBad : 0u;
  if (status) status[g] = l.lost != 0 && l.unrecoverable ? 1 : 0;
  uint64_t* __restrict__ mo = masks_out + g * kWideMaskWords;
  mo[0] = m.w[0], mo[1] = m.w[1], mo[2] = m.w[2], mo[3] = m.w[3];
  if (symlen_out) symlen_out[g] = symlen[threadIdx.x];
}

// One wave per group (4 per workgroup).  `lens` and `symlen` are read only when VAR.
template <int POL, bool VAR>
__global__ __launch_bounds__(256) void recover_scatter_wide(const uint64_t* __restrict__ addrs,
                                                            const uint32_t* __restrict__ lens,
                                                            const uint64_t* __restrict__ dests,
                                                            const uint32_t* __restrict__ rec_off,
                                                            const uint32_t* __restrict__ symlen,
                                                            const uint8_t* __restrict__ arena, uint64_t groups,
                                                            uint32_t P, uint32_t k, uint32_t r, uint32_t m0,
                                                            uint32_t swz) {
  constexpr int MAXE = static_cast<int>(kWidePassRows);
  __shared__ uint64_t slices[4 * kWideMaxShards];
  __shared__ uint64_t dest_slices[4 * MAXE];
  __shared__ uint32_t len_slices[VAR ? 4 * kWideMaxShards : 4];
  __shared__ uint32_t shortest[4];
  const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const uint64_t gw = static_cast<uint64_t>(decode_block(swz)) * 4u + wave;
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
  if (rec >= kRecBad) return;
  const WideHead h{reinterpret_cast<const uint32_t*>(arena + static_cast<uint64_t>(rec) * 32u)};
  const uint32_t e = h.e();
  const bool xor_only = h.xor_only();
  if (m0 >= e) return;
  uint32_t L = P;
  if constexpr (VAR) L = min_u32(__builtin_amdgcn_readfirstlane(symlen[gw]), P);
  if (L == 0) return;  // nothing to write, nothing dereferenced
  const Tab* tabs = h.tabs();
  const uint64_t* __restrict__ ga = addrs + gw * (k + r);
  const uint64_t* __restrict__ gd = dests + gw * k;
  uint64_t* slice = slices + wave * kWideMaxShards;
  uint64_t* dest_slice = dest_slices + wave * MAXE;
  uint32_t* len_slice = len_slices + (VAR ? wave * kWideMaxShards : 0u);
  const uint8_t* ids = reinterpret_cast<const uint8_t*>(h.rw);
  if (lane == 0) shortest[wave] = P;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t s = lane; s < k; s += 64u) {  // survivor s of the record, k <= 255
    const uint32_t sid = ids[s];
    slice[s] = ga[sid];
    if constexpr (VAR) {
      const uint32_t l = min_u32(lens[gw * (k + r) + sid], P);
      len_slice[s] = l;
      atomicMin(&shortest[wave], l);
    }
  }
  if (lane < MAXE) dest_slice[lane] = m0 + lane < e ? gd[ids[wide_erased_at<POL> + m0 + lane]] : 0;  // row m0 + lane of the record
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint32_t minlen = __builtin_amdgcn_readfirstlane(shortest[wave]);
  const auto plain = [slice](uint32_t s) { return shard_ptr(slice[s]); };
  const auto rows = [dest_slice](uint32_t m) { return dest_ptr(dest_slice[m]); };
  if constexpr (VAR)
    scatter_decode<0, MAXE, POL, true>(h.rw, tabs, k, P, lane, e, m0, xor_only, L, minlen, plain,
                                       VarSurvivorsLds{slice, len_slice}, rows);
  else
    scatter_decode<0, MAXE, POL, false>(h.rw, tabs, k, P, lane, e, m0, xor_only, L, P, plain, plain, rows);
}

hipError_t run_classify_table_wide(const WideTableLaunch& a, hipStream_t s) {
  const uint64_t n = a.k + a.r;
  return for_chunks(a.groups, max_launch_threads(), [&](uint64_t g0, uint64_t gn) {
    trace_launch(launch_record(static_cast<int64_t>(WideTableLaunchForm::kClassifyTableWide), blocks_for(gn), 256, g0, gn));
    hipLaunchKernelGGL(classify_table_wide, dim3(blocks_for(gn)), dim3(256), 0, s, a.addrs + g0 * n,
                       a.lens ? a.lens + g0 * n : nullptr, gn, a.k, a.r, a.P, a.rec_off + g0,
                       a.status ? a.status + g0 : nullptr, a.masks + g0 * kWideMaskWords,
                       a.symlen ? a.symlen + g0 : nullptr);
  });
}

// The row passes over groups [c0, c0 + cn), their records in the arena.  The instantiations over
// the deep record (kDeepRecord) are traced under a form of their own.
template <int POL, bool VAR>
hipError_t run_recover_scatter_wide(const WideTableLaunch& a, uint64_t c0, uint64_t cn, hipStream_t s) {
  constexpr int64_t kForm = (POL & kDeepRecord) != 0 ? static_cast<int64_t>(WideDeepLaunchForm::kRecoverScatterWideDeep)
                                                     : static_cast<int64_t>(WideTableLaunchForm::kRecoverScatterWide);
  const uint64_t n = a.k + a.r;
  const uint32_t rows = a.k < a.r ? a.k : a.r;
  return for_wave_passes(cn, rows, kWidePassRows, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    const uint64_t first = c0 + g0;
    LaunchRecord t = launch_record(kForm, bn, 256, first, gn);
    t.k = 0, t.r = kWidePassRows, t.first = VAR, t.pol = POL, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((recover_scatter_wide<POL, VAR>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                       a.addrs + first * n, VAR ? a.lens + first * n : nullptr, a.dests + first * a.k, a.rec_off + first,
                       VAR ? a.symlen + first : nullptr, a.plan.arena, gn, a.P, a.k, a.r, m0,
                       static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
  });
}

}  // namespace

// classify_table_wide and the row passes of one plan chunk for a call on the deep path
// (fec_wide_deep.hip, which has checked the launch and built the chunk's deep records).
hipError_t launch_classify_table_wide(const WideTableLaunch& a, hipStream_t s) {
  if (a.addrs == nullptr || a.masks == nullptr || a.rec_off == nullptr || a.groups == 0) return hipErrorInvalidValue;
  return run_classify_table_wide(a, s);
}
hipError_t launch_recover_scatter_wide_deep_rows(const WideTableLaunch& a, uint64_t first_group, uint64_t groups, hipStream_t s) {
  if (a.addrs == nullptr || a.dests == nullptr || a.rec_off == nullptr || a.plan.arena == nullptr ||
      (a.lens != nullptr && a.symlen == nullptr) || first_group + groups > a.groups)
    return hipErrorInvalidValue;
  return a.lens ? run_recover_scatter_wide<kWideDeepTablePol, true>(a, first_group, groups, s)
                : run_recover_scatter_wide<kWideDeepTablePol, false>(a, first_group, groups, s);
}

hipError_t launch_recover_scatter_wide(const WideTableLaunch& a, hipStream_t s) {
  // a slot holds the shape's largest record and a chunk has at most per_chunk groups (for_plan_chunks):
  // every record lies inside the arena
  if (wide_served(a.groups, a.k, a.r, a.P) != WideRefusal::kServed || a.addrs == nullptr || a.dests == nullptr ||
      a.masks == nullptr || a.rec_off == nullptr || a.plan.arena == nullptr || a.plan.matrix == nullptr ||
      a.plan.per_chunk == 0 || a.plan.stride != wide_slot_stride(a.k, a.r))
    return hipErrorInvalidValue;
  if (a.lens != nullptr && a.symlen == nullptr) return hipErrorInvalidValue;  // the kernel reads the symbol lengths
  return for_plan_chunks(
      a.groups, a.plan.per_chunk, [&] { return run_classify_table_wide(a, s); },
      [&](uint64_t c0, uint64_t cn) {
        return launch_build_records_wide(a.plan, a.masks, a.rec_off, a.status, c0, cn, a.k, a.r, s);
      },
      [&](uint64_t c0, uint64_t cn) {
        return a.lens ? run_recover_scatter_wide<kWideTablePol, true>(a, c0, cn, s)
                      : run_recover_scatter_wide<kWideTablePol, false>(a, c0, cn, s);
      });
}

}  // namespace qfec
