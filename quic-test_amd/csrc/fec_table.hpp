// fec_table.hpp — what the address-table kernel units (fec_gather.hip, fec_gather_var.hip,
// fec_scatter.hip, fec_scatter_encode.hip, fec_wide_table.hip, fec_wide_encode.hip) share, stated once:
//  * shard_ptr / dest_ptr: a table entry as a global-memory pointer; min_u32; load_masked, the
//    piece load cut at a shard's length; VarSurvivors<K> / VarSurvivorsLds, a group's survivors
//    with their lengths as decode_piece's loading functor;
//  * classify_scan<LENS>: the scan of a workgroup's table entries into each group's erasure mask
//    (and, with a length table, its symbol length) with classify_mask on it; classify_table<LENS>,
//    the scan as a kernel, under the arguments the length mode reads; and its one launcher,
//    run_classify_table.
// The recover kernels stay whole in their units, their per-wave setup and survivor fetch
// included: moved into helpers here, these changed the instruction order of the kernels
// (profiles/table_dedupe/VERDICT.md).  Everything is internal to its translation unit (unnamed
// namespace), as fec_device.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fec_device.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_varlen.hpp"

namespace qfec {
namespace {

// A table entry as a packet pointer.  The entry is cast to a global-memory pointer first, so the
// accesses through it are global loads / stores; a pointer made straight from the integer would
// be generic (flat accesses, which also count against the LDS / scalar counter).
__device__ __forceinline__ const uint8_t* shard_ptr(uint64_t addr) {
  typedef const __attribute__((address_space(1))) uint8_t* global_u8p;
  return (const uint8_t*)reinterpret_cast<global_u8p>(addr);
}

__device__ __forceinline__ uint8_t* dest_ptr(uint64_t addr) {
  typedef __attribute__((address_space(1))) uint8_t* global_u8p;
  return (uint8_t*)reinterpret_cast<global_u8p>(addr);
}

__device__ __forceinline__ uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

// The piece at `off` of the shard (p, len): var_load over the form's loads.
template <int NW, int POL>
__device__ __forceinline__ void load_masked(const uint8_t* p, uint32_t off, uint32_t len, uint32_t (&v)[NW]) {
  var_load<NW>(
      p, off, len, v, [](const uint8_t* q, uint32_t(&w)[NW]) { ldw<NW, POL>(q, w); },
      [](const uint8_t* q) { return *q; });
}

// The survivors of a group as decode_piece's functor, loading through the mask (`loads_piece`).
// Compile-time k: bases and clamped lengths in SGPRs.
template <int K>
struct VarSurvivors {
  using loads_piece = void;
  const uint8_t* base[K];
  uint32_t len[K];
  template <int NW, int POL>
  __device__ __forceinline__ void load(uint32_t s, uint32_t off, uint32_t (&v)[NW]) const {
    load_masked<NW, POL>(base[s], off, len[s], v);
  }
};

// Runtime k: addresses and clamped lengths in the wave's two LDS slices.
struct VarSurvivorsLds {
  using loads_piece = void;
  const uint64_t* addr;
  const uint32_t* len;
  template <int NW, int POL>
  __device__ __forceinline__ void load(uint32_t s, uint32_t off, uint32_t (&v)[NW]) const {
    load_masked<NW, POL>(shard_ptr(addr[s]), off, len[s], v);
  }
};

// The length table of a classify: none (every present shard has P bytes, no symbol length is
// formed), given, or given unless NULL (NULL: every present shard has P bytes).
enum class Lens { kNone, kGiven, kNullable };

// The length table as the scan takes it: a global-memory pointer, as the kernel's argument is.
// (As a generic pointer the scan's "is there a table" test is folded, before the scan meets the
// kernel, otherwise than in a kernel that tests its own argument; the code is then not the one the
// scan had as a kernel's body.)
typedef const __attribute__((address_space(1))) uint32_t* global_u32p;

// The classify scan of a workgroup: 256 lanes = 256 consecutive groups.  The groups' table entries
// are one contiguous run, read by consecutive lanes; a zero entry sets its bit in the group's mask
// in LDS, any other raises the group's symbol length, the largest min(len, P) over its present
// entries, beside it.  Lane t then classifies group t (classify_mask).  Without a length table
// (Lens::kNone) `lens`, `P` and `symlen_out` are not read and no symbol length is kept.
template <Lens LENS>
__device__ __forceinline__ void classify_scan(const uint64_t* addrs, global_u32p lens, uint64_t groups, uint32_t k,
                                              uint32_t r, uint32_t P, const uint64_t* binom, const LevelMeta& meta,
                                              uint32_t* rec_off, uint8_t* status, uint64_t* masks_out,
                                              uint32_t* symlen_out) {
  __shared__ unsigned long long lost[256];
  __shared__ uint32_t symlen[LENS != Lens::kNone ? 256 : 1];
  const uint64_t g0 = static_cast<uint64_t>(blockIdx.x) * 256u;
  const uint32_t gn = groups - g0 < 256u ? static_cast<uint32_t>(groups - g0) : 256u;
  const uint32_t n = k + r;
  lost[threadIdx.x] = 0;
  if constexpr (LENS != Lens::kNone) symlen[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t* __restrict__ tab = addrs + g0 * n;
  const global_u32p ltab = LENS == Lens::kGiven || lens ? lens + g0 * n : nullptr;
  const uint32_t entries = gn * n;  // at most 256 * 64
  for (uint32_t i = threadIdx.x; i < entries; i += 256u) {
    if (tab[i] == 0) {
      atomicOr(&lost[i / n], 1ull << (i % n));  // a lost entry's length is ignored
    } else if constexpr (LENS != Lens::kNone) {
      atomicMax(&symlen[i / n], LENS == Lens::kGiven || ltab ? min_u32(ltab[i], P) : P);
    }
  }
  __syncthreads();
  if (threadIdx.x >= gn) return;
  const uint64_t g = g0 + threadIdx.x;
  const uint64_t m = lost[threadIdx.x];
  const Classified c = classify_mask(m, k, r, binom, meta);
  rec_off[g] = c.rec;
  if (status) status[g] = c.status;
  if (masks_out) masks_out[g] = m;
  if constexpr (LENS != Lens::kNone) {
    if (symlen_out) symlen_out[g] = symlen[threadIdx.x];
  }
}

// The scan as a kernel, classify_table<LENS>, under one of two argument lists.  With a length
// table (Lens::kGiven, Lens::kNullable) ...
template <Lens LENS, std::enable_if_t<LENS != Lens::kNone, int> = 0>
__global__ __launch_bounds__(256) void classify_table(const uint64_t* __restrict__ addrs,
                                                      const uint32_t* __restrict__ lens, uint64_t groups,
                                                      uint32_t k, uint32_t r, uint32_t P,
                                                      const uint64_t* __restrict__ binom, LevelMeta meta,
                                                      uint32_t* __restrict__ rec_off,
                                                      uint8_t* __restrict__ status,
                                                      uint64_t* __restrict__ masks_out,
                                                      uint32_t* __restrict__ symlen_out) {
  classify_scan<LENS>(addrs, (global_u32p)lens, groups, k, r, P, binom, meta, rec_off, status, masks_out, symlen_out);
}

// ... and without one (Lens::kNone) only the arguments the scan then reads, so that no dead
// argument shifts the others in the kernel's argument segment.
template <Lens LENS, std::enable_if_t<LENS == Lens::kNone, int> = 0>
__global__ __launch_bounds__(256) void classify_table(const uint64_t* __restrict__ addrs, uint64_t groups,
                                                      uint32_t k, uint32_t r,
                                                      const uint64_t* __restrict__ binom, LevelMeta meta,
                                                      uint32_t* __restrict__ rec_off,
                                                      uint8_t* __restrict__ status,
                                                      uint64_t* __restrict__ masks_out) {
  classify_scan<LENS>(addrs, nullptr, groups, k, r, 0, binom, meta, rec_off, status, masks_out, nullptr);
}

// The classify of a table recover, with a.lens and a.symlen as LENS reads them; `form` is the id
// the caller's launch trace records for it.
template <Lens LENS>
hipError_t run_classify_table(const TableRecoverLaunch& a, int64_t form, hipStream_t s) {
  const uint64_t n = a.k + a.r;
  return for_chunks(a.groups, max_launch_threads(), [&](uint64_t g0, uint64_t gn) {
    trace_launch(launch_record(form, blocks_for(gn), 256, g0, gn));
    uint8_t* status = a.status ? a.status + g0 : nullptr;
    uint64_t* masks_out = a.masks_out ? a.masks_out + g0 : nullptr;
    if constexpr (LENS == Lens::kNone) {
      hipLaunchKernelGGL(classify_table<LENS>, dim3(blocks_for(gn)), dim3(256), 0, s, a.addrs + g0 * n, gn, a.k, a.r,
                         a.binom, a.meta, a.rec_off + g0, status, masks_out);
    } else {
      hipLaunchKernelGGL(classify_table<LENS>, dim3(blocks_for(gn)), dim3(256), 0, s, a.addrs + g0 * n,
                         a.lens ? a.lens + g0 * n : nullptr, gn, a.k, a.r, a.P, a.binom, a.meta, a.rec_off + g0,
                         status, masks_out, a.symlen ? a.symlen + g0 : nullptr);
    }
  });
}

// The launches of a table recover once its form is chosen: classify(a) -- the call's
// run_classify_table -- then run(a, s), every pass of its kernel.  With records built on the device
// (a.plan.arena set, fec_forms.hpp PlanLaunch): the classify on an all-zero level table (0 where a
// record is needed, else kRecNone / kRecBad; status, masks and symbol lengths as ever), then per
// chunk of the arena build_records from the masks the classify wrote and run() on the chunk
// (plan_chunk: rec_ready, the arena as codebook).
template <typename C>
hipError_t run_table_recover(const TableRecoverLaunch& a, C classify,
                             hipError_t (*run)(const TableRecoverLaunch&, hipStream_t), hipStream_t s) {
  if (a.plan.arena == nullptr) {
    const hipError_t e = a.rec_ready ? hipSuccess : classify(a);
    return e != hipSuccess ? e : run(a, s);
  }
  if (a.masks_out == nullptr || a.plan.per_chunk == 0) return hipErrorInvalidValue;
  return for_plan_chunks(
      a.groups, a.plan.per_chunk,
      [&] {
        TableRecoverLaunch c = a;
        c.meta = LevelMeta{};
        return classify(c);
      },
      [&](uint64_t g0, uint64_t gn) {
        return launch_build_records(a.plan, a.masks_out + g0, a.rec_off + g0, a.status ? a.status + g0 : nullptr, g0, gn,
                                    a.k, a.r, s);
      },
      [&](uint64_t g0, uint64_t gn) { return run(plan_chunk(a, g0, gn), s); });
}

}  // namespace
}  // namespace qfec
