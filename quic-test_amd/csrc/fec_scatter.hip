// fec_scatter.hip — gfx950 kernels of fec_recover_scatter_rs_dev: recover from an address table
// (with or without a length per entry) and write every rebuilt packet where the caller's table of
// destinations says, exactly the group's symbol length L of it.  Destinations that are the holes
// of the caller's arena give in-place gathered decode, destinations back to back packed output.
//
//  * classify_table<Lens::kNullable> (fec_table.hpp; the launch trace's classify_scatter): the
//    classify scan with a nullable length table (NULL: every present shard has P bytes) -- the
//    mask, the status, the codebook record and the symbol length of each group.
//  * recover_scatter<K, MAXE, POL, VAR>: one wave per group, record-addressed like recover_gather /
//    recover_gather_var (VAR: with the length table).  The survivors' addresses (and lengths) are
//    fetched once per group as there; so are the destinations of the rows of the pass, row m0 + m
//    from the entry of shard id rec_byte(rw, 64 + m0 + m) (compile-time k: scalar loads into SGPRs;
//    runtime k: a per-wave LDS slice).  The wave walks [0, L) instead of [0, P) (scatter_walk), so
//    the rebuilt zeros past L are neither loaded for nor stored; VAR loads stay masked per shard
//    (var_load).  Which bytes a lane stores is decided in fec_scatter_cut.hpp and nowhere else.
// The rule, the record header, the piece rebuild and the GF(2^8) product are fec_device.hpp's;
// the classify scan, the table-entry pointers (shard_ptr, dest_ptr), the masked piece load and
// the survivor functors are fec_table.hpp's; the destination functor and the walk's choice of loads
// (ScatterDst, scatter_decode) are fec_scatter_decode.hpp's, shared with fec_wide_table.hip.
//
// A lost shard's source entry, a parity row the rule does not use, and the destination entry of
// any shard the call does not rebuild are never read.  A destination of 0 is not stored to.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fec_device.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_scatter_cut.hpp"
#include "fec_scatter_decode.hpp"  // ScatterDst, scatter_decode
#include "fec_table.hpp"
#include "fec_varlen.hpp"

namespace qfec {
namespace {

// One wave per group (4 per workgroup), the shapes of recover_gather.  `lens` and `symlen` are
// read only when VAR.
template <int K, int MAXE, int POL, bool VAR>
__global__ __launch_bounds__(256) void recover_scatter(const uint64_t* __restrict__ addrs,
                                                       const uint32_t* __restrict__ lens,
                                                       const uint64_t* __restrict__ dests,
                                                       const uint32_t* __restrict__ rec_off,
                                                       const uint32_t* __restrict__ symlen,
                                                       const uint8_t* __restrict__ codebook, uint64_t groups,
                                                       uint32_t P, uint32_t k_rt, uint32_t r, uint32_t m0,
                                                       uint32_t swz) {
  const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const uint64_t gw = static_cast<uint64_t>(decode_block(swz)) * 4u + wave;
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t rec = __builtin_amdgcn_readfirstlane(rec_off[gw]);
  if (rec >= kRecBad) return;
  const uint32_t k = K > 0 ? static_cast<uint32_t>(K) : k_rt;
  const RecHead h = rec_head(codebook, rec);
  const uint32_t e = h.e();
  const bool xor_only = h.xor_only();
  if (m0 >= e) return;
  uint32_t L = P;
  if constexpr (VAR) L = min_u32(__builtin_amdgcn_readfirstlane(symlen[gw]), P);
  if (L == 0) return;  // nothing to write, nothing dereferenced
  const Tab* tabs = h.tabs();
  const uint64_t* __restrict__ ga = addrs + gw * (k + r);
  const uint64_t* __restrict__ gd = dests + gw * k;
  if constexpr (K > 0) {
    uint8_t* row[MAXE];
#pragma unroll
    for (int m = 0; m < MAXE; ++m) row[m] = m0 + m < e ? dest_ptr(gd[rec_byte(h.rw, 64 + m0 + m)]) : nullptr;
    const auto rows = [&row](uint32_t m) { return row[m]; };
    if constexpr (VAR) {
      const uint32_t* __restrict__ gl = lens + gw * (k + r);
      VarSurvivors<K> sv;
      uint32_t minlen = P;
#pragma unroll
      for (int s = 0; s < K; ++s) {
        const uint32_t sid = rec_byte(h.rw, s);
        sv.base[s] = shard_ptr(ga[sid]);
        sv.len[s] = min_u32(gl[sid], P);
        minlen = min_u32(minlen, sv.len[s]);
      }
      const auto plain = [&sv](uint32_t s) { return sv.base[s]; };
      scatter_decode<K, MAXE, POL, true>(h.rw, tabs, k, P, lane, e, m0, xor_only, L, minlen, plain, sv, rows);
    } else {
      const uint8_t* base[K];
#pragma unroll
      for (int s = 0; s < K; ++s) base[s] = shard_ptr(ga[rec_byte(h.rw, s)]);
      const auto plain = [&base](uint32_t s) { return base[s]; };
      scatter_decode<K, MAXE, POL, false>(h.rw, tabs, k, P, lane, e, m0, xor_only, L, P, plain, plain, rows);
    }
  } else {
    __shared__ uint64_t slices[4 * 64];
    __shared__ uint64_t dest_slices[4 * MAXE];
    __shared__ uint32_t len_slices[VAR ? 4 * 64 : 4];
    __shared__ uint32_t shortest[4];
    uint64_t* slice = slices + wave * 64u;
    uint64_t* dest_slice = dest_slices + wave * MAXE;
    uint32_t* len_slice = len_slices + (VAR ? wave * 64u : 0u);
    const uint8_t* ids = reinterpret_cast<const uint8_t*>(h.rw);
    if (lane == 0) shortest[wave] = P;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < k) {  // survivor `lane` of the record
      const uint32_t sid = ids[lane];
      slice[lane] = ga[sid];
      if constexpr (VAR) {
        const uint32_t l = min_u32(lens[gw * (k + r) + sid], P);
        len_slice[lane] = l;
        atomicMin(&shortest[wave], l);
      }
    }
    if (lane < MAXE) dest_slice[lane] = m0 + lane < e ? gd[ids[64 + m0 + lane]] : 0;  // row m0 + lane of the record
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t minlen = __builtin_amdgcn_readfirstlane(shortest[wave]);
    const auto plain = [slice](uint32_t s) { return shard_ptr(slice[s]); };
    const auto rows = [dest_slice](uint32_t m) { return dest_ptr(dest_slice[m]); };
    if constexpr (VAR)
      scatter_decode<K, MAXE, POL, true>(h.rw, tabs, k, P, lane, e, m0, xor_only, L, minlen, plain,
                                         VarSurvivorsLds{slice, len_slice}, rows);
    else
      scatter_decode<K, MAXE, POL, false>(h.rw, tabs, k, P, lane, e, m0, xor_only, L, P, plain, plain, rows);
  }
}

template <int K, int MAXE, int POL, bool VAR>
hipError_t run_recover_scatter(const TableRecoverLaunch& a, hipStream_t s) {
  const uint64_t n = a.k + a.r;
  return for_wave_passes(a.groups, a.r, MAXE, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    LaunchRecord t = launch_record(static_cast<int64_t>(ScatterLaunchForm::kRecoverScatter), bn, 256, g0, gn);
    t.k = K, t.r = MAXE, t.first = VAR, t.pol = POL, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((recover_scatter<K, MAXE, POL, VAR>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                       a.addrs + g0 * n, VAR ? a.lens + g0 * n : nullptr, a.dests + g0 * a.k, a.rec_off + g0,
                       VAR ? a.symlen + g0 : nullptr, a.codebook, gn, a.P, a.k, a.r, m0,
                       static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
  });
}

}  // namespace

// Which form runs is decided in fec_forms.hpp (table_recover_form); this only launches it.  Every
// form of the list once without (VAR = false) and once with the length table.
hipError_t launch_recover_scatter(const TableRecoverLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  const TableRecoverForm f = table_recover_form(a.k, a.r, a.P, a.lens != nullptr);
  if (!f.supported) return hipErrorInvalidValue;
  if (f.VAR && a.symlen == nullptr) return hipErrorInvalidValue;  // the kernel reads the symbol lengths
  hipError_t (*run)(const TableRecoverLaunch&, hipStream_t) = nullptr;
#define QFEC_SCATTER(VV, KK, MM, PP) \
  if (f.K == KK && f.MAXE == MM && f.POL == (PP) && f.VAR == VV) run = run_recover_scatter<KK, MM, PP, VV>;
  QFEC_TABLE_RECOVER_FORMS(QFEC_SCATTER, false)
  QFEC_TABLE_RECOVER_FORMS(QFEC_SCATTER, true)
#undef QFEC_SCATTER
  if (run == nullptr) return hipErrorNotSupported;
  const auto classify = [s](const TableRecoverLaunch& c) {
    return run_classify_table<Lens::kNullable>(c, static_cast<int64_t>(ScatterLaunchForm::kClassifyScatter), s);
  };
  return run_table_recover(a, classify, run, s);
}

}  // namespace qfec
