// fec_gather.hip — gfx950 kernels of fec_recover_gather_rs_dev: recover from shards wherever they
// are in device memory.  The caller hands over a table of absolute shard addresses, k + r per
// group (data shards, then parity rows; 0 = lost), instead of contiguous data / parity buffers
// and erasure masks.
//
//  * classify_table<Lens::kNone> (fec_table.hpp; the launch trace's classify_gather): forms each
//    group's erasure mask from its table entries (bit s set where entry s is 0); the status byte
//    and the codebook record come from classify_mask, the rule `classify` (fec_decode.hip)
//    applies to a given mask.
//  * recover_gather<K, MAXE, POL>: one wave per group, record-addressed like decode_wave.  The
//    base address of the record's survivor s is the group's table entry of that shard id, fetched
//    once per group (compile-time k: scalar loads into SGPRs; runtime k: a per-wave LDS slice)
//    and handed to decode_walk as its survivor functor; the rebuilt rows go to the compact slot
//    layout, out + (g * r + m) * P (kCompactOut).
// The rule, the record header, the piece rebuild and the walk are fec_device.hpp's, the classify
// scan and the table-entry pointer fec_table.hpp's; this file holds only what the address table
// adds to the recover.
//
// Shards may have any byte alignment (unaligned 16-B / 4-B global access, as in fec_encode.hip and fec_decode.hip)
// and P >= 16.  A lost shard's entry and a parity row the decode rule does not use are never
// dereferenced: the record lists only the k survivors it rebuilds from.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_table.hpp"

namespace qfec {
namespace {

// One wave per group (4 per workgroup).  K > 0: compile-time k, one pass of MAXE = r rows, the k
// survivor addresses in SGPRs.  K = 0: runtime k, rows [m0, m0 + MAXE) per launch, the addresses
// in the wave's LDS slice (64 entries: k + r <= 64).
template <int K, int MAXE, int POL>
__global__ __launch_bounds__(256) void recover_gather(const uint64_t* __restrict__ addrs,
                                                      const uint32_t* __restrict__ rec_off,
                                                      const uint8_t* __restrict__ codebook, uint64_t groups,
                                                      uint32_t P, uint32_t k_rt, uint32_t r, uint32_t m0,
                                                      uint8_t* __restrict__ out, uint32_t swz) {
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
  const Tab* tabs = h.tabs();
  const uint64_t* __restrict__ ga = addrs + gw * (k + r);
  uint8_t* og = out + gw * r * static_cast<uint64_t>(P);
  // decode_walk with the survivors' bases from the table; rows to the compact layout
  static_assert((POL & kCompactOut) != 0, "recover_gather writes compact rows");
  if constexpr (K > 0) {
    const uint8_t* base[K];
#pragma unroll
    for (int s = 0; s < K; ++s) base[s] = shard_ptr(ga[rec_byte(h.rw, s)]);
    const auto src = [&base](int s) { return base[s]; };
    decode_walk<K, MAXE, POL>(h.rw, tabs, nullptr, nullptr, og, k, P, lane, e, m0, xor_only, src);
  } else {
    __shared__ uint64_t slices[4 * 64];
    uint64_t* slice = slices + wave * 64u;
    if (lane < k) slice[lane] = ga[reinterpret_cast<const uint8_t*>(h.rw)[lane]];  // survivor `lane` of the record
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const auto src = [slice](uint32_t s) { return shard_ptr(slice[s]); };
    decode_walk<K, MAXE, POL>(h.rw, tabs, nullptr, nullptr, og, k, P, lane, e, m0, xor_only, src);
  }
}

template <int K, int MAXE, int POL>
hipError_t run_recover_gather(const TableRecoverLaunch& a, hipStream_t s) {
  const uint64_t n = a.k + a.r;
  return for_wave_passes(a.groups, a.r, MAXE, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    LaunchRecord t = launch_record(static_cast<int64_t>(GatherLaunchForm::kRecoverGather), bn, 256, g0, gn);
    t.k = K, t.r = MAXE, t.pol = POL, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((recover_gather<K, MAXE, POL>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                       a.addrs + g0 * n, a.rec_off + g0, a.codebook, gn, a.P, a.k, a.r, m0,
                       a.out + g0 * a.r * static_cast<uint64_t>(a.P), static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
  });
}

}  // namespace

// Which form runs is decided in fec_forms.hpp (table_recover_form); this only launches it.
hipError_t launch_recover_gather(const TableRecoverLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  const TableRecoverForm f = table_recover_form(a.k, a.r, a.P, false);
  if (!f.supported) return hipErrorInvalidValue;
  hipError_t (*run)(const TableRecoverLaunch&, hipStream_t) = nullptr;
#define QFEC_GATHER(_, KK, MM, PP) \
  if (f.K == KK && f.MAXE == MM && f.POL == (PP)) run = run_recover_gather<KK, MM, PP>;
  QFEC_TABLE_RECOVER_FORMS(QFEC_GATHER, ~)
#undef QFEC_GATHER
  if (run == nullptr) return hipErrorNotSupported;
  const auto classify = [s](const TableRecoverLaunch& c) {
    return run_classify_table<Lens::kNone>(c, static_cast<int64_t>(GatherLaunchForm::kClassifyGather), s);
  };
  return run_table_recover(a, classify, run, s);
}

}  // namespace qfec
