// fec_wide_encode.hip — gfx950 kernel of fec_encode_scatter_wide_rs_dev: the scatter encode
// (fec_scatter_encode.hip) for groups of up to 256 shards, k + r <= 256 with no cap on min(k, r).
// Packets are taken where they lie, through a table of addresses (0 = absent, counts as zeros) with
// a nullable table of lengths; every parity row goes where a table of destinations says, exactly
// the group's symbol length L of it.  An encode builds no record: its "record" is the shape's static
// r x k coefficient table (row 0, the ones, as entries like any other row), its "survivors" the k
// packets, its "lost rows" the r parity rows.
//
//  * encode_scatter_wide<POL, VAR>: recover_scatter_wide's form (fec_wide_table.hip).  One wave per
//    group, four per workgroup, runtime k, groups in decode_block's XCD-aware order, 8 rows per pass
//    (kWidePassRows), so ceil(r / 8) launches.  Per pass the lanes stride once over j < k: address j,
//    and its clamped length when VAR, go into per-wave LDS slices, and in that same sweep the wave
//    forms L (the longest present packet) and the shortest packet, both wave-uniform.  The wave of
//    the first pass writes L out.  A group with L = 0 leaves there, before any destination entry or
//    packet byte is read.  Then the pass's up-to-8 destinations (rows m0 .. m0 + 7 below r) are
//    fetched; a pass none of whose rows is wanted leaves before any packet load (wave-uniform).  The
//    slices of a workgroup are the recover's: 4 x 256 u64 of addresses (8,192 B), 4 x 256 u32 of
//    lengths when VAR (4,096 B), 4 x 8 u64 of destinations (256 B) and 2 x 4 u32 (32 B): 12,576 B.
//    The walk is scatter_decode's over [0, L) (fec_scatter_decode.hpp); which bytes are stored is
//    fec_scatter_cut.hpp's; the arithmetic is decode_piece<0, 8, POL, NW> unchanged, r = 1 on its XOR
//    path (no table).  Not tuned.
//
// Absent packets: an absent packet counts as a packet of length 0 in the sweep, with or without a
// length table.  So the shortest length of a group with an absent packet is 0, no pass of it takes
// the plain (unmasked) loads, and every load of it goes through load_masked (fec_table.hpp), which
// dereferences nothing at length 0: with a length table from the length slice (VarSurvivorsLds),
// without one from the address alone (PresentPackets: P when present, 0 when absent).  A group
// whose packets are all present and at least as long as a pass's end takes the plain loads there.
// (encode_scatter's other way, loading a present packet in the absent one's place and zeroing the
// value, is not used.)
//
// An absent packet's address, a present packet of length 0 and a destination of 0 are never
// dereferenced; an absent packet's length entry is read and ignored.
//
// Algorithmic bytes per group: packet reads k * L * ceil(r / 8) (passes with a wanted row), the
// table rows k * 8 (with lengths * 12) + 8 * 8 per pass, r * k * 32 of coefficient table per walk
// pass, writes r * L.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"
#include "fec_forms.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_scatter_cut.hpp"
#include "fec_scatter_decode.hpp"  // ScatterDst, scatter_decode
#include "fec_table.hpp"
#include "fec_varlen.hpp"

namespace qfec {
namespace {

static_assert(kWidePassRows == 8, "encode_scatter_wide forms decode_piece<0, 8>'s rows per pass");

// Without a length table: a group's packets as decode_piece's loading functor when one of them is
// absent.  A present packet has P bytes, an absent one none (load_masked then reads nothing).
struct PresentPackets {
  using loads_piece = void;
  const uint64_t* addr;
  uint32_t P;
  template <int NW, int POL>
  __device__ __forceinline__ void load(uint32_t s, uint32_t off, uint32_t (&v)[NW]) const {
    const uint64_t a = addr[s];
    load_masked<NW, POL>(shard_ptr(a), off, a != 0 ? P : 0u, v);
  }
};

// One wave per group (4 per workgroup).  `lens` is read only when VAR; `tabs` not when r == 1.
template <int POL, bool VAR>
__global__ __launch_bounds__(256) void encode_scatter_wide(const uint64_t* __restrict__ addrs,
                                                           const uint32_t* __restrict__ lens,
                                                           const uint64_t* __restrict__ dests,
                                                           uint32_t* __restrict__ symlen_out,
                                                           const Tab* __restrict__ tabs, uint64_t groups,
                                                           uint32_t P, uint32_t k, uint32_t r, uint32_t m0,
                                                           uint32_t swz) {
  constexpr int MAXE = static_cast<int>(kWidePassRows);
  __shared__ uint64_t slices[4 * kWideMaxShards];
  __shared__ uint64_t dest_slices[4 * MAXE];
  __shared__ uint32_t len_slices[VAR ? 4 * kWideMaxShards : 4];
  __shared__ uint32_t shortest[4];
  __shared__ uint32_t longest[4];
  const uint32_t wave = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  const uint64_t gw = static_cast<uint64_t>(decode_block(swz)) * 4u + wave;
  if (gw >= groups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t* __restrict__ ga = addrs + gw * k;
  const uint64_t* __restrict__ gd = dests + gw * r;
  uint64_t* slice = slices + wave * kWideMaxShards;
  uint64_t* dest_slice = dest_slices + wave * MAXE;
  uint32_t* len_slice = len_slices + (VAR ? wave * kWideMaxShards : 0u);
  if (lane == 0) shortest[wave] = P, longest[wave] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  for (uint32_t j = lane; j < k; j += 64u) {  // packet j, k <= 255
    const uint64_t a = ga[j];
    uint32_t l = P;
    if constexpr (VAR) l = min_u32(lens[gw * k + j], P);
    l = a != 0 ? l : 0u;  // absent: length 0, whatever its length entry says
    slice[j] = a;
    if constexpr (VAR) len_slice[j] = l;
    atomicMin(&shortest[wave], l);
    atomicMax(&longest[wave], l);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint32_t L = __builtin_amdgcn_readfirstlane(longest[wave]);
  const uint32_t minlen = __builtin_amdgcn_readfirstlane(shortest[wave]);
  if (m0 == 0 && symlen_out != nullptr && lane == 0) symlen_out[gw] = L;
  if (L == 0) return;  // nothing to write: no destination entry read, nothing dereferenced
  const uint64_t d = lane < static_cast<uint32_t>(MAXE) && m0 + lane < r ? gd[m0 + lane] : 0;  // row m0 + lane
  if (__ballot(d != 0) == 0) return;  // no row of this pass is wanted
  if (lane < static_cast<uint32_t>(MAXE)) dest_slice[lane] = d;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const auto plain = [slice](uint32_t s) { return shard_ptr(slice[s]); };
  const auto rows = [dest_slice](uint32_t m) { return dest_ptr(dest_slice[m]); };
  // VAR = true of scatter_decode in both forms: the plain loads only below the shortest packet
  if constexpr (VAR)
    scatter_decode<0, MAXE, POL, true>(nullptr, tabs, k, P, lane, r, m0, r == 1u, L, minlen, plain,
                                       VarSurvivorsLds{slice, len_slice}, rows);
  else
    scatter_decode<0, MAXE, POL, true>(nullptr, tabs, k, P, lane, r, m0, r == 1u, L, minlen, plain,
                                       PresentPackets{slice, P}, rows);
}

template <int POL, bool VAR>
hipError_t run_encode_scatter_wide(const WideEncodeLaunch& a, const WideEncodeForm& f, hipStream_t s) {
  return for_wave_passes(a.groups, a.r, f.pass_rows, [&](uint64_t g0, uint64_t gn, uint64_t bn, uint32_t m0) {
    LaunchRecord t = launch_record(static_cast<int64_t>(WideEncodeLaunchForm::kEncodeScatterWide), bn, 256, g0, gn);
    t.k = 0, t.r = kWidePassRows, t.first = VAR, t.pol = POL, t.aux = m0;
    trace_launch(t);
    hipLaunchKernelGGL((encode_scatter_wide<POL, VAR>), dim3(static_cast<uint32_t>(bn)), dim3(256), 0, s,
                       a.addrs + g0 * a.k, VAR ? a.lens + g0 * a.k : nullptr, a.dests + g0 * a.r,
                       a.symlen_out ? a.symlen_out + g0 : nullptr, static_cast<const Tab*>(a.tables), gn, a.P, a.k,
                       a.r, m0, static_cast<uint32_t>(kDecodeWaveXcdSwizzle));
  });
}

}  // namespace

// The passes of wide_encode_form (fec_forms.hpp).  This only launches what is decided there.
hipError_t launch_encode_scatter_wide(const WideEncodeLaunch& a, hipStream_t s) {
  if (wide_encode_served(a.groups, a.k, a.r, a.P) != WideEncodeRefusal::kServed || a.addrs == nullptr || a.dests == nullptr)
    return hipErrorInvalidValue;
  const WideEncodeForm f = wide_encode_form(a.k, a.r, a.P, a.lens != nullptr);
  if (!f.supported || f.pass_rows != kWidePassRows || (!f.xor_only && a.tables == nullptr)) return hipErrorInvalidValue;
  if (f.POL != kWideEncodePol) return hipErrorNotSupported;
  return f.VAR ? run_encode_scatter_wide<kWideEncodePol, true>(a, f, s)
               : run_encode_scatter_wide<kWideEncodePol, false>(a, f, s);
}

}  // namespace qfec
