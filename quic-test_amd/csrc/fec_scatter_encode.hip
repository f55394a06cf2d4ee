// fec_scatter_encode.hip — gfx950 kernel of fec_encode_scatter_rs_dev: encode from an address table
// (with or without a length per packet) and write every parity row where the caller's table of
// destinations says, exactly the group's symbol length L of it.  Destinations that are the holes
// behind the repair headers of the caller's send ring give repair packets in place, destinations
// back to back packed repair payloads.
//
//  * encode_scatter<0, R, FIRST, VAR>: encode_gather_var's mapping with the output cut.  One lane
//    per 16-B column of a group, flat over the launch's groups (ceil(P / 16) lanes per group: the
//    grid does not depend on the lengths, which live on the device), runtime k, rows
//    [row0, row0 + R) per launch.  A lane first forms L from its group's k table entries (VAR: the
//    largest min(len, P) of the present packets; else P when any packet is present), the lane of
//    column 0 of the first pass writes it out, and a column with no byte below L leaves before any
//    packet load.  VAR: every packet load is masked by its length (load_masked); else plain loads
//    (L = P, so the piece lies inside every present packet).  Address 0 (absent) contributes
//    zeros.  Which piece a column holds and which bytes it stores is decided in
//    fec_scatter_encode_cut.hpp and nowhere else.
// The GF(2^8) product is fec_device.hpp's; the table-entry pointers (shard_ptr, dest_ptr) and the
// masked piece load are fec_table.hpp's.
//
// An absent packet's address, a present packet of length 0 and a destination of 0 are never
// dereferenced; a group with L = 0 reads no packet and writes nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"
#include "fec_kernels.hpp"
#include "fec_knobs.hpp"
#include "fec_launch.hpp"
#include "fec_scatter_encode_cut.hpp"
#include "fec_table.hpp"
#include "fec_varlen.hpp"

namespace qfec {
namespace {

template <int K, int R, bool FIRST, bool VAR>
__global__ __launch_bounds__(256) void encode_scatter(const uint64_t* __restrict__ addrs,
                                                      const uint32_t* __restrict__ lens,
                                                      const uint64_t* __restrict__ dests,
                                                      uint32_t* __restrict__ symlen_out, uint32_t nthreads,
                                                      uint32_t cpp, uint32_t P, uint32_t k, uint32_t r_total,
                                                      uint32_t row0, const Tab* __restrict__ tabs) {
  static_assert(K == 0, "encode_scatter takes k at run time");
  constexpr int POL = kTableEncodePol;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  const uint32_t g = t / cpp;
  const uint32_t col = t - g * cpp;
  const uint64_t* __restrict__ ga = addrs + static_cast<uint64_t>(g) * k;
  const uint32_t* __restrict__ gl = VAR ? lens + static_cast<uint64_t>(g) * k : nullptr;
  // L from the group's k entries, without a branch per entry so that the loads go out together
  // (an absent packet's length entry is read and ignored).  `any`: the address of a present packet.
  uint32_t L = 0;
  uint64_t any = 0;
#pragma unroll 8
  for (uint32_t j = 0; j < k; ++j) {
    const uint64_t a = ga[j];
    if constexpr (VAR) {
      const uint32_t len = min_u32(gl[j], P);
      L = a != 0 && len > L ? len : L;
    } else {
      any = a != 0 ? a : any;
    }
  }
  if constexpr (!VAR) L = any != 0 ? P : 0u;
  if (FIRST && col == 0 && symlen_out) symlen_out[g] = L;
  const EncodeCutPiece pc = scatter_encode_piece(L, col);
  if (pc.kind == EncodeCut::kNone) return;  // no byte below L: nothing loaded, nothing stored
  uint32_t acc[R][4];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = 0;
#pragma unroll 4
  for (uint32_t j = 0; j < k; ++j) {
    const uint64_t a = ga[j];
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    if constexpr (VAR) {
      const uint32_t clamped = min_u32(gl[j], P);
      const uint32_t len = a != 0 ? clamped : 0u;  // absent: all zero, never dereferenced
      load_masked<4, POL>(shard_ptr(a), pc.off, len, x);
    } else {
      // pc.off + 16 <= L = P.  No branch per packet: an absent one loads the piece of a present
      // packet instead (there is one, L > 0) and counts as zeros.
      ldw<4, POL>(shard_ptr(a != 0 ? a : any) + pc.off, x);
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] = a != 0 ? x[q] : 0u;
    }
    SelN<4> sel;
    sel_split(x, sel);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (FIRST && i == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[0][q] ^= x[q];
      } else {
        const Tab& tb = tabs[(row0 + static_cast<uint32_t>(i) - 1u) * k + j];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] ^= gmul(sel.s0[q], sel.s1[q], sel.s2[q], tb);
      }
    }
  }
  const uint64_t* __restrict__ gd = dests + static_cast<uint64_t>(g) * r_total + row0;
#pragma unroll
  for (int i = 0; i < R; ++i)
    scatter_encode_store(
        dest_ptr(gd[i]), pc, L, acc[i], [](uint8_t* q, const uint32_t(&w)[4]) { stw<4, POL>(q, w); },
        [](uint8_t* q, uint32_t d) {
          const uint32_t w[1] = {d};
          stw<1, POL>(q, w);
        },
        [](uint8_t* q, uint8_t b) { *q = b; });
}

template <int R, bool FIRST, bool VAR>
hipError_t run_encode_scatter(const TableEncodeLaunch& a, uint32_t row0, hipStream_t s) {
  const uint32_t cpp = (a.P + 15u) / 16u;
  return for_chunks(a.groups, groups_per_launch(cpp), [&](uint64_t g0, uint64_t gn) {
    const uint32_t n = static_cast<uint32_t>(gn * cpp);
    LaunchRecord t = launch_record(static_cast<int64_t>(ScatterEncodeLaunchForm::kEncodeScatter), blocks_for(n), 256, g0, gn);
    t.k = 0, t.r = R, t.first = FIRST, t.pol = kTableEncodePol, t.direct = VAR, t.tile = 0, t.aux = row0;
    trace_launch(t);
    hipLaunchKernelGGL((encode_scatter<0, R, FIRST, VAR>), dim3(blocks_for(n)), dim3(256), 0, s, a.addrs + g0 * a.k,
                       VAR ? a.lens + g0 * a.k : nullptr, a.dests + g0 * a.r,
                       a.symlen_out ? a.symlen_out + g0 : nullptr, n, cpp, a.P, a.k, a.r, row0,
                       static_cast<const Tab*>(a.tables));
  });
}

}  // namespace

// The passes of table_encode_form (fec_forms.hpp); the first owns the XOR row.  This only
// launches what is decided there.
hipError_t launch_encode_scatter(const TableEncodeLaunch& a, hipStream_t s) {
  if (a.groups == 0) return hipSuccess;
  const TableEncodeForm f = table_encode_form(a.k, a.r, a.P, a.lens != nullptr);
  if (!f.supported) return hipErrorInvalidValue;
  return for_row_passes(a.r, [&](uint32_t row0, uint32_t rows, bool first) {
    hipError_t (*run)(const TableEncodeLaunch&, uint32_t, hipStream_t) = nullptr;
#define QFEC_SCATTER_ENCODE(FF, VV, RR) \
  if (rows == RR && first == FF && f.VAR == VV) run = run_encode_scatter<RR, FF, VV>;
    QFEC_SCATTER_ENCODE_FORMS(QFEC_SCATTER_ENCODE)
#undef QFEC_SCATTER_ENCODE
    return run == nullptr ? hipErrorNotSupported : run(a, row0, s);
  });
}

}  // namespace qfec
