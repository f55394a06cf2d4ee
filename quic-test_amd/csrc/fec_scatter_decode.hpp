// fec_scatter_decode.hpp — what the scatter recovers (recover_scatter, fec_scatter.hip;
// recover_scatter_wide, fec_wide_table.hip) and the wide scatter encode (encode_scatter_wide,
// fec_wide_encode.hip: its rows are the parity rows) share past fec_table.hpp: decode_piece's destination
// functor over a table of destinations and the walk of a wave over [0, L) with its choice of loads.
// Which bytes a lane stores stays fec_scatter_cut.hpp's.  Internal to its translation unit (unnamed
// namespace), as fec_table.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "fec_device.hpp"
#include "fec_scatter_cut.hpp"
#include "fec_table.hpp"

namespace qfec {
namespace {

// decode_piece's destination functor: rows(m) is the destination of row m0 + m (nullptr: not
// wanted).  BYTES: the byte-wise pass of L < 4.  The stores are fec_scatter_cut.hpp's.
template <typename ROWS, bool BYTES>
struct ScatterDst {
  ROWS rows;
  uint32_t lane, L;
  template <int NW, int POL>
  __device__ __forceinline__ void store(uint32_t m, uint32_t off, const uint32_t (&v)[NW]) const {
    if constexpr (BYTES) {
      static_assert(NW == 1, "the byte-wise pass rebuilds one dword");
      scatter_store_byte(rows(m), lane, L, v[0], [](uint8_t* q, uint8_t b) { *q = b; });
    } else {
      scatter_store<NW>(rows(m), off, v, [](uint8_t* q, const uint32_t(&w)[NW]) { stw<NW, POL>(q, w); });
    }
  }
};

// The walk of a wave over [0, L) (scatter_walk) with the choice of loads per pass.  VAR: a pass
// whose bytes lie below `minlen`, the shortest survivor (wave-uniform), takes `plain` (s -> base,
// unmasked loads), any other pass `masked`, as fec_gather_var.hip's var_walk.  Without a length
// table every pass takes `plain`.
template <int K, int MAXE, int POL, bool VAR, typename PLAIN, typename MASKED, typename ROWS>
__device__ __forceinline__ void scatter_decode(const uint32_t* rw, const Tab* tabs, uint32_t k, uint32_t P,
                                               uint32_t lane, uint32_t e, uint32_t m0, bool xor_only, uint32_t L,
                                               uint32_t minlen, PLAIN plain, MASKED masked, ROWS rows) {
  const auto piece = [&](auto nw, auto bytes, uint32_t end, uint32_t off) {
    constexpr int NW = decltype(nw)::value;
    const ScatterDst<ROWS, decltype(bytes)::value> dst{rows, lane, L};
    if constexpr (VAR) {
      if (end <= minlen) decode_piece<K, MAXE, POL, NW>(rw, tabs, nullptr, nullptr, nullptr, k, P, off, e, m0, xor_only, plain, dst);
      else decode_piece<K, MAXE, POL, NW>(rw, tabs, nullptr, nullptr, nullptr, k, P, off, e, m0, xor_only, masked, dst);
    } else {
      decode_piece<K, MAXE, POL, NW>(rw, tabs, nullptr, nullptr, nullptr, k, P, off, e, m0, xor_only, plain, dst);
    }
  };
  using W4 = std::integral_constant<int, 4>;
  using W1 = std::integral_constant<int, 1>;
  scatter_walk(
      L, lane, [&](uint32_t base, uint32_t off) { piece(W4{}, std::false_type{}, base + 1024u, off); },
      [&](uint32_t base, uint32_t off) { piece(W1{}, std::false_type{}, min_u32(base + 256u, L), off); },
      [&]() { piece(W1{}, std::true_type{}, 4u, 0u); });
}

}  // namespace
}  // namespace qfec
