// fec_scatter_cut.hpp — which bytes a lane stores in the scatter recovers (fec_recover_scatter_rs_dev,
// fec_scatter.hip; fec_recover_scatter_wide_rs_dev, fec_wide_table.hip): a rebuilt packet goes to a destination of the caller's, exactly L bytes of it
// (L = the group's symbol length, wave-uniform), at any byte alignment.
//
// scatter_walk is the walk of one wave (64 lanes) over [0, L) instead of [0, P): the rebuilt bytes
// past L are zero by construction, so they are neither loaded for nor stored.
//   L >= 4   whole 1 KiB passes of one 16-B piece per lane, then the remainder (< 1 KiB) in 256-B
//            passes of one 4-B piece per lane, tail pieces past L shifted back to [L - 4, L) (a
//            neighbour's bytes, same values): decode_walk's walk with L for P;
//   L = 1..3 one pass: every lane rebuilds the 4-B piece at offset 0 and lane i < L stores byte i;
//   L = 0    nothing.
// Every piece lies inside [0, L), so scatter_store / scatter_store_byte never touch a byte before
// the destination or at or past destination + L (the wide scatter encode, fec_wide_encode.hip, stores
// its parity rows through them too); a destination of NULL ("not wanted") is never
// dereferenced.  The kernels call these and nothing else decides where a lane stores.  Plain C++
// with no HIP dependency: a host program runs every (L, lane) into a heap block of exactly L bytes
// under AddressSanitizer (tests/csrc/scatter_cut_test.cpp).
#pragma once

#include <cstdint>

#include "fec_varlen.hpp"  // QFEC_HD

namespace qfec {

constexpr uint32_t kScatterLanes = 64;

// piece16(base, off) / piece4(base, off): the lane's 16-B / 4-B piece at byte offset `off` of the
// pass that covers [base, min(base + 1024 or 256, L)); bytes(): the byte-wise pass of L < 4.
template <typename F16, typename F4, typename FB>
QFEC_HD void scatter_walk(uint32_t L, uint32_t lane, F16 piece16, F4 piece4, FB bytes) {
  if (L < 4u) {
    if (L != 0u) bytes();
    return;
  }
  const uint32_t main_end = L & ~1023u;
  for (uint32_t base = 0; base < main_end; base += 1024u) piece16(base, base + lane * 16u);
  for (uint32_t base = main_end; base < L; base += 256u) {
    const uint32_t o = base + lane * 4u;
    piece4(base, o + 4u <= L ? o : L - 4u);
  }
}

// The lane's piece v (NW dwords: the rebuilt bytes [off, off + 4 NW)) to dst + off.  st(q, v)
// stores NW dwords at q (any alignment).
template <int NW, typename ST>
QFEC_HD void scatter_store(uint8_t* dst, uint32_t off, const uint32_t (&v)[NW], ST st) {
  if (dst != nullptr) st(dst + off, v);
}

// The byte-wise pass (L < 4): v is the rebuilt piece at offset 0, lane i < L stores its byte i.
// stb(q, b) stores the byte b at q.
template <typename STB>
QFEC_HD void scatter_store_byte(uint8_t* dst, uint32_t lane, uint32_t L, uint32_t v, STB stb) {
  if (dst != nullptr && lane < L) stb(dst + lane, static_cast<uint8_t>(v >> (8u * lane)));
}

}  // namespace qfec
