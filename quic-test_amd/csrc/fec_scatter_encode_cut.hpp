// fec_scatter_encode_cut.hpp — which bytes a lane stores in the scatter encode
// (fec_encode_scatter_rs_dev, fec_scatter_encode.hip): parity row i of group g goes to a
// destination of the caller's, exactly L bytes of it (L = the group's symbol length), at any byte
// alignment.  The row's bytes past L are zero by construction, so they are neither loaded for nor
// stored.
//
// One lane holds one 16-B column of a group (column c of ceil(P / 16)); scatter_encode_piece says
// what the lane of column c does at symbol length L:
//   L >= 16     column c < ceil(L / 16) holds the 16 bytes at min(16c, L - 16) and stores them whole
//               (kColumn): the last column is shifted back to end at L and rewrites a neighbour's
//               bytes with the same values.  Columns with 16c >= L do nothing (kNone).
//   4 <= L < 16 column 0 alone holds the piece at offset 0 (kDwords) and stores ceil(L / 4) dwords
//               at 0, 4, ..., the last shifted back to L - 4.  The dword stored at offset o is the
//               piece's bytes [o, o + 4): scatter_encode_dword moves the piece down by o bytes
//               (var_shift_down, fec_varlen.hpp) and takes its first dword, so a shifted-back dword
//               (o no multiple of 4) comes from the two dwords it straddles.
//   1 <= L < 4  column 0 stores bytes 0 .. L - 1 of the piece at offset 0 (kBytes).
//   L == 0      nothing.
// Every store lies inside [0, L), so scatter_encode_store never touches a byte before the
// destination or at or past destination + L; a destination of NULL ("not wanted") is never
// dereferenced.  The kernel calls these and nothing else decides where a lane loads its piece from
// or stores it.  Plain C++ with no HIP dependency: a host program runs every (L, column) into a
// heap block of exactly L bytes under AddressSanitizer (tests/csrc/scatter_encode_cut_test.cpp).
#pragma once

#include <cstdint>

#include "fec_varlen.hpp"  // QFEC_HD, var_shift_down

namespace qfec {

enum class EncodeCut : uint32_t { kNone = 0, kColumn = 1, kDwords = 2, kBytes = 3 };

struct EncodeCutPiece {
  EncodeCut kind;
  uint32_t off;  // byte offset of the lane's 16-B piece in the row (and in every packet)
};

QFEC_HD EncodeCutPiece scatter_encode_piece(uint32_t L, uint32_t col) {
  if (col * 16u >= L) return {EncodeCut::kNone, 0u};
  if (L >= 16u) return {EncodeCut::kColumn, col * 16u + 16u <= L ? col * 16u : L - 16u};
  return {L >= 4u ? EncodeCut::kDwords : EncodeCut::kBytes, 0u};
}

// Bytes [o, o + 4) of the piece v (16 bytes as 4 little-endian dwords), o <= 12.
QFEC_HD uint32_t scatter_encode_dword(const uint32_t (&v)[4], uint32_t o) {
  uint32_t w[4] = {v[0], v[1], v[2], v[3]};
  var_shift_down<4>(w, o);
  return w[0];
}

// The lane's piece v (the row's bytes [pc.off, pc.off + 16), zero past L) to dst.  st16(q, v)
// stores 4 dwords at q, st4(q, d) one dword, stb(q, b) one byte (any alignment).
template <typename ST16, typename ST4, typename STB>
QFEC_HD void scatter_encode_store(uint8_t* dst, EncodeCutPiece pc, uint32_t L, const uint32_t (&v)[4], ST16 st16,
                                  ST4 st4, STB stb) {
  if (dst == nullptr || pc.kind == EncodeCut::kNone) return;
  if (pc.kind == EncodeCut::kColumn) {
    st16(dst + pc.off, v);
  } else if (pc.kind == EncodeCut::kDwords) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < 4u; ++q) {
      if (q * 4u < L) {
        const uint32_t o = q * 4u + 4u <= L ? q * 4u : L - 4u;
        st4(dst + o, scatter_encode_dword(v, o));
      }
    }
  } else {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 3u; ++i)
      if (i < L) stb(dst + i, static_cast<uint8_t>(v[0] >> (8u * i)));
  }
}

}  // namespace qfec
