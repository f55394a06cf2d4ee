// fec_varlen.hpp — the length-masked piece load of the variable-length address-table calls
// (fec_recover_gather_var_rs_dev, fec_encode_gather_var_rs_dev; fec_gather_var.hip).
//
// A shard of `len` readable bytes stands for the P-byte symbol  byte i = i < len ? p[i] : 0.  A
// lane's piece is the NB = 4 or 16 bytes at byte offset `off` of that symbol (any `off`: tail
// pieces are shifted back to end at P).  var_window decides where the lane reads:
//   kNone   off >= len: nothing is read, the piece is zero;
//   kFull   the piece lies inside [0, len): one NB-byte load at `off`;
//   kBack   the piece crosses `len` and len >= NB: one NB-byte load of [len - NB, len), the value
//           moved down by off - (len - NB) bytes and zero-filled above;
//   kBytes  the piece crosses `len` and len < NB: byte loads of [off, len).
// No byte at or past p + len is read in any case, and with len = 0 `p` is never dereferenced.
// var_load assembles the piece from the window through the caller's loads; the kernels call it
// and nothing else decides where a lane reads.  Plain C++ with no HIP dependency, so a host
// program checks every (NB, len, off) against the byte-wise definition under AddressSanitizer
// (tests/csrc/varlen_window_test.cpp).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define QFEC_HD __host__ __device__ __forceinline__
#else
#define QFEC_HD inline
#endif

namespace qfec {

enum class VarKind : uint32_t { kNone = 0, kFull = 1, kBack = 2, kBytes = 3 };

struct VarWindow {
  VarKind kind;
  uint32_t at;  // byte offset of the first byte read (kFull, kBack, kBytes)
  uint32_t n;   // kBack: bytes the loaded value moves down (1 .. NB - 1); kBytes: bytes read (1 .. NB - 1)
};

template <int NB>
QFEC_HD VarWindow var_window(uint32_t off, uint32_t len) {
  if (off >= len) return {VarKind::kNone, 0u, 0u};
  if (len - off >= static_cast<uint32_t>(NB)) return {VarKind::kFull, off, 0u};
  if (len >= static_cast<uint32_t>(NB)) return {VarKind::kBack, len - NB, off - (len - NB)};
  return {VarKind::kBytes, off, len - off};
}

// v (NW little-endian dwords) moved down by `bytes` (0 .. 4 * NW - 1), zeros moving in from above.
template <int NW>
QFEC_HD void var_shift_down(uint32_t (&v)[NW], uint32_t bytes) {
  if constexpr (NW == 4) {
    if (bytes & 4u) v[0] = v[1], v[1] = v[2], v[2] = v[3], v[3] = 0u;
    if (bytes & 8u) v[0] = v[2], v[1] = v[3], v[2] = 0u, v[3] = 0u;
  }
  const uint32_t bits = (bytes & 3u) * 8u;
  for (int q = 0; q < NW; ++q) {
    const uint64_t pair = (static_cast<uint64_t>(q + 1 < NW ? v[q + 1] : 0u) << 32) | v[q];
    v[q] = static_cast<uint32_t>(pair >> bits);
  }
}

// The piece at `off` of the shard (p, len) into v.  ld(q, v) loads NW dwords from q (any
// alignment); ldb(q) loads the byte at q.
template <int NW, typename LD, typename LDB>
QFEC_HD void var_load(const uint8_t* p, uint32_t off, uint32_t len, uint32_t (&v)[NW], LD ld, LDB ldb) {
  constexpr int NB = 4 * NW;
  const VarWindow w = var_window<NB>(off, len);
  for (int q = 0; q < NW; ++q) v[q] = 0u;
  if (w.kind == VarKind::kFull || w.kind == VarKind::kBack) {
    ld(p + w.at, v);
    if (w.kind == VarKind::kBack) var_shift_down<NW>(v, w.n);
  } else if (w.kind == VarKind::kBytes) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < NB - 1; ++i)  // constant indices into v: the piece stays in registers
      if (static_cast<uint32_t>(i) < w.n) v[i >> 2] |= static_cast<uint32_t>(ldb(p + w.at + i)) << (8 * (i & 3));
  }
}

}  // namespace qfec
