// scatter_encode_cut_test.cpp — which bytes a lane of the scatter encode stores
// (csrc/fec_scatter_encode_cut.hpp), with no GPU.
//
// For P in {16, 17, 260, 1025, 1200, 2100} and every L in 0..P: the destination is a heap block of
// exactly L bytes (filled 0xEE); every column 0..ceil(P/16)-1 asks scatter_encode_piece(L, column)
// for its piece and stores it through scatter_encode_store, the piece being the 16 bytes at its
// offset of the expected row  byte i = i < L ? expected(P, L, i) : 0  (non-zero below L, as a parity
// row is zero past the symbol length).  Afterwards every byte of [0, L) must hold its expected value.
// Built plain and with -fsanitize=address,undefined (tests/test_scatter_encode_forms.py): the block
// begins at dst and ends at dst + L, so a store before it or at or past its end is a report.  With
// L = 0 the block pointer is replaced by an address that must never be dereferenced.  Every (P, L)
// is run a second time with a NULL destination ("not wanted"): nothing may be stored.
// scatter_encode_dword is also checked alone, at every offset 0..12 of a piece.
// Prints how many fell to each case, then "ok":
//   column      (P, L, column) whose 16-B piece is stored whole at 16 * column
//   columnback  (P, L, column) whose piece is shifted back to [L - 16, L)
//   dword       dword stores of 4 <= L < 16 at their own place 0, 4, ...
//   dwordback   dword stores of 4 <= L < 16 shifted back to [L - 4, L)
//   byte        byte stores of 1 <= L < 4
//   none        (P, L, column) with no byte below L (both runs), every column at L = 0
//   null        (P, L, column) with a piece that met the NULL destination
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/scatter_encode_cut_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "fec_scatter_encode_cut.hpp"

using namespace qfec;

namespace {

enum Case { kColumn, kColumnBack, kDword, kDwordBack, kByte, kNone, kNull, kCases };
uint64_t g_count[kCases];

uint8_t expected(uint32_t P, uint32_t L, uint32_t i) {
  return i < L ? static_cast<uint8_t>(1 + (i * 37u + L * 11u + P) % 255u) : 0;
}

// Every column of (P, L) into dst (nullptr: not wanted).  false: a piece outside [0, L) or a store
// of a kind its piece does not have.
bool run(uint32_t P, uint32_t L, uint8_t* dst) {
  bool ok = true;
  const uint32_t cpp = (P + 15u) / 16u;
  for (uint32_t col = 0; col < cpp; ++col) {
    const EncodeCutPiece pc = scatter_encode_piece(L, col);
    if (pc.kind == EncodeCut::kNone) {
      if (col * 16u < L) ok = false;  // a column with bytes below L has a piece
      ++g_count[kNone];
    } else {
      if (col * 16u >= L) ok = false;
      if (pc.kind == EncodeCut::kColumn && (pc.off + 16u > L || L < 16u)) ok = false;  // the loads stay below L <= P too
      if (pc.kind != EncodeCut::kColumn && (pc.off != 0u || col != 0u || L >= 16u)) ok = false;
      if ((pc.kind == EncodeCut::kBytes) != (L < 4u)) ok = false;
    }
    uint8_t b[16];
    for (uint32_t i = 0; i < 16u; ++i) b[i] = expected(P, L, pc.off + i);
    uint32_t v[4];
    std::memcpy(v, b, sizeof(b));
    uint32_t stores = 0;
    scatter_encode_store(
        dst, pc, L, v,
        [&](uint8_t* q, const uint32_t(&w)[4]) {
          if (pc.kind != EncodeCut::kColumn || q != dst + pc.off) ok = false;
          std::memcpy(q, w, sizeof(w));  // 16 bytes at q, as the kernel's dwordx4 store
          ++stores;
          ++g_count[pc.off == col * 16u ? kColumn : kColumnBack];
        },
        [&](uint8_t* q, uint32_t d) {
          const uint32_t o = static_cast<uint32_t>(q - dst);
          if (pc.kind != EncodeCut::kDwords || o + 4u > L) ok = false;
          std::memcpy(q, &d, 4);
          ++stores;
          ++g_count[o % 4u == 0u ? kDword : kDwordBack];
        },
        [&](uint8_t* q, uint8_t x) {
          if (pc.kind != EncodeCut::kBytes || static_cast<uint32_t>(q - dst) >= L) ok = false;
          *q = x;
          ++stores;
          ++g_count[kByte];
        });
    if (dst == nullptr && pc.kind != EncodeCut::kNone) ++g_count[kNull];
    if ((dst == nullptr || pc.kind == EncodeCut::kNone) && stores != 0) ok = false;
    if (dst != nullptr && pc.kind != EncodeCut::kNone && stores == 0) ok = false;
  }
  return ok;
}

// Bytes [o, o + 4) of a piece, against memcpy.
bool dword_alone() {
  uint8_t b[16];
  for (uint32_t i = 0; i < 16u; ++i) b[i] = static_cast<uint8_t>(0x11u * i + 7u);
  uint32_t v[4];
  std::memcpy(v, b, sizeof(b));
  for (uint32_t o = 0; o <= 12u; ++o) {
    uint32_t want;
    std::memcpy(&want, b + o, 4);
    if (scatter_encode_dword(v, o) != want) return false;
  }
  return true;
}

}  // namespace

int main() {
  const uint16_t probe = 1;
  if (*reinterpret_cast<const uint8_t*>(&probe) != 1) {
    std::fprintf(stderr, "little-endian hosts only\n");
    return 2;
  }
  if (!dword_alone()) {
    std::fprintf(stderr, "scatter_encode_dword: wrong bytes\n");
    return 1;
  }
  for (uint32_t P : {16u, 17u, 260u, 1025u, 1200u, 2100u}) {
    for (uint32_t L = 0; L <= P; ++L) {
      // exactly L bytes; L = 0: an address nothing may touch
      uint8_t* block = L ? static_cast<uint8_t*>(std::malloc(L)) : nullptr;
      if (L) std::memset(block, 0xEE, L);
      uint8_t* dst = L ? block : reinterpret_cast<uint8_t*>(uintptr_t{0x10});
      if (!run(P, L, dst)) {
        std::fprintf(stderr, "P=%u L=%u: a piece outside [0, L) or a store its piece does not have\n", P, L);
        return 1;
      }
      for (uint32_t i = 0; i < L; ++i) {
        if (block[i] != expected(P, L, i)) {
          std::fprintf(stderr, "P=%u L=%u byte %u: got %02x want %02x\n", P, L, i, block[i], expected(P, L, i));
          return 1;
        }
      }
      std::free(block);
      if (!run(P, L, nullptr)) return 1;  // not wanted: nothing is dereferenced
    }
  }
  const char* names[kCases] = {"column", "columnback", "dword", "dwordback", "byte", "none", "null"};
  for (int c = 0; c < kCases; ++c) std::printf("%s %llu\n", names[c], static_cast<unsigned long long>(g_count[c]));
  std::printf("ok\n");
  return 0;
}
