// scatter_cut_test.cpp — which bytes a lane of the scatter recover stores (csrc/fec_scatter_cut.hpp),
// with no GPU.
//
// For P in {16, 17, 260, 1025, 1200, 2100} and every L in 0..P: the destination is a heap block of
// exactly L bytes (filled 0xEE); every lane 0..63 runs scatter_walk(L, lane, ...) and stores each of
// its pieces through scatter_store / scatter_store_byte, the piece being bytes of the expected
// packet  byte i = expected(P, L, i)  (non-zero).  Afterwards every byte of [0, L) must hold its
// expected value.  Built plain and with -fsanitize=address,undefined (tests/test_scatter_forms.py):
// the block begins at dst and ends at dst + L, so a store before it or at or past its end is a
// report.  With L = 0 the block pointer is replaced by an address that must never be dereferenced.
// Every (P, L) is run a second time with a NULL destination ("not wanted"): nothing may be stored.
// Prints the number of (P, L, pass, lane) stores that fell to each case, then "ok":
//   piece16    a 16-B piece of a 1-KiB pass
//   piece4     a 4-B piece of a 256-B pass at its own place
//   piece4back a 4-B tail piece shifted back to [L - 4, L)
//   byte       one byte of the byte-wise pass (L < 4, lane < L)
//   none       a lane of the byte-wise pass with lane >= L, and every lane at L = 0
//   null       a piece that met the NULL destination
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/scatter_cut_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "fec_scatter_cut.hpp"

using namespace qfec;

namespace {

enum Case { kPiece16, kPiece4, kPiece4Back, kByte, kNone, kNull, kCases };
uint64_t g_count[kCases];

uint8_t expected(uint32_t P, uint32_t L, uint32_t i) { return static_cast<uint8_t>(1 + (i * 37u + L * 11u + P) % 255u); }

// The lane's rebuilt piece at `off`: NW little-endian dwords of the expected packet.
template <int NW>
void rebuilt(uint32_t P, uint32_t L, uint32_t off, uint32_t (&v)[NW]) {
  uint8_t b[4 * NW];
  for (int i = 0; i < 4 * NW; ++i) b[i] = expected(P, L, off + i);
  std::memcpy(v, b, sizeof(b));
}

bool run(uint32_t P, uint32_t L, uint8_t* dst) {
  bool ok = true;
  for (uint32_t lane = 0; lane < kScatterLanes; ++lane) {
    uint64_t stores = 0;
    const auto piece = [&](auto nw, uint32_t base, uint32_t off, uint32_t pass) {
      constexpr int NW = decltype(nw)::value;
      if (off + 4 * NW > L || off + 4 * NW > base + pass) ok = false;  // inside [0, L) and inside its pass
      uint32_t v[NW];
      rebuilt<NW>(P, L, off, v);
      bool stored = false;
      scatter_store<NW>(dst, off, v, [&](uint8_t* q, const uint32_t(&w)[NW]) {
        std::memcpy(q, w, sizeof(w));  // 4 NW bytes at q, as the kernels' dword / dwordx4 stores
        stored = true;
      });
      ++stores;
      ++g_count[!stored ? kNull : NW == 4 ? kPiece16 : off == base + lane * 4u ? kPiece4 : kPiece4Back];
    };
    scatter_walk(
        L, lane, [&](uint32_t base, uint32_t off) { piece(std::integral_constant<int, 4>{}, base, off, 1024u); },
        [&](uint32_t base, uint32_t off) { piece(std::integral_constant<int, 1>{}, base, off, 256u); },
        [&]() {
          uint32_t v[1];
          uint8_t b[4] = {0xFF, 0xFF, 0xFF, 0xFF};  // the rebuilt piece at 0; its bytes past L are not looked at
          for (uint32_t i = 0; i < L; ++i) b[i] = expected(P, L, i);
          std::memcpy(v, b, 4);
          bool stored = false;
          scatter_store_byte(dst, lane, L, v[0], [&](uint8_t* q, uint8_t x) {
            *q = x;
            stored = true;
          });
          ++stores;
          ++g_count[stored ? kByte : dst == nullptr ? kNull : kNone];
        });
    if (stores == 0) ++g_count[kNone];  // L = 0
  }
  return ok;
}

}  // namespace

int main() {
  const uint16_t probe = 1;
  if (*reinterpret_cast<const uint8_t*>(&probe) != 1) {
    std::fprintf(stderr, "little-endian hosts only\n");
    return 2;
  }
  for (uint32_t P : {16u, 17u, 260u, 1025u, 1200u, 2100u}) {
    for (uint32_t L = 0; L <= P; ++L) {
      // exactly L bytes; L = 0: an address nothing may touch
      uint8_t* block = L ? static_cast<uint8_t*>(std::malloc(L)) : nullptr;
      if (L) std::memset(block, 0xEE, L);
      uint8_t* dst = L ? block : reinterpret_cast<uint8_t*>(uintptr_t{0x10});
      if (!run(P, L, dst)) {
        std::fprintf(stderr, "P=%u L=%u: a piece outside [0, L) or outside its pass\n", P, L);
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
  const char* names[kCases] = {"piece16", "piece4", "piece4back", "byte", "none", "null"};
  for (int c = 0; c < kCases; ++c) std::printf("%s %llu\n", names[c], static_cast<unsigned long long>(g_count[c]));
  std::printf("ok\n");
  return 0;
}
