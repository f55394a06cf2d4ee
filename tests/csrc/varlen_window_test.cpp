// varlen_window_test.cpp — the length-masked piece load of the variable-length address-table
// calls (csrc/fec_varlen.hpp) against its byte-wise definition, with no GPU.
//
// For NB in {4, 16}, every len in 0..96 and every off in 0..96: the packet is a heap block of
// exactly `len` non-zero bytes; the piece assembled by var_load through host loads must equal
//   byte i of the piece = off + i < len ? p[off + i] : 0.
// Built plain and with -fsanitize=address,undefined (tests/test_gather_var_forms.py): the heap
// block ends at p + len, so a read at or past it is a report -- the no-over-read rule.  With
// len = 0 the block pointer is replaced by an address that must never be dereferenced.
// Prints one line per (NB, kind) with the number of windows of that kind, then "ok".
//
// Build: g++ -std=c++17 -I quic-test_amd/csrc tests/csrc/varlen_window_test.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fec_varlen.hpp"

using namespace qfec;

namespace {

uint64_t g_kinds[2][4];
uint64_t g_loads, g_byte_loads;

template <int NW>
bool check(const uint8_t* p, uint32_t off, uint32_t len) {
  constexpr int NB = 4 * NW;
  uint32_t v[NW];
  for (int q = 0; q < NW; ++q) v[q] = 0xDEADBEEFu;
  var_load<NW>(
      p, off, len, v,
      [](const uint8_t* q, uint32_t(&w)[NW]) {
        ++g_loads;
        std::memcpy(w, q, sizeof(w));  // NB bytes at q, as the kernels' dword / dwordx4 loads
      },
      [](const uint8_t* q) {
        ++g_byte_loads;
        return *q;
      });
  uint8_t got[NB];
  std::memcpy(got, v, NB);  // little-endian dwords, as on the device
  for (int i = 0; i < NB; ++i) {
    const uint8_t want = off + i < len ? p[off + i] : 0;
    if (got[i] != want) {
      std::fprintf(stderr, "NB=%d len=%u off=%u byte %d: got %02x want %02x\n", NB, len, off, i, got[i], want);
      return false;
    }
  }
  ++g_kinds[NW == 4][static_cast<uint32_t>(var_window<NB>(off, len).kind)];
  return true;
}

}  // namespace

int main() {
  static_assert(sizeof(uint32_t) == 4, "dwords");
  const uint16_t probe = 1;
  if (*reinterpret_cast<const uint8_t*>(&probe) != 1) {
    std::fprintf(stderr, "little-endian hosts only\n");
    return 2;
  }
  for (uint32_t len = 0; len <= 96; ++len) {
    // exactly len bytes, non-zero; len = 0: an address nothing may read
    uint8_t* block = len ? static_cast<uint8_t*>(std::malloc(len)) : nullptr;
    for (uint32_t i = 0; i < len; ++i) block[i] = static_cast<uint8_t>(1 + (i * 37u + len * 11u) % 255u);
    const uint8_t* p = len ? block : reinterpret_cast<const uint8_t*>(uintptr_t{0x10});
    for (uint32_t off = 0; off <= 96; ++off) {
      if (!check<1>(p, off, len) || !check<4>(p, off, len)) return 1;
    }
    std::free(block);
  }
  const char* names[4] = {"none", "full", "back", "bytes"};
  for (int w = 0; w < 2; ++w)
    for (int kd = 0; kd < 4; ++kd)
      std::printf("NB=%d %s %llu\n", w ? 16 : 4, names[kd], static_cast<unsigned long long>(g_kinds[w][kd]));
  std::printf("loads %llu byte_loads %llu\n", static_cast<unsigned long long>(g_loads),
              static_cast<unsigned long long>(g_byte_loads));
  std::printf("ok\n");
  return 0;
}
