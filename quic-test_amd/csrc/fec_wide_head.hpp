// fec_wide_head.hpp — the wide record's header as the kernels that consume a wide record read it
// (fec_plan_build_wide.hpp states the layout): decode_wide (fec_wide.hip), recover_scatter_wide
// (fec_wide_table.hip) and recover_packed_wide (fec_packed.hip); the deep record's (fec_plan_build_deep.hpp) is the same header but for the
// place of the erased ids, which a kernel takes from its form bits (wide_erased_at).  And a group's
// mask as the record builders load it (build_records_wide, fec_wide.hip; build_records_deep,
// fec_wide_deep.hip).  Internal to its translation unit (unnamed namespace), as fec_device.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"  // Tab
#include "fec_forms.hpp"   // kDeepRecord
#include "fec_mask_wide.hpp"
#include "fec_plan_build_deep.hpp"
#include "fec_plan_build_wide.hpp"

namespace qfec {
namespace {

struct WideHead {
  const uint32_t* rw;
  __device__ uint32_t e() const { return rw[kWideCountAt / 4u] & 0xFFu; }
  __device__ bool xor_only() const { return ((rw[kWideXorAt / 4u] >> 8) & 0xFFu) != 0; }
  __device__ const Tab* tabs() const { return reinterpret_cast<const Tab*>(reinterpret_cast<const uint8_t*>(rw) + kWideHeaderBytes); }
};
static_assert(kWideCountAt % 4u == 0 && kWideXorAt == kWideCountAt + 1u, "e and the flag are bytes 0 and 1 of one word");

// Where the erased ids start in the record a kernel with form bits POL reads.
template <int POL>
constexpr uint32_t wide_erased_at = (POL & kDeepRecord) != 0 ? kDeepErasedAt : kWideErasedAt;

// decode_piece's SRC over the contiguous layouts: the base of survivor s from the header's id
// (decode_wide, fec_wide.hip; recover_packed_wide, fec_packed.hip).
struct WideBases {
  const uint32_t* rw;
  const uint8_t* dg;
  const uint8_t* pg;
  uint32_t k, P;
  __device__ __forceinline__ const uint8_t* operator()(uint32_t s) const {
    const uint32_t sid = rec_byte(rw, s);
    return sid < k ? dg + sid * static_cast<uint64_t>(P) : pg + (sid - k) * static_cast<uint64_t>(P);
  }
};

typedef uint32_t u32x4m __attribute__((ext_vector_type(4), aligned(8)));  // a mask's half: the caller's u64 alignment

// Group g's mask, two 16-B loads.
__device__ __forceinline__ WideMask load_wide_mask(const uint64_t* __restrict__ masks, uint64_t g) {
  const u32x4m* p = reinterpret_cast<const u32x4m*>(masks + g * kWideMaskWords);
  const u32x4m lo = p[0], hi = p[1];
  return {{static_cast<uint64_t>(lo.y) << 32 | lo.x, static_cast<uint64_t>(lo.w) << 32 | lo.z,
           static_cast<uint64_t>(hi.y) << 32 | hi.x, static_cast<uint64_t>(hi.w) << 32 | hi.z}};
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
  return static_cast<uint64_t>(hi) << 32 | lo;
}

}  // namespace
}  // namespace qfec
