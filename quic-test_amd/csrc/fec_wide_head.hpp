// fec_wide_head.hpp — the wide record's header as the kernels that consume a wide record read it
// (fec_plan_build_wide.hpp states the layout): decode_wide (fec_wide.hip) and recover_scatter_wide
// (fec_wide_table.hip).  Internal to its translation unit (unnamed namespace), as fec_device.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fec_device.hpp"  // Tab
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

}  // namespace
}  // namespace qfec
