// fec_scan.hpp — the block-wide scan and sum of the row-prefix kernels: rows_block_sums,
// rows_scan_blocks and rows_write over one-word masks (fec_runs.hip), rows_block_sums_wide and
// rows_write_wide over four-word masks (fec_packed.hip).  256-thread workgroups.  Internal to its
// translation unit (unnamed namespace), as fec_device.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace qfec {
namespace {

// Inclusive scan of one value per thread over a 256-thread block (LDS, 8 steps).
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t* lds) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    const uint32_t add = t >= d ? lds[t - d] : 0u;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  return lds[t];
}

// Sum of one value per thread over a 256-thread block (wave reduction, then 4 partials).
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t total = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return total;
}

}  // namespace
}  // namespace qfec
